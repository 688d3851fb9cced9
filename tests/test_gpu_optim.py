"""GPU: the fused Adam step (kernels_optim.hip; holo_adam_step, holo_grad_norm, holo_unet_adam_step; optim.HoloAdam) against
torch.optim.Adam - the reference's optimiser (trainer/optimizer_factory.py:78-149) - and, for the denoiser, against a freshly
bound net: after a native step the library's packed weight copies must be the ones a re-bind would make.

Tolerance of every parity check (measured here, per tensor, for parameters and both moments): with f64 = torch's Adam on
the CPU in float64 on the same float32 inputs,  max|hip - f64| <= 2 * max|torch fp32 on the CPU - f64| + 1 ulp(max|f64|):
the kernel performs torch's operations with the same number of roundings, possibly contracted differently."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, optim, runtime  # noqa: E402
from holo_diffusion_amd._lib import HoloError  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

EMU = os.environ.get("HOLO_TEST_EMU") == "1"
C, NT = optim.ADAM_CHUNK, optim.ADAM_TABLE_TENSORS
PAD, SENTINEL, STEPS = 64, 12345.678, 5
# one-digit sizes and sizes around the 16-byte / chunk / table boundaries; (NT + 1) two-element tensors force a second launch;
# the last tensor is a view at storage offset 1 (not 16-byte aligned: the scalar path)
SIZES = [1, 3, 5, 64, 1023, C, C + 1, 3 * C + 7] + [2] * (NT + 1) + [1001]
HYPER = {"plain": dict(weight_decay=0.0, adamw=False), "l2": dict(weight_decay=0.01, adamw=False),
         "adamw": dict(weight_decay=0.01, adamw=True)}
LR = 1e-3


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


@pytest.fixture(scope="module")
def inputs():
    """Parameters in +-0.05 and STEPS gradient sets spanning 1e-6 .. 1 in magnitude, every 7th element exactly 0."""
    gen = torch.Generator().manual_seed(2024)
    params = [(torch.rand(n, generator=gen) * 2 - 1) * 0.05 for n in SIZES]

    def grad(n):
        g = torch.pow(10.0, -6.0 * torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
        g[::7] = 0.0
        return g.float()
    return params, [[grad(n) for n in SIZES] for _ in range(STEPS)]


def _torch_adam(params, grad_steps, dtype, hyper, max_norm=0.0):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    cls = torch.optim.AdamW if hyper["adamw"] else torch.optim.Adam
    opt = cls(ps, lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=hyper["weight_decay"], foreach=False)
    for grads in grad_steps:
        for p, g in zip(ps, grads):
            p.grad = g.to(dtype).clone()
        if max_norm:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps])


def _carve(values, dev, off=0):
    """`values` inside a larger buffer of sentinels: (buffer, view)."""
    n = values.numel()
    buf = torch.full((n + 2 * PAD + 4,), SENTINEL, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off:PAD + off + n]
    view.copy_(values)
    return buf, view


def _sentinels_intact(buf, view):
    lo = view.storage_offset()
    want = torch.full((1,), SENTINEL).view(torch.int32).item()
    edges = torch.cat([buf[:lo], buf[lo + view.numel():]]).cpu().view(torch.int32)
    return bool((edges == want).all())


def _hip_adam(params, grad_steps, hyper, dev, max_norm=0.0):
    """HoloAdam over tensors that all live between sentinels; returns (p, m, v, optimiser) on the CPU after checking them."""
    bufs, named, state = [], {}, []
    for i, p in enumerate(params):
        off = 1 if i == len(params) - 1 else 0
        pb, pv = _carve(p, dev, off)
        mb, mv = _carve(torch.zeros_like(p), dev)
        vb, vv = _carve(torch.zeros_like(p), dev)
        assert (pv.data_ptr() % 16 == 0) == (off == 0)
        bufs += [(pb, pv), (mb, mv), (vb, vv)]
        named[f"t{i}"] = pv
        state.append((mv, vv))
    opt = hda.HoloAdam(lr=LR, max_grad_norm=max_norm, **hyper).add_tensors(named, "g")
    grp = opt._groups[0]
    for j, (mv, vv) in enumerate(state):  # the moments are the caller's memory: here, memory with sentinels around it
        grp.exp_avg[j], grp.exp_avg_sq[j] = mv, vv
    for grads in grad_steps:
        gd = {}
        for i, g in enumerate(grads):
            gb, gv = _carve(g, dev)
            bufs.append((gb, gv))
            gd[f"t{i}"] = gv
        opt.step({"g": gd})
    torch.cuda.synchronize()
    assert all(_sentinels_intact(b, v) for b, v in bufs), "a write outside a tensor"
    return ([named[f"t{i}"].cpu() for i in range(len(params))], [m.cpu() for m, _ in state], [v.cpu() for _, v in state], opt)


def _parity(tag, hip, t32, t64):
    for what, hs, as_, bs in zip(("param", "exp_avg", "exp_avg_sq"), hip, t32, t64):
        worst = (0.0, -1)
        for i, (h, a, b) in enumerate(zip(hs, as_, bs)):
            b = b.reshape(-1)
            err = (h.reshape(-1).double() - b).abs().max().item()
            ref = (a.reshape(-1).double() - b).abs().max().item()
            bound = 2.0 * ref + float(np.spacing(np.float32(b.abs().max().item())))
            worst = max(worst, (err / bound, i))
            assert err <= bound, (tag, what, i, h.numel(), err, ref, bound)
        print(f"{tag} {what}: worst error / bound {worst[0]:.3f} (tensor {worst[1]})")


@pytest.mark.parametrize("mode", list(HYPER))
def test_generic_step_parity_and_bounds(gu, inputs, mode):
    """Five steps over every size class, in the three decay modes, inside sentinels (checked in _hip_adam)."""
    params, grad_steps = inputs
    hip = _hip_adam(params, grad_steps, HYPER[mode], gu.DEV)[:3]
    _parity(mode, hip, _torch_adam(params, grad_steps, torch.float32, HYPER[mode]),
            _torch_adam(params, grad_steps, torch.float64, HYPER[mode]))


def test_a_tensor_longer_than_one_table(gu):
    """More chunks than one launch has entries: the tensor continues in the next table (the 14 M-element weights of the
    north-star net do), and the tensor behind it starts there too.  One clipped step, inside sentinels."""
    entries = optim.ADAM_TABLE_ENTRIES
    gen = torch.Generator().manual_seed(77)
    sizes = [entries * C + 5, 9]
    params = [(torch.rand(n, generator=gen) * 2 - 1) * 0.05 for n in sizes]
    grads = [[torch.randn(n, generator=gen) * 1e-2 for n in sizes]]
    max_norm = 0.5 * math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads[0]))
    hip = _hip_adam(params, grads, HYPER["l2"], gu.DEV, max_norm=max_norm)
    assert abs(hip[3].last_grad_norm.item() - 2.0 * max_norm) <= 2e-6 * max_norm
    _parity("long", hip[:3], _torch_adam(params, grads, torch.float32, HYPER["l2"], max_norm),
            _torch_adam(params, grads, torch.float64, HYPER["l2"], max_norm))


def _native_norm(grads, max_norm, dev):
    L = runtime.lib()
    arr = (_lib.HoloAdamTensor * len(grads))()
    for i, g in enumerate(grads):
        arr[i].grad, arr[i].numel = g.data_ptr(), g.numel()
    ws = torch.empty(int(L.holo_grad_norm_workspace_bytes(arr, len(grads))) // 8 + 1, dtype=torch.float64, device=dev)
    out = torch.zeros(2, device=dev)
    _lib.check(L, L.holo_grad_norm(runtime.ctx(dev), arr, len(grads), max_norm, runtime.ptr(ws), ws.numel() * 8, runtime.ptr(out),
                                   ctypes.c_void_p(out.data_ptr() + 4), runtime.stream_ptr(dev)), "holo_grad_norm")
    torch.cuda.synchronize()
    return out.cpu()


def test_grad_norm_and_clipping(gu, inputs):
    params, grad_steps = inputs
    grads = grad_steps[0]
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    dg = [g.to(gu.DEV) for g in grads]
    a, b = _native_norm(dg, 0.5 * want, gu.DEV), _native_norm(dg, 0.5 * want, gu.DEV)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two identical calls differ"
    assert abs(a[0].item() - want) <= 1e-6 * want, (a[0].item(), want)
    assert abs(a[1].item() - 0.5 * want / (want + 1e-6)) <= 1e-6
    assert _native_norm(dg, 2.0 * want, gu.DEV)[1].item() == 1.0
    # max_norm above the norm: the coefficient is 1, the step is the unclipped step bit for bit
    one = grad_steps[:1]
    free = _hip_adam(params, one, HYPER["plain"], gu.DEV)
    loose = _hip_adam(params, one, HYPER["plain"], gu.DEV, max_norm=2.0 * want)
    assert abs(loose[3].last_grad_norm.item() - want) <= 1e-6 * want and free[3].last_grad_norm is None
    for xs, ys in zip(free[:3], loose[:3]):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(xs, ys))
    # max_norm at half the norm: torch with clip_grad_norm_ applied first
    hip = _hip_adam(params, grad_steps, HYPER["plain"], gu.DEV, max_norm=0.5 * want)[:3]
    _parity("clipped", hip, _torch_adam(params, grad_steps, torch.float32, HYPER["plain"], 0.5 * want),
            _torch_adam(params, grad_steps, torch.float64, HYPER["plain"], 0.5 * want))


UNET_CFGS = {"wide": uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2,
                                channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2),
             "deep": uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=32, num_res_blocks=1,
                                channel_mult=(1, 2, 3), attention_resolutions=(4,), num_heads=2)}


def _unet_case(gu, cfg):
    net, sd = gu.make_unet(cfg, seed=5)
    shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(1, shape)).to(gu.DEV)
    t = torch.tensor([437], dtype=torch.int64, device=gu.DEV)
    G = torch.from_numpy(np_noise(2, (1, cfg.out_channels) + (cfg.image_size,) * 3)).to(gu.DEV)
    return net, sd, x, t, G


@pytest.mark.parametrize("cfg_name", list(UNET_CFGS))
def test_denoiser_step_leaves_the_packed_weights_current(gu, cfg_name):
    """Two native steps with a fresh backward between them: parameters and moments against torch's Adam on the same
    gradients; then forward and backward bit-identical to a second net that loads the updated state dict and binds it the
    ordinary way (forward packs, Winograd copies, transposed packs, the Downsample pair) - without a single re-bind."""
    if EMU:
        pytest.skip("backward tests run on the device")
    cfg = UNET_CFGS[cfg_name]
    net, sd, x, t, G = _unet_case(gu, cfg)
    hyper = dict(weight_decay=0.0, adamw=False)
    opt = hda.HoloAdam(lr=LR).add_unet(net)
    _, _, g1 = net.backward(x, t, G)  # binds the parameters, prepares the transposed weights
    names = list(sd)
    versions = {k: p._version for k, p in net._net.named_parameters()}
    epoch, rebinds = net.weights_epoch(), net.rebinds
    opt.step(g1)  # (one group: its flat gradient dict)
    assert net.weights_epoch() > epoch
    assert all(p._version > versions[k] for k, p in net._net.named_parameters())
    net.forward_train(x, t)
    _, g2 = net.backward_taped(G)
    opt.step({"unet": g2})
    assert net.rebinds == rebinds, "a native step must not leave the net dirty"
    grad_steps = [[g[k].cpu().reshape(-1) for k in names] for g in (g1, g2)]
    params = [sd[k].reshape(-1) for k in names]
    got = dict(net._net.named_parameters())
    grp = opt._groups[0]
    where = {k: j for j, k in enumerate(grp.names)}
    hip = ([got[k].detach().cpu() for k in names], [grp.exp_avg[where[k]].cpu() for k in names],
           [grp.exp_avg_sq[where[k]].cpu() for k in names])
    _parity(cfg_name, hip, _torch_adam(params, grad_steps, torch.float32, hyper), _torch_adam(params, grad_steps, torch.float64, hyper))
    # the same values bound the ordinary way
    fresh, _ = gu.make_unet(cfg, seed=99)
    fresh.load_state_dict(net.state_dict())
    fresh = fresh.to(gu.DEV)
    with torch.no_grad():
        assert torch.equal(net(x, t), fresh(x, t))
    ya, gxa, ga = net.backward(x, t, G)
    yb, gxb, gb = fresh.backward(x, t, G)
    assert torch.equal(ya, yb) and torch.equal(gxa, gxb)
    assert set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    net.forward_train(x, t)
    net.backward_taped(G)
    assert net.rebinds == rebinds and fresh.rebinds >= 2


def test_a_native_step_drops_the_tape(gu):
    """forward_train, a step, backward_taped: the taped activations belong to the old weights (what
    test_tape_does_not_survive_a_handle_switch_or_a_weight_update pins for torch-side updates)."""
    if EMU:
        pytest.skip("backward tests run on the device")
    net, sd, x, t, G = _unet_case(gu, UNET_CFGS["wide"])
    _, _, g = net.backward(x, t, G)
    opt = hda.HoloAdam(lr=LR).add_unet(net)
    net.forward_train(x, t)
    opt.step(g)
    with pytest.raises(HoloError):
        net.backward_taped(G)
    with pytest.raises(HoloError):  # all or none for the denoiser
        opt.step({k: v for k, v in g.items() if k != "out.2.bias"})


def test_model_level_training_loop(gu):
    """HoloAdam.from_model(model).step(model.training_step(...)): the denoiser and the RenderMLP move, the RenderMLP's
    owners re-bind through the version counters, a second step runs clean."""
    if EMU:
        pytest.skip("backward tests run on the device")
    import torch.nn.functional as F
    R, Cf, P, Pf, n_rays = 8, 16, 16, 16, 29
    model, *_ = gu.make_model(R, Cf, 16, 16, dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2)), n_fine=64)
    model.n_train_target_views = 2
    model.raysampler.n_pts_per_ray_training = P
    model.renderer.n_pts_per_ray_fine_training = Pf
    cams = hda.get_simple_360_camera_trajectory(2 * math.pi, 3, -0.5, 10, (0.0, -1.0, 0.0), 3.2).to(gu.DEV)
    vf = torch.tanh(torch.from_numpy(np_noise(5, (1, Cf, R, R, R)))).to(gu.DEV)
    u = lambda s, shp: torch.from_numpy(np_noise(s, shp)).mul(0.5).erf().add(1).mul(0.5).clamp(0, 0.999999)  # noqa: E731
    rs = {"u_coarse": u(1200, (2, n_rays, P)), "u_fine": u(1201, (2, n_rays, Pf)),
          "noise_coarse": torch.from_numpy(np_noise(1202, (2, n_rays, P))),
          "noise_fine": torch.from_numpy(np_noise(1203, (2, n_rays, P + Pf))),
          "xys": (torch.from_numpy(np_noise(13, (2, n_rays, 2))).clamp(-2, 2) * 0.45).contiguous(),
          "timesteps": torch.tensor([420]), "q_noise": torch.from_numpy(np_noise(41, tuple(vf.shape))), "bootstrap": False}
    rs = {k: (v.to(gu.DEV) if torch.is_tensor(v) else v) for k, v in rs.items()}
    target = torch.from_numpy(np_noise(51, (2, 3, n_rays, 1))).mul(0.3).add(0.5).clamp(0, 1).to(gu.DEV)
    loss_fn = lambda p: F.mse_loss(p["images_render"], target) + F.mse_loss(p["images_render_coarse"], target)  # noqa: E731
    mlp = model._implicit_functions[0]._fn.render_mlp
    feats = torch.from_numpy(np_noise(7, (11, Cf))).to(gu.DEV)
    dirs = torch.nn.functional.normalize(torch.from_numpy(np_noise(8, (11, 3))), dim=-1).to(gu.DEV)
    before = [o.clone() for o in mlp(feats, dirs)[:2]]
    w0 = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = hda.HoloAdam.from_model(model, lr=1e-2, max_grad_norm=1.0)
    assert [g.name for g in opt._groups] == ["unet", "render_mlp"]
    out = model.training_step(camera=cams, voxel_features=vf, rng_streams=rs, loss_fn=loss_fn)
    opt.step(out)
    assert torch.isfinite(opt.last_grad_norm).item() and opt.last_grad_norm.item() > 0
    moved = [k for k, p in model.named_parameters() if not torch.equal(p, w0[k])]
    assert any(k.startswith("net_3d.") for k in moved) and any("render_mlp" in k for k in moved)
    after = mlp(feats, dirs)[:2]
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    out2 = model.training_step(camera=cams, voxel_features=vf, rng_streams=rs, loss_fn=loss_fn)
    assert torch.isfinite(out2["loss"]).item() and out2["loss"].item() != out["loss"].item()
    opt.step(out2)
    assert all(torch.isfinite(p).all() for p in model.parameters())
