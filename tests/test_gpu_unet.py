"""GPU parity: the HIP denoiser (through SimpleUnet3D -> C ABI) vs the golden vectors recorded from the
reference and vs the CPU oracle.  Tolerances (fp32 path): block outputs and full forward
max|d| <= 2e-3 * max|y| (reassociation over K <= 27*1024), observed ~1e-5."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, runtime  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import NORTH_CFG, PLUMB_CFG, TINY_CFG, digest, seeded_input  # noqa: E402

TOL = 2e-3


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def test_native_library_loaded():
    lib = runtime.lib()
    assert lib.holo_abi_version() == _lib.ABI_VERSION == 6
    assert os.path.basename(_lib.LIB_PATH) == "libholo_mi355x.so"


def test_tiny_unet_vs_reference_golden(gu, golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_unet.npz"))
    os.environ["HOLO_KEEP_INTERMEDIATES"] = "1"
    try:
        net, _ = gu.make_unet(TINY_CFG)
        for t in (0, 500, 999):
            x = seeded_input(TINY_CFG, 7 + t).to(gu.DEV)
            y = net(x, torch.tensor([t], device=gu.DEV))
            assert gu.rel_err(y, torch.from_numpy(g[f"t{t}.y"])) < TOL, t
        # every block output of the last forward at t=500
        x = seeded_input(TINY_CFG, 7 + 500).to(gu.DEV)
        net(x, torch.tensor([500], device=gu.DEV))
        L = runtime.lib()
        ws = runtime.workspace(net, gu.DEV, 0)
        for k in g.files:
            if not k.startswith("t500.") or k in ("t500.y", "t500.emb"):
                continue
            ref = torch.from_numpy(g[k])
            dst = torch.empty(ref.shape, device=gu.DEV)
            n = C.c_int64()
            _lib.check(L, L.holo_unet_fetch_block(net._handle, k[5:].encode(), runtime.ptr(dst), dst.numel(),
                                                  C.byref(n), runtime.ptr(ws), runtime.stream_ptr(gu.DEV)), k)
            assert n.value == ref.numel()
            assert gu.rel_err(dst, ref) < TOL, k
    finally:
        os.environ.pop("HOLO_KEEP_INTERMEDIATES", None)


def test_fetch_block_after_workspace_size_queries(gu, golden_dir, monkeypatch):
    """The workspace-size queries plan aside and leave the plan of the last forward alone: a block output reads the same,
    bit for bit, after sizes that no cache holds yet were asked for (the forward at another batch, the training plan)."""
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    ref = torch.from_numpy(np.load(os.path.join(golden_dir, "tiny_unet.npz"))["t500.middle_block"])
    net, _ = gu.make_unet(TINY_CFG)
    net(seeded_input(TINY_CFG, 7 + 500).to(gu.DEV), torch.tensor([500], device=gu.DEV))
    before = net.fetch_block("middle_block", tuple(ref.shape)).clone()
    assert gu.rel_err(before, ref) < TOL
    assert net.workspace_bytes(3, gu.DEV) > 0
    assert runtime.lib().holo_unet_backward_workspace_bytes(net._handle, 1) > 0
    after = net.fetch_block("middle_block", tuple(ref.shape))
    assert torch.equal(before, after)


def test_tiny_unet_batch2(gu, golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_unet_b2.npz"))
    net, _ = gu.make_unet(TINY_CFG)
    x2 = torch.cat([seeded_input(TINY_CFG, 100), seeded_input(TINY_CFG, 101)]).to(gu.DEV)
    y = net(x2, torch.tensor([17, 803], device=gu.DEV))
    assert gu.rel_err(y, torch.from_numpy(g["y"])) < TOL
    # batch rows are independent chains
    y0 = net(x2[:1], torch.tensor([17], device=gu.DEV))
    assert gu.rel_err(y0, torch.from_numpy(g["y"][:1])) < TOL


def test_cond_features_concat(gu):
    """SimpleUnet3D.forward concatenates cond_features on the channel axis (diffusion_utils.py:83-84)."""
    net, sd = gu.make_unet(TINY_CFG)
    x = seeded_input(TINY_CFG, 5)
    y = net(x[:, :20].to(gu.DEV), torch.tensor([3], device=gu.DEV), cond_features=x[:, 20:].to(gu.DEV))
    ref = uo.unet_forward(sd, TINY_CFG, x, torch.tensor([3]))
    assert gu.rel_err(y, ref) < TOL


@pytest.mark.parametrize("image,mc,mult,attn,batch", [
    (8, 64, (1, 2), (2,), 1),      # fused 1x1x1 skip + split-K on the LDS-halo kernel, small-M kernel below
    (16, 64, (1, 2, 2), (4,), 2),  # 64-voxel halo tiles, stride-2 gather kernel, batch 2
    (16, 32, (1, 1), (), 1),       # 32-wide Cout tiles (NWN=2) on both halo tile depths
])
def test_mid_size_unet_vs_oracle_blockwise(gu, image, mc, mult, attn, batch):
    """Sizes between the reference goldens: every block output against the pinned oracle (per-op tolerance of
    SURVEY.md 8c: rtol 1e-4 of the tensor scale)."""
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=2,
                     channel_mult=mult, attention_resolutions=attn, num_heads=2)
    import os
    os.environ["HOLO_KEEP_INTERMEDIATES"] = "1"
    try:
        net, sd = gu.make_unet(cfg, seed=99)
        from oracle.common import np_noise
        x = torch.from_numpy(np_noise(11, (batch, 16, image, image, image)))
        t = torch.tensor([321, 17][:batch], dtype=torch.int64)
        trace = {}
        ref = uo.unet_forward(sd, cfg, x, t, trace)
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        assert gu.rel_err(y, ref) < 1e-4
        gu.block_outputs_vs_oracle(net, trace, 1e-4)
    finally:
        del os.environ["HOLO_KEEP_INTERMEDIATES"]


@pytest.mark.parametrize("wino_kernel,wino_env", [("conv_wino3_kernel", "2"), ("conv_wino2_kernel", "2")])
@pytest.mark.parametrize("image,mc,mult,attn,batch", [(16, 64, (1, 2), (), 1), (8, 64, (1, 2, 2), (2,), 2),
                                                       (16, 32, (1, 1), (), 1)])  # 32-channel convs: two-wave-row variant
def test_winograd_kernels_blockwise(gu, image, mc, mult, attn, batch, wino_kernel, wino_env, monkeypatch):
    """conv_wino3_kernel / conv_wino2_kernel (the Winograd F(2,3) forms over all three axes - what the 64^3 and 32^3
    levels of the north-star net run on -, over (depth, height)) forced onto small grids: plain,
    fused-skip, upsample-on-load, virtual-concat and split-K launches, every block output against the pinned oracle at
    the SAME per-op tolerance as the direct kernel."""
    monkeypatch.setenv("HOLO_CONV_FORCE_TZ2", "1")
    monkeypatch.setenv("HOLO_CONV_WINO", wino_env)  # anything but 0 (the default): the Winograd weights prepared
    if wino_kernel == "conv_wino3_kernel":
        monkeypatch.setenv("HOLO_CONV_WINO3_MIN_ITEMS", "1")  # the three-axis form on work lists far below one per CU
        if mc == 32:
            pytest.skip("the three-axis form needs 64-channel output blocks")
    else:
        monkeypatch.setenv("HOLO_CONV_WINO3", "0")
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=2,
                     channel_mult=mult, attention_resolutions=attn, num_heads=2)
    net, sd = gu.make_unet(cfg, seed=77)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(19, (batch, 16, image, image, image)))
    t = torch.tensor([611, 3][:batch], dtype=torch.int64)
    trace = {}
    ref = uo.unet_forward(sd, cfg, x, t, trace)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    assert gu.rel_err(y, ref) < 1e-4
    for tag, r in trace.items():
        if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block":
            assert gu.rel_err(net.fetch_block(tag, tuple(r.shape)), r) < 1e-4, tag
    # (time_ops runs its own forward on random data: only after the block outputs of OUR forward have been read)
    kernels = {o["kernel"] for o in net.time_ops(batch, 1, gu.DEV) if o["op"] == "conv"} if not gu.EMU else {wino_kernel}
    assert wino_kernel in kernels  # the knobs really put launches on the kernel under test
    # and the direct kernel on the same net agrees with it to rounding
    monkeypatch.setenv("HOLO_CONV_FORCE_TZ2", "0")
    monkeypatch.setenv("HOLO_CONV_WINO", "0")
    monkeypatch.setenv("HOLO_CONV_WINO3", "0")
    net2, _ = gu.make_unet(cfg, seed=77)
    with torch.no_grad():
        y2 = net2(x.to(gu.DEV), t.to(gu.DEV))
    assert gu.rel_err(y2, y.cpu()) < 1e-5


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_forward_channels_last_equals_forward(gu, compute):
    """holo_unet_forward_cl (ABI 5): the forward on (N, R, R, R, C) tensors - the first convolution reads the caller's tensor, the
    last one writes the caller's tensor, no layout pass - is bit-equal to the NCDHW call; batch 2; also after a plain call on
    the same handle (the two entries share the plan).  bf16 storage mode (ABI 6): an element-wise cast of the caller's tensor
    replaces the transposing layout pass (same rounding), the last convolution writes the caller's fp32 tensor."""
    net, _ = gu.make_unet(TINY_CFG, compute_dtype=compute)
    x = torch.cat([seeded_input(TINY_CFG, 21), seeded_input(TINY_CFG, 22)]).to(gu.DEV)
    t = torch.tensor([640, 3], device=gu.DEV)
    y = net(x, t)
    x_cl = x.permute(0, 2, 3, 4, 1).contiguous()
    y_cl = net.forward_channels_last(x_cl, t)
    assert y_cl.shape == x_cl.shape and torch.equal(y_cl.permute(0, 4, 1, 2, 3), y)
    assert torch.equal(net(x, t), y) and torch.equal(net.forward_channels_last(x_cl, t), y_cl)
    from holo_diffusion_amd._lib import HoloError
    with pytest.raises(HoloError):
        net.forward_channels_last(x, t)  # an NCDHW tensor is not (N, R, R, R, C)


def test_streaming_skip_connection_blockwise(gu, monkeypatch):
    """conv1x1_stream_kernel - a ResBlock's 1x1x1 skip_connection (unet.py:222) as a launch of its own, the form the 64^3
    level of the north-star net runs (its output is the residual of the block's second convolution) - forced onto a small
    grid: every block output against the pinned oracle at the per-op tolerance, plain and virtual-concat inputs (64 -> 128
    on the way down; (128 + 128) -> 128, (128 + 64) -> 128 / 64 and (64 + 64) -> 64 on the way up), and equal to the
    all-fused plan up to rounding."""
    monkeypatch.setenv("HOLO_SKIP_FUSION_BELOW_R", "8")
    monkeypatch.setenv("HOLO_CONV1X1_STREAM_MIN_M", "64")
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                     attention_resolutions=(), num_heads=2)
    net, sd = gu.make_unet(cfg, seed=61)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(29, (2, 16, 16, 16, 16)))
    t = torch.tensor([77, 901], dtype=torch.int64)
    trace = {}
    ref = uo.unet_forward(sd, cfg, x, t, trace)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    assert gu.rel_err(y, ref) < 1e-4
    for tag, r in trace.items():
        if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block":
            assert gu.rel_err(net.fetch_block(tag, tuple(r.shape)), r) < 1e-4, tag
    if not gu.EMU:
        ops = [o for o in net.time_ops(2, 1, gu.DEV) if o["op"] == "conv"]
        assert sum(o["kernel"] == "conv1x1_stream_kernel" for o in ops) == 5, [(o["kernel"], o["ksz"], o["cin"]) for o in ops]
        assert not any(o["fused_skip"] for o in ops)
    monkeypatch.setenv("HOLO_SKIP_FUSION_BELOW_R", "1000")  # the fused form on the same net
    net2, _ = gu.make_unet(cfg, seed=61)
    with torch.no_grad():
        y2 = net2(x.to(gu.DEV), t.to(gu.DEV))
    assert gu.rel_err(y2, y.cpu()) < 1e-5


@pytest.mark.parametrize("tag,cfg,compute", [("plumb32x16", PLUMB_CFG, "f32"), ("north64x32", NORTH_CFG, "f32"),
                                             ("north64x32", NORTH_CFG, "f32_bf16x3")])
def test_full_size_unet_vs_reference_digest(gu, golden_dir, tag, cfg, compute):
    """BASELINE configs[0] (32^3x16) and configs[1] (64^3x32): digests of the REFERENCE output; the fp32-accurate
    bf16x3 mode is held to the same tolerance as the exact-fp32 path."""
    g = np.load(os.path.join(golden_dir, "full_unet_digests.npz"))
    net, _ = gu.make_unet(cfg, compute_dtype=compute)
    for t in (0, 500, 999):
        y = net(seeded_input(cfg, 7 + t).to(gu.DEV), torch.tensor([t], device=gu.DEV)).cpu()
        assert torch.isfinite(y).all()
        d = digest(y)
        scale = np.abs(g[f"{tag}.t{t}.head"]).max()
        assert np.abs(d["head"] - g[f"{tag}.t{t}.head"]).max() < TOL * scale
        assert np.abs(d["probe"] - g[f"{tag}.t{t}.probe"]).max() < TOL * scale
        np.testing.assert_allclose(d["mean"], g[f"{tag}.t{t}.mean"], atol=TOL * scale)
        np.testing.assert_allclose(d["std"], g[f"{tag}.t{t}.std"], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(d["min"], g[f"{tag}.t{t}.min"], atol=TOL * scale)
        np.testing.assert_allclose(d["max"], g[f"{tag}.t{t}.max"], atol=TOL * scale)


def test_forward_is_deterministic_and_param_rebind(gu):
    net, sd = gu.make_unet(TINY_CFG)
    x = seeded_input(TINY_CFG, 1).to(gu.DEV)
    t = torch.tensor([10], device=gu.DEV)
    a, b = net(x, t), net(x, t)
    assert torch.equal(a, b)  # split-K reduces in a fixed order: bit-reproducible
    # changing a parameter and re-binding changes the output accordingly
    sd2 = dict(sd)
    sd2["out.2.bias"] = sd["out.2.bias"] + 1.0
    net.load_state_dict({"_net." + k: v for k, v in sd2.items()})
    c = net(x, t)
    torch.testing.assert_close(c, a + 1.0, rtol=1e-5, atol=1e-5)


def test_in_place_parameter_update_is_noticed_without_a_hint(gu):
    """An optimiser step / ``p.add_()`` goes through none of the module hooks: the plugin compares every parameter's
    (storage, version counter) on each call and re-uploads (round-3 advisor finding: the forward kept the old weights
    while the transposed dgrad weights were refreshed)."""
    net, sd = gu.make_unet(TINY_CFG)
    x = seeded_input(TINY_CFG, 1).to(gu.DEV)
    t = torch.tensor([10], device=gu.DEV)
    a = net(x, t)
    e0 = net.weights_epoch()
    with torch.no_grad():
        dict(net.named_parameters())["_net.out.2.bias"].add_(1.0)  # no mark_parameters_changed()
    assert net.weights_epoch() == e0 + 1
    b = net(x, t)
    torch.testing.assert_close(b, a + 1.0, rtol=1e-5, atol=1e-5)
    # a convolution weight: forward AND backward must both see the new values (oracle on the updated state dict)
    name = "input_blocks.1.0.in_layers.2.weight"
    with torch.no_grad():
        dict(net.named_parameters())["_net." + name].mul_(1.5)
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["out.2.bias"] += 1.0
    sd2[name] *= 1.5
    xr = seeded_input(TINY_CFG, 1).requires_grad_(True)
    with torch.enable_grad():
        yr = uo.unet_forward.__wrapped__(sd2, TINY_CFG, xr, torch.tensor([10]))
        w = torch.from_numpy(np.random.RandomState(3).randn(*yr.shape).astype(np.float32))
        gxr, = torch.autograd.grad((yr * w).sum(), xr)
    y, gx, _ = net.backward(x, t, w.to(gu.DEV), params=[])
    assert gu.rel_err(y, yr.detach()) < TOL
    assert gu.rel_err(gx, gxr) < 2e-3
    assert gu.rel_err(net(x, t), yr.detach()) < TOL


def test_backward_after_a_grid_size_switch(gu):
    """A forward at another grid size recreates the native handle; the transposed (dgrad) weights of the new handle must
    be prepared again even if malloc hands out the old address (round-3 advisor finding)."""
    net, sd = gu.make_unet(TINY_CFG)
    R = TINY_CFG.image_size
    t = torch.tensor([10], device=gu.DEV)
    x = seeded_input(TINY_CFG, 1).to(gu.DEV)
    g = torch.ones_like(x)
    _, gx_a, _ = net.backward(x, t, g, params=[])
    big = torch.zeros(1, TINY_CFG.in_channels, 2 * R, 2 * R, 2 * R, device=gu.DEV)
    net(big, t)  # switches the plan (and the handle) to the larger grid
    net.backward(big, t, torch.ones_like(big), params=[])
    _, gx_b, _ = net.backward(x, t, g, params=[])  # and back
    assert torch.equal(gx_a, gx_b)


def test_wrong_shape_and_unset_errors(gu):
    net, _ = gu.make_unet(TINY_CFG)
    for bad in ((1, 16, 8, 8, 8), (1, 32, 7, 7, 7), (1, 32, 8, 8, 4)):  # channels; not a multiple of 2^(levels-1); not cubic
        with pytest.raises(_lib.HoloError):
            net(torch.zeros(*bad, device=gu.DEV), torch.zeros(1, dtype=torch.long, device=gu.DEV))


def test_128_cubed_forward_vs_oracle(gu):
    """BASELINE configs[4] (donut.yaml: 128^3 x 32 grid).  (1) the fp32 path: full forward against the pinned oracle
    run on the host cores (the oracle takes ~1 min at this size), tolerance of SURVEY.md 8c for a full forward;
    (2) the opt-in bf16 mode at the SAME size against the SAME fp32 oracle output at rtol 2e-2, which
    reaches the shared-tile bf16 attention kernel natively (T = 32 768 tokens at the 32^3 level, no env knob);
    (3) one rendered 200x200 frame of tanh(y): bf16-denoised grid vs oracle grid, PSNR >= 40 dB."""
    import math

    import holo_diffusion_amd as hda
    from oracle import render_oracle as ro
    cfg = uo.UNetCfg(image_size=128, in_channels=32, out_channels=32, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 1, 2, 4, 8), attention_resolutions=(4, 8), num_heads=2)
    net, sd = gu.make_unet(cfg, seed=1234)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(31, (1, 32, 128, 128, 128)))
    t = torch.tensor([500], dtype=torch.int64)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
        y2 = net(x.to(gu.DEV), t.to(gu.DEV))
    assert torch.equal(y, y2)  # deterministic (no atomics anywhere on the path)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = uo.unet_forward(sd, cfg, x, t)
    assert torch.isfinite(y).all()
    assert (y.cpu() - ref).abs().max() <= 2e-3 * ref.abs().max()
    # (2) donut.yaml's arithmetic: bf16 products / fp32 accumulate, judged against the fp32 oracle
    net.compute_dtype = "bf16"
    with torch.no_grad():
        ybf = net(x.to(gu.DEV), t.to(gu.DEV))
    err = gu.rel_err(ybf, ref)
    assert 1e-5 < err < 2e-2, err
    # (3) rendered-frame PSNR of the bf16 result against the oracle grid (same HIP renderer, exact fp32)
    H = W = 200
    fn = hda.HoloVoxelGridImplicitFunction(resol=128, n_hidden=32, feature_dim=0)
    msd = gu.synth_state_dict(ro.render_mlp_param_shapes(ro.RenderCfg(resol=128, feature_size=32)), 4321)
    fn.render_mlp.load_state_dict(msd)
    fn.to(gu.DEV)
    wrap = hda.render.ImplicitFunctionWrapper(fn)
    renderer = hda.HoloMultiPassEmissionAbsorptionRenderer(
        raymarcher_EmissionAbsorptionRaymarcher_args=dict(bg_color=(1.0, 1.0, 1.0)))
    cams = hda.get_simple_360_camera_trajectory(2 * math.pi, 4, -30.0 * (2 * math.pi / 360), 10, (0.0, -1.0, 0.0), 3.2)
    sampler = hda.render.AdaptiveRaySampler(image_width=W, image_height=H, scene_extent=4.0)
    frames = []
    for grid in (torch.tanh(ybf), torch.tanh(ref.to(gu.DEV))):
        wrap.bind_args(voxel_grid_features=grid)
        out = renderer(ray_bundle=sampler(cams[[1]], hda.render.EvaluationMode.EVALUATION),
                       implicit_functions=[wrap, wrap])
        frames.append(out.features.clone())
    mse = ((frames[0] - frames[1]) ** 2).mean().item()
    psnr = 10.0 * math.log10(1.0 / max(mse, 1e-20))
    assert psnr >= 40.0, psnr


@pytest.mark.parametrize("image,mc,mult,attn", [(8, 64, (1, 2), (2,)), (16, 64, (1, 2, 2), (4,)), (16, 32, (1, 1), ())])
def test_bf16_compute_mode_vs_oracle(gu, image, mc, mult, attn):
    """Opt-in bf16 mode (bf16 activations in HBM, bf16 products / fp32 accumulate, fp32 GroupNorm statistics) against
    the fp32 oracle: tolerance of SURVEY.md 8c for the bf16 path (rtol 2e-2 of the tensor scale); the error must also
    be bf16-sized, not zero."""
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=2,
                     channel_mult=mult, attention_resolutions=attn, num_heads=2)
    net, sd = gu.make_unet(cfg, seed=99, compute_dtype="bf16")
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(11, (2, 16, image, image, image)))
    t = torch.tensor([321, 17], dtype=torch.int64)
    ref = uo.unet_forward(sd, cfg, x, t)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    err = gu.rel_err(y, ref)
    assert 1e-5 < err < 2e-2, err


def test_bf16_compute_mode_full_size_vs_fp32_path(gu):
    """64^3 x 32 north-star net: bf16 mode (bf16 storage, wide-tile kernel on the 64^3 level by the planner's own choice)
    against the (oracle-pinned) fp32 path on the same device."""
    n32, _ = gu.make_unet(NORTH_CFG)
    nbf, _ = gu.make_unet(NORTH_CFG, compute_dtype="bf16")
    assert any(o.get("kernel") == "conv_bf16t_kernel" for o in nbf.time_ops(1, 1, gu.DEV))
    assert nbf.workspace_bytes(1, gu.DEV) < 0.8 * n32.workspace_bytes(1, gu.DEV)  # bf16 activations: smaller HBM footprint
    x = seeded_input(NORTH_CFG, 7 + 500).to(gu.DEV)
    t = torch.tensor([500], device=gu.DEV)
    with torch.no_grad():
        y32 = n32(x, t)
        ybf = nbf(x, t)
    err = ((ybf - y32).abs().max() / y32.abs().max()).item()
    assert 1e-5 < err < 2e-2, err
    # switching back restores the exact fp32 arithmetic
    nbf.compute_dtype = "f32"
    with torch.no_grad():
        y2 = nbf(x, t)
    assert torch.equal(y2, y32)
    # and every mode can be entered from every other on a live net (the plan and its workspace are rebuilt)
    for mode, tol in (("f32_bf16x3", 1e-4), ("bf16", 2e-2), ("f32_bf16x3", 1e-4), ("f32", 0.0)):
        n32.compute_dtype = mode
        with torch.no_grad():
            ym = n32(x, t)
        assert ((ym - y32).abs().max() / y32.abs().max()).item() <= tol, mode


@pytest.mark.parametrize("image,mc,mult,attn", [(16, 64, (1, 2, 2), (1, 2)), (16, 128, (1, 2), (2,))])
def test_bf16_flash_attention_vs_oracle(gu, image, mc, mult, attn, monkeypatch):
    """The bf16 attention kernel forced on at T = 4096 / 512 with head channels 32, 64 and 128 inside the bf16 mode,
    against the fp32 oracle (rtol 2e-2 of the scale): packed operands, transposed V, 32x32x16 tiles, key split +
    recombination (at these sizes the key range IS split 2-8 ways)."""
    monkeypatch.setenv("HOLO_BF16_FLASH_MIN_T", "0")
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=2,
                     channel_mult=mult, attention_resolutions=attn, num_heads=2)
    net, sd = gu.make_unet(cfg, seed=7, compute_dtype="bf16")
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(13, (2, 16, image, image, image)))  # batch 2: (sample, head, query tile) decode
    t = torch.tensor([77, 901], dtype=torch.int64)
    ref = uo.unet_forward(sd, cfg, x, t)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    err = gu.rel_err(y, ref)
    assert 1e-5 < err < 2e-2, err


@pytest.mark.parametrize("wide_tile", ["0", "1", "p"])
def test_bf16_storage_mode_blockwise(gu, wide_tile, monkeypatch):
    """bf16 mode = bf16 activations in HBM: every block output (read back from the bf16 workspace) against the fp32
    oracle at the bf16 tolerance, once on the 64/128-voxel bf16 halo kernels, once with the wide-tile kernel
    (8x8x8 tiles, fused skip from global operands, LDS-transposed epilogue, per-tile GroupNorm slabs) forced onto this
    small grid, and once ("p") with its persistent wave-specialised form (conv_bf16p_kernel: producer waves stage the
    activated halo and the raw centre of a fused skip into two LDS buffers, consumer waves multiply; several tiles per
    workgroup, the 128-output-channel launches as two slices per tile) forced onto it."""
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_CONV_BF16T", "1" if wide_tile == "p" else wide_tile)
    monkeypatch.setenv("HOLO_CONV_BF16P", "1" if wide_tile == "p" else "0")
    if wide_tile == "p":
        monkeypatch.setenv("HOLO_CONV_BF16P_WGS", "8")  # (8 workgroups: the 16^3 level's 2 x 8 tiles are two items per workgroup)
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 2, 2), attention_resolutions=(4,), num_heads=2)
    net, sd = gu.make_unet(cfg, seed=99, compute_dtype="bf16")
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(11, (2, 16, 16, 16, 16)))
    t = torch.tensor([321, 17], dtype=torch.int64)
    trace = {}
    ref = uo.unet_forward(sd, cfg, x, t, trace)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    assert 1e-5 < gu.rel_err(y, ref) < 2e-2
    gu.block_outputs_vs_oracle(net, trace, 2e-2)
    kernels = {o.get("kernel") for o in net.time_ops(2, 1, gu.DEV) if o["op"] == "conv"}
    assert ("conv_bf16t_kernel" in kernels) == (wide_tile == "1"), kernels
    assert ("conv_bf16p_kernel" in kernels) == (wide_tile == "p"), kernels


@pytest.mark.parametrize("mc,heads", [(64, 2), (128, 4), (128, 2)])
def test_bf16_qkv_convolution_fused_with_the_attention_packing(gu, mc, heads, monkeypatch):
    """bf16 storage mode: the qkv convolution of the long-sequence attention blocks writing the packed bf16 operands of
    flash_attn_bf16v2_kernel itself (conv1x1_qkv_bf16_kernel: Q scaled, K, V transposed; 128 and 256 input channels, head
    channels 64 / 64 / 128) against the unfused chain (row-tile kernel -> fp32 qkv -> attn_pack_kernel) on the same net, and
    both against the fp32 oracle block by block - reference guided_diffusion/unet.py:300-305, 436-455."""
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_BF16_FLASH_MIN_T", "256")  # (the 8^3 level's 512 tokens reach the bf16 attention kernel)
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=1,
                     channel_mult=(1, 2), attention_resolutions=(2,), num_heads=heads)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(5, (2, 16, 16, 16, 16)))
    t = torch.tensor([640, 3], dtype=torch.int64)
    trace, outs = {}, {}
    for knob in ("0", "1"):
        monkeypatch.setenv("HOLO_CONV_QKV_FUSED", knob)
        net, sd = gu.make_unet(cfg, seed=41, compute_dtype="bf16")
        if not trace:
            ref = uo.unet_forward(sd, cfg, x, t, trace)
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        assert 1e-5 < gu.rel_err(y, ref) < 2e-2
        tags = [tag for tag in trace if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block"]
        outs[knob] = {tag: net.fetch_block(tag, tuple(trace[tag].shape)).float().cpu() for tag in tags}
        for tag in tags:
            assert gu.rel_err(outs[knob][tag], trace[tag]) < 2e-2, (knob, tag)
        kernels = [o.get("kernel") for o in net.time_ops(2, 1, gu.DEV) if o["op"] == "conv" and o["ksz"] == 1 and o["cout"] == 6 * mc]
        assert len(kernels) == 4 and all((k == "conv1x1_qkv_bf16_kernel") == (knob == "1") for k in kernels), kernels
    # the first attention block sees identical input in both runs: its output differs by the rounding of a few elements
    a, b = outs["0"]["input_blocks.3"], outs["1"]["input_blocks.3"]
    d = (a - b).abs()
    print(f"first attention block: max|d| {float(d.max()):.2e} of {float(a.abs().max()):.2e}, {100 * float((d > 0).float().mean()):.3f} % differ")
    assert float(d.max()) <= 2.0 ** -6 * float(a.abs().max()) and float((d > 0).float().mean()) < 0.05


def test_bf16_attention_lazy_pass_and_its_exact_fallback(gu, monkeypatch):
    """flash_attn_bf16v2_kernel: the reference-free LAZY pass (no running maximum; exact while a query's scores stay inside
    2^+-100) against the exact online-softmax loop on the same bf16 operands, (a) with ordinary weights - no workgroup leaves
    the range - and (b) with the qkv weights of every attention block scaled by 24, which puts the scores in the thousands:
    every workgroup's sums overflow, the LAZY kernel writes nothing but its redo flags and the exact kernel behind it redoes
    the call.  Both ways the block outputs agree with the exact-only run to the rounding of a few bf16 values - reference
    guided_diffusion/unet.py:436-455 (softmax over the keys, float32)."""
    import holo_diffusion_amd as hda
    from holo_diffusion_amd.weights import synth_state_dict
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_BF16_FLASH_MIN_T", "256")
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1,
                     channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(5, (2, 16, 16, 16, 16)))
    t = torch.tensor([640, 3], dtype=torch.int64)
    for scale in (1.0, 24.0):
        sd = synth_state_dict(uo.unet_param_shapes(cfg), 41)
        for k in sd:
            if k.endswith("qkv.weight"):
                sd[k] = sd[k] * scale
        trace = {}
        uo.unet_forward(sd, cfg, x, t, trace)
        tags = [tag for tag in trace if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block"]
        outs = {}
        for exact in ("1", ""):
            if exact:
                monkeypatch.setenv("HOLO_ATTN_EXACT", exact)
            else:
                monkeypatch.delenv("HOLO_ATTN_EXACT")
            net = hda.SimpleUnet3D(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1,
                                   channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2, compute_dtype="bf16")
            net.load_state_dict({"_net." + k: v for k, v in sd.items()})
            net = net.to(gu.DEV)
            with torch.no_grad():
                y = net(x.to(gu.DEV), t.to(gu.DEV))
            assert torch.isfinite(y).all()
            outs[exact] = {tag: net.fetch_block(tag, tuple(trace[tag].shape)).float().cpu() for tag in tags}
        a, b = outs["1"]["input_blocks.3"], outs[""]["input_blocks.3"]  # the first attention block: identical input in both runs
        d = (a - b).abs()
        print(f"qkv weights x {scale:g}: first attention block, LAZY (+ fallback) vs exact: max|d| {float(d.max()):.2e} of "
              f"{float(a.abs().max()):.2e}, {100 * float((d > 0).float().mean()):.3f} % of the elements differ")
        # (P = 2^S and P = 2^(S - m) round to bf16 differently: one ulp on a tenth of the block's bf16 outputs, never more)
        assert float(d.max()) <= 2.0 ** -6 * float(a.abs().max()) and float((d > 0).float().mean()) < 0.3
        if scale == 1.0:  # (with ordinary weights the whole net also sits at the bf16 tolerance of the fp32 oracle)
            for tag in tags:
                assert gu.rel_err(outs[""][tag], trace[tag]) < 2e-2, tag


@pytest.mark.parametrize("mc", [64, 128])
def test_bf16_streaming_1x1_convolution(gu, mc, monkeypatch):
    """bf16 storage mode: the attention's proj_out (+ bias, + residual x, GroupNorm slabs of the block output) on
    conv1x1_bf16_stream_kernel (weights of the workgroup in LDS, rows straight from global memory in MFMA-operand layout, 64 and
    128 input channels, two samples) against the row-tile kernel on the same net and against the fp32 oracle block by block -
    reference guided_diffusion/unet.py:306 (x + proj_out(h))."""
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=1,
                     channel_mult=(1, 2), attention_resolutions=(1,), num_heads=2)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(9, (2, 16, 16, 16, 16)))
    t = torch.tensor([77, 940], dtype=torch.int64)
    trace, outs = {}, {}
    for knob in ("0", "1"):
        monkeypatch.setenv("HOLO_CONV1X1_BF16_STREAM", knob)
        net, sd = gu.make_unet(cfg, seed=23, compute_dtype="bf16")
        if not trace:
            ref = uo.unet_forward(sd, cfg, x, t, trace)
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        assert 1e-5 < gu.rel_err(y, ref) < 2e-2
        tags = [tag for tag in trace if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block"]
        outs[knob] = {tag: net.fetch_block(tag, tuple(trace[tag].shape)).float().cpu() for tag in tags}
        for tag in tags:
            assert gu.rel_err(outs[knob][tag], trace[tag]) < 2e-2, (knob, tag)
        kernels = [o.get("kernel") for o in net.time_ops(2, 1, gu.DEV) if o["op"] == "conv" and o["ksz"] == 1 and o["cout"] == mc and o["out_dim"] == 16]
        assert len(kernels) == 3 and all((k == "conv1x1_bf16_stream_kernel") == (knob == "1") for k in kernels), kernels  # (one input, two output blocks)
    a, b = outs["0"]["input_blocks.1"], outs["1"]["input_blocks.1"]  # the first attention block: identical input in both runs
    d = (a - b).abs()
    print(f"first attention block: max|d| {float(d.max()):.2e} of {float(a.abs().max()):.2e}, {100 * float((d > 0).float().mean()):.3f} % differ")
    assert float(d.max()) <= 2.0 ** -6 * float(a.abs().max()) and float((d > 0).float().mean()) < 0.05


def test_bf16_stride2_halo_kernel_blockwise(gu, monkeypatch):
    """The Downsample convolutions of the bf16 storage mode on conv_s2_bf16_kernel (2 x 8 x 8 output tiles, the 5 x 17 x 17
    input region de-interleaved along x in LDS, per-tile GroupNorm slabs), forced onto a 32^3 net (32^3 -> 16^3 with 64
    channels, 16^3 -> 8^3 with 128: two output-channel blocks, tiles on every face of the grid, batch 2): every block output
    against the fp32 oracle at the bf16 tolerance, and the two Downsample outputs against the row-tile kernel's (the first: same bf16
    operands, fp32 accumulation in another order - at most one bf16 ulp apart, and only rarely) - reference
    guided_diffusion/unet.py:109-138."""
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = uo.UNetCfg(image_size=32, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 2, 2), attention_resolutions=(), num_heads=2)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(5, (2, 16, 32, 32, 32)))
    t = torch.tensor([640, 3], dtype=torch.int64)
    trace = {}
    outs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("HOLO_CONV_S2T", knob)
        net, sd = gu.make_unet(cfg, seed=41, compute_dtype="bf16")
        if not trace:
            ref = uo.unet_forward(sd, cfg, x, t, trace)
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        assert 1e-5 < gu.rel_err(y, ref) < 2e-2
        for tag, r in trace.items():
            if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block":
                assert gu.rel_err(net.fetch_block(tag, tuple(r.shape)), r) < 2e-2, (knob, tag)
        outs[knob] = {tag: net.fetch_block(tag, tuple(trace[tag].shape)).float().cpu() for tag in ("input_blocks.3", "input_blocks.6")}
        kernels = [o.get("kernel") for o in net.time_ops(2, 1, gu.DEV) if o["op"] == "conv" and o["stride"] == 2]
        assert len(kernels) == 2 and all((k == "conv_s2_bf16_kernel") == (knob == "1") for k in kernels), kernels
    for tag in outs["0"]:
        a, b = outs["0"][tag], outs["1"][tag]
        d = (a - b).abs()
        print(f"{tag}: max|d| {float(d.max()):.2e} of {float(a.abs().max()):.2e}, {100 * float((d > 0).float().mean()):.3f} % of the elements differ")
        assert float(d.max()) <= 2.0 ** -7 * float(a.abs().max()), tag           # one bf16 ulp of the largest value
        if tag == "input_blocks.3":  # (the first Downsample sees identical input in both runs; the second one's input already differs)
            assert float((d > 0).float().mean()) < 0.02, tag                     # ... on a few elements that sat on a rounding edge
        else:
            assert float(d.mean()) < 2e-3 * float(a.abs().mean()), tag


@pytest.mark.parametrize("image,mc,mult,attn,batch", [(8, 64, (1, 2), (2,), 1), (16, 64, (1, 2, 2), (4,), 2)])
def test_f32_bf16x3_mode_meets_the_fp32_tolerance(gu, image, mc, mult, attn, batch):
    """fp32 operands split exactly into three bf16 terms, six bf16 MFMAs per product: every block output against the
    pinned oracle at the SAME per-op tolerance as the exact-fp32 path (rtol 1e-4 of the tensor scale)."""
    import os
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=2,
                     channel_mult=mult, attention_resolutions=attn, num_heads=2)
    os.environ["HOLO_KEEP_INTERMEDIATES"] = "1"
    try:
        net, sd = gu.make_unet(cfg, seed=99, compute_dtype="f32_bf16x3")
        from oracle.common import np_noise
        x = torch.from_numpy(np_noise(11, (batch, 16, image, image, image)))
        t = torch.tensor([321, 17][:batch], dtype=torch.int64)
        trace = {}
        ref = uo.unet_forward(sd, cfg, x, t, trace)
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        assert gu.rel_err(y, ref) < 1e-4
        gu.block_outputs_vs_oracle(net, trace, 1e-4)
    finally:
        del os.environ["HOLO_KEEP_INTERMEDIATES"]


@pytest.mark.parametrize("compute,env", [("f32", {}), ("bf16", {}), ("bf16", {"HOLO_BF16_FLASH_MIN_T": "0"}), ("f32_bf16x3", {})])
@pytest.mark.parametrize("image,mc,mult,attn", [(16, 128, (1, 2), (2,)), (16, 64, (1, 2, 2), (1, 2))])
def test_forward_does_not_depend_on_workspace_contents(gu, compute, env, image, mc, mult, attn, monkeypatch):
    """The caller-owned workspace may hold anything (the caching allocator hands back blocks of earlier work): a forward on
    a workspace filled with 0xFF bytes (NaN as fp32 and as bf16) must give bit-identical, finite output to one on a zeroed
    workspace, in every arithmetic mode and with the bf16 attention kernel forced on."""
    from holo_diffusion_amd import runtime
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=2,
                     channel_mult=mult, attention_resolutions=attn, num_heads=2)
    net, sd = gu.make_unet(cfg, seed=7, compute_dtype=compute)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(13, (2, 16, image, image, image))).to(gu.DEV)
    t = torch.tensor([77, 901], dtype=torch.int64, device=gu.DEV)
    outs = []
    for fill in (0, 0xFF, 0x7F):
        ws = runtime.workspace(net, gu.DEV, net.workspace_bytes(2, gu.DEV))
        ws.fill_(fill)
        with torch.no_grad():
            outs.append(net(x, t).clone())
    assert torch.isfinite(outs[1]).all() and torch.isfinite(outs[2]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = uo.unet_forward(sd, cfg, x.cpu(), t.cpu())
    assert gu.rel_err(outs[1], ref) < (2e-2 if compute == "bf16" else 2e-3)


def test_simple_unet3d_reference_test_configuration(gu):
    """`SimpleUnet3D()` with the reference's DEFAULTS (128 -> 128 channels, model_channels 128, channel_mult (1,2,4,8),
    attention_resolutions (8,16), image_size 64) on the input of its own test (holo_diffusion/tests/test_diffusion_utils.py:
    16-30): a (1, 128, 32, 32, 32) grid - NOT image_size^3: UNetModel is fully convolutional - and a random timestep.
    Shape and no-NaN (the reference's checks) plus the full forward against the pinned oracle (2e-3 of the output scale,
    SURVEY.md 8c).  Channel counts up to 1024 and attention with 512 head channels at 4^3 are outside the released YAMLs."""
    import os
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("a 128..1024-channel net is not an emulation size")
    net = hda.SimpleUnet3D()
    assert (net.image_size, net.in_channels, net.model_channels, net.channel_mult, net.attention_resolutions) == \
        (64, 128, 128, (1, 2, 4, 8), (8, 16))
    cfg = uo.UNetCfg(image_size=32, in_channels=128, out_channels=128, model_channels=128, num_res_blocks=2,
                     channel_mult=(1, 2, 4, 8), attention_resolutions=(8, 16), num_heads=2)
    sd = gu.synth_state_dict(uo.unet_param_shapes(cfg), 77)
    net.load_state_dict({"_net." + k: v for k, v in sd.items()})
    net.to(gu.DEV)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(21, (1, 128, 32, 32, 32)))
    t = torch.tensor([437], dtype=torch.int64)
    with torch.no_grad():
        y = net(x=x.to(gu.DEV), timesteps=t.to(gu.DEV))
    assert y.shape == (1, 128, 32, 32, 32) and not torch.isnan(y).any()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = uo.unet_forward(sd, cfg, x, t)
    assert (y.cpu() - ref).abs().max() <= 2e-3 * ref.abs().max()
    # the same object still serves grids of its configured size (the plan follows the input)
    small = hda.SimpleUnet3D(image_size=8, in_channels=16, out_channels=16, model_channels=32, channel_mult=(1, 2),
                             attention_resolutions=(2,)).to(gu.DEV)
    with torch.no_grad():
        a = small(torch.zeros(1, 16, 8, 8, 8, device=gu.DEV), torch.zeros(1, dtype=torch.long, device=gu.DEV))
        b = small(torch.zeros(1, 16, 16, 16, 16, device=gu.DEV), torch.zeros(1, dtype=torch.long, device=gu.DEV))
        a2 = small(torch.zeros(1, 16, 8, 8, 8, device=gu.DEV), torch.zeros(1, dtype=torch.long, device=gu.DEV))
    assert a.shape[-1] == 8 and b.shape[-1] == 16 and torch.equal(a, a2)


@pytest.mark.parametrize("compute,image,batch", [("bf16", 32, 1), ("bf16", 32, 2), ("f32", 16, 2)])
def test_repeated_forwards_are_bit_identical(gu, compute, image, batch):
    """Run-to-run repeatability with the default (buffer re-using) workspace plan.  Round 4 found the planner handing the
    first bytes of a split-K scratch it had just released to the GroupNorm statistics buffer of the SAME launch: the reduce
    kernel then wrote statistics over partial sums other workgroups had not read yet - sample 0 of the bf16 net at 32^3
    came out wrong in ~25 % of the runs (and this, not a stale cache line, is what round 3's "wrong timestep" runs were).
    40 forwards on fresh pageable host->device copies of the input and the timesteps: all bit-equal, and right."""
    cfg = uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=128, num_res_blocks=2, channel_mult=(1, 2),
                     attention_resolutions=(2,), num_heads=2)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(13, (batch, 16, image, image, image)))
    t = torch.tensor([77, 901][:batch], dtype=torch.int64)
    net, sd = gu.make_unet(cfg, seed=7, compute_dtype=compute)
    ref = uo.unet_forward(sd, cfg, x, t)
    first = None
    for i in range(4 if gu.EMU else 40):
        junk = torch.full((1 + (i * 7919) % 3_000_000,), float("nan"), device=gu.DEV)  # vary what the allocator hands out
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        if first is None:
            first = y.clone()
            assert gu.rel_err(y, ref) < (2e-2 if compute == "bf16" else TOL)
        assert torch.equal(y, first), (compute, image, batch, i, float((y - first).abs().max()))
        del junk


def _res_block_f64(sd, p, x, emb, slabs):
    """ResBlock (unet.py:236-256, scale-shift norm) in float64 end to end - F.group_norm on doubles, not the reference's
    fp32 GroupNorm32 - evaluated on the output planes of every (z0, z1) in ``slabs``: the second float64 convolution runs on
    a slab's planes + one halo plane each side (the GroupNorm statistics need h on the whole grid, so the first
    convolution is the full one, computed once)."""
    import torch.nn.functional as F
    d = {k: v.double() for k, v in sd.items() if k.startswith(p + ".")}
    D = x.shape[2]
    h = F.silu(F.group_norm(x, 32, d[p + ".in_layers.0.weight"], d[p + ".in_layers.0.bias"], eps=1e-5))
    h = F.conv3d(h, d[p + ".in_layers.2.weight"], d[p + ".in_layers.2.bias"], padding=1)
    e = F.linear(F.silu(emb), d[p + ".emb_layers.1.weight"], d[p + ".emb_layers.1.bias"])[..., None, None, None]
    scale, shift = torch.chunk(e, 2, dim=1)
    h = F.silu(F.group_norm(h, 32, d[p + ".out_layers.0.weight"], d[p + ".out_layers.0.bias"], eps=1e-5) * (1 + scale) + shift)
    outs = []
    for z0, z1 in slabs:
        lo, hi = max(z0 - 1, 0), min(z1 + 1, D)
        pad = (1, 1, 1, 1, 1 if lo == z0 else 0, 1 if hi == z1 else 0)  # zero padding only at the true grid faces
        y = F.conv3d(F.pad(h[:, :, lo:hi], pad), d[p + ".out_layers.3.weight"], d[p + ".out_layers.3.bias"])
        xs = x[:, :, z0:z1]
        if (p + ".skip_connection.weight") in d:
            xs = F.conv3d(xs, d[p + ".skip_connection.weight"], d[p + ".skip_connection.bias"])
        outs.append(xs + y)
    return outs


@pytest.mark.parametrize("image,cin,mc,mult,slab", [
    (64, 32, 64, (1, 1, 1), 4),   # the 64^3 level of the north-star net: 64 -> 64 and (64 + 64) -> 64 with fused skip
    (16, 16, 256, (1, 2), 8),     # long K: (512 + 256) -> 256 at 16^3 and (512 + 512) -> 512 at 8^3 (split-K): K = 27 x 1024
])
def test_three_axis_winograd_vs_float64(gu, image, cin, mc, mult, slab, monkeypatch):
    """The accuracy claim of DESIGN.md for the F(2x2x2, 3x3x3) form, as a test: every single-ResBlock block of a net whose
    stride-1 convolutions run on conv_wino3_kernel is compared with the SAME block evaluated in float64 on the kernel's own
    block input (so nothing compounds and the figure is the block's own rounding), once for the default plan and once for
    the direct (27-tap) kernels; the Winograd form may be at most 2x the direct form's error (+ 1e-7 of the block's scale)
    and both stay below 2e-5 (observed 1e-6 ... 5e-6)."""
    if gu.EMU:
        image, cin, mc, mult, slab = 16, 16, 64, (1, 2), 4
    cfg = uo.UNetCfg(image_size=image, in_channels=cin, out_channels=cin, model_channels=mc, num_res_blocks=1,
                     channel_mult=mult, attention_resolutions=(), num_heads=2)
    inputs, middle, outputs, _ = uo.unet_structure(cfg)
    from oracle.common import np_noise
    x = torch.from_numpy(np_noise(23, (1, cin, image, image, image)))
    t = torch.tensor([407], dtype=torch.int64)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")

    def block_errors(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        net, sd = gu.make_unet(cfg, seed=31)
        with torch.no_grad():
            net(x.to(gu.DEV), t.to(gu.DEV))
        emb = uo.time_embed(sd, cfg, t).double()
        # block output shapes without running the oracle at the large size: channels from the structure, size from the level
        fetched, errs, size, hs = {}, {}, image, []
        def fetch(tag, ch, sz):
            if tag not in fetched:
                fetched[tag] = net.fetch_block(tag, (1, ch, sz, sz, sz)).cpu()
            return fetched[tag]
        prev = None
        for i, layers in enumerate(inputs):
            tag = f"input_blocks.{i}"
            if any(b.kind == "down" for b in layers):
                size //= 2
            out = fetch(tag, layers[-1].cout, size)
            if len(layers) == 1 and layers[0].kind == "res":
                errs[tag] = (layers[0].prefix, prev, out)
            hs.append((out, size))
            prev = out
        prev = fetch("middle_block", middle[-1].cout, size)
        for i, layers in enumerate(outputs):
            tag = f"output_blocks.{i}"
            skip, ssize = hs.pop()
            assert ssize == size
            xin = torch.cat([prev, skip], dim=1)
            osize = size * 2 if any(b.kind == "up" for b in layers) else size
            out = fetch(tag, layers[-1].cout, osize)
            if len(layers) == 1 and layers[0].kind == "res":
                errs[tag] = (layers[0].prefix, xin, out)
            size, prev = osize, out
        res = {}
        for tag, (p, xin, out) in errs.items():
            D = xin.shape[2]
            worst, scale = 0.0, 0.0
            slabs = ((0, slab), (D // 2 - 1, D // 2 - 1 + slab), (D - slab, D)) if D > 2 * slab else ((0, D),)
            for zs, ref in zip(slabs, _res_block_f64(sd, p, xin.double(), emb, slabs)):
                worst = max(worst, float((out[:, :, zs[0]:zs[1]].double() - ref).abs().max()))
                scale = max(scale, float(ref.abs().max()))
            res[tag] = worst / scale
        kinds = {o["kernel"] for o in net.time_ops(1, 1, gu.DEV) if o["op"] == "conv"} if not gu.EMU else set()
        return res, kinds

    e_w3, k_w3 = block_errors({"HOLO_CONV_WINO3_MIN_ITEMS": "1"})
    e_dir, k_dir = block_errors({"HOLO_CONV_WINO3": "0", "HOLO_CONV_WINO": "0", "HOLO_CONV_WINO_SMALL": "0"})
    if not gu.EMU:
        assert "conv_wino3_kernel" in k_w3 and not any(k.startswith("conv_wino") for k in k_dir), (k_w3, k_dir)
    assert e_w3 and set(e_w3) == set(e_dir)
    for tag in e_w3:
        print(f"  {tag}: three-axis Winograd {e_w3[tag]:.2e}, direct {e_dir[tag]:.2e} (relative to the block's scale, vs float64)")
        assert e_w3[tag] < 2e-5 and e_dir[tag] < 2e-5, tag
        assert e_w3[tag] <= 2.0 * e_dir[tag] + 1e-7, tag
