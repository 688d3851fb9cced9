"""GPU parity of the denoiser on cubic grids whose edge is NOT a power of two (12, 20, 24, 40, 48, 96): every level of such
a net has a tile count per axis of 3, 5, 6 or 12, a voxel count that is no multiple of 128 (12^3 = 1728 = 13.5 row tiles),
or an odd edge (3^3 = 27, 5^3 = 125 voxels / attention tokens) - none of which the power-of-two sizes of the other files
reach.  Reference: the pinned CPU oracle (oracle/unet_oracle.py), for gradients torch autograd through it.  Tolerances are
the project's existing ones (as in test_gpu_unet.py / test_gpu_backward.py): fp32 and f32_bf16x3 block by
block rel_err < 1e-4; a full fp32 forward max|d| <= 2e-3 max|ref|; bf16 mode 1e-5 < err < 2e-2; two kernels on the same
bf16 operands at most one bf16 ulp of the largest value apart (2^-7); gradients 1e-3 of the tensor's scale."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.test_gpu_backward import _check, _oracle_grads  # noqa: E402

TILED = {"conv_halo_kernel", "conv_wino2_kernel", "conv_wino3_kernel", "conv_bf16t_kernel", "conv_bf16p_kernel"}
TIMESTEPS = [321, 17, 803]


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _cfg(image, mc, mult, attn, nrb=2):
    return uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=nrb,
                      channel_mult=mult, attention_resolutions=attn, num_heads=2)


def _heavy(gu, why="not an emulation size"):
    if gu.EMU:
        pytest.skip(why)


_ORACLE = {}  # the last oracle run: the compute modes of one net follow each other and share it


def _oracle(sd_seed, cfg, x_seed, batch, sd):
    key = (sd_seed, repr(cfg), x_seed, batch)
    if key not in _ORACLE:
        _ORACLE.clear()
        torch.set_num_threads(min(32, torch.get_num_threads()))
        R = cfg.image_size
        x = torch.from_numpy(np_noise(x_seed, (batch, cfg.in_channels, R, R, R)))
        t = torch.tensor(TIMESTEPS[:batch], dtype=torch.int64)
        trace = {}
        ref = uo.unet_forward(sd, cfg, x, t, trace)
        tags = [k for k in trace if k.startswith(("input_blocks", "output_blocks")) or k == "middle_block"]
        _ORACLE[key] = (x, t, ref, {k: trace[k] for k in tags})
    return _ORACLE[key]


def _forward_blockwise(gu, cfg, batch, compute, sd_seed, x_seed, label):
    """One forward with HOLO_KEEP_INTERMEDIATES=1 (the caller sets it): `y` and every block output against the oracle at the
    bound of the compute mode; returns the net and its block outputs."""
    net, sd = gu.make_unet(cfg, seed=sd_seed, compute_dtype=compute)
    x, t, ref, trace = _oracle(sd_seed, cfg, x_seed, batch, sd)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    outs = {tag: net.fetch_block(tag, tuple(r.shape)).float().cpu() for tag, r in trace.items()}
    errs = {tag: gu.rel_err(outs[tag], trace[tag]) for tag in trace}
    ey = gu.rel_err(y, ref)
    worst = max(errs, key=errs.get)
    print(f"{label} {compute}: y {ey:.2e}, worst block {errs[worst]:.2e} ({worst})")
    assert torch.isfinite(y).all()
    if compute == "bf16":
        assert 1e-5 < ey < 2e-2, ey
        for tag in trace:
            assert errs[tag] < 2e-2, (tag, errs[tag])
    else:
        assert ey < 1e-4, ey
        for tag in trace:
            assert errs[tag] < 1e-4, (tag, errs[tag])
    return net, y, outs


def _conv_ops(gu, net, batch):
    # (time_ops runs its own forward on random data: only after the block outputs of OUR forward have been read)
    return [o for o in net.time_ops(batch, 1, gu.DEV) if o["op"] == "conv"]


def _op_names(gu, net, batch):
    return [o["op"] for o in net.time_ops(batch, 1, gu.DEV)]


# ---- 1. forward, block by block ------------------------------------------------------------------------------------------
# (image, model_channels, channel_mult, attention_resolutions, batch, emulation size).  The middle block always holds an
# attention block, so every net also runs attention at its deepest level.  Behind each row: the convolution kernels and
# attention launches `time_ops` reported on the MI355X (256 CUs, the planner's own choices) and the worst error seen.
ROWS = {
    # no level is tileable: gather / row-tile kernels with partial row tiles (1728, 216 rows); T = 216 on GEMM + softmax.
    # f32: conv_igemm_kernel, conv_small_kernel; 12 gemm launches, no flash_attn; y 1.2e-6, worst block 1.3e-6
    "12-6": (12, 32, (1, 2), (2,), 1, True),
    # T = 1728 and 216 on GEMM + softmax, the 64-channel row-tile kernel with split-K, batch 2.
    # f32: conv_igemm_kernel, conv_small_kernel, conv1x1_small_kernel (1728 % 16 == 0); 22 gemm; y 1.8e-6, block 1.7e-6
    "12-6-wide": (12, 64, (1, 2), (1, 2), 2, False),
    # an odd level: stride 2 from 6 to 3, upsample 3 to 6, GroupNorm over 27 voxels, T = 27 (gemm_scalar_kernel), odd batch.
    # all three modes: conv_igemm_kernel, conv_small_kernel; 22 gemm; f32 and f32_bf16x3 y 1.3e-6, block 1.6e-6; bf16 y 9.0e-3,
    # block 1.2e-2
    "12-6-3": (12, 32, (1, 1, 2), (2, 4), 3, True),
    # 8000 rows (62.5 row tiles), T = 125 (gemm_scalar_kernel).
    # f32: conv_igemm_kernel, conv_small_kernel; 12 gemm; y 1.3e-6, block 1.2e-6
    "20-10-5": (20, 32, (1, 1, 2), (4,), 1, False),
    # 3 tiles per axis on the tiled kernels, fused skip, virtual concat, upsample-on-load 12 -> 24; middle attention T = 1728.
    # f32: conv_wino3_kernel + conv_halo_kernel at 24^3, conv_small_kernel, conv1x1_small_kernel below; 2 gemm; y 2.1e-6
    # f32_bf16x3: conv_halo_kernel at 24^3, conv_small_kernel below; y 2.3e-6, block 1.8e-6
    "24-12": (24, 64, (1, 2), (), 1, False),
    # T = 13824 = 108 x 128 on the split-key flash attention, T = 216 next to it.
    # f32: conv_wino3_kernel + conv_halo_kernel at 24^3, conv_small_kernel; 5 flash_attn, 12 gemm; y 1.8e-6, block 1.8e-6
    # bf16: conv_bf16t_kernel + conv_halo_kernel at 24^3, conv1x1_qkv_bf16_kernel, conv1x1_bf16_stream_kernel,
    #       conv_small_kernel; 5 flash_attn (the bf16 kernel), 12 gemm; y 1.3e-2, block 1.3e-2
    # f32_bf16x3: conv_halo_kernel, conv_small_kernel; 5 flash_attn, 12 gemm; y 2.0e-6, block 1.9e-6
    "24-12-6": (24, 64, (1, 2, 2), (1, 4), 1, False),
    # 5 tiles per axis; 20^3 is even but not tileable; the middle block's attention at T = 8000 on GEMM + softmax.
    # f32: conv_wino3_kernel + conv_halo_kernel at 40^3, conv_small_kernel at 20^3; 2 gemm; y 1.9e-6, block 1.8e-6
    "40-20": (40, 64, (1, 2), (), 1, False),
    # 6 / 3 tiles per axis: the planner's own conv_wino3_kernel on work lists that are no power of two.
    # f32: conv_wino3_kernel + conv_halo_kernel at 48^3, conv_small_kernel, conv1x1_small_kernel; 12 gemm; y 2.1e-6
    # bf16: conv_bf16t_kernel + conv_halo_kernel at 48^3, conv_s2_bf16_kernel (48 -> 24), conv_small_kernel; y 1.1e-2, block 1.2e-2
    "48-24-12": (48, 64, (1, 1, 2), (4,), 1, False),
}
CASES = [(r, "f32") for r in ROWS] + [(r, "bf16") for r in ("12-6-3", "24-12-6", "48-24-12")] + \
        [(r, "f32_bf16x3") for r in ("12-6-3", "24-12", "24-12-6")]
CASES.sort(key=lambda c: list(ROWS).index(c[0]))  # (the modes of a row follow each other: one oracle run per row)


@pytest.mark.parametrize("row,compute", CASES)
def test_grid_sizes_vs_oracle_blockwise(gu, row, compute, monkeypatch):
    """Every block output and `y` of the nets of ROWS against the pinned oracle, then - on the device - that the row
    reached the kernels it is there for (the planner's own choices, no knob)."""
    image, mc, mult, attn, batch, emu_size = ROWS[row]
    if not emu_size:
        _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = _cfg(image, mc, mult, attn)
    net, _, _ = _forward_blockwise(gu, cfg, batch, compute, 99, 11, row)
    if gu.EMU:
        return
    ops = net.time_ops(batch, 1, gu.DEV)
    convs = [o for o in ops if o["op"] == "conv"]
    names = [o["op"] for o in ops]
    top = {o["kernel"] for o in convs if o["out_dim"] == image and o["ksz"] == 3}
    kernels = {o["kernel"] for o in convs}
    print(f"{row} {compute}: kernels {sorted(kernels)}; top level {sorted(top)}; "
          f"{names.count('gemm')} gemm, {names.count('flash_attn')} flash_attn launches")
    if image in (12, 20):
        assert not (kernels & TILED), kernels
        assert names.count("flash_attn") == 0 and names.count("gemm") >= 2
    else:
        assert top & TILED, top
    if row == "24-12-6":  # 2 + 3 attention blocks at 24^3 (flash), 2 + 3 at 6^3 and the middle block (two GEMMs each)
        assert names.count("flash_attn") == 5 and names.count("gemm") == 2 * 6, names
    if row == "48-24-12" and compute == "f32":
        assert "conv_wino3_kernel" in top, top
    if compute == "bf16" and image >= 24:  # the wide-tile kernel by the planner's own choice
        assert "conv_bf16t_kernel" in top, top
    if row == "48-24-12" and compute == "bf16":  # ... and the stride-2 halo kernel on 48 -> 24, not on 24 -> 12
        assert {o["out_dim"] for o in convs if o["kernel"] == "conv_s2_bf16_kernel"} == {24}
    if row == "12-6-wide":  # 1728 rows are a multiple of 16: the small 1x1x1 kernel serves the 12^3 attention blocks
        assert "conv1x1_small_kernel" in kernels, kernels
    if row in ("12-6-3", "20-10-5"):  # the odd level ran its stride-2 convolution, its upsampling one and its attention
        deep = image // 4
        assert any(o["stride"] == 2 and o["out_dim"] == deep for o in convs)
        assert any(o["upsample"] and o["out_dim"] == 2 * deep for o in convs)
        assert any(o["op"] == "gemm" and o["out_dim"] == deep ** 3 for o in ops)


# ---- 2. the forced kernels at three (six) tiles per axis -----------------------------------------------------------------
@pytest.mark.parametrize("wino_kernel", ["conv_wino3_kernel", "conv_wino2_kernel"])
def test_winograd_kernels_at_three_tiles_per_axis(gu, wino_kernel, monkeypatch):
    """test_winograd_kernels_blockwise at 24^3 / 12^3 (3 x 3 tiles of 8 x 8 per plane; 12^3 is not tileable, so forced and
    fallback kernels feed each other): block by block against the oracle, and the direct kernels agree to 1e-5."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_CONV_FORCE_TZ2", "1")
    monkeypatch.setenv("HOLO_CONV_WINO", "2")
    if wino_kernel == "conv_wino3_kernel":
        monkeypatch.setenv("HOLO_CONV_WINO3_MIN_ITEMS", "1")
    else:
        monkeypatch.setenv("HOLO_CONV_WINO3", "0")
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = _cfg(24, 64, (1, 2), ())
    net, y, _ = _forward_blockwise(gu, cfg, 1, "f32", 77, 19, wino_kernel)
    convs = _conv_ops(gu, net, 1)
    # the two convolutions of the five ResBlocks of the 24^3 level (the input convolution's 16 input and the head's 16
    # output channels keep those two on the direct kernel)
    top = [o["kernel"] for o in convs
           if o["out_dim"] == 24 and o["ksz"] == 3 and o["cin"] >= 64 and o["cout"] >= 64 and not o["upsample"]]
    print(f"{wino_kernel}: {len(top)} launches at 24^3: {sorted(set(top))}")
    assert len(top) == 10 and set(top) == {wino_kernel}, top
    monkeypatch.setenv("HOLO_CONV_FORCE_TZ2", "0")
    monkeypatch.setenv("HOLO_CONV_WINO", "0")
    monkeypatch.setenv("HOLO_CONV_WINO3", "0")
    net2, _ = gu.make_unet(cfg, seed=77)
    x, t, _, _ = _oracle(77, cfg, 19, 1, None)
    with torch.no_grad():
        y2 = net2(x.to(gu.DEV), t.to(gu.DEV))
    assert not any(o["kernel"].startswith("conv_wino") for o in _conv_ops(gu, net2, 1))
    assert gu.rel_err(y2, y.cpu()) < 1e-5


def _first_difference(a, b):
    """The first block (execution order) whose output differs between two runs: every block before it is bit-equal, so
    it is the first one that saw identical input on different kernels."""
    for tag in a:
        if not torch.equal(a[tag], b[tag]):
            return tag
    return None


def _ab_one_ulp(a, b, label):
    tag = _first_difference(a, b)
    assert tag is not None, f"{label}: the two runs are bit-equal - the knob changed no kernel"
    d = (a[tag] - b[tag]).abs()
    print(f"{label}: first differing block {tag}: max|d| {float(d.max()):.2e} of {float(a[tag].abs().max()):.2e}, "
          f"{100 * float((d > 0).float().mean()):.3f} % of the elements differ")
    assert float(d.max()) <= 2.0 ** -7 * float(a[tag].abs().max()), tag  # one bf16 ulp of the largest value


@pytest.mark.parametrize("form", ["t", "p"])
def test_bf16_wide_tile_kernels_at_three_tiles_per_axis(gu, form, monkeypatch, capfd):
    """conv_bf16t_kernel ("t") and its persistent form conv_bf16p_kernel ("p", HOLO_CONV_BF16P_WGS=8) forced onto 24^3:
    27 tiles of 8^3 per sample.  The persistent form (HOLO_DEBUG_PLAN: every 24^3 launch `grid_x 8`) deals its 27 items
    (64 output channels) or 54 (the Upsample convolution's 128: two slices per tile) to the 8 workgroups as contiguous ranges
    of ceil(items / 8): 4, 4, 4, 4, 4, 4, 3 and NONE for the eighth workgroup; 7 x 7 and 5 (at 16^3 it was 16 items, two for
    every workgroup).  Block by block against the oracle at the bf16 bound, and - because 2e-2 of a tensor's maximum would let
    one wrong tap at one tile seam through - at most one bf16 ulp of the largest value away from the run on the 64/128-voxel
    halo kernels (HOLO_CONV_BF16T=0) on the first block that differs at all."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    cfg = _cfg(24, 64, (1, 2), ())
    monkeypatch.setenv("HOLO_CONV_BF16T", "0")
    monkeypatch.setenv("HOLO_CONV_BF16P", "0")
    net0, _, base = _forward_blockwise(gu, cfg, 1, "bf16", 99, 11, "bf16 halo kernels")
    assert not ({o["kernel"] for o in _conv_ops(gu, net0, 1)} & {"conv_bf16t_kernel", "conv_bf16p_kernel"})
    monkeypatch.setenv("HOLO_CONV_BF16T", "1")
    if form == "p":
        monkeypatch.setenv("HOLO_CONV_BF16P", "1")
        monkeypatch.setenv("HOLO_CONV_BF16P_WGS", "8")
    capfd.readouterr()
    net1, _, outs = _forward_blockwise(gu, cfg, 1, "bf16", 99, 11, "wide tile " + form)
    plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan] conv") and "@24^3" in ln]
    kernels = {o["kernel"] for o in _conv_ops(gu, net1, 1) if o["out_dim"] == 24 and o["ksz"] == 3}
    want = "conv_bf16p_kernel" if form == "p" else "conv_bf16t_kernel"
    assert want in kernels and ("conv_bf16t_kernel" in kernels) == (form == "t"), kernels
    if form == "p":  # every persistent launch of the 24^3 level: 8 workgroups for its 27 tiles
        lines = [ln for ln in plan if "conv_bf16p_kernel" in ln]
        print("\n".join(lines))
        assert lines and all(re.search(r"grid_x 8,", ln) for ln in lines), lines
    _ab_one_ulp(base, outs, "wide tile " + form)


def test_bf16_stride2_halo_kernel_at_48_and_its_fallback_at_24(gu, monkeypatch):
    """HOLO_CONV_S2T=1 on a 48 -> 24 -> 12 net: the first Downsample (24^3 output: 12 x 3 x 3 tiles of 2 x 8 x 8) runs on
    conv_s2_bf16_kernel, the second (12^3 output, 12 % 8 != 0) must fall back to the row-tile kernel; block by block against
    the oracle, and one bf16 ulp from the all-row-tile run (HOLO_CONV_S2T=0) on the first block that differs."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = _cfg(48, 64, (1, 2, 2), ())
    outs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("HOLO_CONV_S2T", knob)
        net, _, outs[knob] = _forward_blockwise(gu, cfg, 1, "bf16", 41, 5, "S2T=" + knob)
        s2 = {o["out_dim"]: o["kernel"] for o in _conv_ops(gu, net, 1) if o["stride"] == 2}
        assert set(s2) == {24, 12}, s2
        assert (s2[24] == "conv_s2_bf16_kernel") == (knob == "1"), s2
        assert s2[12] != "conv_s2_bf16_kernel", s2
    assert _first_difference(outs["0"], outs["1"]) == "input_blocks.3"  # (the first Downsample)
    _ab_one_ulp(outs["0"], outs["1"], "stride-2 halo kernel")


@pytest.mark.parametrize("split", ["5", "27"])
def test_split_key_flash_attention_at_13824_tokens(gu, split, monkeypatch, capfd):
    """On 256 CUs the planner leaves T = 13824 un-split (864 query tiles), so HOLO_FLASH_SPLIT deals the 432 key tiles of 32
    to 4 x 5 = 20 waves (21 or 22 tiles each: they do not divide) and to 4 x 27 = 108 waves (4 each) of the fp32 flash
    kernel + its merge kernel: every block against the oracle at the fp32 bound."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_FLASH_SPLIT", split)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    capfd.readouterr()
    _forward_blockwise(gu, _cfg(24, 64, (1, 2), (1,), nrb=1), 1, "f32", 7, 13, f"{split} key splits")
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan] attention")]
    # (one line per attention block and planning pass: one block down, two up)
    assert len({ln.split(":")[0] for ln in lines}) == 3, lines
    assert all(f"T=13824 C=64 heads=2 -> fp32 flash kernel, {split} key splits" in ln for ln in lines), lines


@pytest.mark.parametrize("attn,expect_bf16_flash", [((2,), False), ((1,), True)])
def test_bf16_flash_attention_at_24(gu, attn, expect_bf16_flash, monkeypatch, capfd):
    """HOLO_BF16_FLASH_MIN_T=0 at 24^3: with attention on the 12^3 level (T = 1728, no multiple of 256 nor of 128) no flash
    kernel may be chosen - GEMM + softmax - and the result is right; with attention on the 24^3 level (T = 13824 = 54 x
    256) the bf16 flash kernel is chosen and is right (the middle block, T = 1728, stays on the GEMM path)."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_BF16_FLASH_MIN_T", "0")
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    capfd.readouterr()
    net, _, _ = _forward_blockwise(gu, _cfg(24, 64, (1, 2), attn, nrb=1), 1, "bf16", 7, 13, f"attention {attn}")
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan] attention")]
    names = _op_names(gu, net, 1)
    if expect_bf16_flash:  # one attention block down, two up
        assert names.count("flash_attn") == 3 and names.count("gemm") == 2, names
        assert lines and all("T=13824" in ln and "bf16 flash kernel" in ln for ln in lines), lines
    else:  # one down, the middle block, two up
        assert names.count("flash_attn") == 0 and names.count("gemm") == 2 * 4, names
        assert not lines, lines


@pytest.mark.parametrize("knob_name,kernel", [("HOLO_CONV_QKV_FUSED", "conv1x1_qkv_bf16_kernel"),
                                              ("HOLO_CONV1X1_BF16_STREAM", "conv1x1_bf16_stream_kernel")])
def test_bf16_attention_1x1_kernels_at_24(gu, knob_name, kernel, monkeypatch):
    """The qkv convolution fused with the attention's operand packing, and proj_out on the streaming 1x1x1 kernel, at
    T = 13824 rows (108 row tiles of 128) against the row-tile kernel on the same net and against the oracle block by block -
    as test_bf16_qkv_convolution_fused_with_the_attention_packing / test_bf16_streaming_1x1_convolution do at 16^3."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    mc = 64
    cfg = _cfg(24, mc, (1, 2), (1,), nrb=1)
    cout = 3 * mc if "QKV" in knob_name else mc
    outs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv(knob_name, knob)
        net, _, outs[knob] = _forward_blockwise(gu, cfg, 1, "bf16", 23, 9, f"{knob_name}={knob}")
        kernels = [o["kernel"] for o in _conv_ops(gu, net, 1) if o["ksz"] == 1 and o["cout"] == cout and o["out_dim"] == 24]
        assert len(kernels) == 3 and all((k == kernel) == (knob == "1") for k in kernels), kernels
    a, b = outs["0"]["input_blocks.1"], outs["1"]["input_blocks.1"]  # the first attention block: identical input in both runs
    d = (a - b).abs()
    print(f"first attention block: max|d| {float(d.max()):.2e} of {float(a.abs().max()):.2e}, {100 * float((d > 0).float().mean()):.3f} % differ")
    assert float(d.max()) <= 2.0 ** -6 * float(a.abs().max()) and float((d > 0).float().mean()) < 0.05


# ---- 3. backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net_name,env", [("12-6-3", {}), ("12-6-3", {"HOLO_DGRAD_S2_DIRECT": "1"}),
                                          ("24-12", {}), ("24-12", {"HOLO_WGRAD_REDUCE_TILE_MIN": "1"}),
                                          ("24-12", {"HOLO_DGRAD_S2_DIRECT": "1"})])
def test_backward_at_odd_and_three_tile_levels(gu, net_name, env, monkeypatch):
    """`12-6-3` (batch 2): weight gradients with 27 and 216 voxels as their K dimension, the dgrad of the stride-2 convolutions
    from 3^3 to 6^3 and 6^3 to 12^3, GroupNorm backward over 27 voxels, attention backward at T = 27 (gemm_scalar_kernel) and
    216.  (The planner takes the zero-insertion dgrad only where the finer edge is a multiple of 8, so on this net the
    default IS conv_dgrad_s2_kernel and HOLO_DGRAD_S2_DIRECT=1 changes nothing; the two forms meet on the other net.)
    `24-12`: the LDS-halo dgrad kernels at 3 tiles per axis, the zero-insertion dgrad 12^3 -> 24^3 and the direct form in its
    place, attention backward at T = 1728, and the weight-gradient reduce's tile form.  Every parameter gradient and grad_x
    against autograd through the oracle (seen: grad_x 1.7e-6 / 2.5e-6, worst parameter 3.2e-4 / 1.4e-5 of its scale)."""
    if gu.EMU:
        pytest.skip("backward tests run on the device")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, batch = {"12-6-3": (_cfg(12, 32, (1, 1, 2), (2, 4), nrb=1), 2),
                  "24-12": (_cfg(24, 64, (1, 2), (2,), nrb=1), 1)}[net_name]
    net, sd = gu.make_unet(cfg, seed=5)
    shape = (batch, 16) + (cfg.image_size,) * 3
    x = torch.from_numpy(np_noise(1, shape))
    t = torch.tensor([437, 12][:batch], dtype=torch.int64)
    G = torch.from_numpy(np_noise(2, shape))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    y_ref, gx_ref, g_ref = _oracle_grads(sd, cfg, x, t, G)
    y, gx, grads = net.backward(x.to(gu.DEV), t.to(gu.DEV), G.to(gu.DEV))
    floor = 1e-2 * float(np.median([g_ref[k].abs().max().item() for k in sd]))
    worst = max(((grads[k].cpu() - g_ref[k]).abs().max().item() / max(g_ref[k].abs().max().item(), floor), k) for k in sd)
    print(f"backward {net_name} {env}: grad_x {gu.rel_err(gx, gx_ref):.2e}, worst relative gradient error {worst[0]:.2e} ({worst[1]})")
    _check(y, y_ref, "forward output", 2e-3)
    _check(gx, gx_ref, "grad_x")
    assert set(grads) == set(sd)
    for k in sd:
        _check(grads[k], g_ref[k], k, floor=floor)


# ---- 4. the other entry points ---------------------------------------------------------------------------------------------
def _small_or_tiled(image):
    """The 12^3 net is an emulation size (32 channels, attention away from the 12^3 level); the 24^3 one is not."""
    return _cfg(12, 32, (1, 2), (2,), nrb=1) if image == 12 else _cfg(24, 64, (1, 2), (2,), nrb=1)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("image", [12, 24])
def test_forward_channels_last_at_grid_sizes(gu, image, compute):
    """forward_channels_last on (2, R, R, R, C) is bit-equal to the NCDHW call at R = 12 and R = 24."""
    if image != 12:
        _heavy(gu)
    cfg = _small_or_tiled(image)
    net, _ = gu.make_unet(cfg, seed=3, compute_dtype=compute)
    x = torch.from_numpy(np_noise(21, (2, 16, image, image, image))).to(gu.DEV)
    t = torch.tensor([640, 3], device=gu.DEV)
    with torch.no_grad():
        y = net(x, t)
        x_cl = x.permute(0, 2, 3, 4, 1).contiguous()
        y_cl = net.forward_channels_last(x_cl, t)
        assert y_cl.shape == x_cl.shape and torch.equal(y_cl.permute(0, 4, 1, 2, 3), y)
        assert torch.equal(net(x, t), y) and torch.equal(net.forward_channels_last(x_cl, t), y_cl)


@pytest.mark.parametrize("image", [12, 24])
def test_batch_invariant_rows_at_grid_sizes(gu, image):
    """set_batch_invariant(True), batch 3, fp32: every row is bit-equal to the batch-1 forward of that row."""
    if image != 12:
        _heavy(gu)
    cfg = _small_or_tiled(image)
    net, sd = gu.make_unet(cfg, seed=3)
    xs = torch.from_numpy(np_noise(40, (3, 16, image, image, image)))
    ts = torch.tensor([999, 500, 3])
    ref = uo.unet_forward(sd, cfg, xs, ts)
    xs, ts = xs.to(gu.DEV), ts.to(gu.DEV)
    with torch.no_grad():
        y1_off = net(xs[:1], ts[:1])
        net.set_batch_invariant(True)
        assert torch.equal(net(xs[:1], ts[:1]), y1_off)
        yb = net(xs, ts)
        assert gu.rel_err(yb, ref) < 1e-4
        for b in range(3):
            assert torch.equal(yb[b:b + 1], net(xs[b:b + 1], ts[b:b + 1])), b


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_workspace_independence_at_24(gu, compute):
    """A forward at 24^3 on a workspace filled with 0x00 / 0xFF / 0x7F bytes: bit-identical and finite (a partial tile that
    reads past its slab shows up here as a NaN), and right."""
    _heavy(gu)
    from holo_diffusion_amd import runtime
    cfg = _cfg(24, 64, (1, 2, 2), (1, 2))
    net, sd = gu.make_unet(cfg, seed=7, compute_dtype=compute)
    x = torch.from_numpy(np_noise(13, (2, 16, 24, 24, 24))).to(gu.DEV)
    t = torch.tensor([77, 901], dtype=torch.int64, device=gu.DEV)
    outs = []
    for fill in (0, 0xFF, 0x7F):
        ws = runtime.workspace(net, gu.DEV, net.workspace_bytes(2, gu.DEV))
        ws.fill_(fill)
        with torch.no_grad():
            outs.append(net(x, t).clone())
    assert torch.isfinite(outs[1]).all() and torch.isfinite(outs[2]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = uo.unet_forward(sd, cfg, x.cpu(), t.cpu())
    assert gu.rel_err(outs[1], ref) < (2e-2 if compute == "bf16" else 2e-3)


def test_repeated_forwards_at_24_are_bit_identical(gu):
    """Ten forwards at 24^3, bf16, batch 2, on fresh copies of the input while the allocator's hand-outs vary: bit-equal (the
    buffer re-use planner at buffer sizes that are no power of two), and right."""
    _heavy(gu)
    cfg = _cfg(24, 128, (1, 2), (2,))
    x = torch.from_numpy(np_noise(13, (2, 16, 24, 24, 24)))
    t = torch.tensor([77, 901], dtype=torch.int64)
    net, sd = gu.make_unet(cfg, seed=7, compute_dtype="bf16")
    ref = uo.unet_forward(sd, cfg, x, t)
    first = None
    for i in range(10):
        junk = torch.full((1 + (i * 7919) % 3_000_000,), float("nan"), device=gu.DEV)
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        if first is None:
            first = y.clone()
            assert gu.rel_err(y, ref) < 2e-2
        assert torch.equal(y, first), (i, float((y - first).abs().max()))
        del junk


def test_96_cubed_forward_vs_oracle(gu):
    """96^3 x 32 (the size between the 64^3 north-star net and the 128^3 donut net; levels 96, 48, 24, 12; attention at
    T = 13824 and 1728): the full fp32 forward at
    2e-3 of the output scale, the bf16 mode at its 2e-2, both against the pinned oracle."""
    _heavy(gu)
    cfg = uo.UNetCfg(image_size=96, in_channels=32, out_channels=32, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 1, 2, 4), attention_resolutions=(4, 8), num_heads=2)
    net, sd = gu.make_unet(cfg, seed=1234)
    x = torch.from_numpy(np_noise(31, (1, 32, 96, 96, 96)))
    t = torch.tensor([500], dtype=torch.int64)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
        y2 = net(x.to(gu.DEV), t.to(gu.DEV))
    assert torch.equal(y, y2)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = uo.unet_forward(sd, cfg, x, t)
    assert torch.isfinite(y).all()
    print(f"96^3 f32: max|d| {float((y.cpu() - ref).abs().max()):.2e} of {float(ref.abs().max()):.2e}")
    assert (y.cpu() - ref).abs().max() <= 2e-3 * ref.abs().max()
    net.compute_dtype = "bf16"
    with torch.no_grad():
        ybf = net(x.to(gu.DEV), t.to(gu.DEV))
    err = gu.rel_err(ybf, ref)
    print(f"96^3 bf16: {err:.2e}")
    assert 1e-5 < err < 2e-2, err
