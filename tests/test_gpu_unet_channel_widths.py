"""GPU parity of the denoiser at channel widths OFF the power-of-two grid: model_channels 96, 160 and 224 (block widths 96,
160, 192, 224 - padded to 128, 192, 192, 256 output channels by the planner), in_channels != out_channels and neither a
multiple of 16 (4, 8, 12, 20, 36), head counts 3 and 7, head widths 48 and 96 (no flash kernel).  These are the numbers
conv_plan, the stride-2 / 1x1x1 bf16 kernels, the dgrad weight packing, gn_finalize_kernel (channels per group 3, 5, 6, 7,
9, 10; a group that straddles the two sources of a concat) and flash_attn_supported branch on; the other files keep every
block width a power of two and in_channels == out_channels.  Reference: the pinned CPU oracle (oracle/unet_oracle.py), for
gradients torch autograd through it.  Bounds are those of test_gpu_unet_grid_sizes.py: fp32 and f32_bf16x3 block by block
rel_err < 1e-4; bf16 mode 1e-5 < err(y) < 2e-2 and every block < 2e-2; two fp32 kernel families 1e-5 apart; two bf16 kernels
on the same operands at most one bf16 ulp of the largest value apart (2^-7); gradients 1e-3 of the tensor's scale."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.test_gpu_backward import _check, _oracle_grads  # noqa: E402
from tests.test_gpu_unet_grid_sizes import _ab_one_ulp, _forward_blockwise  # noqa: E402
from tests.test_gpu_wino3_item_boundary import DIRECT_ENV  # noqa: E402

WINO = {"conv_wino2_kernel", "conv_wino3_kernel"}
BF16_WIDE = {"conv_bf16t_kernel", "conv_bf16p_kernel"}


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _heavy(gu, why="not an emulation size"):
    if gu.EMU:
        pytest.skip(why)


# ---- 1. forward, block by block ------------------------------------------------------------------------------------------
# (image, in_channels, out_channels, model_channels, channel_mult, attention_resolutions, num_heads, batch).  Two ResBlocks
# per level; the middle block always holds an attention block.  Behind each row: the convolution kernels and attention
# launches `time_ops` reported on the MI355X (256 CUs, the planner's own choices) and the worst error seen.
ROWS = {
    # Cout 96 (padded to 128) at 16^3 and 192 at 8^3; concats 192+192, 192+96 (9 channels per group: a group across the two
    # sources) and 96+96; fused 1x1x1 skip 288 -> 96; three heads of 64 channels on the flash kernels; first convolution with
    # 12 input channels (% 16 fails), last one with 20 output channels (padded to 32).
    # every mode: 12 -> 96 and the stride-2 96 -> 96 on conv_small_kernel; 6 flash_attn, no gemm
    # f32: 96-wide (96 / 192 / 288 -> 96, 96 -> 96 + skip 288, 96 -> 20) conv_halo_kernel; 192-wide at 8^3 conv_wino2_kernel
    #      (96 / 192 / 288 -> 192, 192 -> 192 + skip) and conv_wino3_kernel (384 -> 192, the Upsample 192 -> 192 at 16^3);
    #      qkv 192 -> 576 and proj_out conv1x1_small_kernel; y 1.9e-6, worst block 1.8e-6
    # bf16: conv_bf16t_kernel wherever K >= 192 (192 / 288 -> 96, 96 -> 96 + skip 288 at 16^3; 192 / 288 / 384 -> 192 at 8^3,
    #       the Upsample), conv_halo_kernel for 96 -> 96, 96 -> 192, 96 -> 20; 1x1x1 on conv_small_kernel; y 1.1e-2, block 1.1e-2
    # f32_bf16x3: conv_halo_kernel for every stride-1 3x3x3 from 96 inputs on, every 1x1x1 (the skips are launches of their
    #       own) on conv_small_kernel; y 2.0e-6, block 2.0e-6
    "96-192": (16, 12, 20, 96, (1, 2), (2,), 3, 1),
    # head widths 48 (8^3, T = 512) and 96 (4^3, T = 64): GEMM + softmax; qkv with 288 and 576 output channels; batch 2.
    # f32: 8^3: conv_halo_kernel (96-wide, 96 -> 20), conv_small_kernel (12 -> 96, qkv 96 -> 288, proj_out 96 -> 96),
    #      conv_wino3_kernel for the Upsample 192 -> 192; 4^3: conv_small_kernel (192-wide, stride 2), conv1x1_small_kernel (qkv
    #      192 -> 576, proj_out); 22 gemm, no flash_attn; y 2.0e-6, block 1.7e-6
    "96-heads2": (8, 12, 20, 96, (1, 2), (1, 2), 2, 2),
    # Cout 160 (padded to 192), 5 channels per group, concat 320 (10 per group), 4 input channels, head width 80.
    # f32: conv_halo_kernel (160 / 320 -> 160, 160 -> 160 + skip, 160 -> 8), conv_small_kernel (4 -> 160, qkv 160 -> 480,
    #      proj_out); 2 gemm; y 2.9e-6, block 2.2e-6
    "160": (16, 4, 8, 160, (1,), (), 2, 1),
    # 7 channels per group, Cout 224 (padded to 256), seven heads of 32 channels on the flash kernel, qkv Cout 672.
    # f32: conv_halo_kernel (224 / 448 -> 224, 224 -> 224 + skip, 224 -> 4), conv_small_kernel (8 -> 224, qkv 224 -> 672,
    #      proj_out); 6 flash_attn, no gemm; y 1.7e-6, block 1.5e-6
    "224": (8, 8, 4, 224, (1,), (1,), 7, 1),
    # 36 input channels (padded to 64), 4 output channels, widths 32 and 96 on the `c < 64 -> 32` side of the Cout padding.
    # every mode: 8^3: conv_igemm_kernel (36 -> 32, the 1x1x1 skips 64 / 128 -> 32, stride 2), conv_halo_kernel (32 / 64 / 128
    #      -> 32, 32 -> 4, the Upsample 96 -> 96); 4^3: conv_small_kernel (96-wide, qkv 96 -> 288, proj_out; f32 fuses the
    #      skips, the other two launch them); 12 gemm, no flash_attn
    # f32 y 1.9e-6, block 1.6e-6; bf16 y 8.8e-3, block 1.1e-2; f32_bf16x3 y 1.9e-6, block 1.6e-6
    "36-to-4": (8, 36, 4, 32, (1, 3), (2,), 2, 2),
    # 36 OUTPUT channels, the forward twin of what `36-to-4` meets in the backward (where the transposed first convolution has
    # 36 output channels): a Cout between 32 and 64 is two 32-wide tiles, its packed weights are padded to 64.  One level.
    # every mode: conv_halo_kernel (32 / 64 -> 32, 32 -> 36), conv_igemm_kernel (4 -> 32, the 1x1x1 skips), conv_small_kernel
    #      (qkv 32 -> 96); 1 flash_attn; f32 and f32_bf16x3 y 1.6e-6, block 1.6e-6; bf16 y 1.1e-2, block 8.1e-3
    #      (with the weights padded to 32, as they were: y 1.09 in every mode, grad_x of `36-to-4` 1.02)
    "4-to-36": (8, 4, 36, 32, (1,), (), 2, 1),
}
EMU_CASE = ("36-to-4", "f32")  # the one emulation size (at batch 1 there)
CASES = [(r, "f32") for r in ROWS] + [(r, c) for r in ("96-192", "36-to-4", "4-to-36") for c in ("bf16", "f32_bf16x3")]
CASES.sort(key=lambda c: list(ROWS).index(c[0]))  # (the modes of a row follow each other: one oracle run per row)


def _cfg(row):
    image, cin, cout, mc, mult, attn, heads, _ = ROWS[row]
    return uo.UNetCfg(image_size=image, in_channels=cin, out_channels=cout, model_channels=mc, num_res_blocks=2,
                      channel_mult=mult, attention_resolutions=attn, num_heads=heads)


def _describe(ops):
    convs = [o for o in ops if o["op"] == "conv"]
    names = [o["op"] for o in ops]
    lines = sorted({f"{o['kernel']} {o['cin']}->{o['cout']} k{o['ksz']}{' s2' if o['stride'] == 2 else ''}"
                    f"{' up' if o['upsample'] else ''}{' +skip' if o['fused_skip'] else ''} @{o['out_dim']}^3" for o in convs})
    return convs, names, lines


@pytest.mark.parametrize("row,compute", CASES)
def test_channel_widths_vs_oracle_blockwise(gu, row, compute, monkeypatch):
    """Every block output and `y` of the nets of ROWS against the pinned oracle, then - on the device - the kernels the
    planner chose by itself (printed), held against the conditions of conv_plan and flash_attn_supported."""
    batch = ROWS[row][7]
    if gu.EMU:
        if (row, compute) != EMU_CASE:
            pytest.skip("not an emulation size")
        batch = 1
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = _cfg(row)
    net, _, _ = _forward_blockwise(gu, cfg, batch, compute, 99, 11, row)
    if gu.EMU:
        return
    convs, names, lines = _describe(net.time_ops(batch, 1, gu.DEV))
    print(f"{row} {compute}: {names.count('gemm')} gemm, {names.count('flash_attn')} flash_attn launches; convolutions:\n  " +
          "\n  ".join(lines))
    for o in convs:  # a kernel family never serves a width its condition in conv_plan excludes
        k, desc = o["kernel"], (o["kernel"], o["cin"], o["cout"], o["out_dim"])
        if o["cout"] % 64:
            assert k not in ("conv_wino3_kernel", "conv_s2_bf16_kernel", "conv1x1_small_kernel", "conv1x1_stream_kernel"), desc
            assert k != "conv_wino2_kernel" or o["cout"] == 32, desc
        if o["cout"] % 32 or o["cin"] % 16:
            assert k not in BF16_WIDE | {"conv1x1_qkv_bf16_kernel", "conv1x1_bf16_stream_kernel"}, desc
        if o["cin"] % 16:
            assert k in ("conv_small_kernel", "conv_igemm_kernel"), desc
    first, last = convs[0], convs[-1]
    assert (first["cin"], last["cout"]) == (cfg.in_channels, cfg.out_channels), (first, last)
    if row == "96-192":  # 5 + 1 attention blocks at 8^3, three heads of 64 channels: the flash kernel in every mode
        assert names.count("flash_attn") == 6 and names.count("gemm") == 0, names
    if row in ("96-heads2", "160", "36-to-4"):  # head widths 48 / 96, 80 and 48: no flash kernel, two GEMMs per attention block
        assert names.count("flash_attn") == 0 and names.count("gemm") >= 2, names
    if row == "224":  # seven heads of 32 channels, T = 512: 2 + 1 + 3 attention blocks on the flash kernel
        assert names.count("flash_attn") == 6 and names.count("gemm") == 0, names


def test_bf16_1x1_at_96_input_channels_leaves_the_streaming_kernels(gu, monkeypatch, capfd):
    """A bf16-mode forward with a 1x1x1 convolution of 96 input channels over 4096 voxels - the smallest net that has one the bf16
    streaming kernels' conditions used to admit: the un-fused skip_connection 96 -> 32 of the first ResBlock below the top level
    (channel_mult (3, 1) at model_channels 32; 32 output channels, so it is not fused into the 3x3x3 convolution).
    conv1x1_bf16_stream_kernel and conv1x1_qkv_bf16_kernel exist for 64 / 128 / 192 / 256 input channels only; the planner
    used to pick the former here and the launcher then refused the forward.  (An attention block 96 wide never met this: its qkv
    and proj_out have 288 and 96 output channels, not the whole 64-wide tiles those kernels ask for.)  The forward runs to the
    end, no [plan] line names either kernel, and `y` and every block meet the bf16 bound of this file against the oracle."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    cfg = uo.UNetCfg(image_size=32, in_channels=4, out_channels=4, model_channels=32, num_res_blocks=1, channel_mult=(3, 1),
                     attention_resolutions=(), num_heads=1)
    capfd.readouterr()
    _forward_blockwise(gu, cfg, 1, "bf16", 99, 11, "96-to-32")
    cap = capfd.readouterr()
    plan = [line for line in cap.err.splitlines() if line.startswith("[plan] conv ")]
    print(cap.out + "\n".join(plan))
    skips = [line for line in plan if line.startswith("[plan] conv 96->32 k1 s1 @16^3 ")]
    assert skips, plan
    for line in plan:
        assert "conv1x1_qkv_bf16_kernel" not in line and "conv1x1_bf16_stream_kernel" not in line, line


# ---- 2. forced kernel families on `96-192` ---------------------------------------------------------------------------------
# Seen on the MI355X: every setting leaves 12 -> 96 and the stride-2 96 -> 96 on conv_small_kernel, 96 -> 20 and - in fp32 -
# every 96-wide convolution on conv_halo_kernel; the 14 192-wide ones and the Upsample 192 -> 192 move to the forced family,
# in bf16 "1" / "p" the ten 96-wide ones (Cout % 32 == 0) too.  Against the oracle: fp32 y 1.7e-6 .. 1.9e-6, worst block
# 1.7e-6 .. 2.0e-6; bf16 y 1.0e-2 .. 1.2e-2, worst block 1.1e-2 .. 1.2e-2.  Winograd against direct: y 1.4e-6 .. 1.6e-6,
# worst block 1.5e-6 .. 1.6e-6.  bf16 "1" / "p" against "0": first differing block input_blocks.1 (a 96-wide ResBlock),
# max|d| 1.56e-2 of 4.0 = half a bf16 ulp of the largest value, 0.7 % of the elements differ.
FORCED = {
    # exact fp32
    ("f32", "direct"): DIRECT_ENV,
    ("f32", "wino3-min-items"): {"HOLO_CONV_WINO3_MIN_ITEMS": "1"},
    ("f32", "wino3"): {"HOLO_CONV_FORCE_TZ2": "1", "HOLO_CONV_WINO": "2", "HOLO_CONV_WINO3_MIN_ITEMS": "1"},
    ("f32", "wino2"): {"HOLO_CONV_FORCE_TZ2": "1", "HOLO_CONV_WINO": "2", "HOLO_CONV_WINO3": "0"},
    # bf16 storage mode: the 64/128-voxel halo kernels, the wide-tile kernel, its persistent form, the stride-2 halo kernel
    ("bf16", "0"): {"HOLO_CONV_BF16T": "0", "HOLO_CONV_BF16P": "0"},
    ("bf16", "1"): {"HOLO_CONV_BF16T": "1", "HOLO_CONV_BF16P": "0"},
    ("bf16", "p"): {"HOLO_CONV_BF16T": "1", "HOLO_CONV_BF16P": "1", "HOLO_CONV_BF16P_WGS": "8"},
    ("bf16", "s2"): {"HOLO_CONV_BF16T": "0", "HOLO_CONV_BF16P": "0", "HOLO_CONV_S2T": "1"},
}
_RUNS = {}  # (compute, setting) -> (y, block outputs, convolution ops) of the forced runs: each runs once, the A/B checks share them


def _forced_run(gu, monkeypatch, compute, setting):
    key = (compute, setting)
    if key not in _RUNS:
        monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
        for k, v in FORCED[key].items():
            monkeypatch.setenv(k, v)
        net, y, outs = _forward_blockwise(gu, _cfg("96-192"), 1, compute, 99, 11, f"96-192 [{setting}]")
        convs, _, lines = _describe(net.time_ops(1, 1, gu.DEV))
        print(f"96-192 {compute} [{setting}]: convolutions:\n  " + "\n  ".join(lines))
        for k in FORCED[key]:
            monkeypatch.delenv(k)
        _RUNS[key] = (y.cpu(), outs, convs)
    return _RUNS[key]


def _plain3(convs, cout=None):
    """The stride-1 3x3x3 convolutions that read their input as it is stored (no upsampling on load)."""
    return [o for o in convs if o["ksz"] == 3 and o["stride"] == 1 and not o["upsample"] and (cout is None or o["cout"] == cout)]


def _kernels_differ(a, b):
    return [(x["kernel"], x["tile_depth"], x["nsplit"]) for x in a] != [(x["kernel"], x["tile_depth"], x["nsplit"]) for x in b]


@pytest.mark.parametrize("setting", ["direct", "wino3-min-items", "wino3", "wino2"])
def test_forced_fp32_families_at_96_and_192(gu, setting, monkeypatch):
    """`96-192` in exact fp32 with the Winograd families forced on (and off): block by block against the oracle at the fp32
    bound; the 192-wide 3x3x3 convolutions (8^3: 4 tiles of 2 x 8 x 8, three 64-channel output blocks, Cin 96 / 192 / 288 /
    384) run on the forced family, the 96- and 20-wide ones (Cout % 64 != 0) never do; and every block agrees with the
    all-direct run within 1e-5."""
    _heavy(gu)
    y, outs, convs = _forced_run(gu, monkeypatch, "f32", setting)
    wide, narrow = _plain3(convs, 192), [o for o in convs if o["cout"] % 64]
    # (two convolutions in each of the 2 + 2 + 3 ResBlocks of the 8^3 level and the middle block)
    assert len(wide) == 14 and all(o["cin"] % 32 == 0 and o["out_dim"] == 8 for o in wide), wide
    assert {o["cout"] for o in narrow} == {96, 20}, narrow
    assert not any(o["kernel"] in WINO for o in narrow), narrow
    want = {"direct": None, "wino3-min-items": "conv_wino3_kernel", "wino3": "conv_wino3_kernel", "wino2": "conv_wino2_kernel"}[setting]
    if want is None:
        assert not any(o["kernel"] in WINO for o in convs), convs
        return
    assert all(o["kernel"] == want for o in wide), [(o["kernel"], o["cin"]) for o in wide]
    yd, outs_d, convs_d = _forced_run(gu, monkeypatch, "f32", "direct")
    assert _kernels_differ(convs, convs_d)
    worst = max((gu.rel_err(outs[tag], outs_d[tag]), tag) for tag in outs)
    print(f"96-192 [{setting}] against the direct kernels: y {gu.rel_err(y, yd):.2e}, worst block {worst[0]:.2e} ({worst[1]})")
    assert gu.rel_err(y, yd) < 1e-5
    for tag in outs:
        assert gu.rel_err(outs[tag], outs_d[tag]) < 1e-5, tag


@pytest.mark.parametrize("setting", ["0", "1", "p", "s2"])
def test_forced_bf16_kernels_at_96_and_192(gu, setting, monkeypatch):
    """`96-192` in the bf16 storage mode on the halo kernels ("0"), with the wide-tile kernel ("1") and its persistent form
    ("p") forced onto every launch their conditions admit, and with the stride-2 halo kernel's knob ("s2"): block by block
    against the oracle at the bf16 bound.  The 192-wide 3x3x3 convolutions run on the forced form; the convolutions with 12
    input or 20 output channels never do; the one Downsample convolution is 96 wide (Cout % 64 != 0), so it must stay off
    conv_s2_bf16_kernel - the "s2" run plans exactly as "0" does and is bit-equal to it.  Where the kernels differ, the first
    block that differs at all is at most one bf16 ulp of its largest value away from the halo kernels' run."""
    _heavy(gu)
    y, outs, convs = _forced_run(gu, monkeypatch, "bf16", setting)
    wide = _plain3(convs, 192)
    assert len(wide) == 14, wide
    for o in convs:
        if o["cout"] % 32 or o["cin"] % 16:
            assert o["kernel"] not in BF16_WIDE, (o["kernel"], o["cin"], o["cout"])
    s2 = [o for o in convs if o["stride"] == 2]
    assert len(s2) == 1 and s2[0]["cout"] == 96 and s2[0]["kernel"] != "conv_s2_bf16_kernel", s2
    kernels = {o["kernel"] for o in convs}
    if setting in ("0", "s2"):
        assert not (kernels & BF16_WIDE), kernels
    else:
        want = "conv_bf16p_kernel" if setting == "p" else "conv_bf16t_kernel"
        assert all(o["kernel"] == want for o in wide), [(o["kernel"], o["cin"]) for o in wide]
        assert ("conv_bf16t_kernel" in kernels) == (setting == "1"), kernels
    if setting == "0":
        return
    y0, outs0, convs0 = _forced_run(gu, monkeypatch, "bf16", "0")
    if setting == "s2":
        assert not _kernels_differ(convs, convs0)
        assert torch.equal(y, y0) and all(torch.equal(outs[tag], outs0[tag]) for tag in outs)
    else:
        assert _kernels_differ(convs, convs0)
        _ab_one_ulp(outs0, outs, "96-192 wide tile " + setting)


# ---- 3. backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"HOLO_DGRAD_S2_DIRECT": "1"}, {"HOLO_WGRAD_REDUCE_TILE_MIN": "1"}],
                         ids=["default", "dgrad-s2-direct", "wgrad-reduce-tile"])
@pytest.mark.parametrize("row,batch", [("96-heads2", 1), ("36-to-4", 2), ("4-to-36", 1)])
def test_backward_at_channel_widths(gu, row, batch, env, monkeypatch):
    """Every parameter gradient, grad_x and y against autograd through the oracle: the dgrad weights packed with the padded
    widths of 12 / 36 input channels (output channels of the transposed convolution), the weight-gradient kernels at 20 and 4
    (`4-to-36`: 36) output channels, grad_x back to NCDHW at 12 and 36 channels, GroupNorm backward with 3 and 6 (9 across a concat) channels
    per group, attention backward at head widths 48 and 96; also with the direct stride-2 dgrad and the weight-gradient
    reduce's tile form.  Seen: `96-heads2` y 1.7e-6, grad_x 2.6e-6 (2.7e-6 with the direct stride-2 dgrad), worst parameter
    4.8e-6 of its scale; `36-to-4` y 1.8e-6, grad_x 1.9e-6, worst parameter 1.3e-4 (a bias in front of a GroupNorm);
    `4-to-36` y 2.3e-6, grad_x 2.1e-6, worst parameter 7.0e-5 (the same bias)."""
    if gu.EMU:
        pytest.skip("backward tests run on the device")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = _cfg(row)
    net, sd = gu.make_unet(cfg, seed=5)
    x = torch.from_numpy(np_noise(1, (batch, cfg.in_channels) + (cfg.image_size,) * 3))
    t = torch.tensor([437, 12][:batch], dtype=torch.int64)
    G = torch.from_numpy(np_noise(2, (batch, cfg.out_channels) + (cfg.image_size,) * 3))
    key = (row, batch)
    if key not in _GRADS:
        _GRADS.clear()
        torch.set_num_threads(min(32, torch.get_num_threads()))
        _GRADS[key] = _oracle_grads(sd, cfg, x, t, G)
    y_ref, gx_ref, g_ref = _GRADS[key]
    y, gx, grads = net.backward(x.to(gu.DEV), t.to(gu.DEV), G.to(gu.DEV))
    floor = 1e-2 * float(np.median([g_ref[k].abs().max().item() for k in sd]))
    worst = max(((grads[k].cpu() - g_ref[k]).abs().max().item() / max(g_ref[k].abs().max().item(), floor), k) for k in sd)
    print(f"backward {row} batch {batch} {env}: y {gu.rel_err(y, y_ref):.2e}, grad_x {gu.rel_err(gx, gx_ref):.2e}, "
          f"worst relative gradient error {worst[0]:.2e} ({worst[1]})")
    _check(y, y_ref, "forward output", 2e-3)
    _check(gx, gx_ref, "grad_x")
    assert set(grads) == set(sd)
    for k in sd:
        _check(grads[k], g_ref[k], k, floor=floor)


_GRADS = {}  # the last autograd run through the oracle: the knob settings of one net follow each other and share it


# ---- 4. equalities at these widths, on `96-heads2` -------------------------------------------------------------------------
def _heads2_inputs(gu, batch, seed):
    cfg = _cfg("96-heads2")
    x = torch.from_numpy(np_noise(seed, (batch, cfg.in_channels) + (cfg.image_size,) * 3))
    return cfg, x, torch.tensor([640, 3, 999][:batch], dtype=torch.int64)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_forward_channels_last_at_12_and_20_channels(gu, compute):
    """forward_channels_last on (2, 8, 8, 8, 12) -> (2, 8, 8, 8, 20) is bit-equal to the NCDHW call: the layout kernels move
    32-channel tiles, 12 and 20 channels leave partial ones, and the two tensors differ in width."""
    _heavy(gu)
    cfg, x, t = _heads2_inputs(gu, 2, 21)
    net, _ = gu.make_unet(cfg, seed=3, compute_dtype=compute)
    x, t = x.to(gu.DEV), t.to(gu.DEV)
    with torch.no_grad():
        y = net(x, t)
        x_cl = x.permute(0, 2, 3, 4, 1).contiguous()
        y_cl = net.forward_channels_last(x_cl, t)
        assert y_cl.shape == (2, 8, 8, 8, 20) and torch.equal(y_cl.permute(0, 4, 1, 2, 3), y)
        assert torch.equal(net(x, t), y) and torch.equal(net.forward_channels_last(x_cl, t), y_cl)
    from holo_diffusion_amd._lib import HoloError
    with pytest.raises(HoloError):
        net.forward_channels_last(x, t)  # an NCDHW tensor is not (N, R, R, R, C)


def test_batch_invariant_rows_at_96_channels(gu):
    """set_batch_invariant(True), batch 3, fp32: every row is bit-equal to the batch-1 forward of that row, and right."""
    _heavy(gu)
    cfg, xs, ts = _heads2_inputs(gu, 3, 40)
    net, sd = gu.make_unet(cfg, seed=3)
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
def test_workspace_independence_at_96_channels(gu, compute):
    """A forward on a workspace filled with 0x00 / 0xFF / 0x7F bytes: bit-identical and finite (a padded channel - 96 of
    128, 20 of 32, 12 of 32 - that is read without having been written shows up here as a NaN), and right."""
    _heavy(gu)
    from holo_diffusion_amd import runtime
    cfg, x, t = _heads2_inputs(gu, 2, 13)
    net, sd = gu.make_unet(cfg, seed=7, compute_dtype=compute)
    ref = uo.unet_forward(sd, cfg, x, t)
    x, t = x.to(gu.DEV), t.to(gu.DEV)
    outs = []
    for fill in (0, 0xFF, 0x7F):
        ws = runtime.workspace(net, gu.DEV, net.workspace_bytes(2, gu.DEV))
        ws.fill_(fill)
        with torch.no_grad():
            outs.append(net(x, t).clone())
    assert torch.isfinite(outs[1]).all() and torch.isfinite(outs[2]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert gu.rel_err(outs[1], ref) < (2e-2 if compute == "bf16" else 2e-3)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_two_forwards_at_96_channels_are_bit_identical(gu, compute):
    _heavy(gu)
    cfg, x, t = _heads2_inputs(gu, 2, 13)
    net, _ = gu.make_unet(cfg, seed=7, compute_dtype=compute)
    with torch.no_grad():
        a = net(x.to(gu.DEV), t.to(gu.DEV)).clone()
        junk = torch.full((123_457,), float("nan"), device=gu.DEV)  # (vary what the allocator hands out)
        b = net(x.to(gu.DEV), t.to(gu.DEV))
    assert torch.isfinite(a).all() and torch.equal(a, b)
    del junk


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("in_channels", 6), ("out_channels", 10), ("model_channels", 48), ("model_channels", 288)])
def test_unsupported_widths_are_refused(gu, field, value):
    """Widths outside the served set (in / out channels a multiple of 4, model_channels a multiple of 32 up to 256): the
    first use of the net raises HoloError("... unsupported configuration"), nothing is launched."""
    from holo_diffusion_amd import SimpleUnet3D
    from holo_diffusion_amd._lib import HoloError
    kw = dict(image_size=8, in_channels=8, out_channels=8, model_channels=32, num_res_blocks=1, channel_mult=(1, 2),
              attention_resolutions=(2,), num_heads=2)
    kw[field] = value
    with pytest.raises(HoloError, match="unsupported configuration"):
        net = SimpleUnet3D(**kw).to(gu.DEV)
        net(torch.zeros(1, kw["in_channels"], 8, 8, 8, device=gu.DEV), torch.zeros(1, dtype=torch.long, device=gu.DEV))
