"""Deep levels apply GroupNorm (+ SiLU) once per tensor (HOLO_ROWTILE_PREACT, unetplan::preactivate_rowtile): where a row-tile
convolution (conv_small_kernel) at 4^3 and below would apply the coefficients and the SiLU once per (tap, Cout tile)
workgroup, the gn_finalize launch in front writes the activated tensor once (gn_finalize_act_kernel) and the convolution reads
it as raw input.  The arithmetic is the same - one fused multiply-add on the same fp32 (a, b), the same quotient - so the bound
is bit-equality: every block output of a forward with the knob at 1 is torch.equal to the one with the knob at 0.

Every case first reads the "[plan] ... pairs pre-activated" line of HOLO_DEBUG_PLAN and asserts the number of rewritten pairs it
was built for (0 pairs would compare a plan with itself).  The nets are two- and three-level nets of one ResBlock per block
on an 8^3 grid, whose 4^3 (and 2^3) levels run on the row-tile kernel under the default knobs; model_channels M, the deep level
has 2M channels, and the way up reads the concats (2M + 2M) and (2M + M):

  c64      M = 64: 4 and 8 channels per group (128, 256 channels); the (128 + 64) concat has 6 and is declined, as is the 64
           channel input of the first 4^3 ResBlock (2 per group); second convolutions with a fused 1x1x1 skip over two sources
  c64-b3   M = 64, channel_mult (1, 2, 4), batch 3: a 2^3 level, whose 24 rows put two samples into one 64-row tile
  c160     M = 160: 320 channels are 10 per group - declined -, the (320 + 320) concat has 20 - rewritten -, (320 + 160) 15
  c256     M = 256 with attention at 4^3: 16 and 32 per group, the (512 + 256) concat 24 per group with the group at the seam
           straddling it (512 = 21 * 24 + 8), and the 1x1x1 qkv convolution 512 -> 1536, affine only, 24 Cout tiles

Weights and inputs (all but the oracle case): +-10 on the biases in front of every GroupNorm (offset inputs: |mean| many times
the spread) and beta = -100 on two channels of every GroupNorm that feeds a SiLU: those values lie outside 2^-60 <= |v| <= 64,
so the parent's convolution takes its IEEE division for their waves and the shortened one elsewhere (rowtile_silu.h); the
finalize launch takes silu_f everywhere.  One case (c64, plain weights) is also held against the oracle block by block at
1e-4, the blockwise bound of tests/test_gpu_unet.py."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

# case: (model_channels, channel_mult, attention_resolutions, batch, pairs the default knobs must rewrite)
#   pairs of a (1, 2) net: 4^3 ResBlock down (second convolution; the first too where M / 32 % 4 == 0), two middle ResBlocks
#   (2 each), (2M + 2M) ResBlock (both), (2M + M) ResBlock (second; first where 3M / 32 % 4 == 0), + 4 qkv with attention
CASES = {
    "c64": (64, (1, 2), (), 1, 1 + 4 + 2 + 1),
    "c64-b3": (64, (1, 2, 4), (), 3, None),  # (counted from the plan line: at least the c64 ones and one at 2^3)
    "c160": (160, (1, 2), (), 1, 0 + 0 + 1 + 0),
    "c256": (256, (1, 2), (2,), 1, 2 + 4 + 2 + 2 + 4),
}
PAIRS = re.compile(r"\[plan\] batch (\d+): (\d+) finalize \+ row-tile convolution pairs pre-activated")


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _cfg(case):
    mc, mult, attn, _, _ = CASES[case]
    return uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=1, channel_mult=mult,
                      attention_resolutions=attn, num_heads=2)


def _stress(sd, d=10.0, seed=5):
    """Offsets in front of every GroupNorm and two saturated channels (beta = -100) per GroupNorm that feeds a SiLU."""
    rng = np.random.RandomState(seed)
    for k in sorted(sd):
        if k == "input_blocks.0.0.bias" or k.endswith((".in_layers.2.bias", ".out_layers.3.bias", ".op.bias", ".conv.bias")):
            c = sd[k].shape[0]
            sign = torch.from_numpy(rng.choice([-1.0, 1.0], 4).astype(np.float32)).repeat_interleave(c // 4)
            sd[k] = sd[k] + d * sign
        if k == "out.0.bias" or k.endswith((".in_layers.0.bias", ".out_layers.0.bias")):
            b = sd[k].clone()
            b[torch.from_numpy(rng.choice(b.shape[0], 2, replace=False))] = -100.0
            sd[k] = b
    return sd


def _forward(gu, case, monkeypatch, capfd, knob, stress):
    """One forward under HOLO_ROWTILE_PREACT=knob: ({tag: block output}, y, the pairs the placed plan pre-activated)."""
    import holo_diffusion_amd as hda
    from holo_diffusion_amd.weights import synth_state_dict
    _, _, _, batch, _ = CASES[case]
    cfg = _cfg(case)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    monkeypatch.setenv("HOLO_ROWTILE_PREACT", str(knob))
    sd = synth_state_dict(uo.unet_param_shapes(cfg), 61)
    if stress:
        sd = _stress(sd)
    net = hda.SimpleUnet3D(image_size=cfg.image_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                           model_channels=cfg.model_channels, num_res_blocks=cfg.num_res_blocks, channel_mult=cfg.channel_mult,
                           attention_resolutions=cfg.attention_resolutions, num_heads=cfg.num_heads)
    net.load_state_dict({"_net." + k: v for k, v in sd.items()})
    net = net.to(gu.DEV)
    x = torch.from_numpy(np_noise(62, (batch, 16, 8, 8, 8)))
    if stress:
        x = x * 0.5 + 3.0
    t = torch.tensor([433, 12, 871][:batch], dtype=torch.int64)
    capfd.readouterr()
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV)).cpu()
    err = capfd.readouterr().err
    found = [(int(b), int(n)) for b, n in PAIRS.findall(err)]
    assert found and all(b == batch for b, _ in found), found
    assert len({n for _, n in found}) == 1, found  # the sizing pass and the placed pass agree
    outs = {tag: net.fetch_block(tag, (batch,) + shape).float().cpu() for tag, shape in block_shapes(cfg).items()}
    return outs, y, found[-1][1], (sd, x, t)


def block_shapes(cfg):
    """{tag: (C, R, R, R)} of every block output: the reference's block structure."""
    M, R, shapes = cfg.model_channels, cfg.image_size, {}
    ins = [(M, R)]
    for level, mult in enumerate(cfg.channel_mult):
        ins += [(M * mult, R)] * cfg.num_res_blocks
        if level != len(cfg.channel_mult) - 1:
            R //= 2
            ins.append((M * mult, R))
    outs = []
    for level, mult in reversed(list(enumerate(cfg.channel_mult))):
        for i in range(cfg.num_res_blocks + 1):
            if level and i == cfg.num_res_blocks:
                R *= 2
            outs.append((M * mult, R))
    for i, (c, r) in enumerate(ins):
        shapes[f"input_blocks.{i}"] = (c, r, r, r)
    shapes["middle_block"] = (ins[-1][0],) + (ins[-1][1],) * 3
    for i, (c, r) in enumerate(outs):
        shapes[f"output_blocks.{i}"] = (c, r, r, r)
    return shapes


@pytest.mark.parametrize("case", list(CASES))
def test_preactivated_equals_parent_form_bit_for_bit(gu, case, monkeypatch, capfd):
    if gu.EMU and case in ("c160", "c256"):
        pytest.skip("too large for the host emulation")
    on, y_on, pairs_on, _ = _forward(gu, case, monkeypatch, capfd, 1, True)
    off, y_off, pairs_off, _ = _forward(gu, case, monkeypatch, capfd, 0, True)
    print(f"  {case}: {pairs_on} pairs pre-activated, {pairs_off} with the knob at 0")
    want = CASES[case][4]
    assert pairs_off == 0
    assert pairs_on == want if want is not None else pairs_on > CASES["c64"][4], pairs_on
    assert pairs_on >= 1
    assert set(on) == set(off) and len(on) >= 7
    for tag in on:
        assert torch.isfinite(on[tag]).all(), tag
        assert torch.equal(on[tag], off[tag]), tag
    assert torch.equal(y_on, y_off)


def test_preactivated_vs_oracle(gu, monkeypatch, capfd):
    """c64 on plain weights and input against the oracle, block by block and at the output."""
    outs, y, pairs, (sd, x, t) = _forward(gu, "c64", monkeypatch, capfd, 1, False)
    assert pairs == CASES["c64"][4]
    trace = {}
    ref = uo.unet_forward(sd, _cfg("c64"), x, t, trace)
    assert gu.rel_err(y, ref) < 1e-4
    for tag, got in outs.items():
        e = gu.rel_err(got, trace[tag])
        print(f"  {tag}: rel_err {e:.2e}")
        assert e < 1e-4, tag
