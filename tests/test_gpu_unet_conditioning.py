"""GPU parity of the denoiser on ILL-CONDITIONED inputs: peaked attention (A, B), GroupNorm inputs whose group mean dominates
their spread (C, D), and saturated SiLU (E).  Every other parity file builds its nets with `weights.synth_state_dict` and
feeds N(0, 1) noise: attention scores (exp2 domain) stay inside +-6, the largest softmax weight of a row averages 0.01 of 512
keys, and |group mean| / group std stays below 0.6 - every rescale factor of the online softmax is ~1 and E[x^2] - mean^2
never cancels.  Here the same nets get weights that move those two quantities, nothing else.

Reference: the oracle in FLOAT64 (`uo.unet_forward(..., dtype=torch.float64)`), never another HIP run.  The fp32 oracle
against it gives `e32`, what a correct fp32 implementation loses on that input; it is asserted small next to every bound,
so each bound keeps its headroom over the conditioning of the case itself.  Bounds are the project's own: fp32 and
f32_bf16x3 block outputs rel_err <= 1e-4, bf16 storage mode 2e-2, gradients 1e-3 of the tensor's scale.

A. Peaked attention, forward.  The q and k rows of every qkv.weight / qkv.bias times s (scores times s^2); compared: the
   FIRST attention block only (behind it the fp32 oracle itself drifts from fp64).  Measured on the fp64 oracle:
     16^3 net (input_blocks.3: T = 512, head width 64, batch 2, weights seed 41)
     s   exp2-domain scores   mean top softmax weight   e32 of the block
     1     -6 ..   5              0.01                  9.0e-7
     4    -99 ..  81              0.74                  7.0e-6
     5   -155 .. 126              0.83                  1.1e-5
     8   -398 .. 322              0.94                  1.6e-5
     8^3 net (input_blocks.1: head width 32, weights seed 7): s = 4 -89 .. 102, e32 3.9e-6; s = 8 -357 .. 410, e32 1.2e-5
     (seed 41 gives e32 2.7e-5 on this net at s = 8, above the 2.5e-5 asserted for the reference: hence its own seed).
   fp32 / f32_bf16x3 at s = 4, 8: flash_attn_kernel with HOLO_FLASH_SPLIT "", 1, 3 (+ flash_attn_merge_kernel), GEMM +
   softmax_rows + GEMM (HOLO_NO_FLASH_ATTN), and head width 32 on the 8^3 net; s = 8 overflows exp without a correct
   maximum.  MI355X: s = 4: 3.9e-6 .. 5.8e-6, s = 8: 1.3e-5 .. 1.8e-5 in every family - the fp32 oracle's own e32.
   bf16 storage mode (HOLO_BF16_FLASH_MIN_T=256), HOLO_FLASH_V2_KSPLIT 1 and 2, at the mixed s also HOLO_CONV_QKV_FUSED 0.
   In this mode the block's input is not the oracle's: the bf16 activations in front are 5.3e-3 off, and the float64 block
   evaluated on them is itself 2.9e-2 (s = 4) / 4.7e-2 (s = 5) away from the trace.  So the ResBlock in front of the compared
   attention block is made an exact pass-through (isolate_first_attention), the block input is fetched from the very run,
   and the reference is the float64 attention block ON THAT INPUT - the same input on both sides, as the issue wants it.
   s = 1, 4 and S_MIXED = 4.7 (moved from 5, inside the issue's 4.5 .. 5.5, until the flags of the isolated nets are mixed
   with no workgroup inside 2^(99 .. 101)); 16^3 net and, so that the host emulation can run them, the 8^3 net (head width
   32), there also s = 8.  The LAZY flags (a workgroup = 256 queries x one key split leaves 2^+-100) are computed HERE from
   the fp64 scores, never read from the kernel: 16^3 net at 4.7: 2 of 8 workgroups with one split, 2 of 16 with two (|log2
   sum| 89 .. 97 and 104, 123); 8^3 net: 7 of 8 and 10 of 16; with two splits some queries merge a LAZY partial (reference
   0) with an exact one; s = 1 and 4 flag none, s = 8 all.  Asserted: planned kernels, finite, LAZY + fallback within 2^-6 of
   the exact loop (MI355X: 3.9e-3 .. 6.4e-3), and both within 2x the FORMAT FLOOR of the float64 block - the same block with
   each bf16 rounding of the mode applied once in float64 (bf16_attention_own_input).  MI355X, kernel = floor to three digits
   in every case: 16^3 net s = 1 3.3e-3, s = 4 1.9e-2 (LAZY) / 1.85e-2, s = 4.7 3.05e-2; 8^3 net s = 4 2.2e-2, 4.7 2.76e-2,
   8 7.4e-2.  Against the issue's 2e-2 (16^3 net): s = 1 and 4 hold it; s = 4.7 cannot - the floor is 3.05e-2 - and is an
   expected failure only under that in-test finding (test_peaked_attention_bf16_against_f64).  The issue's estimate of
   1.2e-2 at s = 5 left out the rounding of the qkv convolution's operands.
B. Peaked attention, backward: `wide` with only middle_block.1 scaled by 4 and 6, and an 8^3 net whose one scaled block
   (input_blocks.1.1) runs the attention backward at T = 512, s = 6; fp64 autograd; e32 <= 1e-4 asserted (reference alone:
   wide s = 6 y 1.8e-6, grad_x 2.4e-5, parameters 3.6e-5; T = 512 3.0e-6, 1.2e-5, 1.4e-5).  MI355X: wide s = 6 y 1.9e-6,
   grad_x 1.8e-5, worst parameter 2.7e-5; T = 512 4.2e-6, 1.9e-5, 2.7e-5.
C. Offset GroupNorm inputs, forward: d * sign added to the bias of every convolution that feeds a GroupNorm (one sign per
   run of Cout / 16 channels: a whole number of groups for the direct consumer - 32 groups - and for a concat of two equally
   wide tensors).  |mean| / std of the fp64 trace's block outputs: d = 3 up to 10.2 (8^3 net) / 7.9 (16^3 net), d = 10 33.4
   / 25.7, d = 30 100.7 / 76.4; the fp32 oracle stays <= 1.7e-6.  Kernel families: planner's
   choice, direct, wino2, wino3 (HOLO_CONV_FORCE_TZ2), HOLO_NO_SKIP_FUSION; 16^3 cases for the 512-voxel slabs; and a
   32-channel net whose 4^3 level and Downsample run on conv_igemm_kernel, which writes no statistics slabs: the stand-alone
   gn_stats launch, asserted from time_ops (at 64 channels every kernel the planner can choose writes slabs: asserted too).
   The offsets lift a block's maximum - the bound's denominator - to 330 at d = 30, and a variance formed in FLOAT in
   gn_finalize_kernel costs only 9.7e-6 of it.  So every block is ALSO held to 1e-4 of its SPREAD (largest |x - channel
   mean|: what the next GroupNorm keeps); the fp32 oracle stays below 4.8e-6 of it (asserted at 1e-5).  MI355X, worst block
   at d = 30, of its maximum / of its spread: planner and direct 2.1e-6 / 3.9e-5, wino2 3.5e-6 / 7.1e-5, wino3 3.2e-6 /
   6.3e-5, f32_bf16x3 1.1e-6 / 2.3e-5, 16^3 net 1.2e-6 / 8.3e-6, narrow net 2.0e-6 / 3.2e-5; d = 10 and 3 lie below.
   The host emulation build misses the spread bound at d = 30 (1.25e-4 at input_blocks.2; 1.7e-5 at d = 10): its MFMA model
   sums in another order than the device; the float-variance mutant reads 2.1e-4 there.
   The bf16 storage mode is NOT a case: storing a 28 sigma offset in bf16 costs 28 * 2^-9 sigma = 5 % by construction.
D. Offset GroupNorm, backward (`wide`, d = 3, 10; gn_bwd_* read the stored float moments): reference alone 3.5e-6 / 6.4e-6;
   MI355X d = 10: y 1.5e-6, grad_x 7.0e-6, worst parameter 1.3e-5.
E. Saturated SiLU: beta = -100 on two channels of every GroupNorm that feeds a SiLU: the SiLU is 0 on both sides and exp
   overflows inside silu_fast / w3_silu / silu_b.  Negative beta only: no tensor's maximum (the bounds' denominators) moves.
   MI355X: worst block 1.4e-6 forward, worst parameter gradient 1.4e-5."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.test_gpu_backward import BACKWARD_CFGS, _check, _oracle_grads  # noqa: E402
from tests.test_gpu_wino3_item_boundary import DIRECT_ENV  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _heavy(gu, why="not an emulation size"):
    if gu.EMU:
        pytest.skip(why)


def _rel(got, ref):
    """max|got - ref| / max|ref| in double (gu.rel_err rounds the reference to float first)."""
    return ((got.detach().cpu().double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300)).item()


def _rel_spread(got, ref):
    """max|got - ref| over the largest |ref - its per-(sample, channel) mean|: the error as the GroupNorm behind the tensor
    sees it - channel offsets are what it removes, and they may be 20x the spread here."""
    ref = ref.double()
    spread = (ref - ref.mean(dim=(2, 3, 4), keepdim=True)).abs().max().clamp_min(1e-300)
    return ((got.detach().cpu().double() - ref).abs().max() / spread).item()


def _blocks(trace):
    return [k for k in trace if k.startswith(("input_blocks", "output_blocks")) or k == "middle_block"]


_CACHE = {}  # references (fp64 trace, e32, ...) computed once per case and never written to afterwards


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _make_net(gu, cfg, sd, compute="f32"):
    import holo_diffusion_amd as hda
    net = hda.SimpleUnet3D(image_size=cfg.image_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                           model_channels=cfg.model_channels, num_res_blocks=cfg.num_res_blocks, channel_mult=cfg.channel_mult,
                           attention_resolutions=cfg.attention_resolutions, num_heads=cfg.num_heads, compute_dtype=compute)
    net.load_state_dict({"_net." + k: v for k, v in sd.items()})
    return net.to(gu.DEV)


def _forward_refs(cfg, sd, x, t):
    """fp64 trace and output, and the fp32 oracle's error against them: (trace64, y64, {tag: e32}, e32 of y)."""
    t64, t32 = {}, {}
    y64 = uo.unet_forward(sd, cfg, x, t, t64, dtype=F64)
    y32 = uo.unet_forward(sd, cfg, x, t, t32)
    assert y64.dtype == F64 and all(v.dtype == F64 for v in t64.values())
    return t64, y64, {k: _rel(t32[k], t64[k]) for k in _blocks(t64)}, _rel(y32, y64)


# ---- the weight edits ------------------------------------------------------------------------------------------------------
def scale_qk(sd, prefix, s, heads):
    """The q and k rows of ``prefix``.qkv (QKVAttentionLegacy, unet.py:436-455: rows [head][q | k | v][ch]) times s."""
    w = sd[prefix + ".qkv.weight"]
    ch = w.shape[0] // (3 * heads)
    qk = (torch.arange(w.shape[0]) % (3 * ch)) < 2 * ch
    sd[prefix + ".qkv.weight"] = torch.where(qk[:, None, None], w * s, w)
    sd[prefix + ".qkv.bias"] = torch.where(qk, sd[prefix + ".qkv.bias"] * s, sd[prefix + ".qkv.bias"])


def isolate_first_attention(sd, tag):
    """The ResBlock in front of the attention block of ``tag`` as an EXACT pass-through in every arithmetic: its second
    convolution 0 (weight and bias), its 1x1x1 skip - where the width changes - a stacked identity (output channel c copies
    input channel c % Cin; products by 1.0 and sums with 0 round nowhere).  The attention block's input is then the previous
    block's output, which fetch_block returns: both sides of a comparison can be given the SAME attention input."""
    p = tag + ".0"
    sd[p + ".out_layers.3.weight"] = torch.zeros_like(sd[p + ".out_layers.3.weight"])
    sd[p + ".out_layers.3.bias"] = torch.zeros_like(sd[p + ".out_layers.3.bias"])
    if p + ".skip_connection.weight" in sd:
        w = torch.zeros_like(sd[p + ".skip_connection.weight"])
        w[torch.arange(w.shape[0]), torch.arange(w.shape[0]) % w.shape[1]] = 1.0
        sd[p + ".skip_connection.weight"] = w
        sd[p + ".skip_connection.bias"] = torch.zeros_like(sd[p + ".skip_connection.bias"])


def attention_prefixes(cfg):
    inputs, middle, outputs, _ = uo.unet_structure(cfg)
    return [b.prefix for layers in inputs + [middle] + outputs for b in layers if b.kind == "attn"]


def offset_biases(sd, d, seed=7):
    """+-d on the bias of every convolution whose output reaches a GroupNorm; one sign per run of Cout / 16 channels."""
    rng = np.random.RandomState(seed)
    n = 0
    for k in sorted(sd):
        if k == "input_blocks.0.0.bias" or k.endswith((".in_layers.2.bias", ".out_layers.3.bias", ".op.bias", ".conv.bias")):
            c = sd[k].shape[0]
            assert c % 16 == 0
            sign = torch.from_numpy(rng.choice([-1.0, 1.0], 16).astype(np.float32)).repeat_interleave(c // 16)
            sd[k] = sd[k] + d * sign
            n += 1
    assert n > 0
    return sd


def saturate_silu(sd, seed=3):
    """beta = -100 on two channels of every GroupNorm that feeds a SiLU (ResBlock in / out norms, the output norm)."""
    rng = np.random.RandomState(seed)
    for k in sorted(sd):
        if k == "out.0.bias" or k.endswith((".in_layers.0.bias", ".out_layers.0.bias")):
            b = sd[k].clone()
            b[torch.from_numpy(rng.choice(b.shape[0], 2, replace=False))] = -100.0
            sd[k] = b
    return sd


def mean_over_std(trace):
    """max over the block outputs and their 32 GroupNorm groups of |group mean| / group std."""
    worst = 0.0
    for tag in _blocks(trace):
        v = trace[tag]
        g = v.reshape(v.shape[0], 32, -1)
        worst = max(worst, float((g.mean(-1).abs() / g.std(-1, unbiased=False)).max()))
    return worst


# ---- A. peaked attention, forward ------------------------------------------------------------------------------------------
NET16 = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                   attention_resolutions=(2,), num_heads=2)     # first attention block input_blocks.3: T = 512, head width 64
NET8 = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                  attention_resolutions=(1, 2), num_heads=2)    # first attention block input_blocks.1: T = 512, head width 32
PEAKED = {"16": (NET16, "input_blocks.3", "input_blocks.2"), "8": (NET8, "input_blocks.1", "input_blocks.0")}
A_BATCH = 2
A_SEED = {"16": 41, "8": 7}  # (weights; the input's seed is one more)


def first_attention_scores(cfg, sd, trace64, tag, prev_tag):
    """exp2-domain scores [N * heads, T queries, T keys] of the first attention block, in float64, from the fp64 trace."""
    sd64 = {k: v.double() for k, v in sd.items()}
    h = uo.res_block(sd64, tag + ".0", trace64[prev_tag], trace64["emb"], F64)
    p = tag + ".1"
    xf = h.reshape(h.shape[0], h.shape[1], -1)
    qkv = F.conv1d(uo.group_norm32(xf, sd64[p + ".norm.weight"], sd64[p + ".norm.bias"], F64), sd64[p + ".qkv.weight"], sd64[p + ".qkv.bias"])
    ch = qkv.shape[1] // (3 * cfg.num_heads)
    q, k, _ = qkv.reshape(qkv.shape[0] * cfg.num_heads, 3 * ch, -1).split(ch, dim=1)
    return torch.einsum("bct,bcs->bts", q, k) / math.sqrt(ch) * math.log2(math.e)


def lazy_flags(scores, ksplit):
    """What flash_attn_bf16v2_kernel's LAZY pass must decide: per (sample * head, key split, 256-query workgroup), whether any
    query's sum over the split's keys of 2^score is outside (2^-100, 2^100).  Returns (bool tensor [B, ksplit, T / 256],
    fraction of the queries that leave the range, the largest |log2 sum| of each workgroup in the same layout)."""
    B, T, _ = scores.shape
    lg = torch.logsumexp(scores.reshape(B, T, ksplit, T // ksplit) * math.log(2.0), dim=-1) / math.log(2.0)  # log2 of the sum
    out = (lg >= 100.0) | (lg <= -100.0)                                                                    # [B, T, ksplit]
    extreme = lg.abs().reshape(B, T // 256, 256, ksplit).max(2).values.permute(0, 2, 1)  # a workgroup's largest |log2 sum|
    return out.reshape(B, T // 256, 256, ksplit).any(2).permute(0, 2, 1), float(out.any(-1).double().mean()), extreme


def _peaked_case(net_id, s, isolated=False):
    """``isolated``: the ResBlock in front of the compared attention block is a pass-through (isolate_first_attention)."""
    def make():
        cfg, tag, prev = PEAKED[net_id]
        from holo_diffusion_amd.weights import synth_state_dict
        sd = synth_state_dict(uo.unet_param_shapes(cfg), A_SEED[net_id])
        for p in attention_prefixes(cfg):
            scale_qk(sd, p, float(s), cfg.num_heads)
        if isolated:
            isolate_first_attention(sd, tag)
        x = torch.from_numpy(np_noise(A_SEED[net_id] + 1, (A_BATCH, 16) + (cfg.image_size,) * 3))
        t = torch.tensor([433, 12], dtype=torch.int64)
        t64, _, e32, _ = _forward_refs(cfg, sd, x, t)
        S = first_attention_scores(cfg, sd, t64, tag, prev)
        top = float(torch.softmax(S * math.log(2.0), -1).max(-1).values.mean())
        print(f"peaked {net_id}{' isolated' if isolated else ''} s={s:g}: scores {float(S.min()):.0f} .. {float(S.max()):.0f}, mean top weight {top:.2f}, "
              f"e32({tag}) {e32[tag]:.1e}")
        return cfg, tag, sd, x, t, t64[tag], e32[tag], S, top
    return _cached(("peaked", net_id, s, isolated), make)


FP32_VARIANTS = {"split-auto": {}, "split-1": {"HOLO_FLASH_SPLIT": "1"}, "split-3": {"HOLO_FLASH_SPLIT": "3"},
                 "gemm-softmax": {"HOLO_NO_FLASH_ATTN": "1"}}
A_FP32 = [("16", v) for v in FP32_VARIANTS] + [("8", "split-auto"), ("8", "split-3")]


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("compute", ["f32", "f32_bf16x3"])
@pytest.mark.parametrize("net_id,variant", A_FP32)
def test_peaked_attention_fp32(gu, net_id, variant, compute, s, monkeypatch, capfd):
    """A, fp32 and f32_bf16x3: the first attention block against fp64 at the fp32 block bound."""
    if net_id == "16":
        _heavy(gu)
    cfg, tag, sd, x, t, ref, e32, S, top = _peaked_case(net_id, s)
    assert e32 < 2.5e-5, e32                      # (the reference alone: the bound below keeps 4x over the conditioning)
    assert top > 0.5 and float(S.max()) > 60.0    # (... and the case IS peaked: a later weight generator cannot defuse it)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    for k, v in FP32_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    net = _make_net(gu, cfg, sd, compute)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    got = net.fetch_block(tag, tuple(ref.shape))
    plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith(f"[plan] attention {tag}.1:")]
    err = _rel(got, ref)
    with capfd.disabled():
        print(f"peaked fp32 {net_id} {variant} {compute} s={s}: block {err:.2e} (e32 {e32:.1e})")
    assert torch.isfinite(got).all() and torch.isfinite(y).all()
    assert err <= 1e-4, err
    if gu.EMU:
        return
    if variant == "gemm-softmax":
        assert not plan, plan
        names = [o["op"] for o in net.time_ops(A_BATCH, 1, gu.DEV)]
        assert names.count("flash_attn") == 0 and names.count("softmax") > 0 and names.count("gemm") > 0, names
    else:
        assert plan and "T=512" in plan[0] and "fp32 flash kernel" in plan[0], plan
        if variant != "split-auto":
            assert plan[0].rstrip().endswith(f"{variant[-1]} key splits"), plan


S_MIXED = 4.7  # (between 4.5 and 5.5: where the flags of the isolated nets below are mixed, with the margin asserted there)
A_BF16 = [("16", 1, 1, "1"), ("16", 1, 2, "1"), ("16", 4, 1, "1"), ("16", 4, 2, "1"), ("16", S_MIXED, 1, "1"), ("16", S_MIXED, 2, "1"),
          ("16", S_MIXED, 1, "0"), ("16", S_MIXED, 2, "0"), ("8", 4, 1, "1"), ("8", S_MIXED, 1, "1"), ("8", S_MIXED, 2, "1"),
          # scores of +-400: a query's maximum moves more than 2^128 past its first key block, so the exact loop (every
          # workgroup is redone by it) must re-reference or overflow; bounded by the format floor only, 2e-2 is no bound here
          ("8", 8, 1, "1"), ("8", 8, 2, "1")]
_BF16_RUNS = {}  # case -> (outputs of the LAZY + fallback run and of the exact loop, fp64 reference, format floor): run once


def _bf(v):
    return v.float().bfloat16().double()


def bf16_attention_own_input(cfg, sd, emb64, tag, xin):
    """The attention block of ``tag`` on the block input ``xin`` (what the kernel itself read: a bf16 tensor), (a) in float64
    and (b) in float64 with nothing but the bf16 mode's ROUNDINGS applied once each - the operands of the qkv convolution
    (normalised input, weight), q * scale, k, v, P, the attention output, proj_out's weight, the stored block.  Returns
    (reference, rel. error of (b) against it): the floor the number format itself puts under any bf16 kernel on this input."""
    sd64 = {k: v.double() for k, v in sd.items()}
    h = uo.res_block(sd64, tag + ".0", xin, emb64, F64)  # (the pass-through ResBlock: h is xin, widened where the skip is)
    p = tag + ".1"
    ref = uo.attention_block(sd64, p, h, cfg.num_heads, F64)
    b, c = h.shape[:2]
    xf = h.reshape(b, c, -1)
    g = _bf(uo.group_norm32(xf, sd64[p + ".norm.weight"], sd64[p + ".norm.bias"], F64))
    qkv = F.conv1d(g, _bf(sd64[p + ".qkv.weight"]), sd64[p + ".qkv.bias"])
    ch = qkv.shape[1] // (3 * cfg.num_heads)
    q, k, v = qkv.reshape(b * cfg.num_heads, 3 * ch, -1).split(ch, dim=1)
    S = torch.einsum("bct,bcs->bts", _bf(q / math.sqrt(ch) * math.log2(math.e)), _bf(k))
    P = torch.exp2(S - S.max(-1, keepdim=True).values)
    a = _bf(torch.einsum("bts,bcs->bct", _bf(P), _bf(v)) / P.sum(-1)[:, None, :]).reshape(b, -1, xf.shape[-1])
    out = _bf(xf + F.conv1d(a, _bf(sd64[p + ".proj_out.weight"]), sd64[p + ".proj_out.bias"]))
    return ref, _rel(out.reshape(ref.shape), ref)


def _bf16_runs(gu, net_id, s, ksplit, fused, monkeypatch, capfd):
    key = (net_id, s, ksplit, fused)
    if key in _BF16_RUNS:
        return _BF16_RUNS[key]
    cfg, tag, sd, x, t, ref, e32, S, top = _peaked_case(net_id, s, True)
    prev = PEAKED[net_id][2]
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    monkeypatch.setenv("HOLO_BF16_FLASH_MIN_T", "256")
    monkeypatch.setenv("HOLO_FLASH_V2_KSPLIT", str(ksplit))
    monkeypatch.setenv("HOLO_CONV_QKV_FUSED", fused)
    outs, xins, checks = {}, {}, []
    for exact in ("", "1"):
        if exact:
            monkeypatch.setenv("HOLO_ATTN_EXACT", "1")
        else:
            monkeypatch.delenv("HOLO_ATTN_EXACT", raising=False)
        capfd.readouterr()
        net = _make_net(gu, cfg, sd, "bf16")
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        outs[exact] = net.fetch_block(tag, tuple(ref.shape)).float().cpu()
        xins[exact] = net.fetch_block(prev, (A_BATCH, cfg.model_channels) + tuple(ref.shape[2:])).float().cpu()
        plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith(f"[plan] attention {tag}.1:")]
        qkv = None if gu.EMU else [o["kernel"] for o in net.time_ops(A_BATCH, 1, gu.DEV)
                                   if o["op"] == "conv" and o["ksz"] == 1 and o["cout"] == 3 * o["cin"] and o["out_dim"] == ref.shape[-1]]
        checks.append((exact, bool(torch.isfinite(outs[exact]).all() and torch.isfinite(y).all()), plan, qkv))
    assert torch.equal(xins[""], xins["1"])  # (both runs read the same block input: everything in front is the same launches)
    emb64 = uo.time_embed({k: v.double() for k, v in sd.items()}, cfg, t, F64)
    own, floor = bf16_attention_own_input(cfg, sd, emb64, tag, xins[""].double())
    _BF16_RUNS[key] = (outs, own, floor, checks)
    return _BF16_RUNS[key]


@pytest.mark.parametrize("net_id,s,ksplit,fused", A_BF16)
def test_peaked_attention_bf16_lazy_against_exact(gu, net_id, s, ksplit, fused, monkeypatch, capfd):
    """A, bf16 storage mode: flash_attn_bf16v2_kernel's LAZY pass + exact fallback and its exact loop alone: the planned
    kernels ran, both are finite, 2^-6 of the block's maximum apart, and each within TWICE the number format's own floor
    (bf16_attention_own_input: every rounding of the mode applied once, in float64) of the float64 block on the kernel's own
    input - a bound that, unlike an expected failure, no wrong maximum, reference or merge can meet.  s = S_MIXED: some
    workgroups keep their LAZY result (reference 0), the others are redone by the exact loop (their own reference), and with
    two key splits attn_combine_kernel merges both kinds for the same query.  The flags are computed here from the fp64
    scores; the kernel decides on bf16-rounded q and k, which move a sum near 2^100 by at most 100 * 2 * 2^-9 = 0.4 in the
    exponent, so no workgroup's extreme may lie in 2^(99 .. 101)."""
    if net_id == "16":
        _heavy(gu)
    cfg, tag, sd, x, t, ref, e32, S, top = _peaked_case(net_id, s, True)
    flags, frac, extreme = lazy_flags(S, ksplit)
    n_flag, n_all = int(flags.sum()), flags.numel()
    with capfd.disabled():
        print(f"peaked bf16 {net_id} s={s} ksplit={ksplit} fused={fused}: {n_flag} of {n_all} workgroups leave the LAZY range "
              f"({100 * frac:.1f} % of the queries); |log2 sum| per workgroup {sorted(round(float(v), 1) for v in extreme.flatten())}")
    assert n_all == A_BATCH * cfg.num_heads * ksplit * 2
    assert not ((extreme > 99.0) & (extreme < 101.0)).any()
    if s == 1:
        assert n_flag == 0
    if s == S_MIXED:
        assert 0 < n_flag < n_all, (n_flag, n_all)
        if ksplit > 1:  # ... also among the splits of one query
            assert (flags.any(1) & ~flags.all(1)).any()
    outs, own, floor, checks = _bf16_runs(gu, net_id, s, ksplit, fused, monkeypatch, capfd)
    for exact, finite, plan, qkv in checks:
        assert finite, exact
        assert plan and "T=512" in plan[0] and "bf16 flash kernel" in plan[0], plan
        assert qkv is None or (qkv and all((k == "conv1x1_qkv_bf16_kernel") == (fused == "1") for k in qkv)), qkv
    d = (outs[""] - outs["1"]).abs().max().item()
    errs = {k: _rel(v, own) for k, v in outs.items()}
    with capfd.disabled():
        print(f"  LAZY + fallback vs exact loop: {d / outs['1'].abs().max().item():.2e} of the block's maximum; against fp64 on the "
              f"kernel's own input: LAZY + fallback {errs['']:.2e}, exact loop {errs['1']:.2e}; format floor {floor:.2e}")
    assert d <= 2.0 ** -6 * outs["1"].abs().max().item()
    assert errs[""] <= 2.0 * floor and errs["1"] <= 2.0 * floor, (errs, floor)


@pytest.mark.parametrize("net_id,s,ksplit,fused", [c for c in A_BF16 if c[0] == "16"])
def test_peaked_attention_bf16_against_f64(gu, net_id, s, ksplit, fused, monkeypatch, capfd):
    """A, bf16 storage mode: the attention block of both runs against the float64 block on the SAME input at the bf16
    bound, 2e-2.  The ResBlock in front is a pass-through (isolate_first_attention), so the kernel's attention input is the
    previous block's output, fetched from the very run and handed to the float64 block.  MI355X: s = 1 3.3e-3, s = 4 1.9e-2
    - and at s = 4.7 3.05e-2, which is to three digits the format floor of bf16_attention_own_input: the bf16 operands of
    conv1x1_qkv_bf16_kernel / flash_attn_bf16v2_kernel (normalised input, q * scale, k, P) cost that much on scores of
    +-120 whatever the kernel does.  Known limit: such a case is reported as an expected failure ONLY while the
    test itself finds the floor above the bound and the kernel within 2x of the floor; any other miss fails."""
    _heavy(gu)
    outs, own, floor, checks = _bf16_runs(gu, net_id, s, ksplit, fused, monkeypatch, capfd)
    assert all(finite for _, finite, _, _ in checks)
    errs = {k: _rel(v, own) for k, v in outs.items()}
    worst = max(errs.values())
    if worst > 2e-2 and floor > 2e-2 and worst <= 2.0 * floor:
        pytest.xfail(f"flash_attn_bf16v2_kernel behind conv1x1_qkv_bf16_kernel, s = {s}: {worst:.2e} of the float64 block on the same "
                     f"input, bound 2e-2; the bf16 roundings alone cost {floor:.2e} there")
    assert errs[""] <= 2e-2 and errs["1"] <= 2e-2, (errs, floor)


# ---- B. peaked attention, backward -----------------------------------------------------------------------------------------
T512_BWD = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                      attention_resolutions=(1,), num_heads=2)  # input_blocks.1.1: the attention backward at T = 512
BWD_NETS = {"wide": (BACKWARD_CFGS["wide"], "middle_block.1"), "T512": (T512_BWD, "input_blocks.1.1")}


def _backward_refs(key, cfg, edit):
    """fp64 autograd (y, grad_x, parameter gradients) of the edited net and the fp32 oracle's errors against it."""
    def make():
        from holo_diffusion_amd.weights import synth_state_dict
        sd = synth_state_dict(uo.unet_param_shapes(cfg), 5)
        edit(sd)
        shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
        x = torch.from_numpy(np_noise(1, shape))
        t = torch.tensor([437], dtype=torch.int64)
        G = torch.from_numpy(np_noise(2, (1, cfg.out_channels) + (cfg.image_size,) * 3))
        y64, gx64, g64 = _oracle_grads(sd, cfg, x, t, G, F64)
        y32, gx32, g32 = _oracle_grads(sd, cfg, x, t, G)
        floor = 1e-2 * float(np.median([g64[k].abs().max().item() for k in sd]))
        e32 = dict(y=_rel(y32, y64), grad_x=_rel(gx32, gx64),
                   params=max((g32[k].double() - g64[k]).abs().max().item() / max(g64[k].abs().max().item(), floor) for k in sd))
        print(f"backward reference {key}: fp32 oracle vs fp64: y {e32['y']:.1e}, grad_x {e32['grad_x']:.1e}, worst parameter {e32['params']:.1e}")
        return sd, x, t, G, y64, gx64, g64, floor, e32
    return _cached(("bwd",) + key, make)


def _backward_vs_f64(gu, cfg, refs, label):
    sd, x, t, G, y64, gx64, g64, floor, e32 = refs
    assert max(e32.values()) <= 1e-4, e32  # (the reference alone: 10x headroom of the 1e-3 below over the conditioning)
    net = _make_net(gu, cfg, sd)
    y, gx, grads = net.backward(x.to(gu.DEV), t.to(gu.DEV), G.to(gu.DEV))
    assert torch.isfinite(y).all() and torch.isfinite(gx).all() and all(torch.isfinite(v).all() for v in grads.values())
    worst = max(((grads[k].cpu().double() - g64[k]).abs().max().item() / max(g64[k].abs().max().item(), floor), k) for k in sd)
    print(f"backward {label}: y {_rel(y, y64):.2e}, grad_x {_rel(gx, gx64):.2e}, worst parameter {worst[0]:.2e} ({worst[1]})")
    _check(y, y64, "forward output", 2e-3)
    _check(gx, gx64, "grad_x")
    assert set(grads) == set(sd)
    for k in sd:
        _check(grads[k], g64[k], k, floor=floor)


@pytest.mark.parametrize("net_id,s", [("wide", 4), ("wide", 6), ("T512", 6)])
def test_peaked_attention_backward(gu, net_id, s):
    """B: one attention block scaled, every gradient against fp64 autograd at the backward bounds."""
    if gu.EMU:
        pytest.skip("backward tests run on the device")
    cfg, prefix = BWD_NETS[net_id]
    refs = _backward_refs(("peaked", net_id, s), cfg, lambda sd: scale_qk(sd, prefix, float(s), cfg.num_heads))
    _backward_vs_f64(gu, cfg, refs, f"peaked {net_id} s={s}")


# ---- C. offset GroupNorm inputs, forward -----------------------------------------------------------------------------------
OFFSET8 = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2, channel_mult=(1, 2),
                     attention_resolutions=(2,), num_heads=2)
OFFSET16 = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                      attention_resolutions=(), num_heads=2)
# 32 channels wide: below 64 output channels the 4^3 level and the Downsample run on conv_igemm_kernel, which writes no statistics
# slabs - the stand-alone gn_stats launch sums the offset tensor, and gn_finalize_kernel merges its records with slab ones
OFFSET_NARROW = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=32, num_res_blocks=1, channel_mult=(1, 1),
                           attention_resolutions=(), num_heads=2)
OFFSET_NETS = {"8": (OFFSET8, 2), "16": (OFFSET16, 1), "narrow": (OFFSET_NARROW, 2)}
# |mean| / std the fp64 trace must reach (measured: see the module docstring)
OFFSET_MIN_RATIO = {3: 5.0, 10: 15.0, 30: 45.0}
FAMILIES = {
    "planner": ({}, None),
    "direct": (DIRECT_ENV, "conv_halo_kernel"),
    "wino2": ({"HOLO_CONV_FORCE_TZ2": "1", "HOLO_CONV_WINO": "2", "HOLO_CONV_WINO3": "0"}, "conv_wino2_kernel"),
    "wino3": ({"HOLO_CONV_FORCE_TZ2": "1", "HOLO_CONV_WINO": "2", "HOLO_CONV_WINO3_MIN_ITEMS": "1"}, "conv_wino3_kernel"),
    "no-skip-fusion": ({"HOLO_NO_SKIP_FUSION": "1"}, None),
}


def _offset_case(net_id, d):
    def make():
        cfg, batch = OFFSET_NETS[net_id]
        from holo_diffusion_amd.weights import synth_state_dict
        sd = offset_biases(synth_state_dict(uo.unet_param_shapes(cfg), 99), float(d))
        x = torch.from_numpy(np_noise(11, (batch, 16) + (cfg.image_size,) * 3))
        t = torch.tensor([321, 17][:batch], dtype=torch.int64)
        t64, y64, e32, ey32 = _forward_refs(cfg, sd, x, t)
        t32 = {}
        uo.unet_forward(sd, cfg, x, t, t32)
        e32s = max(_rel_spread(t32[k], t64[k]) for k in _blocks(t64))
        ratio = mean_over_std(t64)
        print(f"offset {net_id} d={d:g}: |mean| / std up to {ratio:.1f}; fp32 oracle vs fp64: y {ey32:.1e}, worst block {max(e32.values()):.1e}, "
              f"of the block's spread {e32s:.1e}")
        return cfg, batch, sd, x, t, t64, y64, (max(max(e32.values()), ey32), e32s), ratio
    return _cached(("offset", net_id, d), make)


C_CASES = [("8", fam, c) for fam in FAMILIES for c in ("f32", "f32_bf16x3") if not (c == "f32_bf16x3" and fam.startswith("wino"))]
C_CASES += [("16", "planner", "f32"), ("16", "planner", "f32_bf16x3"), ("16", "direct", "f32"), ("narrow", "planner", "f32")]


@pytest.mark.parametrize("d", [3, 10, 30])
@pytest.mark.parametrize("net_id,family,compute", C_CASES)
def test_offset_groupnorm_forward(gu, net_id, family, compute, d, monkeypatch):
    """C: every block output against fp64 at the fp32 block bound while the group means are 5 .. 80 group standard deviations:
    the fp32 (ssum, ssq) slabs of the convolution epilogues, their double records and gn_finalize_kernel's E[x^2] - mean^2.
    (The Winograd families exist in exact fp32 only; bf16 storage is no case - module docstring.)"""
    if net_id == "16":
        _heavy(gu)
    cfg, batch, sd, x, t, t64, y64, (e32, e32s), ratio = _offset_case(net_id, d)
    assert e32 <= 5e-6 and e32s <= 1e-5, (e32, e32s)  # (the reference alone: 10x below the two bounds)
    assert ratio >= OFFSET_MIN_RATIO[d], ratio    # (... and the case really moves the group means)
    env, want = FAMILIES[family]
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = _make_net(gu, cfg, sd, compute)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    got = {tag: net.fetch_block(tag, tuple(t64[tag].shape)).float().cpu() for tag in _blocks(t64)}
    errs = {tag: _rel(got[tag], t64[tag]) for tag in got}
    errs_s = {tag: _rel_spread(got[tag], t64[tag]) for tag in got}
    worst, worst_s = max(errs, key=errs.get), max(errs_s, key=errs_s.get)
    print(f"offset {net_id} {family} {compute} d={d}: y {_rel(y, y64):.2e}, worst block {errs[worst]:.2e} ({worst}), "
          f"of its spread {errs_s[worst_s]:.2e} ({worst_s})")
    assert torch.isfinite(y).all()
    assert _rel(y, y64) <= 1e-4
    for tag in errs:
        assert errs[tag] <= 1e-4, (tag, errs[tag])
    # The offsets are most of a block's maximum (up to 330 at d = 30), which the next GroupNorm removes again: the same bound
    # against what it keeps, the spread.  This is the check an error in rstd cannot hide from.
    for tag in errs_s:
        assert errs_s[tag] <= 1e-4, (tag, errs_s[tag])
    if gu.EMU:
        return
    ops = net.time_ops(batch, 1, gu.DEV)
    convs = [o for o in ops if o["op"] == "conv"]
    kernels = sorted({o["kernel"] for o in convs})
    names = sorted({o["op"] for o in ops})
    print(f"  kernels {kernels}; ops {names}")
    if want is not None and compute == "f32":
        assert want in kernels, kernels
    assert ("gn_stats" in names) == (net_id == "narrow"), names  # (64 channels and up: every chosen kernel writes slabs)
    if family == "direct":
        assert not any(k.startswith("conv_wino") for k in kernels), kernels
    if family == "no-skip-fusion":
        assert not any(o["fused_skip"] for o in convs)
    elif compute == "f32" and net_id == "8":
        assert any(o["fused_skip"] for o in convs)


# ---- D. offset GroupNorm, backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 10])
def test_offset_groupnorm_backward(gu, d):
    """D: gn_bwd_* on the stored float moments of groups whose mean dominates, every gradient against fp64 autograd."""
    if gu.EMU:
        pytest.skip("backward tests run on the device")
    cfg = BACKWARD_CFGS["wide"]
    refs = _backward_refs(("offset", d), cfg, lambda sd: offset_biases(sd, float(d)))
    _backward_vs_f64(gu, cfg, refs, f"offset d={d}")


# ---- E. saturated SiLU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["planner", "direct", "wino3"])
def test_saturated_silu_forward(gu, family, monkeypatch):
    """E, forward: GroupNorm outputs of -100 on two channels per norm (SiLU 0; exp(100) overflows a float) on the direct and
    the three-axis Winograd staging paths: all finite, every block at the fp32 bound."""
    cfg = BACKWARD_CFGS["wide"]

    def make():
        from holo_diffusion_amd.weights import synth_state_dict
        sd = saturate_silu(synth_state_dict(uo.unet_param_shapes(cfg), 99))
        x = torch.from_numpy(np_noise(11, (2, 16, 8, 8, 8)))
        t = torch.tensor([321, 17], dtype=torch.int64)
        return (sd, x, t) + _forward_refs(cfg, sd, x, t)
    sd, x, t, t64, y64, e32, ey32 = _cached(("silu-fwd",), make)
    assert max(max(e32.values()), ey32) <= 5e-6
    env, want = FAMILIES[family]
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = _make_net(gu, cfg, sd)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    assert torch.isfinite(y).all()
    errs = {tag: _rel(net.fetch_block(tag, tuple(t64[tag].shape)), t64[tag]) for tag in _blocks(t64)}
    print(f"saturated SiLU {family}: y {_rel(y, y64):.2e}, worst block {max(errs.values()):.2e}")
    assert _rel(y, y64) <= 1e-4
    for tag in errs:
        assert errs[tag] <= 1e-4, (tag, errs[tag])
    if want is not None and not gu.EMU:
        assert want in {o["kernel"] for o in net.time_ops(2, 1, gu.DEV) if o["op"] == "conv"}


def test_saturated_silu_backward(gu):
    """E, backward: silu_b's derivative at -100 (exp overflows; the derivative is 0): finite, at the backward bounds."""
    if gu.EMU:
        pytest.skip("backward tests run on the device")
    cfg = BACKWARD_CFGS["wide"]
    refs = _backward_refs(("silu",), cfg, saturate_silu)
    _backward_vs_f64(gu, cfg, refs, "saturated SiLU")
