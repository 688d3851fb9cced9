"""The side lane of the exact-fp32 inference plan: the first convolution of an up-path ResBlock over the virtual concat
[h | encoder skip] is split at the seam where no GroupNorm group straddles it - the skip half (its own gn_finalize + a direct
conv_wino3_kernel launch into a partial tensor P) runs on a second stream from the fork in the descent on, the ResBlock then
launches the h half with P as its residual (HOLO_SIDE_LANE_CUS / _MIN_R / _FORK_R; Planner::plan_side_lane).

The net: three levels (16^3, 8^3, 4^3), one ResBlock per level, no attention, channel_mult (1, 1, 2), 64 model channels.  (The
three-axis Winograd kernel takes 64-channel output blocks only, so 64 and not 32 model channels: the 16^3 and 8^3 concat
convolutions are then 64 + 64 -> 64, 4 channels per group.)  The level-edge knobs are lowered to 8 (split) and 4 (fork), and
HOLO_CONV_FORCE_TZ2 / HOLO_CONV_WINO3_MIN_ITEMS put the small grids on conv_wino3_kernel as the other small-grid tests do.
Up-path concat convolutions of the net, in order: (128 + 128) and (128 + 64) at 4^3 (below the minimum edge), (128 + 64) -> 64 at
8^3 (192 channels, 6 per group: 128 is no multiple of 6, the group at the seam straddles it - never split), (64 + 64) -> 64 at
8^3 and twice at 16^3 (split).

Bounds: split against unsplit below 1e-5 relative, the bound test_gpu_unet.py holds the fused and the unfused skip forms to;
each form within 1e-4 of the oracle block by block (the per-op tolerance of every blockwise test); repeated forwards and rows of
a batch-invariant batch bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

from tests.test_gpu_cu_counts import _cu, cu  # noqa: E402,F401  (the fixture: a context that plans for that many CUs)

from tests import gpu_utils as _g  # noqa: E402

# (the host emulation runs the 8^3 / 4^3 end of the same net: two (64 + 64) -> 64 convolutions at 8^3 split, seconds instead of
# the better part of an hour)
CFG = uo.UNetCfg(image_size=8 if _g.EMU else 16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1,
                 channel_mult=(1, 1) if _g.EMU else (1, 1, 2), attention_resolutions=(), num_heads=2)
SMALL_GRID_ENV = {"HOLO_CONV_FORCE_TZ2": "1", "HOLO_CONV_WINO3_MIN_ITEMS": "1"}
SPLIT_ENV = {"HOLO_SIDE_LANE_CUS": "4", "HOLO_SIDE_LANE_MIN_R": "8", "HOLO_SIDE_LANE_FORK_R": "4"}
SEED = 83


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _inputs(batch, seed=41):
    x = torch.from_numpy(np_noise(seed, (batch, 16) + (CFG.image_size,) * 3))
    return x, torch.tensor([611, 3, 250][:batch], dtype=torch.int64)


@pytest.fixture(scope="module")
def oracle_b1():
    """The oracle's forward of the batch-1 input, block by block: computed once, shared, never modified."""
    from holo_diffusion_amd.weights import synth_state_dict
    sd = synth_state_dict(uo.unet_param_shapes(CFG), SEED)
    x, t = _inputs(1)
    trace = {}
    ref = uo.unet_forward(sd, CFG, x, t, trace)
    return ref, trace


def _set(monkeypatch, split):
    env = dict(SMALL_GRID_ENV)
    env.update(SPLIT_ENV)
    if not split:
        env["HOLO_SIDE_LANE_CUS"] = "0"
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _conv_ops(gu, net, batch=1):
    return [o for o in net.time_ops(batch, 1, gu.DEV) if o["op"] == "conv"]


def _both_forms_vs_oracle(gu, monkeypatch, oracle_b1, own=lambda net: net, what=""):
    ref, trace = oracle_b1
    x, t = _inputs(1)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    ys = {}
    for split in (True, False):
        _set(monkeypatch, split)
        net = own(gu.make_unet(CFG, seed=SEED)[0])
        with torch.no_grad():
            y = net(x.to(gu.DEV), t.to(gu.DEV))
        e = gu.rel_err(y, ref)
        print(f"  {'split' if split else 'unsplit'} {what}: output vs oracle {e:.2e}")
        assert e < 1e-4
        gu.block_outputs_vs_oracle(net, trace, 1e-4, "split" if split else "unsplit")
        ys[split] = y.cpu()
        if not gu.EMU:  # the knobs really split / really do not
            whole = [o for o in _conv_ops(gu, net) if o["ksz"] == 3 and o["cin"] == 128 and o["cout"] == 64 and o["out_dim"] >= 8]
            assert (len(whole) == 0) == split and len(whole) in (0, 3), [(o["out_dim"], o["cin"]) for o in whole]
            assert all(o["kernel"] == "conv_wino3_kernel" for o in whole)
    d = gu.rel_err(ys[True], ys[False])
    print(f"  split vs unsplit {what}: {d:.2e}")
    assert d < 1e-5
    return ys


def test_split_vs_unsplit_and_oracle(gu, monkeypatch, oracle_b1):
    """Split and unsplit plans of the same weights and input: within 1e-5 of each other, each within 1e-4 of the oracle block
    by block.  (Also under the emulation build, where both lanes are the caller's stream.)"""
    _both_forms_vs_oracle(gu, monkeypatch, oracle_b1)


@_cu(8, 20, 32)
def test_split_vs_unsplit_under_small_cu_counts(cu, gu, monkeypatch, oracle_b1):
    """The same with the context planning for 8, 20 and 32 CUs (the main half then runs un-split at 16^3), side CU count 4."""
    if gu.EMU:
        pytest.skip("the emulation runs the first and the batch-invariant case")
    _both_forms_vs_oracle(gu, monkeypatch, oracle_b1, own=cu.own, what=f"{cu.n} CUs")


def test_bit_reproducible_and_back_to_back(gu, monkeypatch):
    """Two forwards of the split plan are bit-equal; ten back-to-back forwards with alternating inputs equal the same inputs
    run one at a time with a synchronize between them (a side op of call k racing the start of call k + 1 would show)."""
    _set(monkeypatch, True)
    net, _ = gu.make_unet(CFG, seed=SEED)
    xa, ta = (a.to(gu.DEV) for a in _inputs(1, 41))
    xb, tb = (a.to(gu.DEV) for a in _inputs(1, 42))
    tb = tb + 100
    with torch.no_grad():
        ya = net(xa, ta).clone()
        torch.cuda.synchronize()
        assert torch.equal(net(xa, ta), ya)
        torch.cuda.synchronize()
        yb = net(xb, tb).clone()
        torch.cuda.synchronize()
        assert not torch.equal(ya, yb)
        outs = [net(*((xa, ta) if k % 2 == 0 else (xb, tb))).clone() for k in range(10)]  # no synchronize in between
        torch.cuda.synchronize()
    for k, y in enumerate(outs):
        assert torch.equal(y, ya if k % 2 == 0 else yb), k


def test_batch_invariant_rows_equal_batch1(gu, monkeypatch):
    """Batch 2 under the invariant plan: the sum is split where the batch-1 plan splits it, each row is bit-equal to its
    batch-1 forward.  (Also under the emulation build.)"""
    _set(monkeypatch, True)
    net, _ = gu.make_unet(CFG, seed=SEED)
    net.set_batch_invariant(True)
    x, t = (a.to(gu.DEV) for a in _inputs(2))
    with torch.no_grad():
        yb = net(x, t).clone()
        rows = [net(x[b:b + 1], t[b:b + 1]).clone() for b in range(2)]
    for b in range(2):
        assert torch.equal(yb[b:b + 1], rows[b]), b
    if not gu.EMU:
        assert len([o for o in _conv_ops(gu, net, 2) if o["ksz"] == 3 and o["cin"] == 128 and o["cout"] == 64]) == 0


def _shape(ops):
    return [(o["kernel"], o["out_dim"], o["cin"], o["cout"], o["ksz"], o["nsplit"], int(o["fused_skip"])) for o in ops]


def test_plan_shape(gu, monkeypatch):
    """time_ops (the plan run serially): each of the three eligible blocks shows a side launch (cin == C1 == 64, un-split) in
    front of the deep levels and a main launch (cin == C0 == 64), both on conv_wino3_kernel; the (128 + 64) block at 8^3 keeps
    its single 192-channel launch; with HOLO_SIDE_LANE_CUS=0 the list is the unsplit plan's: the same launches but for the
    three 128-channel ones in place of the six halves, and two ops per split fewer (the skip half's gn_finalize and launch)."""
    if gu.EMU:
        pytest.skip("time_ops needs device events")
    _set(monkeypatch, True)
    net, _ = gu.make_unet(CFG, seed=SEED)
    all_split = net.time_ops(1, 1, gu.DEV)
    split = [o for o in all_split if o["op"] == "conv"]
    _set(monkeypatch, False)
    net0, _ = gu.make_unet(CFG, seed=SEED)
    all_whole = net0.time_ops(1, 1, gu.DEV)
    whole = [o for o in all_whole if o["op"] == "conv"]
    monkeypatch.setenv("HOLO_SIDE_LANE_CUS", "4")
    monkeypatch.setenv("HOLO_SIDE_LANE_MIN_R", "1000")  # the other way to split nothing: the same plan
    net1, _ = gu.make_unet(CFG, seed=SEED)
    assert _shape([o for o in net1.time_ops(1, 1, gu.DEV) if o["op"] == "conv"]) == _shape(whole)
    assert len(all_split) == len(all_whole) + 6 and len(split) == len(whole) + 3

    def first_convs(ops):  # 3x3x3 launches into 64 channels over 64, 128 or 192 input channels at 8^3 and 16^3
        return [o for o in ops if o["ksz"] == 3 and o["cout"] == 64 and o["out_dim"] in (8, 16) and not o["upsample"]]

    # the whole plan: one 192-channel and one 128-channel launch at 8^3, two 128-channel launches at 16^3
    w128 = [o for o in first_convs(whole) if o["cin"] == 128]
    assert [o["out_dim"] for o in w128] == [8, 16, 16] and all(o["kernel"] == "conv_wino3_kernel" for o in w128)
    for ops in (whole, split):
        w192 = [o for o in ops if o["ksz"] == 3 and o["cin"] == 192 and o["cout"] == 64]  # (not the (128 + 64) -> 128 at 4^3)
        assert [(o["out_dim"], o["cout"]) for o in w192] == [(8, 64)], _shape(ops)
    assert not [o for o in split if o["ksz"] == 3 and o["cin"] == 128 and o["cout"] == 64]
    # the side launches stand together, in consumption order, in front of the first 4^3 launch; everything else is the
    # unsplit plan with the 128-channel launches turned into 64-channel ones (the main half may be split-K, the side never)
    k = next(i for i, o in enumerate(split) if o["out_dim"] == 4)
    side = split[k - 3:k]
    assert [(o["out_dim"], o["cin"], o["cout"], o["ksz"], o["nsplit"], o["kernel"]) for o in side] == \
        [(r, 64, 64, 3, 1, "conv_wino3_kernel") for r in (8, 16, 16)], _shape(split)
    rest = split[:k - 3] + split[k:]
    assert len(rest) == len(whole)
    for a, b in zip(rest, whole):
        if b in w128:
            assert (a["kernel"], a["out_dim"], a["cin"], a["cout"], a["ksz"]) == ("conv_wino3_kernel", b["out_dim"], 64, 64, 3)
        else:
            assert _shape([a]) == _shape([b])
