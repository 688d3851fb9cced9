"""Exact-fp32 attention blocks: the key-split flash attention (flash_attn_kernel + flash_attn_merge_kernel) and the
small-grid 1x1x1 convolution of the qkv / proj_out launches (conv1x1_small_kernel), against the pinned oracle block by
block - reference guided_diffusion/unet.py:300-306 (qkv = qkv(norm(x)), QKVAttentionLegacy, x + proj_out(h))."""
import pytest
import torch

from oracle import unet_oracle as uo

pytestmark = pytest.mark.gpu


def _heavy(gu):  # (the host emulation takes tens of minutes per 16^3 net; the reject case below is small enough)
    if gu.EMU:
        pytest.skip("too large for the host emulation")


@pytest.fixture
def gu():
    from tests import gpu_utils
    return gpu_utils


def _blocks(net, trace):
    tags = [tag for tag in trace if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block"]
    return {tag: net.fetch_block(tag, tuple(trace[tag].shape)).float().cpu() for tag in tags}


def _forward(gu, cfg, batch, seed):
    from oracle.common import np_noise
    net, sd = gu.make_unet(cfg, seed=seed)
    x = torch.from_numpy(np_noise(seed + 1, (batch, 16, cfg.image_size, cfg.image_size, cfg.image_size)))
    t = torch.tensor([433, 12][:batch], dtype=torch.int64)
    trace = {}
    ref = uo.unet_forward(sd, cfg, x, t, trace)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV)).float().cpu()
    return net, y, ref, trace


# (T, head channels): 512 tokens of 128 channels (the 8^3 level of the north-star net), 4096 of 64 (its 16^3 level)
CASES = {
    "T512_ch128": dict(image=16, mc=128, mult=(1, 2), attn=(2,), batch=1),
    "T4096_ch64": dict(image=16, mc=128, mult=(1,), attn=(1,), batch=1),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("split", ["", "1", "3"])  # planner's choice, un-split, three splits (12 waves: T/32 does not divide)
def test_split_key_flash_attention_vs_oracle(gu, case, split, monkeypatch):
    _heavy(gu)
    c = CASES[case]
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    if split:
        monkeypatch.setenv("HOLO_FLASH_SPLIT", split)
    cfg = uo.UNetCfg(image_size=c["image"], in_channels=16, out_channels=16, model_channels=c["mc"], num_res_blocks=1,
                     channel_mult=c["mult"], attention_resolutions=c["attn"], num_heads=2)
    net, y, ref, trace = _forward(gu, cfg, c["batch"], seed=41)
    assert gu.rel_err(y, ref) < 1e-4
    got = _blocks(net, trace)
    for tag, r in got.items():
        assert gu.rel_err(r, trace[tag]) < 1e-4, tag
    with torch.no_grad():  # the merge runs in a fixed order: a second forward is bit-identical
        from oracle.common import np_noise
        x = torch.from_numpy(np_noise(42, (c["batch"], 16, c["image"], c["image"], c["image"])))
        y2 = net(x.to(gu.DEV), torch.tensor([433, 12][:c["batch"]], dtype=torch.int64).to(gu.DEV)).float().cpu()
    assert torch.equal(y, y2)


def test_split_key_flash_attention_matches_unsplit(gu, monkeypatch):
    """Two samples, T = 512: the three- and four-way splits agree with the un-split kernel up to fp32 reassociation."""
    _heavy(gu)
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=1,
                     channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2)
    ys = {}
    for split in ("1", "3", "4"):
        monkeypatch.setenv("HOLO_FLASH_SPLIT", split)
        _, ys[split], ref, _ = _forward(gu, cfg, 2, seed=5)
        assert gu.rel_err(ys[split], ref) < 1e-4, split
    assert gu.rel_err(ys["3"], ys["1"]) < 1e-5 and gu.rel_err(ys["4"], ys["1"]) < 1e-5


@pytest.mark.parametrize("mc,batch", [(64, 2), (128, 1)])
def test_small_1x1_convolution_blockwise(gu, mc, batch, monkeypatch):
    """The attention's qkv (GroupNorm affine on load, no residual) and proj_out (bias + residual x + GroupNorm slabs of the
    block output, consumed by the next block) on conv1x1_small_kernel at 16^3 and 8^3 (K = 64 .. 256: one or two chunks per
    wave, and waves without a chunk), against the oracle and against the row-tile kernel on the same net."""
    _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = uo.UNetCfg(image_size=16, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=1,
                     channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2)
    outs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("HOLO_CONV1X1_SMALL", knob)
        net, y, ref, trace = _forward(gu, cfg, batch, seed=17)
        assert gu.rel_err(y, ref) < 1e-4, knob
        outs[knob] = _blocks(net, trace)
        for tag, r in outs[knob].items():
            assert gu.rel_err(r, trace[tag]) < 1e-4, (knob, tag)
        if not gu.EMU:
            conv1 = [o for o in net.time_ops(batch, 1, gu.DEV) if o["op"] == "conv" and o["ksz"] == 1]
            attn1 = [o for o in conv1 if o["cout"] in (o["cin"], 3 * o["cin"])]  # (a skip connection changes the width)
            desc = [(o["kernel"], o["cin"], o["cout"], o["out_dim"]) for o in conv1]
            assert len(attn1) == 2 * 7, desc  # 7 attention blocks: 2 on the way down, the middle one, 4 on the way up
            want = "conv1x1_small_kernel" if knob == "1" else "conv_small_kernel"
            assert all(o["kernel"] == want for o in attn1), desc
            assert not any(o["kernel"] == "conv1x1_small_kernel" for o in conv1 if o not in attn1), desc
    for tag in outs["0"]:
        assert gu.rel_err(outs["1"][tag], outs["0"][tag]) < 1e-5, tag


@pytest.mark.parametrize("mc,mult", [(96, (1,)), (128, (1, 4))])
def test_small_1x1_convolution_rejects_unsupported_widths(gu, mc, mult, monkeypatch):
    """Attention blocks the small-grid kernel does not instantiate: 96 channels (288 / 96 output channels, not a multiple of
    64) and 512 channels at 4^3 (K above 256): the planner keeps the row-tile kernel, and the block outputs still match the
    oracle."""
    if mc > 96:
        _heavy(gu)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    cfg = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=1,
                     channel_mult=mult, attention_resolutions=(len(mult),), num_heads=2)
    net, y, ref, trace = _forward(gu, cfg, 1, seed=3)
    assert gu.rel_err(y, ref) < 1e-4
    for tag, r in _blocks(net, trace).items():
        assert gu.rel_err(r, trace[tag]) < 1e-4, tag
    if not gu.EMU:
        conv1 = [o for o in net.time_ops(1, 1, gu.DEV) if o["op"] == "conv" and o["ksz"] == 1 and o["cout"] in (o["cin"], 3 * o["cin"])]
        assert conv1 and all(o["kernel"] == "conv_small_kernel" for o in conv1), [(o["kernel"], o["cin"], o["cout"]) for o in conv1]
