"""conv_wino3_kernel's upsampling form (conv_wino3_up_kernel, kernels_conv3.hip): an Upsample convolution - nearest x2 on
load, raw input, no fused skip - runs the 27 of the 64 pseudo-taps whose A operands are not identically zero.  Only
additions of exact zeros are left out, so every bit of the result must be what the generic form (HOLO_CONV_WINO3_UP=0)
writes.

Nets of single-ResBlock blocks as in test_gpu_wino3_item_boundary.py, HOLO_CONV_WINO3_MIN_ITEMS=1 (the three-axis kernel
on work lists far below one item per CU) and HOLO_KEEP_INTERMEDIATES=1.  Every case checks:

* every block output with the knob at its default is torch.equal to the output with HOLO_CONV_WINO3_UP=0;
* both are within rel_err < 1e-4 of the oracle (the bound of the neighbouring block tests, test_gpu_unet.py);
* time_ops shows the Upsample convolution as conv_wino3_kernel with flops_executed == flops / 8 at the default (27 pseudo-
  taps per 8 outputs) and flops * 8 / 27 with the knob at 0 (64 per 8).

Cases (the Upsample convolution of the net; its plan on a 256-CU device):
  8from4     128 -> 128 at 8^3 from 4^3: four tiles, every tile on every y / x border; split-K, partial stores, no bias
  16         64 -> 64 at 16^3: two chunks.  (Un-split only on a device of at most 32 CUs - 32 items; on 256 CUs split-K 2:
             the un-split launch with two chunks is row 32-64ch.)
  24from12   64 -> 64 at 24^3 from 12^3: 27 tiles, a work list that is no power of two
  16-b2      128 -> 128 at 16^3, batch 2: two chunks per split
  96ch       96 -> 96 at 16^3: three chunks - but 96 output channels are no multiple of the kernel's 64-channel blocks, so
             conv_plan keeps this convolution OFF conv_wino3_kernel whatever the knob says; the row checks that (and the two
             equalities, which then hold between two runs of another kernel).  Three chunks per split ON the kernel: row
             192ch-b2.
  192ch-b2   192 -> 192 at 16^3, batch 2: six chunks, three Cout blocks, split-K 2 x three chunks
  32-64ch    64 -> 64 at 32^3: 256 items, one per CU - un-split with two chunks: bias and statistics records behind a
             two-stage item
  32         128 -> 128 at 32^3: 512 items on 256 CUs - a workgroup runs two items (the loop's back edge, the first-stage
             copy after an epilogue); un-split with four chunks: bias and statistics records
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

# row: (image, model_channels, channel_mult, batch)
ROWS = {
    "8from4": (8, 64, (1, 2), 1),
    "16": (16, 64, (1, 1), 1),
    "24from12": (24, 64, (1, 1), 1),
    "16-b2": (16, 64, (1, 2), 2),
    "96ch": (16, 32, (1, 3), 1),
    "192ch-b2": (16, 64, (1, 3), 2),
    "32-64ch": (32, 64, (1, 1), 1),
    "32": (32, 64, (1, 2), 1),
}
EMU_ROWS = ("8from4", "16")
TIMESTEPS = [407, 33]
CIN = 16


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _cfg(row):
    image, mc, mult, _ = ROWS[row]
    return uo.UNetCfg(image_size=image, in_channels=CIN, out_channels=CIN, model_channels=mc, num_res_blocks=1,
                      channel_mult=mult, attention_resolutions=(), num_heads=2)


def _run(gu, cfg, x, t, shapes):
    """One forward on a fresh net (the knobs are read when its plan is made): ({tag: block output}, its convolution ops)."""
    net, _ = gu.make_unet(cfg, seed=31)
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV)).float().cpu()
    outs = {tag: net.fetch_block(tag, shape).float().cpu() for tag, shape in shapes.items()}
    outs["out"] = y
    # (time_ops runs its own forward on random data: only after the block outputs of OUR forward have been read)
    convs = [] if gu.EMU else [o for o in net.time_ops(x.shape[0], 1, gu.DEV) if o["op"] == "conv"]
    return outs, convs


@pytest.mark.parametrize("row", list(ROWS))
def test_upsampling_form_equals_generic_form_and_oracle(gu, row, monkeypatch):
    if gu.EMU and row not in EMU_ROWS:
        pytest.skip("not an emulation size")
    image, mc, mult, batch = ROWS[row]
    cfg = _cfg(row)
    _, sd = gu.make_unet(cfg, seed=31)
    x = torch.from_numpy(np_noise(29, (batch, CIN, image, image, image)))
    t = torch.tensor(TIMESTEPS[:batch], dtype=torch.int64)
    trace = {}
    ref = uo.unet_forward(sd, cfg, x, t, trace)  # once: shared by both runs, never written
    refs = {tag: r for tag, r in trace.items() if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block"}
    refs["out"] = ref
    shapes = {tag: tuple(r.shape) for tag, r in refs.items() if tag != "out"}
    up_tags = [f"output_blocks.{i}" for i, layers in enumerate(uo.unet_structure(cfg)[2]) if any(b.kind == "up" for b in layers)]
    assert up_tags, "the net has no Upsample block"

    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_CONV_WINO3_MIN_ITEMS", "1")
    monkeypatch.delenv("HOLO_CONV_WINO3_UP", raising=False)
    outs_up, convs_up = _run(gu, cfg, x, t, shapes)
    monkeypatch.setenv("HOLO_CONV_WINO3_UP", "0")
    outs_gen, convs_gen = _run(gu, cfg, x, t, shapes)

    assert set(outs_up) == set(outs_gen) == set(refs)
    for tag in refs:
        e_up, e_gen = gu.rel_err(outs_up[tag], refs[tag]), gu.rel_err(outs_gen[tag], refs[tag])
        same = torch.equal(outs_up[tag], outs_gen[tag])
        if tag in up_tags or tag == "out" or not same:
            print(f"  {row} {tag}: vs oracle {e_up:.2e} (upsampling form) {e_gen:.2e} (generic form), bit-equal {same}")
        assert same, f"{tag}: the upsampling form differs in bits from the generic form"
        assert e_up < 1e-4 and e_gen < 1e-4, tag
    if gu.EMU:
        return

    ch = int(mc * mult[-1])
    ups_up = [o for o in convs_up if o["upsample"]]
    ups_gen = [o for o in convs_gen if o["upsample"]]
    assert len(ups_up) == len(ups_gen) == len(up_tags)
    for a, b in zip(ups_up, ups_gen):
        print(f"  {row}: Upsample conv {a['cin']} -> {a['cout']} at {a['out_dim']}^3: {a['kernel']}, split-K {a['nsplit']}, "
              f"executed/algorithmic flops {a['flops_executed'] / a['flops']:.4f} (default) {b['flops_executed'] / b['flops']:.4f} (knob 0)")
        assert a["cin"] == a["cout"] == ch and a["ksz"] == 3 and a["flops"] == b["flops"] and a["nsplit"] == b["nsplit"]
        if ch % 64:
            # no multiple of the kernel's 64-channel output blocks: not its launch, with or without the knob
            assert a["kernel"] == b["kernel"] and a["kernel"] != "conv_wino3_kernel", (a, b)
            assert a["flops_executed"] == b["flops_executed"]
            continue
        assert a["kernel"] == "conv_wino3_kernel" and b["kernel"] == "conv_wino3_kernel", (a, b)
        assert a["flops_executed"] == a["flops"] / 8, a                # 27 pseudo-taps per 2 x 2 x 2 outputs of 27 taps each
        assert b["flops_executed"] * 27 == b["flops"] * 8, b           # 64 per 2 x 2 x 2 outputs: flops * 8 / 27
    if row in ("32-64ch", "32"):
        assert all(o["nsplit"] == 1 for o in ups_up), "the 32^3 rows are there for the un-split epilogue"
    if row in ("8from4", "16-b2", "192ch-b2"):
        assert all(o["nsplit"] > 1 for o in ups_up), "no split-K launch of the upsampling form"
