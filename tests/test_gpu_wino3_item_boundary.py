"""conv_wino3_kernel's item boundary - everything an item does outside its chunks: the accumulator reset, the fused-skip
drain, the output transform, residual + bias + GroupNorm statistics, the stores through buffer resources, the step to the
next item of the workgroup's list - on nets of single-ResBlock blocks whose stride-1 convolutions all run on that kernel
(HOLO_CONV_WINO3_MIN_ITEMS=1).

Two checks per net:

* every ResBlock block against the SAME block in float64 on the kernel's own block input, whole volume (so the last tile
  of the tensor, whose offsets are the largest, is inside), at the bounds of
  test_gpu_unet.py::test_three_axis_winograd_vs_float64: below 2e-5 of the block's scale and at most 2x the direct
  kernels' error + 1e-7;
* bit for bit: the SHA-256 of every block output equals the one recorded in tests/golden/wino3_item_boundary.json from the
  build BEFORE the item boundary was rewritten (scripts/make_golden_wino3.py; the record holds the plan it was taken on -
  kernel, split, fused skip of every convolution - and the digests are compared when the device plans the same way; a
  change that alters the kernel's rounding on purpose re-records them).

The rows reach, between them: residual + bias + statistics (every ResBlock's second convolution), split-K (partial sums,
no bias), the fused 1x1x1 skip (output blocks), batch 2, work lists that are no power of two (24^3: 27 tiles, 48^3: 864
tiles, four items per workgroup on 256 CUs) and several items per workgroup (the loop's back edge)."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino3_item_boundary.json")

# row: (image, in_channels, model_channels, channel_mult, batch)
ROWS = {
    # 2 x 256 tiles at 32^3 (two items per workgroup on 256 CUs), 2 x 32 tiles x 2 Cout blocks at 16^3 (split-K); fused skip
    # with one and with two Cout blocks; batch 2
    "32-16-b2": (32, 16, 64, (1, 2), 2),
    # 27 tiles: a short list that is no power of two, split-K at the top level; 12^3 below is not tileable (other kernels)
    "24-12": (24, 16, 64, (1, 2), 1),
    # 864 tiles at 48^3: 216 workgroups x 4 items on 256 CUs; 108 tiles at 24^3
    "48-24": (48, 16, 64, (1, 1), 1),
}
TIMESTEPS = [407, 33]
W3_ENV = {"HOLO_CONV_WINO3_MIN_ITEMS": "1"}
DIRECT_ENV = {"HOLO_CONV_WINO3": "0", "HOLO_CONV_WINO": "0", "HOLO_CONV_WINO_SMALL": "0"}


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _cfg(row):
    image, cin, mc, mult, _ = ROWS[row]
    return uo.UNetCfg(image_size=image, in_channels=cin, out_channels=cin, model_channels=mc, num_res_blocks=1,
                      channel_mult=mult, attention_resolutions=(), num_heads=2)


def _inputs(row):
    image, cin, _, _, batch = ROWS[row]
    x = torch.from_numpy(np_noise(29, (batch, cin, image, image, image)))
    return x, torch.tensor(TIMESTEPS[:batch], dtype=torch.int64)


def _res_block_f64(sd, p, x, emb):
    """ResBlock (scale-shift norm, optional 1x1x1 skip_connection) in float64 end to end, whole volume."""
    import torch.nn.functional as F
    d = {k: v.double() for k, v in sd.items() if k.startswith(p + ".")}
    h = F.silu(F.group_norm(x, 32, d[p + ".in_layers.0.weight"], d[p + ".in_layers.0.bias"], eps=1e-5))
    h = F.conv3d(h, d[p + ".in_layers.2.weight"], d[p + ".in_layers.2.bias"], padding=1)
    e = F.linear(F.silu(emb), d[p + ".emb_layers.1.weight"], d[p + ".emb_layers.1.bias"])[..., None, None, None]
    scale, shift = torch.chunk(e, 2, dim=1)
    h = F.silu(F.group_norm(h, 32, d[p + ".out_layers.0.weight"], d[p + ".out_layers.0.bias"], eps=1e-5) * (1 + scale) + shift)
    y = F.conv3d(h, d[p + ".out_layers.3.weight"], d[p + ".out_layers.3.bias"], padding=1)
    if (p + ".skip_connection.weight") in d:
        x = F.conv3d(x, d[p + ".skip_connection.weight"], d[p + ".skip_connection.bias"])
    return x + y


def run_row(gu, row):
    """One forward of the row's net (the caller has set HOLO_KEEP_INTERMEDIATES=1 and the knobs of W3_ENV or DIRECT_ENV):
    ({tag: block output}, {tag: (ResBlock prefix, block input)} for the single-ResBlock blocks, the net's state dict,
    its convolution ops)."""
    cfg = _cfg(row)
    batch = ROWS[row][4]
    x, t = _inputs(row)
    net, sd = gu.make_unet(cfg, seed=31)
    with torch.no_grad():
        net(x.to(gu.DEV), t.to(gu.DEV))
    inputs, middle, outputs, _ = uo.unet_structure(cfg)
    outs, blocks, size, hs, prev = {}, {}, cfg.image_size, [], None

    def fetch(tag, ch, sz):
        outs[tag] = net.fetch_block(tag, (batch, ch, sz, sz, sz)).float().cpu()
        return outs[tag]

    for i, layers in enumerate(inputs):
        tag = f"input_blocks.{i}"
        if any(b.kind == "down" for b in layers):
            size //= 2
        out = fetch(tag, layers[-1].cout, size)
        if len(layers) == 1 and layers[0].kind == "res":
            blocks[tag] = (layers[0].prefix, prev)
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
            blocks[tag] = (layers[0].prefix, xin)
        size, prev = osize, out
    convs = [] if gu.EMU else [o for o in net.time_ops(batch, 1, gu.DEV) if o["op"] == "conv"]
    return outs, blocks, sd, convs


def plan_of(convs):
    """What a record is valid for: kernel, shape, split and fused skip of every convolution, in execution order."""
    return [[o["kernel"], o["out_dim"], o["cin"], o["cout"], o["ksz"], o["nsplit"], int(o["fused_skip"])] for o in convs]


def digests_of(outs):
    return {tag: hashlib.sha256(o.contiguous().numpy().tobytes()).hexdigest() for tag, o in outs.items()}


def _block_errors(row, outs, blocks, sd):
    cfg = _cfg(row)
    _, t = _inputs(row)
    emb = uo.time_embed(sd, cfg, t).double()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    res = {}
    for tag, (p, xin) in blocks.items():
        ref = _res_block_f64(sd, p, xin.double(), emb)
        d = (outs[tag].double() - ref).abs()
        # (whole volume, and the last tile of the tensor on its own: 2 x 8 x 8 voxels, every channel of the last sample)
        res[tag] = (float(d.max() / ref.abs().max()), float(d[-1, :, -2:, -8:, -8:].max() / ref.abs().max()))
    return res


@pytest.mark.parametrize("row", list(ROWS))
def test_item_boundary_vs_float64_and_recorded_bits(gu, row, monkeypatch):
    if gu.EMU and row != "24-12":
        pytest.skip("not an emulation size")
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    for k, v in W3_ENV.items():
        monkeypatch.setenv(k, v)
    outs, blocks, sd, convs = run_row(gu, row)
    e_w3 = _block_errors(row, outs, blocks, sd)
    for k in W3_ENV:
        monkeypatch.delenv(k)
    for k, v in DIRECT_ENV.items():
        monkeypatch.setenv(k, v)
    outs_d, blocks_d, _, convs_d = run_row(gu, row)
    e_dir = _block_errors(row, outs_d, blocks_d, sd)
    assert e_w3 and set(e_w3) == set(e_dir)
    for tag in e_w3:
        print(f"  {row} {tag}: three-axis Winograd {e_w3[tag][0]:.2e} (last tile {e_w3[tag][1]:.2e}), direct {e_dir[tag][0]:.2e} "
              f"(relative to the block's scale, vs float64)")
    for tag in e_w3:
        assert e_w3[tag][0] < 2e-5 and e_dir[tag][0] < 2e-5, tag
        assert e_w3[tag][0] <= 2.0 * e_dir[tag][0] + 1e-7, tag
    if gu.EMU:
        return
    # the corners the row is there for were reached, on conv_wino3_kernel
    image = ROWS[row][0]
    w3 = [o for o in convs if o["kernel"] == "conv_wino3_kernel"]
    assert not any(o["kernel"].startswith("conv_wino") for o in convs_d), convs_d
    top = [o for o in convs if o["out_dim"] == image and o["ksz"] == 3 and o["cin"] >= 64 and o["cout"] >= 64]
    assert top and all(o["kernel"] == "conv_wino3_kernel" for o in top), top
    assert any(o["fused_skip"] for o in w3), "no fused skip on conv_wino3_kernel"
    print(f"  {row}: {len(w3)} conv_wino3_kernel launches, splits {sorted({o['nsplit'] for o in w3})}, "
          f"{sum(1 for o in w3 if o['fused_skip'])} with a fused skip")
    if row in ("32-16-b2", "24-12"):
        assert any(o["nsplit"] > 1 for o in w3), "no split-K launch of conv_wino3_kernel"
    if row in ("32-16-b2", "48-24"):
        assert any(o["nsplit"] == 1 for o in w3), "no direct (bias / residual / statistics) launch of conv_wino3_kernel"
    # bit for bit against the record
    rec = json.load(open(GOLDEN))[row]
    if rec["plan"] != plan_of(convs):
        print(f"  {row}: this device plans differently from the record ({rec['device']}): digests not compared")
        return
    got = digests_of(outs)
    assert set(got) == set(rec["digests"])
    differing = [tag for tag in got if got[tag] != rec["digests"][tag]]
    assert not differing, f"block outputs differ in bits from the record: {differing}"
