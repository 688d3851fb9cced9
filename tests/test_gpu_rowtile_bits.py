"""conv_small_kernel (the row-tile convolution) on nets of single-ResBlock blocks whose deep levels all run on it, with the
Winograd forms switched off (HOLO_CONV_WINO3=0 HOLO_CONV_WINO=0 HOLO_CONV_WINO_SMALL=0; HOLO_CONV1X1_SMALL=0 where the net has
attention).

Per net:

* every block output against the oracle at rel_err < 1e-4, as tests/test_gpu_attention_fp32.py does (the bf16 net: at the
  bf16 tolerance of tests/test_gpu_unet.py, 2e-2 of the tensor's scale - SURVEY.md 8c; bf16 products cannot meet 1e-4);
* the convolutions the net is there for ran on conv_small_kernel (time_ops);
* bit for bit: the SHA-256 of every block output equals the one recorded in tests/golden/rowtile_bits.json from the build
  BEFORE the kernel's staging was rewritten (scripts/make_golden_rowtile.py; the record holds the plan it was taken on -
  kernel, shape, split and fused skip of every convolution - and the digests are compared when the device plans the same
  way; a change that alters the kernel's rounding on purpose re-records them).

What the nets reach:

  8-b1     8^3, 64 channels, channel_mult (1, 2, 4), batch 1: the stride-2 launches 8^3 -> 4^3 and 4^3 -> 2^3 (raw input),
           activated 3x3x3 convolutions at 4^3 and 2^3 with split-K, the fused 1x1x1 skip chunks on the way up, a two-source
           concat, an Upsample convolution on the kernel
  8-b3     the same net, batch 3: 2^3 has 24 rows, so a tile straddles samples and ends short of 64 rows
  16-attn  16^3, 32 channels, channel_mult (1, 2), attention at the 8^3 level: the 1x1x1 qkv / proj_out with the affine but no
           SiLU, un-split with statistics in the epilogue
  8-bf16   the first net in compute_dtype "bf16": the kernel's bf16 instances

test_silu_division_all_inputs runs the kernel's SiLU (rowtile_silu.h: a shortened division wherever a wave's values are in
range, the IEEE sequence elsewhere) against the plain expression on all 2^32 inputs: tools/silu_div_check.cpp."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "rowtile_bits.json")

# row: (image, model_channels, channel_mult, attention_resolutions, batch, compute_dtype, oracle tolerance)
ROWS = {
    "8-b1": (8, 64, (1, 2, 4), (), 1, "f32", 1e-4),
    "8-b3": (8, 64, (1, 2, 4), (), 3, "f32", 1e-4),
    "16-attn": (16, 32, (1, 2), (2,), 1, "f32", 1e-4),
    "8-bf16": (8, 64, (1, 2, 4), (), 1, "bf16", 2e-2),
}
TIMESTEPS = [433, 12, 871]
DIRECT_ENV = {"HOLO_CONV_WINO3": "0", "HOLO_CONV_WINO": "0", "HOLO_CONV_WINO_SMALL": "0", "HOLO_CONV1X1_SMALL": "0",
              "HOLO_KEEP_INTERMEDIATES": "1"}
ROWTILE = "conv_small_kernel"


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _cfg(row):
    image, mc, mult, attn, _, _, _ = ROWS[row]
    return uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=1,
                      channel_mult=mult, attention_resolutions=attn, num_heads=2)


def run_row(gu, row):
    """One forward of the row's net (the caller has set DIRECT_ENV): ({tag: block output}, the oracle's trace of the same
    forward, the net's convolution ops)."""
    image, _, _, _, batch, compute, _ = ROWS[row]
    cfg = _cfg(row)
    net, sd = gu.make_unet(cfg, seed=23, compute_dtype=compute)
    x = torch.from_numpy(np_noise(24, (batch, 16, image, image, image)))
    t = torch.tensor(TIMESTEPS[:batch], dtype=torch.int64)
    trace = {}
    uo.unet_forward(sd, cfg, x, t, trace)
    with torch.no_grad():
        net(x.to(gu.DEV), t.to(gu.DEV))
    tags = [tag for tag in trace if tag.startswith(("input_blocks", "output_blocks")) or tag == "middle_block"]
    outs = {tag: net.fetch_block(tag, tuple(trace[tag].shape)).float().cpu() for tag in tags}
    convs = [] if gu.EMU else [o for o in net.time_ops(batch, 1, gu.DEV) if o["op"] == "conv"]
    return outs, trace, convs


def plan_of(convs):
    """What a record is valid for: kernel, shape, split and fused skip of every convolution, in execution order."""
    return [[o["kernel"], o["out_dim"], o["cin"], o["cout"], o["ksz"], o["stride"], int(o["upsample"]), o["nsplit"],
             int(o["fused_skip"])] for o in convs]


def digests_of(outs):
    return {tag: hashlib.sha256(o.contiguous().numpy().tobytes()).hexdigest() for tag, o in outs.items()}


def _reached(row, convs):
    """The convolutions the row is there for ran on the row-tile kernel."""
    desc = [(o["kernel"], o["out_dim"], o["cin"], o["cout"], o["ksz"], o["stride"], o["upsample"], o["nsplit"], o["fused_skip"])
            for o in convs]
    on = [o for o in convs if o["kernel"] == ROWTILE]
    assert on, desc
    if ROWS[row][5] == "bf16":  # (the bf16 mode has kernels of its own for some of these shapes: the row-tile ones are in `on`)
        return
    assert not any(o["kernel"].startswith("conv_wino") or o["kernel"] == "conv1x1_small_kernel" for o in convs), desc
    if row == "16-attn":
        attn1 = [o for o in convs if o["ksz"] == 1 and o["cout"] in (o["cin"], 3 * o["cin"])]
        assert len(attn1) == 2 * 4, desc  # four attention blocks at 8^3: one on the way down, the middle one, two on the way up
        assert all(o["kernel"] == ROWTILE and o["nsplit"] == 1 and o["out_dim"] == 8 for o in attn1), desc
        return
    down = [o for o in convs if o["stride"] == 2]
    assert sorted(o["out_dim"] for o in down) == [2, 4] and all(o["kernel"] == ROWTILE for o in down), desc
    deep = [o for o in convs if o["ksz"] == 3 and o["stride"] == 1 and not o["upsample"] and o["out_dim"] in (2, 4)]
    assert deep and all(o["kernel"] == ROWTILE for o in deep), desc
    assert {o["out_dim"] for o in deep} == {2, 4}, desc
    assert any(o["nsplit"] > 1 for o in deep), "no split-K launch at the deep levels"
    assert any(o["fused_skip"] for o in on), "no fused skip on the row-tile kernel"
    assert any(o["upsample"] for o in on), "no Upsample convolution on the row-tile kernel"
    # the way up reads a two-source concat: a deep convolution wider on the input side than any block output of its level
    assert any(o["cin"] > o["cout"] for o in deep), "no concat input at the deep levels"


@pytest.mark.parametrize("row", list(ROWS))
def test_rowtile_vs_oracle_and_recorded_bits(gu, row, monkeypatch):
    if gu.EMU and row == "16-attn":
        pytest.skip("too large for the host emulation")
    for k, v in DIRECT_ENV.items():
        monkeypatch.setenv(k, v)
    outs, trace, convs = run_row(gu, row)
    tol = ROWS[row][6]
    assert outs
    for tag, r in outs.items():
        assert torch.isfinite(r).all(), tag
        e = gu.rel_err(r, trace[tag])
        print(f"  {row} {tag}: rel_err {e:.2e}")
        assert e < tol, tag
    if gu.EMU:
        return
    _reached(row, convs)
    n = sum(1 for o in convs if o["kernel"] == ROWTILE)
    print(f"  {row}: {n} of {len(convs)} convolutions on {ROWTILE}")
    rec = json.load(open(GOLDEN))[row]
    if rec["plan"] != plan_of(convs):
        print(f"  {row}: this device plans differently from the record ({rec['device']}): digests not compared")
        return
    got = digests_of(outs)
    assert set(got) == set(rec["digests"])
    differing = [tag for tag in got if got[tag] != rec["digests"][tag]]
    assert not differing, f"block outputs differ in bits from the record: {differing}"


def test_silu_division_all_inputs(gu, tmp_path):
    """All 2^32 bit patterns of v: the kernel's SiLU equals v / (1 + exp(-v)) bit for bit (a NaN equals any NaN)."""
    if gu.EMU:
        pytest.skip("needs the device's reciprocal and division instructions")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "silu_div_check")
    res = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-I" + os.path.join(REPO, "holo_diffusion_amd", "csrc"),
                          os.path.join(REPO, "tools", "silu_div_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(" ", res.stdout.strip())
    assert res.returncode in (0, 1), res.stdout + res.stderr
    fields = res.stdout.split()
    assert fields[fields.index("inputs") + 1] == "4294967296"
    assert int(fields[fields.index("inside_range") + 1]) > 2 ** 30  # the range test is not vacuous
    assert int(fields[fields.index("differing") + 1]) == 0, res.stdout
