"""What the masked (inpainting) step and a masked chain cost on the north-star grid (64^3 x 32), in one process:

  (a) the step kernels alone on channels-last (1, 64, 64, 64, 32) tensors, alternating, neither writing pred_xstart:
      ddpm_step_philox_kernel (2 reads + 1 write, 101 MB) against ddpm_step_inpaint_philox_kernel (x_t, the model output, the
      known grid, the sample and one mask value per voxel: 4 + 1/32 tensors, 135 MB) with a binary half-grid mask (one draw
      per quad: what a coverage mask gives) and with a soft mask (both draws everywhere), and q_sample_philox_kernel (1 + 1,
      67 MB).  By bytes the masked step should take (4 + 1/32) / 3 = 1.344 of the plain step's time; the probe holds the
      binary-mask figure to 1.25x that ratio and exits non-zero beyond it.
  (b) a 50-step chain (num_steps = 50, in-kernel noise, the denoiser's channels-last chain) on the north-star denoiser, exact
      fp32: unmasked (p_sample_loop) against masked with (jump_length, n_resample) = (10, 1) - 50 denoiser calls - and
      (10, 2) - 90 calls and 4 forward jumps.  The chain ratios are written down, nothing is asserted about them.

Kernels are timed with device events around batches of 50 direct library calls on preallocated tensors, so a figure is an
upper bound on the kernel's time (`host_issue_us`: the host clock's time per call of the same loop).  Chains are timed with
the host clock around work that ends in a device synchronise.  Not a test, not the benchmark.  Writes the figures as JSON to
stdout and as a table to the output file.
  python tools/inpaint_chain_probe.py [timed repetitions, default 10] [output, default profiles/inpaint_chain_probe.md]"""
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import runtime  # noqa: E402

WARMUP = 2
LAUNCHES = 50  # per timed batch of a step kernel
LIMIT = 1.25
reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "inpaint_chain_probe.md")
dev = torch.device("cuda", 0)
w = bench.NORTH
R, C = w["resol"], 32
shape = (1, C, R, R, R)
cl_shape = (1, R, R, R, C)
diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
gen = torch.Generator(device=dev).manual_seed(7)
x, mo, kn = (torch.randn(cl_shape, device=dev, generator=gen) for _ in range(3))
half = torch.zeros(1, 1, R, R, R, device=dev)
half[..., : R // 2] = 1
soft = torch.rand(1, 1, R, R, R, device=dev, generator=gen)
t = torch.tensor([500], device=dev)
known_row = diff.known_coefs([500]).to(dev)
q_row = diff.q_sample_coefs([500]).to(dev)

# the timed loop issues the library entries themselves on a preallocated output: no allocation, no Python step wrapper
L, ctx, stream, P = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev), runtime.ptr
out_s = torch.empty_like(x)
per = x[0].numel()
head = diff._ddpm_head(x, t)
SEED, OFFSET = 7, 500


def masked(mask):
    return lambda: L.holo_ddpm_step_inpaint_philox(ctx, *head, P(known_row), 1, per, C, 0, P(x), P(mo), P(kn), P(mask), SEED,
                                                   OFFSET, None, 0, 1, P(out_s), None, None, None, stream)


KERNELS = {
    "ddpm_step_philox": lambda: L.holo_ddpm_step_philox(ctx, *head, 1, per, P(x), P(mo), SEED, OFFSET, 1, P(out_s), None, None,
                                                        0, stream),
    "ddpm_step_inpaint_philox": masked(half),
    "ddpm_step_inpaint_philox_soft": masked(soft),
    "q_sample_philox": lambda: L.holo_q_sample_philox(ctx, P(q_row), 1, per, P(x), SEED, OFFSET, None, 0, P(out_s), None, 0,
                                                      stream),
}
BY_BYTES = (4 + 1 / C) / 3
RATIOS = (("ddpm_step_inpaint_philox", "ddpm_step_philox", BY_BYTES), ("ddpm_step_inpaint_philox_soft", "ddpm_step_philox", BY_BYTES),
          ("q_sample_philox", "ddpm_step_philox", 2 / 3))
for name, fn in KERNELS.items():
    assert fn() == 0, name


def kernel_us(fn):
    global host_issue_us
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(LAUNCHES):
        fn()
    end.record()
    host_issue_us = min(host_issue_us, (time.perf_counter() - t0) * 1e6 / LAUNCHES)
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / LAUNCHES


host_issue_us = float("inf")
us = {k: [] for k in KERNELS}
for i in range(WARMUP + reps):
    for k, fn in KERNELS.items():
        v = kernel_us(fn)
        if i >= WARMUP:
            us[k].append(v)

model, _, _ = bench.build_model(w, 128, 128, dev)
net = model.net_3d
x_T = torch.randn(shape, device=dev, generator=gen)
known = torch.tanh(torch.randn(shape, device=dev, generator=gen))
perf = hda.ImplicitronGaussianDiffusion(num_steps=50, device_noise_seed=7)  # (the channels-last chain, in-kernel noise)

CHAINS = {
    "ddpm50_unmasked": lambda: perf.p_sample_loop(net, shape, noise=x_T),
    "ddpm50_masked_j10_r1": lambda: perf.inpaint_sample_loop(net, shape, known, half, jump_length=10, n_resample=1, noise=x_T),
    "ddpm50_masked_j10_r2": lambda: perf.inpaint_sample_loop(net, shape, known, half, jump_length=10, n_resample=2, noise=x_T),
}
CALLS = {"ddpm50_unmasked": 50, "ddpm50_masked_j10_r1": 50,
         "ddpm50_masked_j10_r2": sum(1 for op in perf.repaint_schedule(10, 2) if op[0] == "reverse")}


def chain_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


ms = {k: [] for k in CHAINS}
chain_reps = max(2, reps // 4)
for i in range(1 + chain_reps):
    for k, fn in CHAINS.items():
        v = chain_ms(fn)
        if i >= 1:
            ms[k].append(v)

out = {"shape": list(cl_shape), "repetitions": reps, "launches_per_repetition": LAUNCHES, "chain_repetitions": chain_reps,
       "host_issue_us": round(host_issue_us, 2)}
for k, v in us.items():
    out[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
for k, base, by_bytes in RATIOS:
    out[k]["ratio_to_plain"] = round(out[k]["median_us"] / out[base]["median_us"], 3)
    out[k]["ratio_by_bytes"] = round(by_bytes, 3)
    out[k]["over_bytes"] = round(out[k]["ratio_to_plain"] / by_bytes, 3)
for k, v in ms.items():
    out[k] = {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2),
              "denoiser_calls": CALLS[k]}
base_ms = out["ddpm50_unmasked"]["median_ms"]
step_diff_ms = 50 * (out["ddpm_step_inpaint_philox"]["median_us"] - out["ddpm_step_philox"]["median_us"]) * 1e-3
for k in ("ddpm50_masked_j10_r1", "ddpm50_masked_j10_r2"):
    out[k]["ratio_to_unmasked"] = round(out[k]["median_ms"] / base_ms, 4)
out["ddpm50_masked_j10_r1"]["expected_ms"] = round(base_ms + step_diff_ms, 2)
within = out["ddpm_step_inpaint_philox"]["over_bytes"] <= LIMIT
out["within_limit"] = within
print(json.dumps(out))

lines = ["# The masked step kernels and a masked 50-step chain at 64^3 x 32 (tools/inpaint_chain_probe.py)", "",
         f"One process, exact fp32, channels-last tensors, pred_xstart not written; {reps} timed repetitions of {LAUNCHES} "
         f"launches per kernel, {chain_reps} per chain; host issue time {out['host_issue_us']} us per call.", "",
         f"| kernel | median us | min | max | ratio to ddpm_step_philox | ratio by bytes | over bytes (limit {LIMIT}) |",
         "|---|---|---|---|---|---|---|"]
for k in KERNELS:
    r = out[k]
    lines.append(f"| {k} | {r['median_us']} | {r['min_us']} | {r['max_us']} | {r.get('ratio_to_plain', '-')} | "
                 f"{r.get('ratio_by_bytes', '-')} | {r.get('over_bytes', '-')} |")
lines += ["", "ddpm_step_inpaint_philox: a binary half-grid mask, one draw per quad (the limit applies to this row: "
          f"{'inside' if within else 'OUTSIDE'} it).  ddpm_step_inpaint_philox_soft: a mask strictly inside (0, 1), both draws "
          "for every quad - two Philox blocks and four Box-Muller pairs per thread.", "",
          "Chains (num_steps = 50, in-kernel noise, the denoiser's channels-last chain, half-grid mask):", "",
          "| chain | denoiser calls | median ms | min | max | ratio to unmasked |", "|---|---|---|---|---|---|"]
for k in CHAINS:
    r = out[k]
    lines.append(f"| {k} | {r['denoiser_calls']} | {r['median_ms']} | {r['min_ms']} | {r['max_ms']} | "
                 f"{r.get('ratio_to_unmasked', '-')} |")
lines += ["", f"By the kernel figures the r = 1 chain should take the unmasked chain plus 50 step differences: "
          f"{out['ddpm50_masked_j10_r1']['expected_ms']} ms.", ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines))
sys.exit(0 if within else 1)
