"""What the diffusion-loss kernels cost on the north-star grid (64^3 x 32), next to the DDIM step kernel, in one process,
alternating, on (1, 32, 64, 64, 64) tensors:

  ddim_step_kernel (eta 0)             2 reads + 2 writes, 134 MB: the yardstick, measured in the same run
  diffusion_loss_kernel, terms form    2 reads,             67 MB  + loss_finalize_kernel
  diffusion_loss_kernel, grad form     2 reads + 1 write,  101 MB
  diffusion_loss_kernel, fused form    2 reads + 1 write,  101 MB  + loss_finalize_kernel
  vb_terms_kernel (t = 500, t = 0)     4 reads,            134 MB  + loss_finalize_kernel

By bytes a kernel should take its share of the DDIM kernel's time; one more than 1.25x over that ratio is not streaming.
An entry is timed with device events around batches of 50 direct library calls on preallocated tensors, so a figure is the
entry's kernels back to back (streaming launch + the one-workgroup finalize) and an upper bound: `host_issue_us` is the host
clock's time per call of the same loop.  The split between a streaming kernel and its finalize launch comes from a kernel
trace of this script (rocprofv3 --kernel-trace --stats -- python tools/diffusion_loss_probe.py).
Not a test, not the benchmark.
  python tools/diffusion_loss_probe.py [timed repetitions, default 10]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import runtime  # noqa: E402

WARMUP = 2
LAUNCHES = 50  # per timed batch
reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
dev = torch.device("cuda", 0)
w = bench.NORTH
shape = (1, 32, w["resol"], w["resol"], w["resol"])
diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
gen = torch.Generator(device=dev).manual_seed(7)
x0, nz = torch.tanh(torch.randn(shape, device=dev, generator=gen)), torch.randn(shape, device=dev, generator=gen)
mo = (x0 + 0.1 * torch.randn(shape, device=dev, generator=gen)).contiguous()
x_t = diff.q_sample(x0, torch.tensor([500], device=dev), nz).contiguous()
row_ddim = diff.ddim_coefs([500], [499], 0.0).to(dev)
row_vb, row_vb0 = diff.vb_coefs([500]).to(dev), diff.vb_coefs([0]).to(dev)
mo0 = (x0 + 0.0074 * (4 * torch.rand(shape, device=dev, generator=gen) - 2)).contiguous()  # (the t = 0 input condition)

L, ctx, stream, P = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev), runtime.ptr
per = x0[0].numel()
out_s, out_p, grad = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
nbytes = int(L.holo_diffusion_loss_workspace_bytes(1, per))
ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
terms = torch.empty(3, dtype=torch.float64, device=dev)
scale = torch.full((1,), 2.0 / per, device=dev)
KERNELS = {
    "ddim_step_eta0": lambda: L.holo_ddim_step(ctx, P(row_ddim), 1, per, P(x_t), P(mo), None, 1, P(out_s), P(out_p), stream),
    "loss_terms": lambda: L.holo_diffusion_loss(ctx, 1, per, P(x0), P(mo), None, P(terms), None, P(ws), nbytes, stream),
    "loss_grad": lambda: L.holo_diffusion_loss(ctx, 1, per, P(x0), P(mo), P(scale), None, P(grad), P(ws), nbytes, stream),
    "loss_fused": lambda: L.holo_diffusion_loss(ctx, 1, per, P(x0), P(mo), P(scale), P(terms), P(grad), P(ws), nbytes, stream),
    "vb_terms_t500": lambda: L.holo_vb_terms(ctx, P(row_vb), 1, per, P(x0), P(x_t), P(nz), P(mo), 1, P(terms), P(ws), nbytes,
                                             stream),
    "vb_terms_t0": lambda: L.holo_vb_terms(ctx, P(row_vb0), 1, per, P(x0), P(x0), P(nz), P(mo0), 1, P(terms), P(ws), nbytes,
                                           stream),
}
BYTES_MB = {"ddim_step_eta0": 134, "loss_terms": 67, "loss_grad": 101, "loss_fused": 101, "vb_terms_t500": 134, "vb_terms_t0": 134}
values = {}
for name, fn in KERNELS.items():
    assert fn() == 0, (name, L.holo_last_error())
    torch.cuda.synchronize()
    values[name] = [round(v, 9) for v in terms.tolist()]


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

out = {"shape": list(shape), "repetitions": reps, "launches_per_repetition": LAUNCHES, "host_issue_us": round(host_issue_us, 2),
       "partials_per_sample": nbytes // 24, "last_terms": values}
for k, v in us.items():
    out[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
base = out["ddim_step_eta0"]["median_us"]
for k in KERNELS:
    if k != "ddim_step_eta0":
        out[k]["ratio_to_ddim"] = round(out[k]["median_us"] / base, 3)
        out[k]["ratio_by_bytes"] = round(BYTES_MB[k] / BYTES_MB["ddim_step_eta0"], 3)
        out[k]["within_1.25x_of_bytes"] = out[k]["ratio_to_ddim"] <= 1.25 * out[k]["ratio_by_bytes"]
print(json.dumps(out))
