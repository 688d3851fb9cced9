"""What a DPM-Solver++ step and chain cost on the north-star grid (64^3 x 32), next to DDIM, in one process:

  (a) the step kernels alone on (1, 32, 64, 64, 64) tensors, alternating: ddim_step_kernel (eta 0: 2 reads + 2 writes,
      134 MB), dpm_step_kernel at order 2 (3 + 2, 168 MB) and order 3 (4 + 2, 201 MB).  By bytes the DPM kernels should take
      168/134 and 201/134 of the DDIM kernel's time; one more than 1.25x over that ratio is under-vectorised.
  (b) a dpmpp20 chain (order 2, log-SNR spacing) next to a ddim50 chain on the north-star denoiser, exact fp32.

Kernels are timed with device events around batches of 50 direct library calls on preallocated tensors, so a figure is an
upper bound on the kernel's time: if the host cannot issue a call in that time, it is the issue rate (`host_issue_us` is
the host clock's time per call of the same loop; a kernel figure close to it is issue-bound, and the kernel's own time then
needs a kernel trace).  Chains are timed with the host clock around work that ends in a device synchronise.
Not a test, not the benchmark.
  python tools/dpm_chain_probe.py [timed repetitions, default 10]"""
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
from holo_diffusion_amd.structure import unet_param_shapes  # noqa: E402
from holo_diffusion_amd.weights import synth_state_dict  # noqa: E402

WARMUP = 2
LAUNCHES = 50  # per timed batch of a step kernel
reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
dev = torch.device("cuda", 0)
w = bench.NORTH
shape = (1, 32, w["resol"], w["resol"], w["resol"])
diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
gen = torch.Generator(device=dev).manual_seed(7)
x, mo, h1, h2 = (torch.randn(shape, device=dev, generator=gen) for _ in range(4))
idx = diff.dpm_schedule(20)
row2 = diff.dpm_coefs(idx, 2)[0][5:6].to(dev)
row3 = diff.dpm_coefs(idx, 3)[0][5:6].to(dev)
row_ddim = diff.ddim_coefs([idx[5]], [idx[6]], 0.0).to(dev)

# the timed loop issues the library entries themselves on preallocated outputs: no allocation, no Python step wrapper
L, ctx, stream, P = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev), runtime.ptr
out_s, out_p = torch.empty_like(x), torch.empty_like(x)
per = x[0].numel()
KERNELS = {
    "ddim_step_eta0": lambda: L.holo_ddim_step(ctx, P(row_ddim), 1, per, P(x), P(mo), None, 1, P(out_s), P(out_p), stream),
    "dpm_step_order2": lambda: L.holo_dpm_step(ctx, P(row2), 1, per, P(x), P(mo), P(h1), None, 1, P(out_s), P(out_p), stream),
    "dpm_step_order3": lambda: L.holo_dpm_step(ctx, P(row3), 1, per, P(x), P(mo), P(h1), P(h2), 1, P(out_s), P(out_p), stream),
}
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

net = hda.SimpleUnet3D(image_size=w["resol"], in_channels=32, out_channels=32, model_channels=64, channel_mult=w["channel_mult"],
                       attention_resolutions=w["attention_resolutions"])
net.load_state_dict({"_net." + k: v for k, v in synth_state_dict(unet_param_shapes(64, 32, 32, 64, 2, w["channel_mult"],
                                                                                   w["attention_resolutions"]), 1234).items()})
net.to(dev)
x_T = torch.randn(shape, device=dev, generator=gen)
perf = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=7)  # (the DDIM loop's channels-last chain)

CHAINS = {
    "ddim50": lambda: perf.ddim_sample_loop(net, shape, noise=x_T, ddim_steps=50),
    "dpmpp20_order2": lambda: diff.dpm_sample_loop(net, shape, noise=x_T, steps=20, order=2),
}


def chain_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


ms = {k: [] for k in CHAINS}
chain_reps = max(3, reps // 2)
for i in range(1 + chain_reps):
    for k, fn in CHAINS.items():
        v = chain_ms(fn)
        if i >= 1:
            ms[k].append(v)

out = {"shape": list(shape), "repetitions": reps, "launches_per_repetition": LAUNCHES, "chain_repetitions": chain_reps,
       "host_issue_us": round(host_issue_us, 2), "unet_calls": {"ddim50": 50, "dpmpp20_order2": len(idx)}}
for k, v in us.items():
    out[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
base = out["ddim_step_eta0"]["median_us"]
for k, by_bytes in (("dpm_step_order2", 168 / 134), ("dpm_step_order3", 201 / 134)):
    out[k]["ratio_to_ddim"] = round(out[k]["median_us"] / base, 3)
    out[k]["ratio_by_bytes"] = round(by_bytes, 3)
for k, v in ms.items():
    out[k] = {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
print(json.dumps(out))
