"""What the guided step kernels and a guided chain cost on the north-star grid (64^3 x 32), in one process:

  (a) the step kernels alone on (1, 32, 64, 64, 64) tensors, alternating: ddim_step_kernel (eta 0: 2 reads + 2 writes,
      134 MB) against ddim_step_guided_kernel with noise (4 + 2, 201 MB) and at eta 0 (3 + 2, 168 MB); ddpm_step_kernel
      (3 + 2, 168 MB) against ddpm_step_guided_kernel (4 + 2, 201 MB).  By bytes a guided kernel should take 201/134 (168/134)
      and 201/168 of its unguided kernel's time; one more than 1.25x over that ratio is under-vectorised.
  (b) a ddim50 chain (eta 0) on the north-star denoiser, exact fp32: unguided (the loop's channels-last perf chain, and the
      NCDHW chain a guided loop runs on) and guided by PhotometricGuidance on 2 views at 128 x 128 with the ray sampler's
      training ray count and sample counts.

Kernels are timed with device events around batches of 50 direct library calls on preallocated tensors, so a figure is an
upper bound on the kernel's time (`host_issue_us`: the host clock's time per call of the same loop; a kernel figure close
to it is issue-bound).  Chains are timed with the host clock around work that ends in a device synchronise.
Not a test, not the benchmark.  Writes the figures as JSON to stdout and as a table to the output file.
  python tools/guided_chain_probe.py [timed repetitions, default 10] [output, default profiles/guided_chain_probe.md]"""
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
reps = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "guided_chain_probe.md")
dev = torch.device("cuda", 0)
w = bench.NORTH
shape = (1, 32, w["resol"], w["resol"], w["resol"])
diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
gen = torch.Generator(device=dev).manual_seed(7)
x, mo, gr, nz = (torch.randn(shape, device=dev, generator=gen) for _ in range(4))
t = torch.tensor([500], device=dev)
row_ddim = diff.ddim_coefs([500], [480], 0.0).to(dev)
row_g0 = diff.ddim_guided_coefs([500], [480], 0.0).to(dev)
row_g1 = diff.ddim_guided_coefs([500], [480], 1.0).to(dev)

# the timed loop issues the library entries themselves on preallocated outputs: no allocation, no Python step wrapper
L, ctx, stream, P = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev), runtime.ptr
out_s, out_p = torch.empty_like(x), torch.empty_like(x)
per = x[0].numel()
head, ghead = diff._ddpm_head(x, t), diff._ddpm_guided_head(x, t)
KERNELS = {
    "ddim_step_eta0": lambda: L.holo_ddim_step(ctx, P(row_ddim), 1, per, P(x), P(mo), None, 1, P(out_s), P(out_p), stream),
    "ddim_step_guided_noise": lambda: L.holo_ddim_step_guided(ctx, P(row_g1), 1, per, P(x), P(mo), P(gr), P(nz), 1, P(out_s),
                                                              P(out_p), stream),
    "ddim_step_guided_eta0": lambda: L.holo_ddim_step_guided(ctx, P(row_g0), 1, per, P(x), P(mo), P(gr), None, 1, P(out_s),
                                                             P(out_p), stream),
    "ddpm_step": lambda: L.holo_ddpm_step(ctx, *head, 1, per, P(x), P(mo), P(nz), 1, P(out_s), P(out_p), stream),
    "ddpm_step_guided": lambda: L.holo_ddpm_step_guided(ctx, *ghead, 1, per, P(x), P(mo), P(gr), P(nz), 1, P(out_s), P(out_p),
                                                        stream),
}
RATIOS = (("ddim_step_guided_noise", "ddim_step_eta0", 201 / 134), ("ddim_step_guided_eta0", "ddim_step_eta0", 168 / 134),
          ("ddpm_step_guided", "ddpm_step", 201 / 168))
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

H = W = 128
model, _, _ = bench.build_model(w, H, W, dev)
net = model.net_3d
cams = bench.hda_cams(2, dev)
rgb = torch.rand((2, 3, H, W), device=dev, generator=gen)
guide = hda.PhotometricGuidance(model, cams, rgb, scale=1.0, seed=0)
x_T = torch.randn(shape, device=dev, generator=gen)
perf = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=7)  # (the DDIM loop's channels-last chain)

CHAINS = {
    "ddim50_perf": lambda: perf.ddim_sample_loop(net, shape, noise=x_T, ddim_steps=50),
    "ddim50_ncdhw": lambda: diff.ddim_sample_loop(net, shape, noise=x_T, ddim_steps=50, cond_fn=lambda a, b: gr),
    "ddim50_guided": lambda: diff.ddim_sample_loop(net, shape, noise=x_T, ddim_steps=50, cond_fn=guide),
}


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

out = {"shape": list(shape), "repetitions": reps, "launches_per_repetition": LAUNCHES, "chain_repetitions": chain_reps,
       "host_issue_us": round(host_issue_us, 2),
       "guidance": {"views": 2, "frame": [H, W], "rays_per_view": int(model.raysampler.n_rays_per_image_sampled_from_mask),
                    "pts_per_ray": [int(model.raysampler.n_pts_per_ray_training), int(model.renderer.n_pts_per_ray_fine_training)]}}
for k, v in us.items():
    out[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
for k, base, by_bytes in RATIOS:
    out[k]["ratio_to_unguided"] = round(out[k]["median_us"] / out[base]["median_us"], 3)
    out[k]["ratio_by_bytes"] = round(by_bytes, 3)
    out[k]["over_bytes"] = round(out[k]["ratio_to_unguided"] / by_bytes, 3)
for k, v in ms.items():
    out[k] = {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
print(json.dumps(out))

lines = ["# Guided step kernels and a guided ddim50 chain at 64^3 x 32 (tools/guided_chain_probe.py)", "",
         f"One process, exact fp32; {reps} timed repetitions of {LAUNCHES} launches per kernel, {chain_reps} per chain; "
         f"host issue time {out['host_issue_us']} us per call.", "",
         "| kernel | median us | min | max | ratio to unguided | ratio by bytes | over bytes (limit 1.25) |", "|---|---|---|---|---|---|---|"]
for k in KERNELS:
    r = out[k]
    lines.append(f"| {k} | {r['median_us']} | {r['min_us']} | {r['max_us']} | {r.get('ratio_to_unguided', '-')} | "
                 f"{r.get('ratio_by_bytes', '-')} | {r.get('over_bytes', '-')} |")
gd = out["guidance"]
lines += ["", f"Chains (50 denoiser calls each; guidance: {gd['views']} views at {H} x {W}, {gd['rays_per_view']} rays per view, "
          f"{gd['pts_per_ray'][0]} + {gd['pts_per_ray'][1]} samples per ray):", "",
          "| chain | median ms | min | max |", "|---|---|---|---|"]
for k in CHAINS:
    r = out[k]
    lines.append(f"| {k} | {r['median_ms']} | {r['min_ms']} | {r['max_ms']} |")
lines += ["", "ddim50_perf: the unguided loop's channels-last chain with in-kernel noise.  ddim50_ncdhw: the NCDHW chain a guided "
          "loop runs on, with a constant gradient (the guided step kernel, no guidance work).  ddim50_guided: PhotometricGuidance "
          "per step - a taped denoiser forward + backward next to the loop's own forward, a render forward + backward.", ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines))
