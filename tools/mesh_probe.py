"""What the mesh export costs on the north-star grid (R = 64, C = 32, tanh(N(0,1)) features, synthetic RenderMLP) at
lattices of m = 127 (2R - 1) and m = 256, next to ddim_step_kernel on 134 MB in the same process:

  density_lattice    holo_density_lattice: layout pass + density_field_kernel + density_lattice_kernel
  surface_count      holo_surface_count: surface_classify_kernel + the scan (block scans over 3 levels at m = 127, 4 at
                     m = 256, one add-back pass per level but the last) + the totals
  surface_vertices   holo_surface_emit with no face buffer: surface_vertices_kernel
  surface_triangles  holo_surface_emit with no vertex buffer: surface_triangles_kernel

The field meshed is the lattice's own density at its median (about half of the points inside, nearly every cell active: the
dense end of what the extractor meets).  Figures are device events around batches of direct library calls on preallocated
buffers, i.e. upper bounds per CALL (a call is several launches where listed above; a kernel trace separates them), and
where a figure is close to `host issue` it is the host's issue rate.  Bytes are the compulsory traffic of each call (every
operand once; the 8 corner reads of a cell are served by the cache), and `rate / ddim` is bytes / time as a fraction of
ddim_step_kernel's.  Not a test, not the benchmark, no gate.
  python tools/mesh_probe.py [output .md, default profiles/mesh_probe.md] [timed repetitions, default 10]"""
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import mesh, runtime  # noqa: E402
from holo_diffusion_amd.weights import synth_state_dict  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "mesh_probe.md")
reps = max(5, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
WARMUP, LAUNCHES = 2, 20
R, Cf = 64, 32
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(7)
L, ctx, stream, P = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev), runtime.ptr

fn = hda.HoloVoxelGridImplicitFunction(resol=R, n_hidden=Cf, feature_dim=0)
fn.render_mlp.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in fn.render_mlp.state_dict().items()}, 4321))
fn.to(dev)
grid = torch.tanh(torch.randn(1, Cf, R, R, R, device=dev, generator=gen))
h = fn.native_handle(dev)
half = mesh.half_extent(R, fn.volume_extent)
lat_ws = torch.empty(int(L.holo_density_lattice_workspace_bytes(h)), dtype=torch.uint8, device=dev)

# ddim_step_kernel, eta 0: 2 reads + 2 writes of (1, 32, 64, 64, 64) fp32 = 134 MB
diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
x, mo = (torch.randn(1, 32, 64, 64, 64, device=dev, generator=gen) for _ in range(2))
out_s, out_p = torch.empty_like(x), torch.empty_like(x)
row = diff.ddim_coefs([500], [480], 0.0).to(dev)
calls = {"ddim_step_eta0": (lambda: L.holo_ddim_step(ctx, P(row), 1, x[0].numel(), P(x), P(mo), None, 1, P(out_s), P(out_p),
                                                      stream), 4 * x.numel() * 4)}
keep, shapes = [], {}
for m in (127, 256):
    n = m ** 3
    field = torch.empty(m, m, m, device=dev)
    ws = torch.empty(int(L.holo_surface_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    lattice = (lambda m=m, field=field: L.holo_density_lattice(h, P(grid), m, P(field), P(lat_ws), lat_ws.numel(), stream))
    assert lattice() == 0
    level = float(field.median())
    count = (lambda m=m, field=field, level=level, counts=counts, ws=ws:
             L.holo_surface_count(ctx, P(field), m, level, P(counts), P(ws), ws.numel(), stream))
    assert count() == 0
    V, T = counts.tolist()
    verts, faces = torch.empty(V, 3, device=dev), torch.empty(T, 3, dtype=torch.int32, device=dev)
    emit_v = (lambda m=m, field=field, level=level, verts=verts, V=V, ws=ws:
              L.holo_surface_emit(ctx, P(field), m, level, half, P(verts), V, None, 0, P(ws), ws.numel(), stream))
    emit_t = (lambda m=m, field=field, level=level, faces=faces, T=T, ws=ws:
              L.holo_surface_emit(ctx, P(field), m, level, half, None, 0, P(faces), T, P(ws), ws.numel(), stream))
    assert emit_v() == 0 and emit_t() == 0
    assert ws[:8].view(torch.int32).tolist() == [0, 0]
    keep.append((field, ws, counts, verts, faces))
    shapes[m] = (V, T)
    vox = R ** 3
    calls[f"density_lattice m={m}"] = (lattice, 3 * vox * Cf * 4 + 2 * vox * 4 + n * 4)
    calls[f"surface_count m={m}"] = (count, n * (4 + 8 + 32))  # field in, words out, scan and add-back: 2 x (read + write)
    calls[f"surface_vertices m={m}"] = (emit_v, n * (8 + 4) + V * 12)
    calls[f"surface_triangles m={m}"] = (emit_t, n * (8 + 4) + T * 12)

host_issue_us = float("inf")


def call_us(f):
    global host_issue_us
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(LAUNCHES):
        f()
    end.record()
    host_issue_us = min(host_issue_us, (time.perf_counter() - t0) * 1e6 / LAUNCHES)
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / LAUNCHES


us = {k: [] for k in calls}
for i in range(WARMUP + reps):
    for k, (f, _) in calls.items():
        v = call_us(f)
        if i >= WARMUP:
            us[k].append(v)

med = {k: statistics.median(v) for k, v in us.items()}
ddim_rate = calls["ddim_step_eta0"][1] / med["ddim_step_eta0"]
lines = ["# Mesh export on the north-star grid (R = 64, C = 32): tools/mesh_probe.py", "",
         f"{reps} repetitions of {LAUNCHES} calls each, device events; host issue {host_issue_us:.1f} µs per call (the fastest "
         "loop).  A figure is an upper bound for the call's kernels; `rate / ddim` = (bytes / median time) over the same for "
         "`ddim_step_kernel`.  No gate.", ""]
lines += [f"- m = {m}: {V} vertices, {T} triangles at the field's median" for m, (V, T) in shapes.items()]
lines += ["", "| call | median µs | min µs | max µs | MB moved | GB/s | rate / ddim |", "|---|---|---|---|---|---|---|"]
for k, (_, nbytes) in calls.items():
    lines.append(f"| {k} | {med[k]:.1f} | {min(us[k]):.1f} | {max(us[k]):.1f} | {nbytes / 1e6:.1f} | "
                 f"{nbytes / med[k] / 1e3:.0f} | {nbytes / med[k] / ddim_rate:.2f} |")
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
print(text)
