"""GPU: mesh export (kernels_mesh.hip behind holo_density_lattice / holo_surface_count / holo_surface_emit, mesh.py,
HoloDiffusionModel.extract_mesh).

The extractor is held to the numpy restatement of the pinned algorithm (tests/support/surface_nets_ref.py) BIT FOR BIT:
counts, vertex positions and faces, on analytic shapes, smooth and white-noise fields and fields with values exactly at the
level, at lattice sizes that reach every level of the scan (block size 256: 42^3 + 1 > 256^2 words)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, mesh, runtime  # noqa: E402
from oracle import render_oracle as ro  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.support import surface_nets_ref as ref  # noqa: E402

TINY_UNET = dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2))
SENTINEL_F, SENTINEL_I, PAD = -12345.0, -77, 5


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def make_field(kind, m):
    """-> (field (m, m, m) float32 [z][y][x], level, half extent)"""
    h = 3.5
    g = np.linspace(-h, h, m)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    rng = np.random.default_rng(100 + m)
    if kind == "sphere":
        return (2.1 - np.sqrt((X - 0.3) ** 2 + (Y + 0.2) ** 2 + (Z - 0.45) ** 2)).astype(np.float32), 0.0, h
    if kind == "torus":
        return (0.8 - np.sqrt((np.sqrt((X - 0.3) ** 2 + (Y + 0.2) ** 2) - 1.9) ** 2 + (Z - 0.45) ** 2)).astype(np.float32), 0.0, h
    if kind == "smooth":  # a few sinusoids; a level and a half extent that are not dyadic
        f = np.zeros_like(X)
        for _ in range(4):
            k, ph = rng.uniform(0.4, 1.6, 3), rng.uniform(0, 2 * np.pi)
            f += rng.uniform(0.5, 1.0) * np.sin(k[0] * X + k[1] * Y + k[2] * Z + ph)
        return f.astype(np.float32), 0.1, 0.97
    if kind == "noise":
        return rng.standard_normal((m, m, m)).astype(np.float32), 0.0, h
    assert kind == "planted"  # values exactly AT the level (= outside), interior and on the boundary layer
    f = rng.standard_normal((m, m, m)).astype(np.float32) + np.float32(0.25)
    f[rng.random((m, m, m)) < 0.3] = np.float32(0.25)
    f[0, 0, 0] = f[-1, m // 2, 0] = np.float32(0.25)
    return f, 0.25, h


def run_extractor(gu, field, level, half_extent, shrink=(0, 0)):
    """count + emit through the C ABI with capacities = counts - shrink, into buffers padded with a sentinel.
    -> (counts, verts, faces, status words); the padding is checked here."""
    m = field.shape[0]
    dev = gu.DEV
    L, ctx, st = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev)
    fd = torch.from_numpy(np.ascontiguousarray(field)).to(dev)
    ws = torch.zeros(int(L.holo_surface_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    _lib.check(L, L.holo_surface_count(ctx, runtime.ptr(fd), m, level, runtime.ptr(counts), runtime.ptr(ws), ws.numel(), st),
               "holo_surface_count")
    nv, nt = counts.tolist()
    cv, ct = max(nv - shrink[0], 0), max(nt - shrink[1], 0)
    verts = torch.full((cv + PAD, 3), SENTINEL_F, dtype=torch.float32, device=dev)
    faces = torch.full((ct + PAD, 3), SENTINEL_I, dtype=torch.int32, device=dev)
    _lib.check(L, L.holo_surface_emit(ctx, runtime.ptr(fd), m, level, half_extent, runtime.ptr(verts), cv, runtime.ptr(faces),
                                      ct, runtime.ptr(ws), ws.numel(), st), "holo_surface_emit")
    torch.cuda.synchronize()
    verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    assert (verts[cv:] == SENTINEL_F).all() and (faces[ct:] == SENTINEL_I).all(), "emit wrote past a capacity"
    return (nv, nt), verts[:cv], faces[:ct], ws[:8].view(torch.int32).tolist()


@pytest.mark.parametrize("m", [2, 3, 8, 42])
@pytest.mark.parametrize("kind", ["sphere", "torus", "smooth", "noise", "planted"])
def test_extractor_equals_the_restatement_bit_for_bit(gu, kind, m):
    field, level, h = make_field(kind, m)
    rv, rf = ref.surface_nets(field, level, h)
    (nv, nt), verts, faces, status = run_extractor(gu, field, level, h)
    print(f"{kind} m={m}: V={nv} (ref {len(rv)}) T={nt} (ref {len(rf)})")
    assert (nv, nt) == (len(rv), len(rf))
    assert status == [0, 0]
    assert np.array_equal(verts.view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(faces, rf)
    if kind == "noise" and m >= 8:
        assert nv > 0.9 * (m - 3) ** 3  # (nearly) every interior cell is active


def test_public_surface_nets_and_the_cube(gu):
    """mesh.surface_nets returns the same arrays; m = 3 with the centre inside is the cube (V = 8, F = 12); an all-outside
    field and m = 2 are empty and launch no emit."""
    field, level, h = make_field("torus", 8)
    rv, rf = ref.surface_nets(field, level, h)
    v, f = mesh.surface_nets(torch.from_numpy(field).to(gu.DEV), level, h)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.cpu().numpy(), rf)
    cube = -np.ones((3, 3, 3), np.float32)
    cube[1, 1, 1] = 1.0
    v, f = mesh.surface_nets(torch.from_numpy(cube).to(gu.DEV), 0.0, 1.0)
    assert tuple(v.shape) == (8, 3) and tuple(f.shape) == (12, 3)
    for empty in (-np.ones((6, 6, 6), np.float32), np.ones((2, 2, 2), np.float32)):
        v, f = mesh.surface_nets(torch.from_numpy(empty).to(gu.DEV), 0.0, 1.0)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_small_capacities_are_reported_and_respected(gu):
    """Capacities below the counts: nothing is written past them (the sentinel padding survives, checked in
    run_extractor), what fits is what the full emit writes there, and the two status words of the workspace say so."""
    field, level, h = make_field("smooth", 8)
    rv, rf = ref.surface_nets(field, level, h)
    assert len(rv) > 4 and len(rf) > 8
    _, verts, faces, status = run_extractor(gu, field, level, h, shrink=(3, 4))
    assert status == [1, 1]
    assert np.array_equal(verts.view(np.uint32), rv[:-3].view(np.uint32)) and np.array_equal(faces, rf[:-4])
    _, verts, faces, status = run_extractor(gu, field, level, h, shrink=(0, 10 ** 9))
    assert status == [0, 1] and np.array_equal(verts.view(np.uint32), rv.view(np.uint32)) and len(faces) == 0


def test_refusals(gu):
    """m = 1, m = 1025, a null field and a short workspace return an error with a message; the counts stay untouched."""
    dev = gu.DEV
    L, ctx, st = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev)
    fd = torch.zeros(4, 4, 4, device=dev)
    ws = torch.zeros(int(L.holo_surface_workspace_bytes(4)), dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    out = torch.zeros(8, 3, device=dev)
    tri = torch.zeros(8, 3, dtype=torch.int32, device=dev)
    assert L.holo_surface_workspace_bytes(1) == 0 and L.holo_surface_workspace_bytes(1025) == 0
    null = C.c_void_p(None)
    cases = [(runtime.ptr(fd), 1, ws.numel(), b"2 <= m <= 1024"), (runtime.ptr(fd), 1025, ws.numel(), b"2 <= m <= 1024"),
             (null, 4, ws.numel(), b"null"), (runtime.ptr(fd), 4, ws.numel() - 1, b"workspace too small")]
    for field_ptr, m, nbytes, msg in cases:
        rc = L.holo_surface_count(ctx, field_ptr, m, 0.0, runtime.ptr(counts), runtime.ptr(ws), nbytes, st)
        assert rc < 0 and msg in L.holo_last_error(), (m, nbytes, L.holo_last_error())
        rc = L.holo_surface_emit(ctx, field_ptr, m, 0.0, 1.0, runtime.ptr(out), 8, runtime.ptr(tri), 8, runtime.ptr(ws), nbytes, st)
        assert rc < 0 and msg in L.holo_last_error(), (m, nbytes, L.holo_last_error())
    assert L.holo_surface_count(ctx, runtime.ptr(fd), 4, float("nan"), runtime.ptr(counts), runtime.ptr(ws), ws.numel(), st) < 0
    assert b"finite" in L.holo_last_error()
    torch.cuda.synchronize()
    assert counts.tolist() == [-1, -1] and not out.any() and not tri.any()
    # the lattice entry refuses the same sizes
    fn, _ = make_implicit_function(gu, 8, 16)
    grid = torch.zeros(1, 16, 8, 8, 8, device=dev)
    for m in (1, 1025):
        with pytest.raises(ValueError, match="resolution"):
            mesh.density_lattice(fn, grid, m)
    h = fn.native_handle(dev)
    lw = torch.zeros(int(L.holo_density_lattice_workspace_bytes(h)), dtype=torch.uint8, device=dev)
    for m, nbytes, msg in ((1, lw.numel(), b"2 <= m <= 1024"), (1025, lw.numel(), b"2 <= m <= 1024"),
                           (4, lw.numel() - 1, b"workspace too small")):
        rc = L.holo_density_lattice(h, runtime.ptr(grid), m, runtime.ptr(fd), runtime.ptr(lw), nbytes, st)
        assert rc < 0 and msg in L.holo_last_error()
    assert L.holo_density_lattice(h, null, 4, runtime.ptr(fd), runtime.ptr(lw), lw.numel(), st) < 0


def make_implicit_function(gu, R, Cf, seed=811, volume_extent=8.0):
    sd = gu.synth_state_dict(ro.render_mlp_param_shapes(ro.RenderCfg(resol=R, feature_size=Cf)), seed + Cf)
    sd["_density_net.mlp.3.0.bias"][-1] += 0.05
    fn = hda.HoloVoxelGridImplicitFunction(resol=R, n_hidden=Cf, feature_dim=0, volume_extent=volume_extent)
    fn.render_mlp.load_state_dict(sd)
    return fn.to(gu.DEV), sd


def folded_density_row(sd):
    """float64 fold of the four activation-free density layers: (we (C,), be) of the density output (the last row)."""
    W = [sd[f"_density_net.mlp.{i}.0.weight"].double().numpy() for i in range(4)]
    b = [sd[f"_density_net.mlp.{i}.0.bias"].double().numpy() for i in range(4)]
    Hd = W[1].shape[0]
    W2a, W2b = W[2][:, :Hd], W[2][:, Hd:]
    We = W[3] @ (W2a @ W[1] @ W[0] + W2b)
    be = W[3] @ (W2a @ (W[1] @ b[0] + b[1]) + b[2]) + b[3]
    return We[-1], be[-1]


@pytest.mark.parametrize("Cf", [32, 16])
@pytest.mark.parametrize("m", [8, 15, 21])  # on the voxel centres, odd (2R - 1), finer than 2R
def test_density_lattice_equals_the_implicit_function(gu, Cf, m):
    """holo_density_lattice against holo_implicit_eval at the same float32 points (built here by the pinned formula
    i * spacing - h).  Both form the same local coordinates and trilinear weights with the same arithmetic, so they differ
    in summation order only: the lattice sums 8 weighted per-voxel scalars S = w_dens . F (C fused multiply-adds each), the
    implicit function interpolates the C features (8 terms each) and then takes the dot product.  With |F| <= 1 and weights
    that sum to <= 1, every one of the C + 8 + 8 roundings is at most 2^-24 of a partial sum bounded by A = sum|we| + |be|,
    on either side: |difference| <= (C + 16) * 2^-23 * A.  The LeakyReLU (slope <= 1) does not widen it."""
    assert mesh.half_extent(8, 8.0) == 3.5
    lattice_equals_the_implicit_function(gu, Cf, m, 8.0)


def lattice_equals_the_implicit_function(gu, Cf, m, volume_extent):
    """The body of test_density_lattice_equals_the_implicit_function (shared with tests/test_gpu_render_scene.py) on an
    8^3 grid of ``volume_extent``."""
    R = 8
    fn, sd = make_implicit_function(gu, R, Cf, volume_extent=volume_extent)
    grid = torch.tanh(torch.from_numpy(np_noise(60 + Cf, (1, Cf, R, R, R)))).to(gu.DEV)
    h = mesh.half_extent(R, volume_extent)
    field = mesh.density_lattice(fn, grid, m)
    assert tuple(field.shape) == (m, m, m)
    ax = ref.lattice_axis(h, m)
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    pts = torch.from_numpy(np.stack([X, Y, Z], axis=-1).reshape(1, -1, 3).astype(np.float32)).to(gu.DEV)
    dens, _, _ = fn(pts_3d=pts, voxel_grid_features=grid)
    we, be = folded_density_row(sd)
    tol = (Cf + 16) * 2.0 ** -23 * (np.abs(we).sum() + abs(be))
    err = (field.reshape(-1).cpu() - dens.reshape(-1).cpu()).abs().max().item()
    print(f"C={Cf} m={m}: max|lattice - implicit| = {err:.3e}, tolerance {tol:.3e}, A = {np.abs(we).sum() + abs(be):.3f}")
    assert torch.isfinite(field).all() and field.std() > 0
    assert err <= tol


@pytest.fixture(scope="module")
def tiny_model(gu):
    model, *_ = gu.make_model(8, 32, 8, 16, TINY_UNET, density_bias=0.3)
    # a planted blob: a ball of one feature vector in a grid of its negative
    g = np.linspace(-1, 1, 8)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    ball = torch.from_numpy(((X - 0.1) ** 2 + (Y + 0.15) ** 2 + Z ** 2 < 0.45).astype(np.float32))
    vec = torch.tanh(torch.from_numpy(np_noise(91, (32,))))
    vf = (vec[None, :, None, None, None] * (2.0 * ball - 1.0)[None, None]).contiguous().to(gu.DEV)
    return model, vf


def test_model_extract_mesh(gu, tiny_model):
    model, vf = tiny_model
    fn = model._implicit_functions[-1]._fn
    refined = model._refine(vf)
    field = mesh.density_lattice(fn, refined, 15)
    lo, hi = max(field.min().item(), 0.0), field.max().item()
    assert hi > lo, "the test's grid has no positive density to mesh"
    level = 0.5 * (lo + hi)
    out = model.extract_mesh(vf, density_level=level)
    V = out["verts"].shape[0]
    assert V > 0 and out["faces"].shape[0] > 0 and out["density_level"] == level
    assert out["verts"].dtype == torch.float32 and out["faces"].dtype == torch.int32
    assert tuple(out["normals"].shape) == (V, 3) and tuple(out["colours"].shape) == (V, 3)
    faces = out["faces"].cpu().numpy()
    assert faces.min() >= 0 and faces.max() < V
    assert (ref.edge_use(faces)[1] % 2 == 0).all()
    col = out["colours"].cpu()
    assert col.min() >= 0.0 and col.max() <= 1.0
    nn = out["normals"].cpu().norm(dim=1)
    assert (((nn - 1.0).abs() < 1e-5) | (nn == 0.0)).all() and (nn > 0).any()
    assert out["verts"].abs().max().item() <= mesh.half_extent(8, 8.0)
    # ... equal to composing the public functions by hand (default resolution 2 R - 1 = 15)
    verts, tris = mesh.surface_nets(field, level, mesh.half_extent(8, 8.0))
    normals, colours = mesh.vertex_attributes(fn, refined, verts)
    for key, want in (("verts", verts), ("faces", tris), ("normals", normals), ("colours", colours)):
        assert torch.equal(out[key], want), key
    # normals point outward: along falling density
    step = out["verts"] + 0.05 * out["normals"]
    d_out, _, _ = fn(pts_3d=step[None], voxel_grid_features=refined)
    d_at, _, _ = fn(pts_3d=out["verts"][None], voxel_grid_features=refined)
    assert (d_out.reshape(-1) < d_at.reshape(-1))[nn.to(d_at.device) > 0].float().mean().item() > 0.95
    plain = model.extract_mesh(vf, resolution=9, density_level=level, colours=False)
    assert plain["colours"] is None and plain["verts"].shape[0] > 0


def test_model_extract_mesh_arguments(gu, tiny_model):
    model, vf = tiny_model
    with pytest.raises(ValueError, match="one grid"):
        model.extract_mesh(torch.cat([vf, vf]))
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="density_level"):
            model.extract_mesh(vf, density_level=bad)
    out = model.extract_mesh(vf, resolution=5)  # voxel size 1: the default level is ln 2 at opacity 0.5
    assert out["density_level"] == pytest.approx(math.log(2.0), rel=1e-12)
    assert out["faces"].shape[0] == 0 or out["faces"].max().item() < out["verts"].shape[0]
