"""The fused renderer off the diagonal of its supported range: sample counts, kernel instantiations, scheduling forms and
inputs that the tests written with the kernels never reach.

The library takes 3 <= n_pts_coarse <= 64 and 2 <= n_pts_fine <= 128 (holo_renderer_create, render_launch); the other render
files run the coarse count 64 in evaluation mode and five (coarse, fine) pairs in training mode, always with benign inputs and
the default scheduling.  Here:

  A. the (coarse, fine) table below through evaluation mode (both kernels), the training-mode forward and the backward;
  B. rendered normals on the instantiations no other test launches;
  C. the scheduling forms behind the knobs that are read when a renderer handle is created;
  D. inputs at the ends of the compositing arithmetic (saturated, opaque, empty, vanishing densities).

The reference is always oracle/render_oracle.py at the bounds of tests/test_gpu_render.py (evaluation mode) and
tests/test_gpu_training_mode.py (training mode): rgb / mask 2e-4 absolute, coarse depth 2e-4 of the far plane, fine depth
2e-4 (evaluation) / 1e-3 (training) of the far plane, rendered normals 5e-4; the backward criteria are those inside
tests/test_gpu_render_backward.py::_render_rays_backward_case.  Every case prints its worst errors.

Which kernel a case reaches (render_plan, render_plan.h / render_launch, kernels_render.hip; CH = feature_size / 2):
  training mode                                       render2_kernel<CH, 64 | 128, true, NW>
  f32_bf16x3 at 32 features                           render_kernel<16, true, NRM, 64 | 128>      (ray per column)
  normals with more than 32 features or 64 new samples  render_kernel<CH, false, true, 64 | 128>
  other normals                                       render2_kernel<CH, 64, false, 10 | 8, true>
  everything else                                     render2_kernel<CH, 64 | 128, false, NW>
with 64 | 128 by n_pts_fine <= 64 and NW = 12 / 8 (16, 32 / 64 features) for 64 new samples, 8 / 4 for 128.

Every torch.empty of the wrappers is NaN-filled (tests/test_gpu_cu_counts.py::_poison_empty): a ray that a kernel skipped
must not find the right value an earlier identical call left in the block the allocator hands back."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, runtime  # noqa: E402
from holo_diffusion_amd.render import EvaluationMode  # noqa: E402
from oracle import render_oracle as ro  # noqa: E402
from oracle.common import np_noise  # noqa: E402

from tests import gpu_utils as gu  # noqa: E402
from tests import test_gpu_cu_counts as tcc  # noqa: E402
from tests.test_gpu_cu_counts import cu  # noqa: E402,F401  (the fixture)
from tests.test_gpu_render import TINY_UNET  # noqa: E402
from tests.test_gpu_render_backward import _render_rays_backward_case  # noqa: E402
from tests.test_gpu_training_mode import _oracle_training_render, _streams  # noqa: E402

FAR = 14.0  # camera distance 10 + scene extent 4
ZMIN = 6.0
UP = (0.0, -1.0, 0.0)

# (coarse, fine)
COUNTS = [(3, 2),      # the minima: nb = 2 cdf entries
          (5, 3),      # odd / odd, a merged list of 8
          (9, 7),      # one more than a column group of 8 depths
          (33, 65),    # crosses lane 32; the first new-sample count of the 128-wide instantiations
          (63, 127),   # one below each maximum: nm = 190, the last lane's three merged positions partly empty
          (64, 63),    # the 64-wide instantiations one below their cap
          (17, 128),   # the most new samples over a short coarse row
          (64, 128)]   # nm = 192: all three positions of lane 63 in use
_ids = lambda v: f"{v[0]}+{v[1]}" if isinstance(v, tuple) else str(v)  # noqa: E731

_REF = {}


def _cached(key, make):
    """One oracle run (or one default-form render) per case, shared by the tests that need it and left unchanged."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


@pytest.fixture(autouse=True)
def _poisoned_outputs(monkeypatch):
    tcc._poison_empty(monkeypatch)


_KNOBS = ("HOLO_RENDER_V1", "HOLO_RENDER2_NW", "HOLO_RENDER2_NRM_NW", "HOLO_RENDER_STATIC_TILES", "HOLO_RENDER_TAIL",
          "HOLO_RENDER_XCD", "HOLO_RENDER_WGS")


def _cameras(n_cams):
    return hda.get_simple_360_camera_trajectory(2 * math.pi, n_cams, -30.0 * (2 * math.pi / 360), 10, UP, 3.2)


def _noise_grid(seed, C, R, scale=1.0):
    return torch.tanh(torch.from_numpy(np_noise(seed, (1, C, R, R, R)))) * scale


def _blob_grid(seed, C, R, scale=4.0, centre=(3.3, 4.1, 3.6), radius=1.6):
    """A compact object: the noise grid, scaled, inside a ball around ``centre`` (voxel coordinates x, y, z) and zero outside."""
    ax = torch.arange(R, dtype=torch.float32)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    ball = ((xx - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (zz - centre[2]) ** 2) < radius ** 2
    return _noise_grid(seed, C, R, scale) * ball[None, None].float()


def _eval_model(R, C, H, W, nc, nf, bias=0.05, compute="f32", own=lambda m: m, model_kw=None, rcfg_kw=None):
    """The model of tests/test_gpu_render.py::_render_pair with ``nc`` coarse samples in evaluation mode, and the oracle's
    configuration and weights of the same renderer.  ``model_kw`` / ``rcfg_kw``: the scene, see gpu_utils.make_model."""
    model, _, _, _, msd = gu.make_model(R, C, H, W, TINY_UNET, n_fine=nf, density_bias=bias, model_kw=model_kw)
    own(model)
    model.net_3d_enabled = False
    model.raysampler.n_pts_per_ray_evaluation = nc
    model.renderer.compute_dtype = compute
    rcfg = ro.RenderCfg(resol=R, feature_size=C, image_height=H, image_width=W, n_pts_coarse=nc, n_pts_fine=nf,
                        **(rcfg_kw or {}))
    return model, msd, rcfg


def _render_eval(model, grid, cams, normals=False):
    """holo_render through the renderer plugin for all of ``cams``: the planes of both passes, (n_cams, c, H, W) on the CPU."""
    model._implicit_functions[0]._fn.render_normals = bool(normals)
    for fn in model._implicit_functions:
        fn.bind_args(voxel_grid_features=grid.to(gu.DEV))
    try:
        bundle = model.raysampler(cams.to(gu.DEV), EvaluationMode.EVALUATION)
        out = model.renderer(ray_bundle=bundle, implicit_functions=list(model._implicit_functions),
                             evaluation_mode=EvaluationMode.EVALUATION)
    finally:
        for fn in model._implicit_functions:
            fn.unbind_args()
    pl = lambda t: t.permute(0, 3, 1, 2).cpu().clone()  # noqa: E731
    res = {"rgb": pl(out.features), "depth": pl(out.depths), "mask": pl(out.masks), "rgb_c": pl(out.prev_stage.features),
           "depth_c": pl(out.prev_stage.depths), "mask_c": pl(out.prev_stage.masks)}
    if normals:
        res["normals"], res["normals_c"] = pl(out.normals), pl(out.prev_stage.normals)
    else:
        assert out.normals is None and out.prev_stage.normals is None
    return res


def _oracle_eval(grid, msd, cams, rcfg, normals=False):
    """The oracle's planes of the same frames, stacked like _render_eval's."""
    names = {"rgb": "images_render", "depth": "depths_render", "mask": "masks_render", "rgb_c": "images_coarse",
             "depth_c": "depths_coarse", "mask_c": "masks_coarse"}
    if normals:
        names.update({"normals": "normals_render", "normals_c": "normals_coarse"})
    refs = [ro.render(grid, msd, gu.cam_dict(cams, i), rcfg, return_coarse=True, with_normals=normals) for i in range(len(cams))]
    return {k: torch.cat([r[v] for r in refs]) for k, v in names.items()}


EVAL_TOL = {"rgb": 2e-4, "mask": 2e-4, "rgb_c": 2e-4, "mask_c": 2e-4, "depth": 2e-4 * FAR, "depth_c": 2e-4 * FAR,
            "normals": 5e-4, "normals_c": 5e-4}
TRAIN_TOL = dict(EVAL_TOL, depth=1e-3 * FAR)


def _check(got, ref, what, tol=EVAL_TOL, keys=None, far=FAR):
    """Every plane finite and within its bound of the reference; prints the worst error of each (depths as a fraction of
    the far plane).  ``far``: the case's own far plane (gpu_utils.far_plane) where it is not the default scene's 14 - the
    depth bounds of ``tol`` are fractions of it.  Returns the errors."""
    errs = {}
    for k in (keys or ref):
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert torch.isfinite(got[k]).all(), (what, k)
        errs[k] = (got[k] - ref[k]).abs().max().item()
    print(f"\n{what}: " + ", ".join(f"{k} {e / (far if 'depth' in k else 1.0):.1e}" for k, e in errs.items()))
    for k, e in errs.items():
        bound = tol[k] * (far / FAR) if "depth" in k else tol[k]
        assert e < bound, (what, k, e, bound)
    return errs


def _bit_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _scratch_bytes(model, R, C, normals=False):
    """Bytes of per-wave scratch the handle asks for (holo_render_workspace_bytes less the channels-last grid, the 256-byte
    pad and, with normals, the density scalar field and the second copy): 32 KB per resident wave on the ray-per-column
    kernel, the 256-byte counter area on the (ray, depth)-tiled one."""
    nbytes = int(runtime.lib().holo_render_workspace_bytes(model.renderer._handle, 1, 1 if normals else 0))
    nbytes -= R ** 3 * C * 4 + 256
    if normals:
        assert (nbytes - R ** 3 * 4) % 2 == 0
        nbytes = (nbytes - R ** 3 * 4) // 2
    return nbytes


def _on_ray_per_column_kernel(model, R, C, normals=False):
    """Which kernel family the handle's last configuration selects (render_plan), read from its scratch size."""
    nbytes = _scratch_bytes(model, R, C, normals)
    assert nbytes == 256 or (nbytes >= 32768 and nbytes % 32768 == 0), nbytes
    return nbytes != 256


# ==== A. sample counts ==========================================================================================================
def _eval_counts_case(nc, nf, C, compute, own=lambda m: m):
    R, H, W = 8, 6, 7
    model, msd, rcfg = _eval_model(R, C, H, W, nc, nf, compute=compute, own=own)
    grid, cams = _noise_grid(2101 + nc, C, R), _cameras(4)[[1]]
    ref = _cached(("evalA", nc, nf, C), lambda: _oracle_eval(grid, msd, cams, rcfg))
    got = _render_eval(model, grid, cams)
    _check(got, ref, f"evaluation ({nc},{nf}) C={C} {compute}")
    assert float(ref["mask"].min()) < 0.9 and float(ref["mask"].max()) > 0.5  # (not an empty and not a solid frame)
    return model


@pytest.mark.parametrize("counts,C", [(c, 16) for c in COUNTS] + [((33, 65), 64), ((63, 127), 64), ((64, 63), 64)], ids=_ids)
def test_evaluation_mode_counts_exact_fp32(counts, C):
    """Evaluation mode with n_pts_per_ray_evaluation set (no other test does), exact fp32, all six planes of both passes: a
    6 x 7 frame - 11 tiles of four rays, the last one of two; one workgroup, whose last 6 tiles (half its 12 waves; 3 on the
    emulation) go out as single-ray items of 32 depths, so both column mappings clamp at nc - 1.
      16 features: render2_kernel<8, 64, false, 12> up to 64 new samples, render2_kernel<8, 128, false, 8> above;
      64 features: (33,65) and (63,127) on render2_kernel<32, 128, false, 4>, (64,63) on render2_kernel<32, 64, false, 8>."""
    nc, nf = counts
    model = _eval_counts_case(nc, nf, C, "f32")
    assert not _on_ray_per_column_kernel(model, 8, C)


@pytest.mark.parametrize("counts", COUNTS, ids=_ids)
def test_evaluation_mode_counts_ray_per_column_kernel(counts):
    """The same table at 32 features under compute_dtype = "f32_bf16x3": render_kernel<16, true, false, 64> up to 64 new
    samples and render_kernel<16, true, false, 128> above see a coarse count other than 64 (ZCAP rows, MAXC scratch rows).
    That the split is active - 32 features, render_plan picks the ray-per-column family - shows in the handle's scratch: 32 KB per
    resident wave instead of none."""
    nc, nf = counts
    model = _eval_counts_case(nc, nf, 32, "f32_bf16x3")
    assert model.renderer.compute_dtype == "f32_bf16x3" and model._implicit_functions[0]._fn.n_hidden == 32
    assert _on_ray_per_column_kernel(model, 8, 32)


def _training_case(P, Pf, C, which, seed, n_cam=2, n_rays=13, case="", model_kw=None, rcfg_kw=None, cams=None,
                   density_bias=0.0, grid_scale=1.0, probe=None):
    """The body of tests/test_gpu_training_mode.py::test_training_mode_render_vs_oracle at 2 x 13 rays (four tiles per camera,
    the last one of a single ray).  ``case``: the name of a scene other than the default one, given by ``model_kw`` /
    ``rcfg_kw`` (gpu_utils.make_model), ``cams`` (``n_cam`` cameras in place of the orbit's), ``density_bias`` and
    ``grid_scale``; its depth bounds are fractions of its own far plane.  ``probe``: called with (the oracle's planes, grid,
    msd, cams, xys, rs, rcfg) - a caller's check that the inputs are the case it means."""
    R = 8
    model, _, _, _, msd = gu.make_model(R, C, 16, 16, TINY_UNET, n_fine=64, density_bias=density_bias, model_kw=model_kw)
    model.raysampler.n_pts_per_ray_training = P
    model.renderer.n_pts_per_ray_fine_training = Pf
    rcfg = ro.RenderCfg(resol=R, feature_size=C, image_height=16, image_width=16, n_pts_coarse=P, n_pts_fine=Pf,
                        **(rcfg_kw or {}))
    grid = _noise_grid(2201 + P, C, R, grid_scale)
    if cams is None:
        cams = hda.get_simple_360_camera_trajectory(2 * math.pi, n_cam, -0.5, 10, UP, 3.2)
    assert len(cams) == n_cam
    far = gu.far_plane(cams, rcfg) if case else FAR
    xys = (torch.from_numpy(np_noise(2211 + P, (n_cam, n_rays, 2))).clamp(-2, 2) * 0.45).contiguous()
    rs = _streams(n_cam, n_rays, P, Pf, seed)
    if which == "no_u_coarse":  # un-jittered coarse depths under stratified importance samples and noise
        model.raysampler.stratified_point_sampling_training = False
        rs = {k: v for k, v in rs.items() if k != "u_coarse"}
    for fn in model._implicit_functions:
        fn.bind_args(voxel_grid_features=grid.to(gu.DEV))
    bundle = model.raysampler(cams.to(gu.DEV), EvaluationMode.TRAINING, xys=xys.to(gu.DEV))
    out = model.renderer(ray_bundle=bundle, implicit_functions=list(model._implicit_functions),
                         evaluation_mode=EvaluationMode.TRAINING, rng_streams={k: v.to(gu.DEV) for k, v in rs.items()})
    ref = _cached(("train", P, Pf, C, which, seed, case),
                  lambda: {k: v.reshape(n_cam, n_rays, -1) for k, v in
                           _oracle_training_render(grid, msd, cams, xys, rs, rcfg, 1.0, gu).items()})
    g = lambda t: t.reshape(n_cam, n_rays, -1).cpu().clone()  # noqa: E731
    got = {"rgb": g(out.features), "depth": g(out.depths), "mask": g(out.masks), "rgb_c": g(out.prev_stage.features),
           "depth_c": g(out.prev_stage.depths), "mask_c": g(out.prev_stage.masks)}
    _check(got, ref, f"training ({P},{Pf}) C={C} [{which}]" + (" " + case if case else ""), TRAIN_TOL, far=far)
    if probe is not None:
        probe(ref, grid, msd, cams, xys, rs, rcfg)
    return got


@pytest.mark.parametrize("counts,which", [(c, "all") for c in COUNTS] + [((9, 7), "no_u_coarse")], ids=_ids)
def test_training_mode_counts(counts, which):
    """holo_render_rays at 16 features with the random streams injected, 2 cameras x 13 rays, density noise of std 1:
    render2_kernel<8, 64, true, 12> up to 64 new samples, render2_kernel<8, 128, true, 8> above.
      all:         jittered coarse depths (the merged rank is a binary search), unsorted importance samples (the odd-even
                   sort of nf entries), noise indexed by merged position;
      no_u_coarse: the ray sampler's stratification off and no u_coarse stream: the coarse depths stay the linspace and the
                   merged rank of the (sorted, random) importance samples is the arithmetic one with its two fix-up steps,
                   on a row of nine."""
    P, Pf = counts
    _training_case(P, Pf, 16, which, 2300 + P)


@pytest.mark.parametrize("P,Pf,C,R,n_cam,n_rays", [(3, 2, 16, 8, 2, 5), (5, 3, 16, 8, 1, 1), (33, 65, 16, 8, 2, 7),
                                                   (63, 127, 32, 8, 1, 6), (9, 7, 64, 4, 2, 3)])
def test_backward_counts(P, Pf, C, R, n_cam, n_rays):
    """holo_render_rays_backward through _render_rays_backward_case: the training-mode forward above (which hands its merged
    depth list to the backward kernels), rbwd_* over nm = P + Pf points per ray.  All rows stay under the helper's 50 000
    sample threshold: the strict 1e-3 max-norm branch."""
    assert n_cam * n_rays * (P + Pf) <= 50000
    _render_rays_backward_case(gu, P, Pf, C, R, n_cam, n_rays, "all", seed=2400)


@pytest.mark.parametrize("nc,nf", [(2, 64), (65, 64), (64, 1), (64, 129)])
@pytest.mark.parametrize("mode", ["evaluation", "training"])
def test_counts_outside_the_range_are_refused(nc, nf, mode):
    """One below and one above each bound: holo_renderer_create refuses the coarse counts and one new sample, render_launch
    refuses 129 new samples before it launches a render kernel."""
    R, C = 8, 16
    model, msd, rcfg = _eval_model(R, C, 6, 7, nc, nf)
    grid, cams = _noise_grid(2501, C, R), _cameras(4)[[1]]
    if mode == "evaluation":
        with pytest.raises(_lib.HoloError):
            _render_eval(model, grid, cams)
        return
    model.raysampler.n_pts_per_ray_training = nc
    model.renderer.n_pts_per_ray_fine_training = nf
    for fn in model._implicit_functions:
        fn.bind_args(voxel_grid_features=grid.to(gu.DEV))
    bundle = model.raysampler(cams.to(gu.DEV), EvaluationMode.TRAINING, xys=torch.zeros(1, 5, 2, device=gu.DEV))
    with pytest.raises(_lib.HoloError):
        model.renderer(ray_bundle=bundle, implicit_functions=list(model._implicit_functions),
                       evaluation_mode=EvaluationMode.TRAINING)


# ==== B. rendered normals =========================================================================================================
@torch.no_grad()
def _oracle_samples(grid, msd, cam, rcfg):
    """The oracle's sample placement of one frame: origins, directions, and (lengths, weights, raw densities) of both passes."""
    o, d, l = ro.make_rays(cam, rcfg)
    dens, col = ro.implicit_function(grid, msd, o, d, l, rcfg)
    *_, w = ro.ea_raymarch(dens, col, l, rcfg)
    lf = ro.refine_lengths(l, w, rcfg)
    dens_f, col_f = ro.implicit_function(grid, msd, o, d, lf, rcfg)
    *_, wf = ro.ea_raymarch(dens_f, col_f, lf, rcfg)
    return o, d, (l, w, dens[..., 0]), (lf, wf, dens_f[..., 0])


def _face_distance(grid, msd, cam, rcfg):
    """Smallest distance (in voxels) of any coordinate of any oracle sample of weight above 1e-3 from an integer grid
    coordinate - the cell faces, the volume's boundary planes 0 and R - 1 and the ends of the zero padding, -1 and R.  Only
    samples inside the padded cube [-1, R]^3 (the planes themselves included) count: outside it the features are zero in a
    whole neighbourhood and the gradient is zero on both sides of every plane."""
    o, d, coarse, fine = _oracle_samples(grid, msd, cam, rcfg)
    R = rcfg.resol
    half = 0.5 * (R - 1) * (rcfg.volume_extent / R)
    worst = float("inf")
    for z, w, _ in (coarse, fine):
        idx = ((o[:, None, :] + z[:, :, None] * d[:, None, :]) / half + 1.0) * 0.5 * (R - 1)
        inside = ((idx > -1.0 - 1e-3) & (idx < R + 1e-3)).all(dim=-1)
        at_risk = inside & (w > 1e-3)
        if bool(at_risk.any()):
            worst = min(worst, float((idx - idx.round()).abs().amin(dim=-1)[at_risk].min()))
    return worst


NORMALS_CASES = [  # coarse, fine, features, compute, camera (of how many, index), grid seed
    (64, 128, 16, "f32", (7, 0), 2604),         # render_kernel<8, false, true, 128>
    (64, 128, 32, "f32", (7, 0), 2602),         # render_kernel<16, false, true, 128>
    (64, 128, 64, "f32", (7, 0), 2605),         # render_kernel<32, false, true, 128>
    (64, 64, 32, "f32_bf16x3", (7, 0), 2602),   # render_kernel<16, true, true, 64>
    (64, 100, 32, "f32_bf16x3", (7, 0), 2601),  # render_kernel<16, true, true, 128>
    (33, 65, 32, "f32", (11, 6), 2603),         # render_kernel<16, false, true, 128>, 33 coarse
    (17, 31, 64, "f32", (7, 2), 2602),          # render_kernel<32, false, true, 64>, 17 coarse
    (17, 31, 16, "f32", (7, 2), 2601),          # render2_kernel<8, 64, false, 10, true>, 17 coarse
]


@pytest.mark.parametrize("nc,nf,C,compute,cam,seed", NORMALS_CASES, ids=[f"{c[0]}+{c[1]}-C{c[2]}-{c[3]}" for c in NORMALS_CASES])
def test_rendered_normals_on_other_instantiations(nc, nf, C, compute, cam, seed):
    """render_normals = True on a 9 x 11 frame as tests/test_gpu_render.py::test_rendered_normals_vs_oracle checks it: the
    normals of both passes within 5e-4 of the oracle, the other planes within their bounds of the oracle and of the same
    model rendered without normals.  Instantiations: see NORMALS_CASES; render_instance_exists (more than 32 features or 64 new samples: no tiled normals) sends
    all but the last to the ray-per-column kernel, whose normals variants have only run at 64 coarse and at most 64 new
    samples, never under the split arithmetic; the last one is the (ray, depth)-tiled normals kernel (10 waves; 8 on the
    emulation) at a coarse count other than 64.

    The scene is chosen, not filtered afterwards.  The rendered normal is sum_i w_i n_i with n_i the NORMALISED density
    gradient: a sample on a face of its grid cell, on the volume's boundary plane or at the end of the zero padding (an
    integer grid coordinate) has a gradient that jumps - between two unit vectors, or between a unit vector and zero - with
    the rounding of that one coordinate, and an opaque sample there moves the pixel by O(1) while every other plane agrees
    to 1e-6.  So the test computes the grid coordinates of all of the ORACLE's samples and asserts that those of weight
    above 1e-3 keep 1e-4 voxels from every integer; no pixel is set aside.  What that takes:
      - not the orbit of the other render tests: its elevation of -30 degrees (sin = 1 / 2) and azimuths of 90 degrees put
        whole rows of coarse samples on grid planes - the row y_ndc = 0 of an odd-height frame at every depth that is a
        multiple of the voxel size (17 and 33 coarse samples), a pixel column with x_ndc / focal = -1 / 4 on the boundary
        plane (5 x 7: two pixels 0.30 and 1.09 off; the background interval of 1e10 makes such a last sample opaque under a
        positive density bias).  The cameras here have an elevation of -0.5 rad and are picked for the clearance of their
        coarse samples, which depends on no grid;
      - not a grid that fills the volume: importance samples sit where the weight is, so on a full noise grid some 12 000
        samples of the 99 rays x (64 + 128) carry more than 1e-3, three coordinates each, 2e-4 of every unit interval
        forbidden: seven expected violations, and none of 400 grid seeds was free of them.  The scene is a compact object
        (_blob_grid: the noise grid x 4 inside a ball of radius 1.6 voxels, density bias -0.5 so that the rest is empty):
        a dozen rays with a few hundred weighted samples, masks up to 0.3 .. 0.95; the grid seed of each case was picked
        for a clearance of at least 1.5e-4.  The other rays render exact zeros and the background."""
    R, H, W = 8, 9, 11
    model, msd, rcfg = _eval_model(R, C, H, W, nc, nf, bias=-0.5, compute=compute)
    grid = _blob_grid(seed, C, R)
    cams = hda.get_simple_360_camera_trajectory(2 * math.pi, cam[0], -0.5, 10, UP, 3.2)[[cam[1]]]
    ref, clear = _cached(("normals", nc, nf, C), lambda: (_oracle_eval(grid, msd, cams, rcfg, normals=True),
                                                          _face_distance(grid, msd, gu.cam_dict(cams, 0), rcfg)))
    assert 1e-4 <= clear < 1.0, f"an oracle sample of weight > 1e-3 lies {clear:.1e} voxels from a cell face: choose another scene"
    plain = _render_eval(model, grid, cams)
    got = _render_eval(model, grid, cams, normals=True)
    what = f"normals ({nc},{nf}) C={C} {compute} (clearance {clear:.1e} voxels)"
    _check(got, ref, what)
    _check(got, plain, what + " against the render without normals")
    assert float(ref["normals"].abs().max()) > 0.05 and float(ref["normals_c"].abs().max()) > 0.05
    assert float(ref["mask"].max()) > 0.25 and float(ref["mask"].min()) == 0.0
    tiled = C <= 32 and nf <= 64 and compute == "f32"
    assert _on_ray_per_column_kernel(model, R, C, normals=True) == (not tiled)


# ==== C. scheduling forms =========================================================================================================
_SCHED = dict(R=8, C=16, H=9, W=11, nc=64, nf=64)


def _sched_render(monkeypatch, env, normals=False, n_cams=3, own=lambda m: m):
    """The scheduling workload - 8^3 x 16 grid, 9 x 11 frames (25 tiles of four rays a camera, the last one of three),
    (64,64) samples - rendered by a handle created under ``env`` (the knobs are read in holo_renderer_create)."""
    s = _SCHED
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, msd, rcfg = _eval_model(s["R"], s["C"], s["H"], s["W"], s["nc"], s["nf"], own=own)
    grid, cams = _noise_grid(2701, s["C"], s["R"]), _cameras(n_cams)
    got = _render_eval(model, grid, cams, normals=normals)
    return got, (grid, msd, cams, rcfg), model


def _sched_oracle(inputs, normals, n_cams=3):
    grid, msd, cams, rcfg = inputs
    return _cached(("sched", normals, n_cams), lambda: _oracle_eval(grid, msd, cams, rcfg, normals=normals))


_FORMS = {  # name: (environment, normals, bit-equality with the default form asserted)
    "static_tiles": ({"HOLO_RENDER_STATIC_TILES": "1"}, False, True),
    "nw8": ({"HOLO_RENDER2_NW": "8"}, False, True),
    "nrm_nw8": ({"HOLO_RENDER2_NRM_NW": "8"}, True, True),
    "tail0": ({"HOLO_RENDER_TAIL": "0"}, False, False),
    "tail1000": ({"HOLO_RENDER_TAIL": "1000"}, False, False),
    "v1": ({"HOLO_RENDER_V1": "1"}, False, False),
}


@pytest.mark.parametrize("form", list(_FORMS))
def test_scheduling_forms(form, monkeypatch):
    """Three cameras of the scheduling workload - 75 tiles: 7 workgroups of 12 waves by default (10 of 8 under
    HOLO_RENDER2_NW=8, 8 of 10 with normals), dynamic hand-out, the last 42 tiles in single-ray items - under one knob each,
    against the oracle, and compared with the default form (the comparison is printed; asserted where the code gives the
    reason):
      static_tiles  HOLO_RENDER_STATIC_TILES=1: tile = workgroup x waves + wave, then a stride, no tail.  The same 4-ray
                    items in another order, and the tail's single-ray items are the same rays in another column mapping -
                    see tail0; no ray's arithmetic depends on the wave that took it: bit-equal;
      nw8           HOLO_RENDER2_NW=8: render2_kernel<8, 64, false, 8> for <.., 12>: the same body on fewer waves: bit-equal;
      nrm_nw8       HOLO_RENDER2_NRM_NW=8 with normals: render2_kernel<8, 64, false, 8, true> for <.., 10, true>: bit-equal
                    (on the emulation both runs take the 8-wave form);
      tail0         HOLO_RENDER_TAIL=0: every tile as four rays x 8 depths per evaluation;
      tail1000      HOLO_RENDER_TAIL=1000 (clamped to the tile count): every tile as single rays x 32 depths;
      v1            HOLO_RENDER_V1=1: render_kernel<8, false, false, 64>, the ray-per-column kernel - another kernel."""
    env, normals, must_equal = _FORMS[form]
    base, inputs, base_model = _sched_render(monkeypatch, {}, normals=normals)
    ref = _sched_oracle(inputs, normals)
    _check(base, ref, f"scheduling default (normals={normals})")
    got, _, model = _sched_render(monkeypatch, env, normals=normals)
    _check(got, ref, f"scheduling {form}")
    same = _bit_equal(got, base)
    worst = max(float((got[k] - base[k]).abs().max()) for k in got)
    print(f"scheduling {form}: bit-equal to the default form: {same} (largest difference {worst:.1e})")
    s = _SCHED
    assert _on_ray_per_column_kernel(model, s["R"], s["C"], normals) == (form == "v1")
    assert not _on_ray_per_column_kernel(base_model, s["R"], s["C"], normals)
    if must_equal:
        assert same, (form, worst)


@pytest.mark.skipif(gu.EMU, reason="needs a planner CU count")
@tcc._cu(8)
def test_xcd_tile_order(cu, monkeypatch):
    """HOLO_RENDER_XCD=1 against the default tile order where the default has the XCD split ON: under HOLO_NUM_CUS=8 four
    cameras of the scheduling workload are 100 tiles -> ceil(100 / 12) = 9 workgroups, capped to 8 = n_wgs_max, a multiple of
    8 (three cameras would be 7 workgroups: no split).  The default then deals the tiles out in eight ranges of 12 or 13
    (boundaries 100 k / 8, inside cameras), each with its own counter and its own single-ray tail; HOLO_RENDER_XCD=1 in one
    range.  The same rays either way: bit-equal, and both within the bounds of the oracle."""
    n_cams, waves = 4, 12
    tiles = n_cams * ((_SCHED["H"] * _SCHED["W"] + 3) // 4)
    assert min(-(-tiles // waves), cu.n) == cu.n and cu.n % 8 == 0  # (render_launches: n_wgs == wg_cap && n_wgs % xcd == 0)
    base, inputs, _ = _sched_render(monkeypatch, {}, n_cams=n_cams, own=cu.own)
    ref = _sched_oracle(inputs, False, n_cams)
    _check(base, ref, "scheduling, 8 CUs, default XCD ranges")
    got, _, _ = _sched_render(monkeypatch, {"HOLO_RENDER_XCD": "1"}, n_cams=n_cams, own=cu.own)
    _check(got, ref, "scheduling, 8 CUs, HOLO_RENDER_XCD=1")
    same = _bit_equal(got, base)
    print(f"scheduling HOLO_RENDER_XCD=1 under 8 CUs: bit-equal to the default form: {same}")
    assert same


@pytest.mark.parametrize("env", [{"HOLO_RENDER2_NW": "8"}, {"HOLO_RENDER_TAIL": "0"}], ids=lambda e: "-".join(e))
def test_training_mode_under_scheduling_knobs(env, monkeypatch):
    """The training-mode render (2 x 13 rays, (24,20), all streams) by a handle created under HOLO_RENDER2_NW=8 -
    render2_kernel<8, 64, true, 8> for <.., 12> - and under HOLO_RENDER_TAIL=0 (holo_render_rays hands its tiles out with the
    static stride and no tail whatever the knob says: the knob must not reach it), against the oracle at the training-mode
    bounds and bit-equal to the default handle's."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    base = _training_case(24, 20, 16, "all", 2800)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = _training_case(24, 20, 16, "all", 2800)
    assert _bit_equal(got, base), env


# ==== D. inputs at the ends of the compositing arithmetic =======================================================================
_END_MODELS = [(16, "f32"), (32, "f32"), (32, "f32_bf16x3")]  # render2_kernel<8 | 16, 64, false, 12>, render_kernel<16, true, false, 64>


def _end_case(C, compute, nc=64, nf=64, grid_scale=1.0, bias=0.05, density_row_scale=None):
    """Evaluation mode, 6 x 7 frame: the render, the oracle's planes and the oracle's samples of the case."""
    R, H, W = 8, 6, 7
    model, msd, rcfg = _eval_model(R, C, H, W, nc, nf, bias=bias, compute=compute)
    if density_row_scale is not None:
        msd = dict(msd)
        for k in ("_density_net.mlp.3.0.weight", "_density_net.mlp.3.0.bias"):
            msd[k] = msd[k].clone()
            msd[k][-1] *= density_row_scale
        sd = model.state_dict()
        for i in range(model.num_passes):  # (assigned, not scaled in place: the passes may share their parameters)
            for k in ("_density_net.mlp.3.0.weight", "_density_net.mlp.3.0.bias"):
                sd[f"_implicit_functions.{i}._fn.render_mlp.{k}"][-1] = msd[k][-1]
        model.load_state_dict(sd)
    grid, cams = _noise_grid(2901, C, R, grid_scale), _cameras(4)[[1]]
    key = ("end", C, nc, nf, grid_scale, bias, density_row_scale)
    ref, samples = _cached(key, lambda: (_oracle_eval(grid, msd, cams, rcfg),
                                         _oracle_samples(grid, msd, gu.cam_dict(cams, 0), rcfg)))
    got = _render_eval(model, grid, cams)
    return got, ref, samples


def _largest_x(samples):
    """largest delta * relu(density) over the samples of both passes that have a finite interval behind them"""
    return max(float((z.diff(dim=-1) * dens[:, :-1].relu()).max()) for z, _, dens in samples[2:])


@pytest.mark.parametrize("C,compute", _END_MODELS)
@pytest.mark.parametrize("scale", [10.0, 100.0, 3000.0])
def test_saturated_densities(C, compute, scale):
    """The grid scaled by 10, 100 and 3000.  The feature-dependent part of the density pre-activation scales with the grid
    (largest density about 0.4 at scale 1): densities reach 3 to 5 at x 10 and 30 to 50 at x 100, where with the interval
    8 / 63 of 64 coarse samples x = delta * sigma gets to 0.7 and 6.7 - a single sample takes up to 0.9 of a ray, the
    transmittance behind it falls to 1e-3 - and 1000 to 1500 at x 3000: x passes 88, __expf(-x) underflows,
    T = 1 - (1 - __expf(-cum)) is exactly 0 behind that sample and it takes the ray's whole weight; the coarse cdf is a step,
    every importance sample lands in one bin.  All six planes at the plain bounds, finite."""
    got, ref, samples = _end_case(C, compute, grid_scale=scale)
    x = _largest_x(samples)
    sigma = max(float(d.max()) for _, _, d in samples[2:])
    w_top = max(float(w.max()) for _, w, _ in samples[2:])
    print(f"\ngrid x {scale:g}, C={C}: largest density {sigma:.1f}, largest x {x:.2f}, largest single-sample weight {w_top:.7f}")
    assert sigma > 0.2 * scale
    if scale == 3000.0:
        assert x > 88.0 and w_top > 0.999999
    _check(got, ref, f"grid x {scale:g} C={C} {compute}")


@pytest.mark.parametrize("C,compute", _END_MODELS)
@pytest.mark.parametrize("bias", [5.0, 50.0])
def test_opaque_from_the_first_sample(C, compute, bias):
    """Density bias +5 and +50: every sample is dense, the ray is spent within the first few samples - mask exactly 1 in
    both passes (the background interval of 1e10 behind a positive density), depth within 1 / sigma of z_min."""
    got, ref, samples = _end_case(C, compute, bias=bias)
    sigma_min = min(float(d.min()) for _, _, d in samples[2:])
    assert sigma_min > 0.5 * bias  # every sample dense
    assert float(ref["mask"].min()) == 1.0 and float(ref["mask_c"].min()) == 1.0
    assert float(ref["depth"].max()) < ZMIN + 2.0 / sigma_min and float(ref["depth_c"].max()) < ZMIN + 2.0 / sigma_min
    _check(got, ref, f"bias +{bias:g} C={C} {compute}")
    assert bool((got["mask"] == 1.0).all()) and bool((got["mask_c"] == 1.0).all())


@pytest.mark.parametrize("C,compute", _END_MODELS)
@pytest.mark.parametrize("counts", [(64, 64), (9, 7)], ids=_ids)
def test_empty_volume(C, compute, counts):
    """Density bias -5: no sample has a positive density.  Mask exactly 0, rgb the background bit for bit, depth exactly 0,
    in both passes (tests/test_gpu_render.py::test_zero_density_gives_background pins the fine pass at the default counts);
    the cdf is built from the eps terms alone."""
    nc, nf = counts
    got, ref, samples = _end_case(C, compute, nc=nc, nf=nf, bias=-5.0)
    assert max(float(d.max()) for _, _, d in samples[2:]) < 0.0
    assert float(ref["mask"].max()) == 0.0 and float(ref["mask_c"].max()) == 0.0
    _check(got, ref, f"bias -5 ({nc},{nf}) C={C} {compute}")
    for sfx in ("", "_c"):
        assert bool((got["mask" + sfx] == 0.0).all()) and bool((got["depth" + sfx] == 0.0).all())
        assert torch.equal(got["rgb" + sfx], torch.ones_like(got["rgb" + sfx]))  # bg_color (1, 1, 1)


@pytest.mark.parametrize("C,compute", _END_MODELS)
def test_vanishing_densities(C, compute):
    """The density output's weight row and bias entry scaled by 3e-5 (after a density bias of -0.15, which puts the
    pre-activation outside the volume just below zero at 16 and at 32 features): x = delta * sigma is about 1e-6 per
    sample, the cancellation end of 1 - __expf(-x) and of T = 1 - (1 - __expf(-cum)).  A ray whose last sample has no
    density has a mask of 1e-6 to 1e-4 (a few to a hundred such samples); one whose last sample has any takes the background interval of 1e10 and is opaque, with all its weight on that sample - both kinds are in the
    frame.  Held to the plain bounds like everything else; for the faint rays the mask's error RELATIVE to the oracle's mask
    is printed (no bound: the float32 oracle's own 1 - exp(-cumsum) carries 6e-8 absolute there)."""
    got, ref, samples = _end_case(C, compute, bias=-0.15, density_row_scale=3e-5)
    x = _largest_x(samples)
    assert 1e-7 < x < 1e-5, x
    _check(got, ref, f"densities x 3e-5 C={C} {compute}")
    for k in ("mask", "mask_c"):
        faint = ref[k] < 0.5
        assert int(faint.sum()) * 2 >= faint.numel(), (k, int(faint.sum()))
        assert 1e-6 < float(ref[k][faint].max()) < 1e-3, (k, float(ref[k][faint].max()))
        sel = faint & (ref[k] > 0.1 * float(ref[k][faint].max()))
        rel = float(((got[k] - ref[k]).abs()[sel] / ref[k][sel]).max())
        print(f"   {k}: {int(faint.sum())} of {faint.numel()} rays faint, the oracle's largest faint mask {float(ref[k][faint].max()):.2e}, "
              f"worst error relative to the oracle's mask {rel:.1e}")


@pytest.mark.parametrize("name,kw", [("grid_x10", dict(grid_scale=10.0)), ("bias+5", dict(density_bias=5.0))])
def test_backward_at_the_ends(name, kw):
    """The x 10 grid and the bias +5 case through _render_rays_backward_case at (12, 10, 16 features, 8^3, 2 x 9 rays):
    rbwd_composite_kernel works in double and is held to the helper's bounds; the helper's own assertion that the grid
    gradient is not negligible stays."""
    claims = {}

    def probe(grid, msd, cams, xys, rs, rcfg):
        ref = _oracle_training_render(grid, msd, cams, xys, rs, rcfg, 1.0, gu)
        claims["mask_min"], claims["mask_c_min"] = float(ref["mask"].min()), float(ref["mask_c"].min())
        claims["grid_max"] = float(grid.abs().max())

    _render_rays_backward_case(gu, 12, 10, 16, 8, 2, 9, "all", seed=3000, probe=probe, **kw)
    print(f"   backward {name}: oracle's smallest mask {claims['mask_min']:.6f} (coarse {claims['mask_c_min']:.6f}), "
          f"largest grid entry {claims['grid_max']:.2f}")
    if name == "bias+5":
        assert claims["mask_min"] == 1.0 and claims["mask_c_min"] == 1.0
    else:
        assert claims["grid_max"] > 9.0


# ==== E. more cameras than one launch holds =====================================================================================
@pytest.mark.parametrize("C,compute", [(16, "f32"), (32, "f32_bf16x3")])
def test_more_cameras_than_one_launch_holds(C, compute):
    """33 cameras in ONE holo_render call: the launch parameters hold 32, so the call is two launches of 17 + 16 cameras
    (render_launches, render_plan.h) - what the default fly-around of 40 poses does (20 + 20) and no other test reaches.
    5 x 6 frames: eight 4-ray tiles per camera, the last one of two rays; 8^3 grid, (9, 7) samples.
      16 features, exact fp32       the (ray, depth)-tiled kernel: the hand-out counters are zeroed again for the second launch;
      32 features, f32_bf16x3       the ray-per-column kernel: the second launch reuses the per-wave scratch of the first.
    Every plane of every camera finite and within EVAL_TOL of the oracle."""
    R, H, W, nc, nf, n_cams = 8, 5, 6, 9, 7, 33
    model, msd, rcfg = _eval_model(R, C, H, W, nc, nf, compute=compute)
    grid, cams = _noise_grid(3101, C, R), _cameras(n_cams)
    ref = _cached(("two_launches", C), lambda: _oracle_eval(grid, msd, cams, rcfg))
    got = _render_eval(model, grid, cams)
    assert got["rgb"].shape[0] == n_cams
    _check(got, ref, f"{n_cams} cameras, two launches, C={C} {compute}")
    assert _on_ray_per_column_kernel(model, R, C) == (compute == "f32_bf16x3")
    assert float(ref["mask"][17:].max()) > 0.5  # (the second launch's frames are not empty)
