"""The fused renderer off its default scene: volume extents, scene centre and extent, background colour and opacity, and
cameras whose depth bounds and intrinsics differ inside one launch.

Every other render file runs volume_extent 8, scene_center (0, 0, 0), scene_extent 4, a white background, background_opacity
1e10 and cameras of one radius and one focal length: a swapped background channel, a hard-coded last interval, a sign error
on the scene centre, a grid scale that only works for a one-unit voxel or camera 0's depth bounds read for every camera
would pass all of them.  Here:

  A. the scene table SCENES in evaluation mode, all six planes of both passes, on the (ray, depth)-tiled kernel (16 and 64
     features), on the ray-per-column kernel (32 features, f32_bf16x3) and with rendered normals;
  B. four cameras at centre distances 7, 10, 14 and 8.5 with their own focal lengths (fx != fy) and principal points, in one
     launch, over two launches (34 cameras), through the training-mode forward and the backward;
  C. the training-mode forward and the backward off the default scene;
  D. HoloDiffusionModel's pass-through of bg_color / volume_extent and the renderer handle's key on a live model;
  E. the same grid coordinate in the density lattice, the stand-alone implicit function and the mesh export;
  F. what holo_renderer_create and the Python wrapper refuse.

The reference is oracle/render_oracle.py (RenderCfg models every field) at the bounds of
tests/test_gpu_render_sample_counts.py - rgb / mask 2e-4 absolute, coarse depth 2e-4 and fine depth 2e-4 (evaluation) / 1e-3
(training) of the far plane, normals 5e-4, the backward criteria of _render_rays_backward_case - with the far plane the
case's own: the largest depth_bounds(...)[1] over its cameras (gpu_utils.far_plane).

Inputs.  The default noise grid and density bias give solid or empty frames off the default scene (outside the grid the
density is the bias alone, and a positive one times the background interval is opaque), so every scene has its own grid,
(negative) density bias and focal length, found with the oracle on the CPU (INPUTS).  Each evaluation case asserts on the
oracle's planes alone that at least 10 % of the rays have a fine mask below 0.1 and at least 10 % one above 0.5, that the
float32 oracle lies within a quarter of every bound of the same oracle in float64 (the small extents divide by a small
half_extent), and - where the scene is about the background - that swapping two background channels (`bg`, `all`) or
putting the background interval back to 1e10 (`bgop.5`, `bgop0`, `all`) would move the oracle's frame by more than 100
bounds.  Every case prints its errors next to the float32 oracle's own.

Worst errors measured on the MI355X, as fractions of the bound of the plane named (in brackets: the float32 oracle's own
distance from the float64 oracle on that plane, the same fraction):
  A. scene table, 16 features, exact fp32       0.024  rgb      `ve3`     [0.030]
     64 features, exact fp32                    0.017  mask_c   `ve5.3`   [0.017]
     32 features, f32_bf16x3 (ray per column)   0.083  mask     `ve5.3`   [0.006]
     `all` at (64, 64)                          0.005  depth              [0.002]
     `all` with rendered normals                0.131  mask_c   64 feat.  [0.009]; the normals themselves 0.043
  B. four cameras in one launch, 16 features    0.011  mask               [0.006]
     32 features, f32_bf16x3                    0.258  mask               [0.029]
     34 cameras, two launches                   0.05   mask_c (1.0e-5 absolute; bit-equal to the single renders)
     training forward, four cameras             0.004  mask (8.9e-7 absolute)
     backward, four cameras                     7.4e-6 of the gradient's max (bound 1e-3)
  C. backward per scene, (12, 10)               1.3e-5 (`all`, grid), bound 1e-3; at (24, 20, 32, 16^3) 1.0e-4
     training forward per scene                 0.006  mask     `centre` (1.1e-6 absolute)
  D. model level                                0.012  mask (2.4e-6 absolute)
  E. lattice against the implicit function      1.2e-7 of a tolerance of 4.5e-6, at both extents
The emulation (HOLO_TEST_EMU=1) passes every case as well; none of them found a kernel or host fault.

Every torch.empty of the wrappers is NaN-filled, as in tests/test_gpu_render_sample_counts.py."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, mesh, runtime  # noqa: E402
from oracle import render_oracle as ro  # noqa: E402
from oracle.common import np_noise  # noqa: E402

from tests import gpu_utils as gu  # noqa: E402
from tests import test_gpu_mesh as tgm  # noqa: E402
from tests.test_gpu_render import TINY_UNET  # noqa: E402
from tests.test_gpu_render_backward import _render_rays_backward_case  # noqa: E402
from tests.test_gpu_render_sample_counts import (  # noqa: E402,F401  (_poisoned_outputs: the autouse NaN-poisoning fixture)
    EVAL_TOL, FAR, UP, _bit_equal, _blob_grid, _cached, _check, _eval_model, _noise_grid, _on_ray_per_column_kernel,
    _oracle_eval, _poisoned_outputs, _render_eval, _training_case)
from tests.test_gpu_training_mode import _oracle_training_render  # noqa: E402

R, H, W = 8, 9, 11
BG = (0.1, 0.5, 0.9)
CENTRE = (0.7, -0.4, 0.5)

# name: the scene's settings (those not given are the defaults)
SCENES = {
    "default": {},
    "bg": dict(bg_color=BG),
    "bg1": dict(raymarcher_bg=(0.25,)),
    "ve5.3": dict(volume_extent=5.3),
    "ve3": dict(volume_extent=3.0),
    "ve20": dict(volume_extent=20.0),
    "centre": dict(scene_center=CENTRE, scene_extent=2.5),
    "se6": dict(scene_extent=6.0),
    "bgop.5": dict(background_opacity=0.5),
    "bgop0": dict(background_opacity=0.0),
    "all": dict(volume_extent=5.3, scene_center=CENTRE, scene_extent=3.0, bg_color=BG, background_opacity=0.5),
}
# name: the grid (_blob_grid: the noise grid x scale inside a ball of `radius` voxels, zero outside, where the negative density
# bias leaves nothing), the density bias and the focal length - see "Inputs" above.  The background interval only counts where
# the LAST sample has a density: for those scenes the ball sits on the far side of the volume, around the far samples of
# the central rays of camera 1 of 4 (voxel (0.04, 5.5, 3.5) for the central pixel).
_FAR_SIDE = (1.0, 5.5, 3.5)
INPUTS = {
    "default": dict(grid="blob", radius=2.6, scale=8.0, bias=-0.3, focal=3.2),
    "bg": dict(grid="blob", radius=2.6, scale=8.0, bias=-0.3, focal=3.2),
    "bg1": dict(grid="blob", radius=2.6, scale=8.0, bias=-0.3, focal=3.2),
    "ve5.3": dict(grid="blob", radius=3.2, scale=8.0, bias=-0.3, focal=4.5),
    "ve3": dict(grid="blob", radius=3.2, scale=16.0, bias=-0.3, focal=9.0),
    "ve20": dict(grid="blob", radius=2.6, scale=8.0, bias=-0.3, focal=3.2),
    "centre": dict(grid="blob", radius=2.6, scale=16.0, bias=-0.3, focal=3.2),
    "se6": dict(grid="blob", radius=3.2, scale=8.0, bias=-0.3, focal=3.2),
    "bgop.5": dict(grid="blob", radius=2.6, centre=_FAR_SIDE, scale=8.0, bias=-0.3, focal=4.5),
    "bgop0": dict(grid="blob", radius=2.6, centre=_FAR_SIDE, scale=8.0, bias=-0.3, focal=4.5),
    "all": dict(grid="blob", radius=3.2, scale=8.0, bias=-0.3, focal=4.5),
}


def _scene_kw(s):
    """(model_kw, rcfg_kw) of gpu_utils.make_model for the settings ``s`` of one scene."""
    model_kw, rcfg_kw, sampler, marcher = {}, {}, {}, {}
    for k, v in s.items():
        if k == "raymarcher_bg":
            marcher["bg_color"] = v
            rcfg_kw["bg_color"] = tuple(v) * 3 if len(v) == 1 else tuple(v)
            continue
        rcfg_kw[k] = v
        if k in ("volume_extent", "bg_color"):
            model_kw[k] = v
        elif k in ("scene_center", "scene_extent"):
            sampler[k] = v
        else:
            assert k == "background_opacity", k
            marcher[k] = v
    if sampler:
        model_kw["raysampler_AdaptiveRaySampler_args"] = sampler
    if marcher:
        model_kw["renderer_HoloMultiPassEmissionAbsorptionRenderer_args"] = dict(raymarcher_EmissionAbsorptionRaymarcher_args=marcher)
    return model_kw, rcfg_kw


def _orbit(n_cams, focal=3.2, elevation=-30.0 * (2 * math.pi / 360)):
    return hda.get_simple_360_camera_trajectory(2 * math.pi, n_cams, elevation, 10, UP, focal)


def _grid(inp, seed, C_):
    if inp["grid"] == "blob":
        return _blob_grid(seed, C_, R, inp["scale"], radius=inp["radius"], **({"centre": inp["centre"]} if "centre" in inp else {}))
    return _noise_grid(seed, C_, R, inp["scale"])


def _stack(cat, normals, rcfg):
    pl = lambda t, c: t.reshape(1, rcfg.image_height, rcfg.image_width, c).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    res = {"rgb": pl(cat["rgb"], 3), "depth": pl(cat["depth"], 1), "mask": pl(cat["mask"], 1), "rgb_c": pl(cat["rgb_c"], 3),
           "depth_c": pl(cat["depth_c"], 1), "mask_c": pl(cat["mask_c"], 1)}
    if normals:
        res["normals"], res["normals_c"] = pl(cat["normals"], 3), pl(cat["normals_c"], 3)
    return res


def _oracle_eval_f64(grid, msd, cams, rcfg, normals=False):
    """_oracle_eval with the oracle's arithmetic in float64 on the same float32 rays and coarse depths (as
    _render_rays_backward_case.oracle does it), as float32 planes."""
    frames = []
    for i in range(len(cams)):
        o, d, l = ro.make_rays(gu.cam_dict(cams, i), rcfg)
        torch.set_default_dtype(torch.float64)
        try:
            cat = ro.render_rays(grid.double(), {k: v.double() for k, v in msd.items()}, o.double(), d.double(), l.double(),
                                 rcfg, with_normals=normals)
        finally:
            torch.set_default_dtype(torch.float32)
        frames.append(_stack({k: v.float() for k, v in cat.items()}, normals, rcfg))
    return {k: torch.cat([f[k] for f in frames]) for k in frames[0]}


def _bounds(far):
    return {k: (v * (far / FAR) if "depth" in k else v) for k, v in EVAL_TOL.items()}


def _oracle_case(grid, msd, cams, rcfg, normals=False):
    """The float32 oracle's planes and, per plane, its distance from the float64 oracle as a fraction of the bound."""
    ref = _oracle_eval(grid, msd, cams, rcfg, normals=normals)
    ref64 = _oracle_eval_f64(grid, msd, cams, rcfg, normals=normals)
    bound = _bounds(gu.far_plane(cams, rcfg))
    own = {k: float((ref[k] - ref64[k]).abs().max()) / bound[k] for k in ref}
    return ref, own


def _spans(mask, what):
    """At least 10 % of the rays (almost) empty and at least 10 % mostly opaque."""
    lo, hi = float((mask < 0.1).float().mean()), float((mask > 0.5).float().mean())
    assert lo >= 0.1 and hi >= 0.1, (what, lo, hi)
    return lo, hi


def _swapped(rcfg):
    """``rcfg`` with the first two background channels swapped / with the default background interval."""
    b = rcfg.bg_color
    return dataclasses.replace(rcfg, bg_color=(b[1], b[0], b[2])), dataclasses.replace(rcfg, background_opacity=1e10)


def _sensitivity(name, ref, grid, msd, cams, rcfg):
    """What a wrong background would do to the ORACLE's frame, in rgb / mask bounds: (channels swapped, interval 1e10)."""
    s = SCENES[name]
    swap, opaque = _swapped(rcfg)
    d_swap = d_op = None
    if "bg_color" in s:
        other = _oracle_eval(grid, msd, cams, swap)
        d_swap = min(float((other[k] - ref[k]).abs().max()) for k in ("rgb", "rgb_c")) / EVAL_TOL["rgb"]
        assert d_swap > 100.0, (name, d_swap)
    if "background_opacity" in s:
        other = _oracle_eval(grid, msd, cams, opaque)
        d_op = min(float((other[k] - ref[k]).abs().max()) for k in ("mask", "mask_c")) / EVAL_TOL["mask"]
        assert d_op > 100.0, (name, d_op)
    return d_swap, d_op


def _report(what, errs, own, far):
    bound = _bounds(far)
    print(f"   {what}: of the bound: " + ", ".join(f"{k} {errs[k] / bound[k]:.3f} [{own[k]:.3f}]" for k in errs))


# ==== A. the scene table, evaluation mode =========================================================================================
def _scene_case(name, C_, compute, counts=(9, 7), normals=False, elevation=None, cam=(4, 1), seed=3300):
    nc, nf = counts
    inp = INPUTS[name]
    model_kw, rcfg_kw = _scene_kw(SCENES[name])
    model, msd, rcfg = _eval_model(R, C_, H, W, nc, nf, bias=inp["bias"], compute=compute, model_kw=model_kw, rcfg_kw=rcfg_kw)
    grid = _grid(inp, seed, C_)
    cams = (_orbit(cam[0], inp["focal"]) if elevation is None else _orbit(cam[0], inp["focal"], elevation))[[cam[1]]]
    far = gu.far_plane(cams, rcfg)

    def make():
        ref, own = _oracle_case(grid, msd, cams, rcfg, normals)
        return ref, own, _spans(ref["mask"], name), _sensitivity(name, ref, grid, msd, cams, rcfg)

    ref, own, span, sens = _cached(("scene", name, C_, counts, normals), make)
    what = f"scene {name} ({nc},{nf}) C={C_} {compute}" + (" normals" if normals else "")
    print(f"\n{what}: fine mask < 0.1 on {100 * span[0]:.0f} %, > 0.5 on {100 * span[1]:.0f} % of the rays; a wrong background "
          f"moves the oracle by {sens} bounds; far plane {far:.3f}")
    assert max(own.values()) <= 0.25, (what, "the float32 oracle is too far from the float64 one: change the inputs", own)
    got = _render_eval(model, grid, cams, normals=normals)
    errs = _check(got, ref, what, far=far)
    _report(what, errs, own, far)
    return model, got, ref


@pytest.mark.parametrize("name", [n for n in SCENES if n != "default"])
def test_scene_table_default_kernel(name):
    """Every scene on render2_kernel<8, 64, false, 12>: 16 features, exact fp32, a 9 x 11 frame, (9, 7) samples."""
    model, _, _ = _scene_case(name, 16, "f32")
    assert not _on_ray_per_column_kernel(model, R, 16)


@pytest.mark.parametrize("name", ["bg", "ve5.3", "centre", "all"])
@pytest.mark.parametrize("C_,compute", [(64, "f32"), (32, "f32_bf16x3")])
def test_scene_table_other_kernels(name, C_, compute):
    """The scenes that reach every field on render2_kernel<32, 64, false, 8> (64 features) and on the ray-per-column
    render_kernel<16, true, false, 64> (32 features, f32_bf16x3), whose epilogues read the background on their own."""
    model, _, _ = _scene_case(name, C_, compute)
    assert _on_ray_per_column_kernel(model, R, C_) == (compute == "f32_bf16x3")


def test_scene_all_at_full_counts():
    """`all` at (64, 64) on the default kernel: a merged list of 128 over the short depth range of scene_extent 3."""
    _scene_case("all", 16, "f32", counts=(64, 64))


@pytest.mark.parametrize("C_", [16, 64])
def test_scene_all_rendered_normals(C_):
    """`all` with render_normals on both normals forms - render2_kernel<8, 64, false, 10, true> (16 features) and
    render_kernel<32, false, true, 64> (64 features): tri_setup's gradient carries 1 / half_extent.  Normals within 5e-4,
    the other planes at their bounds.  The rendered normal jumps where a weighted sample sits on a cell face
    (tests/test_gpu_render_sample_counts.py::test_rendered_normals_on_other_instantiations), so the camera is one of that
    test's (elevation -0.5 rad) and the float64 oracle has to agree with the float32 one here like on every plane."""
    model, _, ref = _scene_case("all", C_, "f32", normals=True, elevation=-0.5, cam=(7, 2))
    assert float(ref["normals"].abs().max()) > 0.05 and float(ref["normals_c"].abs().max()) > 0.05
    assert _on_ray_per_column_kernel(model, R, C_, normals=True) == (C_ == 64)


# ==== B. cameras that differ inside one launch ====================================================================================
_DIST = (7.0, 10.0, 14.0, 8.5)
_FOCAL = ((3.0, 3.6), (2.6, 2.4), (3.2, 3.2), (4.0, 3.1))
_PP = ((0.2, -0.1), (-0.3, 0.15), (0.05, 0.3), (-0.12, -0.25))


def _varied_cameras(n, elevation=-30.0 * (2 * math.pi / 360)):
    """``n`` cameras of the orbit; camera i at centre distance _DIST[i % 4] (its T scaled) with focal lengths _FOCAL[i % 4]
    and principal point _PP[i % 4]: neighbours differ, and so do the two cameras either side of a launch boundary."""
    base = _orbit(n, 3.2, elevation)
    idx = [i % 4 for i in range(n)]
    scale = torch.tensor([_DIST[i] / 10.0 for i in idx])[:, None]
    return hda.PerspectiveCameras(R=base.R, T=base.T * scale, focal_length=torch.tensor([_FOCAL[i] for i in idx]),
                                  principal_point=torch.tensor([_PP[i] for i in idx]))


_B_INPUT = dict(grid="blob", radius=2.6, scale=8.0, bias=-0.3)


def _assert_bounds_differ(cams, rcfg, n=4):
    zs = [ro.depth_bounds(cams.R[i], cams.T[i], rcfg) for i in range(n)]
    for i in range(n):
        for j in range(i):
            assert abs(zs[i][0] - zs[j][0]) > 1.0 and abs(zs[i][1] - zs[j][1]) > 1.0, (i, j, zs)
    return zs


@pytest.mark.parametrize("C_,compute", [(16, "f32"), (32, "f32_bf16x3")])
def test_four_different_cameras_in_one_launch(C_, compute):
    """Four cameras with pairwise different depth bounds, focal lengths and principal points in ONE holo_render call: each
    against its own oracle frame (the depth bounds fractions of the batch's far plane, 18) and bit-equal to the same camera
    rendered alone - p.cams[g] is read per camera."""
    model, msd, rcfg = _eval_model(R, C_, H, W, 9, 7, bias=_B_INPUT["bias"], compute=compute)
    grid, cams = _grid(_B_INPUT, 3400, C_), _varied_cameras(4)
    zs = _assert_bounds_differ(cams, rcfg)
    far = gu.far_plane(cams, rcfg)
    assert abs(far - 18.0) < 1e-4
    ref, own = _cached(("four", C_), lambda: _oracle_case(grid, msd, cams, rcfg))
    assert max(own.values()) <= 0.25, own
    _spans(ref["mask"], "four cameras")
    for i in range(4):  # (no camera's frame is empty or solid)
        assert float(ref["mask"][i].min()) < 0.1 and float(ref["mask"][i].max()) > 0.5, i
    what = f"four cameras, depth bounds {[(round(a, 2), round(b, 2)) for a, b in zs]}, C={C_} {compute}"
    got = _render_eval(model, grid, cams)
    errs = _check(got, ref, what, far=far)
    _report(what, errs, own, far)
    for i in range(4):
        one = _render_eval(model, grid, cams[[i]])
        assert _bit_equal(one, {k: v[i:i + 1] for k, v in got.items()}), i
    assert _on_ray_per_column_kernel(model, R, C_) == (compute == "f32_bf16x3")


@pytest.mark.parametrize("C_,compute", [(16, "f32"), (32, "f32_bf16x3")])
def test_different_cameras_over_two_launches(C_, compute):
    """34 such cameras in one call: two launches of 17 (render_launches), the four distances and intrinsics cycling, so
    cameras 16 and 17 - the last of the first launch and the first of the second - differ, and slot g of the second launch
    (camera 17 + g, _DIST[(g + 1) % 4]) never holds what slot g of the first did (_DIST[g % 4]).  Every camera bit-equal to
    its single render (5 x 6 frames); the oracle on cameras 0, 15, 16, 17, 18 and 33."""
    n, Hs, Ws = 34, 5, 6
    model, msd, rcfg = _eval_model(R, C_, Hs, Ws, 9, 7, bias=_B_INPUT["bias"], compute=compute)
    grid, cams = _grid(_B_INPUT, 3400, C_), _varied_cameras(n)
    _assert_bounds_differ(cams[[15, 16, 17, 18]], rcfg)
    far = gu.far_plane(cams, rcfg)
    got = _render_eval(model, grid, cams)
    assert got["rgb"].shape[0] == n
    for i in range(n):
        one = _render_eval(model, grid, cams[[i]])
        assert _bit_equal(one, {k: v[i:i + 1] for k, v in got.items()}), i
    subset = [0, 15, 16, 17, 18, 33]
    ref = _cached(("two_launches", C_), lambda: _oracle_eval(grid, msd, cams[subset], rcfg))
    _check({k: v[subset] for k, v in got.items()}, ref, f"34 different cameras, two launches, C={C_} {compute}", far=far)
    assert float(ref["mask"][2:4].max()) > 0.5 and float(ref["mask"][2:4].min()) < 0.1
    assert _on_ray_per_column_kernel(model, R, C_) == (compute == "f32_bf16x3")


def _train_probe(name):
    """A probe for the training-mode helpers, on the ORACLE's frame of their inputs: at least 10 % of the rays (almost)
    empty and 10 % mostly opaque, and what a wrong background would do to it, in bounds."""
    def probe(grid, msd, cams, xys, rs, rcfg):
        render = lambda cfg: _oracle_training_render(grid, msd, cams, xys, rs, cfg, 1.0, gu)  # noqa: E731
        ref = render(rcfg)
        swapped, opaque = _swapped(rcfg)
        span = _spans(ref["mask"], name)
        d_swap = float((render(swapped)["rgb"] - ref["rgb"]).abs().max()) / EVAL_TOL["rgb"]
        d_op = float((render(opaque)["mask"] - ref["mask"]).abs().max()) / EVAL_TOL["mask"]
        print(f"\n   training-mode inputs [{name}]: fine mask < 0.1 on {100 * span[0]:.0f} %, > 0.5 on {100 * span[1]:.0f} % of the "
              f"rays; swapped background channels move the oracle's rgb by {d_swap:.0f} bounds, a background interval of 1e10 "
              f"its mask by {d_op:.0f}")
        s = SCENES.get(name, {})
        assert "bg_color" not in s or d_swap > 100.0
        assert "background_opacity" not in s or d_op > 100.0
    return probe


# The training-mode helpers build their own tanh noise grid, which fills the volume, and add density noise of std 1 before the
# ReLU: the grid x 10 and a density bias of -5 (-1 behind the LeakyReLU's slope of 0.2) give empty and opaque rays in one frame
_TRAIN = dict(grid_scale=10.0, density_bias=-5.0)


def test_different_cameras_training_forward():
    """The four cameras through holo_render_rays (13 rays each, (12, 10), all streams): tiles of one launch read their own
    camera's bounds and intrinsics."""
    cams = _varied_cameras(4, -0.5)
    _assert_bounds_differ(cams, ro.RenderCfg())
    probe = _train_probe("four cameras")
    _training_case(12, 10, 16, "all", 3500, n_cam=4, case="four cameras", cams=cams, probe=lambda ref, *a: probe(*a), **_TRAIN)


def test_different_cameras_backward():
    """... and through holo_render_rays_backward, the helper's criteria unchanged."""
    cams = _varied_cameras(4, -0.5)
    _render_rays_backward_case(gu, 12, 10, 16, 8, 4, 13, "all", seed=3600, cams=cams, probe=_train_probe("four cameras"),
                               **_TRAIN)


# ==== C. training forward and backward off the default scene =====================================================================
@pytest.mark.parametrize("name", ["bg", "bgop.5", "ve5.3", "centre", "all"])
def test_backward_off_the_default_scene(name):
    """_render_rays_backward_case (12, 10, 16 features, 8^3, 3 x 13 rays, all streams, random cotangents on all six
    outputs) per scene.  `bg`: gO = gm - (gr . bg) weighs the rgb cotangents against the mask's with three different
    background channels; `ve5.3` / `all`: tri_setup and the scatter with a voxel of 0.6625; `centre`: the depth bounds of
    an off-origin scene; `bgop.5`: d w_last / d sigma with a finite interval."""
    model_kw, rcfg_kw = _scene_kw(SCENES[name])
    _render_rays_backward_case(gu, 12, 10, 16, 8, 3, 13, "all", seed=3700, probe=_train_probe(name), model_kw=model_kw,
                               rcfg_kw=rcfg_kw, **_TRAIN)


def test_backward_all_at_a_larger_size():
    """`all` at (24, 20, 32 features, 16^3, 3 x 37 rays): a voxel of 0.33125 (44 shorter intervals per ray: the grid x 20,
    density bias -7)."""
    model_kw, rcfg_kw = _scene_kw(SCENES["all"])
    _render_rays_backward_case(gu, 24, 20, 32, 16, 3, 37, "all", seed=3800, probe=_train_probe("all"), model_kw=model_kw,
                               rcfg_kw=rcfg_kw, grid_scale=20.0, density_bias=-7.0)


@pytest.mark.parametrize("name", ["bg", "centre", "all"])
def test_training_forward_off_the_default_scene(name):
    """holo_render_rays per scene at the bounds of tests/test_gpu_training_mode.py::test_training_mode_render_vs_oracle
    (3 x 13 rays, (12, 10)): render2_kernel<8, 64, true, 12>'s own epilogue."""
    model_kw, rcfg_kw = _scene_kw(SCENES[name])
    probe = _train_probe(name)
    _training_case(12, 10, 16, "all", 3900, n_cam=3, case=name, model_kw=model_kw, rcfg_kw=rcfg_kw,
                   probe=lambda ref, *a: probe(*a), **_TRAIN)


# ==== D. model level ==============================================================================================================
def test_model_arguments_reach_the_raymarcher_and_the_implicit_function():
    """HoloDiffusionModel(bg_color=..., volume_extent=5.3) hands the colour to the raymarcher and the extent to the implicit
    function (GenericModel's behaviour); an explicit raymarcher bg_color wins over the model's.  Both by rendering."""
    inp = INPUTS["ve5.3"]
    grid, cams = _grid(inp, 3300, 16), _orbit(4, inp["focal"])[[1]]
    other = (0.9, 0.2, 0.4)
    for what, model_kw, bg in (
            ("model bg_color", dict(bg_color=BG, volume_extent=5.3), BG),
            ("raymarcher bg_color over the model's",
             dict(bg_color=other, volume_extent=5.3, renderer_HoloMultiPassEmissionAbsorptionRenderer_args=dict(
                 raymarcher_EmissionAbsorptionRaymarcher_args=dict(bg_color=BG))), BG)):
        model, msd, rcfg = _eval_model(R, 16, H, W, 9, 7, bias=inp["bias"], model_kw=model_kw,
                                       rcfg_kw=dict(bg_color=bg, volume_extent=5.3))
        assert model.renderer._bg_color() == bg and all(f._fn.volume_extent == 5.3 for f in model._implicit_functions)
        ref = _cached(("model_args",), lambda: _oracle_eval(grid, msd, cams, rcfg))
        wrong = _cached(("model_args", "wrong"), lambda: _oracle_eval(grid, msd, cams, dataclasses.replace(rcfg, bg_color=other)))
        assert float((wrong["rgb"] - ref["rgb"]).abs().max()) > 100 * EVAL_TOL["rgb"]
        _check(_render_eval(model, grid, cams), ref, what, far=gu.far_plane(cams, rcfg))


def test_scene_change_on_a_live_model_rekeys_the_handle():
    """One model: rendered; scene centre, scene extent, background colour and background opacity set on its ray sampler
    and raymarcher; rendered again - the oracle's frame of the NEW scene, not the old handle's; everything set back -
    bit-equal to the first render."""
    inp = INPUTS["bgop.5"]
    model, msd, rcfg = _eval_model(R, 16, H, W, 9, 7, bias=inp["bias"])
    grid, cams = _grid(inp, 3300, 16), _orbit(4, inp["focal"])[[1]]
    new = dataclasses.replace(rcfg, scene_center=CENTRE, scene_extent=2.5, bg_color=BG, background_opacity=0.5)
    ref0 = _cached(("rekey", 0), lambda: _oracle_eval(grid, msd, cams, rcfg))
    ref1 = _cached(("rekey", 1), lambda: _oracle_eval(grid, msd, cams, new))
    for k in ("rgb", "mask", "depth"):
        assert float((ref1[k] - ref0[k]).abs().max()) > 100 * _bounds(FAR)[k], k
    first = _render_eval(model, grid, cams)
    _check(first, ref0, "live model, default scene")
    rm = model.renderer._raymarcher_args
    old = (model.raysampler.scene_center, model.raysampler.scene_extent, rm["bg_color"], rm["background_opacity"])
    model.raysampler.scene_center, model.raysampler.scene_extent = CENTRE, 2.5
    rm["bg_color"], rm["background_opacity"] = BG, 0.5
    _check(_render_eval(model, grid, cams), ref1, "live model, scene changed", far=gu.far_plane(cams, new))
    model.raysampler.scene_center, model.raysampler.scene_extent, rm["bg_color"], rm["background_opacity"] = old
    assert _bit_equal(_render_eval(model, grid, cams), first)


# ==== E. the same coordinate elsewhere ============================================================================================
@pytest.mark.parametrize("volume_extent", [5.3, 20.0])
@pytest.mark.parametrize("m", [8, 15])
def test_density_lattice_equals_the_implicit_function_at_other_extents(volume_extent, m):
    """tests/test_gpu_mesh.py::test_density_lattice_equals_the_implicit_function's assertion, its bound unchanged (it does
    not depend on the extent): both sides divide the same float32 points by the same half extent."""
    tgm.lattice_equals_the_implicit_function(gu, 16, m, volume_extent)


def test_standalone_implicit_function_at_another_extent():
    """tests/test_gpu_render.py::test_standalone_implicit_function_vs_oracle's pts_3d comparison at volume_extent 5.3:
    points in +-4.5, so well outside the half extent 2.31875 too."""
    model, _, _, rcfg, msd = gu.make_model(8, 32, 6, 10, TINY_UNET, density_bias=0.05, model_kw=dict(volume_extent=5.3),
                                           rcfg_kw=dict(volume_extent=5.3))
    fn = model._implicit_functions[0]._fn
    grid = torch.tanh(torch.from_numpy(np_noise(21, (1, 32, 8, 8, 8))))
    pts = (torch.rand(2, 5, 7, 16, 3, generator=torch.Generator().manual_seed(3)) - 0.5) * 9.0
    dens, feats, _ = fn(pts_3d=pts.to(gu.DEV), voxel_grid_features=grid.to(gu.DEV))
    f = ro.trilinear(grid, pts, rcfg)
    inside = (pts.abs() < mesh.half_extent(8, 5.3)).all(dim=-1)
    assert 0.05 < float(inside.float().mean()) < 0.5 and float(f[inside].abs().max()) > 0.5
    dn = torch.nn.functional.normalize(torch.ones(2, 5, 7, 3), dim=-1)[..., None, :].expand(2, 5, 7, 16, 3)
    d_ref, c_ref = ro.render_mlp(msd, f, dn, rcfg)
    assert (dens.cpu() - d_ref).abs().max() < 1e-4 and (feats.cpu() - c_ref).abs().max() < 1e-4


def test_model_extract_mesh_at_another_extent():
    """HoloDiffusionModel.extract_mesh with volume_extent 5.3 (tests/test_gpu_mesh.py::test_model_extract_mesh's planted
    blob, the denoiser off): the vertices lie within mesh.half_extent(8, 5.3) - and past 0.4 of it, so the scale is not
    some other extent's - and equal surface_nets on the model's own field."""
    model, *_ = gu.make_model(8, 32, 8, 16, TINY_UNET, density_bias=0.3, model_kw=dict(volume_extent=5.3))
    model.net_3d_enabled = False
    g = np.linspace(-1, 1, 8)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    ball = torch.from_numpy(((X - 0.1) ** 2 + (Y + 0.15) ** 2 + Z ** 2 < 0.45).astype(np.float32))
    vec = torch.tanh(torch.from_numpy(np_noise(91, (32,))))
    vf = (vec[None, :, None, None, None] * (2.0 * ball - 1.0)[None, None]).contiguous().to(gu.DEV)
    fn = model._implicit_functions[-1]._fn
    h = mesh.half_extent(8, 5.3)
    assert abs(h - 2.31875) < 1e-6
    field = mesh.density_lattice(fn, vf, 15)
    lo, hi = max(field.min().item(), 0.0), field.max().item()
    assert hi > lo
    level = 0.5 * (lo + hi)
    out = model.extract_mesh(vf, density_level=level)
    assert out["verts"].shape[0] > 0 and out["faces"].shape[0] > 0
    assert 0.4 * h < out["verts"].abs().max().item() <= h
    verts, tris = mesh.surface_nets(field, level, h)
    normals, colours = mesh.vertex_attributes(fn, vf, verts)
    for key, want in (("verts", verts), ("faces", tris), ("normals", normals), ("colours", colours)):
        assert torch.equal(out[key], want), key


# ==== F. refusals =================================================================================================================
_NAN, _INF = float("nan"), float("inf")
_REFUSED = [("volume_extent", v) for v in (0.0, -8.0, _NAN, _INF)] + [("scene_extent", v) for v in (0.0, -4.0, _NAN, _INF)] + \
    [("scene_center", (0.0, _NAN, 0.0)), ("scene_center", (_INF, 0.0, 0.0)), ("bg_color", (1.0, 1.0, _NAN)),
     ("bg_color", (-_INF, 1.0, 1.0)), ("background_opacity", _NAN), ("background_opacity", -1.0), ("background_opacity", _INF)]


def _create(**kw):
    L = runtime.lib()
    cfg = _lib.make_render_cfg(8, 16, 9, 11, **kw)
    h = C.c_void_p()
    rc = L.holo_renderer_create(runtime.ctx(gu.DEV), C.byref(cfg), C.byref(h))
    return rc, h, (L.holo_last_error() or b"").decode()


@pytest.mark.parametrize("field,value", _REFUSED, ids=[f"{f}={v}" for f, v in _REFUSED])
def test_renderer_create_refuses(field, value):
    """holo_renderer_create: HOLO_E_INVALID with the field's name in the message and no handle, before anything is
    allocated or launched - a non-finite or non-positive extent, a non-finite centre or colour, a NaN, negative or infinite
    background interval (infinity times a zero density is NaN in the compositing)."""
    rc, h, msg = _create(**{field: value})
    assert rc == -1 and not h.value, (rc, h.value)  # HOLO_E_INVALID
    assert field in msg and "holo_renderer_create" in msg, msg


def test_renderer_create_takes_the_released_defaults():
    """... and the released scene (and a zero background interval, and a scene centre far away) still creates."""
    for kw in ({}, dict(background_opacity=0.0), dict(scene_center=(1e6, -1e6, 0.0)), dict(volume_extent=1e-3, bg_color=(0.0, -2.0, 7.0))):
        rc, h, msg = _create(**kw)
        assert rc == 0 and h.value, (kw, rc, msg)
        runtime.lib().holo_renderer_destroy(h)


@pytest.mark.parametrize("bg", [(), (0.1, 0.2), (0.1, 0.2, 0.3, 0.4)], ids=lambda b: f"len{len(b)}")
def test_bg_color_of_another_length_is_refused(bg):
    """The raymarcher's bg_color is one value for all channels or one per channel; anything else raises before a handle is
    made (a 2-tuple used to index out of range inside make_render_cfg, a 4-tuple was silently cut)."""
    model, msd, rcfg = _eval_model(R, 16, H, W, 9, 7, model_kw=dict(
        renderer_HoloMultiPassEmissionAbsorptionRenderer_args=dict(raymarcher_EmissionAbsorptionRaymarcher_args=dict(bg_color=bg))))
    with pytest.raises(ValueError, match="bg_color"):
        model.renderer._bg_color()
    with pytest.raises(ValueError, match="bg_color"):
        _render_eval(model, _noise_grid(3300, 16, R), _orbit(4)[[1]])
    assert model.renderer._handle is None
