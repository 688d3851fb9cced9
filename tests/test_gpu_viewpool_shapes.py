"""View pooling at the widths, view counts, grids and cameras that tests/test_viewpool.py never runs.

tests/test_viewpool.py runs one family of shapes: maps of 16 / 1 / 3 channels, grids of 8, 16 and once 6, 2-9 views, feature
sizes 16 / 32, cameras with zero principal point and equal focal lengths.  Every MLPMean case there lands on the 48-wide
instantiation of mlp_mean_pool_kernel<DH>, the boundary between the two forms of the AngleWeighted backward (A + 1 <= 160:
view_pool_bwd2_kernel, else view_pool_bwd_kernel) is never approached, and neither 1 nor MAX_VIEWS = 16 views, MAX_FEATS = 8
maps, MAX_AGG = 512 aggregated features, odd grids, R = 2 or a partial 32-voxel MFMA tile are reached.  Here:

  1. AngleWeightedReductionFeatureAggregator: forward, then backward in both kernel forms (HOLO_VIEWPOOL_BWD_V1 unset / 1);
  2. MLPMeanFeatureAggregator: forward and backward at the padded input widths 32 / 64 / 96 / 128 (and 48 where a case needs
     another edge), 1 and 16 views, 125 / 216 / 8 voxels, voxel chunks that are no multiple of 16;
  3. results do not depend on what the pooler's cached workspace held before a call;
  4. what the entry refuses (HoloError, and the process carries on).

The reference is always oracle/viewpool_oracle.py (float32) and torch autograd through it, at the bounds of
tests/test_viewpool.py: forward max|got - ref| < 1e-4, every gradient tensor max|got - ref| / max|ref| < 1e-3, deterministic
against default mode < 2e-5.  Every case prints its worst errors.  ViewPooler is called directly: the model class takes only
the renderer's feature sizes 16 / 32 / 64 / 128.

Inputs: maps tanh(np_noise(seed + i, (n, C, H, W))), cameras simple_360_cameras(n, radius) - "aniso": per-view focal lengths
that differ between the axes and non-zero principal points -, mapper and aggregator weights from synth_state_dict with
0.1-scaled noise biases, volume extent 8.

Variance clamp (AngleWeighted backward): STD = sqrt(clamp(var, 1e-4)) passes no gradient below its bound, and the kernel's
one-pass variance differs from the oracle's two-pass one by up to ~2.4e-7 (4 ulp of S2 / D <= 1): a (voxel, channel) that
close to 1e-4 may take the other branch on one side, which moves a pixel gradient by far more than 1e-3.  The cotangent is
therefore zeroed at every voxel that has a channel with |var - 1e-4| < 1e-6 (var: the pre-clamp variance in float64), at most
10 % of the voxels of a case.  A variance of exactly 0 (voxels outside every view, every voxel with one view) needs no mask.

Which kernels the cases reach (read from the launchers, holo_mlp_mean_create and view_pool_bwd_launch):
  AngleWeighted backward, knob unset: view_pool_bwd2_kernel for A <= 159 (every case but A160 and A512), view_pool_bwd_kernel
  for A160 (A = 160) and A512 (A = 512); knob = 1: view_pool_bwd_kernel for all.
  MLPMean, padded width = channels padded to quads per map + the embedding padded to a quad -> the first of 32 / 48 / 64 / 96 /
  128 that fits: dp32 4 + 24 = 28 -> 32; R5-one-view 24 + 4 = 28 -> 32; R6-max-views 24 + 16 = 40 -> 48; R6-chunk27 and
  F5-forward 24 + 24 = 48; R2-tiny-maps 20 + 24 = 44 -> 48; dp64 40 + 24 = 64; dp96-released 72 + 24 = 96; dp128 72 + 52 =
  124 -> 128.

Measured on an MI355X (forward max|d|; worst gradient error of scale, default form / first form; masked voxels of R^3):
  released 2.7e-7, 1.5e-6 / 2.5e-6, 6 of 512     one-view 1.5e-7, 1.3e-6 / 3.1e-7, 0     max-views 2.0e-7, 3.6e-6 / 7.4e-6, 2
  max-views-inside 1.5e-7, 6.6e-6 / 4.7e-6, 1    odd-maps 1.0e-7, 2.5e-6 / 2.6e-6, 1     A158 3.1e-7, 9.3e-6 / 9.3e-6, 10
  A160 2.4e-7, 2.3e-6 / 2.2e-6, 15               A512 3.9e-7, 2.3e-5 / 2.3e-5, 17 of 216 R2 5.2e-8, 3.2e-7 / 2.1e-7, 0 of 8
  R5 1.8e-7, 3.0e-6 / 1.6e-6, 0 of 125           R7 1.1e-6, 5.8e-6 / 5.8e-6, 3 of 343    R12 2.8e-7, 1.4e-5 / 1.0e-5, 6 of 1728
  F64-forward 2.5e-7
  MLPMean (forward, worst gradient): dp32 9.3e-8, 1.6e-6; dp64 8.7e-8, 1.3e-6; dp96-released 1.6e-7, 1.0e-6; dp128 5.8e-7,
  1.5e-6; R5-one-view 4.5e-8, 2.1e-6; R6-max-views 2.0e-7, 5.2e-6; R6-chunk27 3.0e-7, 4.7e-6 (8 chunks against one 8.1e-7);
  R2-tiny-maps 8.9e-8, 8.4e-7; F5-forward 9.7e-8.  Deterministic against default mode: at most 3.3e-7.  The host emulation
  build reads the same magnitudes (forward at most 1.0e-6, gradients at most 4.6e-5 on A512).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from holo_diffusion_amd import _lib, runtime  # noqa: E402
from holo_diffusion_amd.viewpool import ViewPooler  # noqa: E402
from holo_diffusion_amd.weights import synth_state_dict  # noqa: E402
from oracle import viewpool_oracle as vo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

from tests import gpu_utils as gu  # noqa: E402
from tests.test_viewpool import _cams, _dev_cameras, _rel  # noqa: E402

EXTENT = 8.0
FWD_TOL, GRAD_TOL, DET_TOL = 1e-4, 1e-3, 2e-5

USUAL = ((16, 20, 24), (1, 30, 30), (3, 17, 13))
RELEASED = ((16, 12, 14), (16, 9, 11), (16, 5, 7), (16, 3, 5), (1, 20, 20), (3, 20, 20))  # configs/hydrant.yaml, apple.yaml
ODD = ((5, 9, 7), (6, 7, 9), (2, 11, 11), (1, 1, 1), (3, 1, 5), (7, 2, 2), (4, 13, 3), (9, 6, 6))

# id -> (R, views, radius, maps (C, H, W), F, gamma, min weight, aniso)
ANGLE = {
    "released": (8, 4, 6.0, RELEASED, 32, 1.0, 0.1, False),          # 18 quads: the second trip of the lane loop
    "one-view": (8, 1, 6.0, USUAL, 16, 1.0, 0.1, False),             # every STD clamped
    "max-views": (8, 16, 6.0, USUAL, 16, 1.0, 0.1, False),           # full [16][16] LDS tiles
    "max-views-inside": (8, 16, 3.0, USUAL, 16, 2.0, 0.1, True),     # cameras inside the volume: zero-weight taps, |z| clamp
    "odd-maps": (8, 3, 6.0, ODD, 20, 1.0, 0.1, True),                # 8 maps, padded channels mid-list, 1- and 2-pixel maps
    "A158": (8, 3, 6.0, ((64, 6, 8), (12, 7, 5), (3, 9, 9)), 32, 1.0, 0.1, False),   # last A of the second form, bias row 158
    "A160": (8, 3, 6.0, ((64, 6, 8), (12, 7, 5), (4, 9, 9)), 32, 1.0, 0.1, False),   # first A on the first form by default
    "A512": (6, 2, 6.0, ((128, 4, 5), (128, 5, 4)), 8, 1.0, 0.1, False),             # MAX_AGG; half-empty last voxel group
    "R2": (2, 3, 7.0, USUAL, 16, 3.0, 0.5, True),                    # one half-empty voxel group
    "R5": (5, 3, 7.0, USUAL, 16, 0.5, 0.5, True),                    # odd grid; powf with a fractional exponent (3 views: no
                                                                     # camera opposite view 0, where the base rounds below 0)
    "R7": (7, 3, 7.0, USUAL, 4, 3.0, 0.0, True),                     # F below one lane row; no weight floor
    "R12": (12, 3, 7.0, USUAL, 16, 3.0, 0.5, True),                  # 108 voxel groups
    "F64-forward": (8, 3, 6.0, USUAL, 64, 1.0, 0.1, False),          # forward only: the backward refuses F > 32
}
ANGLE_BWD = [c for c in ANGLE if c != "F64-forward"]

# id -> (R, views, radius, maps, F, dim_out, harmonics, aniso)
MLP = {
    "dp32": (8, 3, 6.0, ((3, 17, 13),), 16, 24, 3, False),                                        # 3 + 21 -> 28 -> 32
    "dp64": (8, 3, 6.0, ((16, 10, 12), (16, 6, 5), (1, 9, 9), (3, 9, 9)), 16, 24, 3, False),      # 40 + 24 = 64: no padding column
    "dp96-released": (8, 4, 6.0, RELEASED, 32, 128, 3, False),                                    # 72 + 24 = 96
    "dp128": (8, 3, 6.0, RELEASED, 32, 128, 8, False),                                            # 72 + 51 -> 124 -> 128
    "R5-one-view": (5, 1, 7.0, USUAL, 20, 1, 0, True),         # 125 voxels: partial MFMA tile; softmax over one view; dim_out 1
    "R6-max-views": (6, 16, 7.0, USUAL, 4, 300, 2, True),      # 16 views; F = 4 (FW = 8); dim_out above 128
    "R6-chunk27": (6, 3, 7.0, USUAL, 16, 24, 3, True),         # HOLO_MLP_MEAN_BWD_CHUNK=27: 8 chunks of 27 voxels
    "R2-tiny-maps": (2, 2, 7.0, ((5, 1, 1), (6, 1, 5), (2, 2, 2)), 12, 24, 3, False),             # 8 voxels; 1-pixel maps
    "F5-forward": (8, 3, 6.0, USUAL, 5, 24, 3, False),         # forward only: rows of G at and beyond F are zero-staged
}
MLP_BWD = [c for c in MLP if c != "F5-forward"]
_EMU_SKIPS_CHUNK = pytest.mark.skipif(gu.EMU, reason="the emulation build ignores HOLO_MLP_MEAN_BWD_CHUNK")

_REF = {}


def _cached(key, make):
    """One oracle run per case, shared by the tests that need it and left unchanged."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _maps(seed, n, shapes):
    return {f"m{i}": torch.tanh(torch.from_numpy(np_noise(seed + i, (n,) + tuple(s)))) for i, s in enumerate(shapes)}


def _cameras(n, radius, aniso):
    c = _cams(n, radius=radius)
    if aniso:
        c["focal"] = torch.stack([torch.linspace(2.4, 3.6, n), torch.linspace(3.9, 2.7, n)], 1)
        c["pp"] = torch.stack([torch.linspace(-0.15, 0.2, n), torch.linspace(0.1, -0.25, n)], 1)
    return c


def _mapper(F, A):
    w = synth_state_dict({"w": (F, A), "b": (F,)}, 9)
    w["b"] = 0.1 * torch.from_numpy(np_noise(4, (F,)))
    return w


def _dev(d):
    return {k: v.to(gu.DEV) for k, v in d.items()}


# ---- 1. AngleWeightedReductionFeatureAggregator ----------------------------------------------------------------------
def _angle_inputs(cid):
    R, n, radius, shapes, F, gamma, minw, aniso = ANGLE[cid]
    feats = _maps(500 + 20 * list(ANGLE).index(cid), n, shapes)
    A = 2 * sum(s[0] for s in shapes)
    return feats, _cameras(n, radius, aniso), _mapper(F, A), R, F, dict(gamma=gamma, min_weight=minw)


def _angle_pooler(kw):
    return ViewPooler(feature_aggregator_AngleWeightedReductionFeatureAggregator_args=dict(
        exclude_target_view=False, exclude_target_view_mask_features=False, weight_by_ray_angle_gamma=kw["gamma"],
        min_ray_angle_weight=kw["min_weight"]))


def _angle_ref(cid):
    """The oracle's forward, the cotangent (zeroed where a variance sits at its clamp, see the module's docstring) and
    autograd's gradients of the maps and the mapper."""
    def make():
        feats, cams_d, w, R, F, kw = _angle_inputs(cid)
        var = torch.cat([v for _, v in vo.pool_views_moments(feats, cams_d, R, EXTENT, dtype=torch.float64, **kw)], dim=-1)
        near = ((var - 1e-4).abs() < 1e-6).any(dim=-1)
        g = torch.from_numpy(np_noise(123, (1, F, R, R, R))).clone()
        g.view(1, F, -1)[:, :, near] = 0.0
        leaves = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
        mw, mb = w["w"].clone().requires_grad_(True), w["b"].clone().requires_grad_(True)
        out = vo.voxel_features_from_views(leaves, cams_d, mw, mb, R, EXTENT, **kw)
        out.backward(g)
        return dict(out=out.detach(), g=g, masked=int(near.sum()), maps={k: v.grad for k, v in leaves.items()}, mw=mw.grad,
                    mb=mb.grad)
    return _cached(("angle", cid), make)


def _angle_forward(vp, cid):
    feats, cams_d, w, R, F, kw = _angle_inputs(cid)
    return vp.pool_to_voxel_features(_dev(feats), _dev_cameras(cams_d), w["w"].to(gu.DEV), w["b"].to(gu.DEV), R, EXTENT)


def _angle_backward(vp, cid, g, **kwargs):
    feats, cams_d, w, R, F, kw = _angle_inputs(cid)
    return vp.pool_to_voxel_features_backward(_dev(feats), _dev_cameras(cams_d), w["w"].to(gu.DEV), w["b"].to(gu.DEV), R, EXTENT,
                                              g.to(gu.DEV), **kwargs)


def _check_angle_grads(what, got, ref):
    """(map gradients, d weight, d bias) of a backward call against ``ref`` (_angle_ref): prints, then asserts."""
    gf, gw, gb = got
    errs = {"weight": _rel(gw, ref["mw"]), "bias": _rel(gb, ref["mb"])}
    for k, r in ref["maps"].items():
        assert gf[k].shape == r.shape, (what, k)
        assert float(r.abs().max()) > 0, (what, k)
        errs[k] = _rel(gf[k], r)
    print(f"[viewpool-shapes] {what}: worst gradient error {max(errs.values()):.2e} of scale "
          f"({max(errs, key=errs.get)}), {ref['masked']} voxels masked")
    for k, e in errs.items():
        assert e < GRAD_TOL, (what, k, e)  # (NaN fails too)


@pytest.mark.parametrize("cid", list(ANGLE))
def test_angle_weighted_forward_vs_oracle(cid):
    """holo_view_pool against the oracle at max|d| < 1e-4: more than 16 channel quads (`released`, `A158`, `A160`, `A512`),
    1 and 16 views, 8 maps with padded channels in the middle of the list and maps of 1 x 1, 1 x 5 and 2 x 2 pixels, cameras
    with a principal point and two focal lengths, grids of 2, 5, 7 and 12, gamma 0.5 / 2 / 3, weight floors 0 / 0.5, feature
    sizes 4, 8, 20 and 64."""
    ref = _angle_ref(cid) if cid in ANGLE_BWD else None
    if ref is None:
        feats, cams_d, w, R, F, kw = _angle_inputs(cid)
        out = _cached(("angle-fwd", cid), lambda: vo.voxel_features_from_views(feats, cams_d, w["w"], w["b"], R, EXTENT, **kw))
    else:
        out = ref["out"]
    got = _angle_forward(_angle_pooler(_angle_inputs(cid)[5]), cid)
    assert got.shape == out.shape
    err = float((got.cpu() - out).abs().max())
    print(f"[viewpool-shapes] angle {cid}: forward max|d| {err:.2e}")
    assert err < FWD_TOL, (cid, err)
    assert out.abs().max() <= 1.0 and out.std() > 0.02


@pytest.mark.parametrize("v1", [None, "1"], ids=["default-form", "first-form"])
@pytest.mark.parametrize("cid", ANGLE_BWD)
def test_angle_weighted_backward_vs_autograd_of_the_oracle(cid, v1, monkeypatch):
    """holo_view_pool_backward against autograd through the oracle, every gradient tensor at 1e-3 of its scale, with
    HOLO_VIEWPOOL_BWD_V1 unset (view_pool_bwd2_kernel up to A = 159: `A158` uses all ten MFMA row tiles and puts the bias row
    at a == A; the first form beyond: `A160`, `A512`) and set to 1 (view_pool_bwd_kernel everywhere)."""
    if v1 is None:
        monkeypatch.delenv("HOLO_VIEWPOOL_BWD_V1", raising=False)
    else:
        monkeypatch.setenv("HOLO_VIEWPOOL_BWD_V1", v1)
    ref = _angle_ref(cid)
    nvox = ANGLE[cid][0] ** 3
    assert ref["masked"] <= 0.1 * nvox, (cid, ref["masked"], nvox)
    vp = _angle_pooler(_angle_inputs(cid)[5])
    _check_angle_grads(f"angle {cid} backward ({'first' if v1 else 'default'} form)", _angle_backward(vp, cid, ref["g"]), ref)


def test_angle_weighted_backward_without_feature_grads_on_the_first_form(monkeypatch):
    """`A160` (the first form by default) with want_feature_grads=False: no map gradients, and the mapper's gradients - fixed-
    order sums - bit-equal to the full call's."""
    monkeypatch.delenv("HOLO_VIEWPOOL_BWD_V1", raising=False)
    ref = _angle_ref("A160")
    vp = _angle_pooler(_angle_inputs("A160")[5])
    gf, gw, gb = _angle_backward(vp, "A160", ref["g"])
    gw, gb = gw.clone(), gb.clone()
    gf2, gw2, gb2 = _angle_backward(vp, "A160", ref["g"], want_feature_grads=False)
    assert gf2 == {} and len(gf) == 3
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb)
    assert _rel(gw2, ref["mw"]) < GRAD_TOL and _rel(gb2, ref["mb"]) < GRAD_TOL


# ---- 2. MLPMeanFeatureAggregator -------------------------------------------------------------------------------------
def _mlp_inputs(cid):
    R, n, radius, shapes, F, dim_out, n_harm, aniso = MLP[cid]
    feats = _maps(900 + 20 * list(MLP).index(cid), n, shapes)
    D = sum(s[0] for s in shapes) + 3 * (2 * n_harm + 1)
    pshapes = vo.mlp_mean_param_shapes(D, 128, dim_out)
    sd = synth_state_dict(pshapes, 21)
    for k in pshapes:
        if k.endswith("bias"):
            sd[k] = 0.1 * torch.from_numpy(np_noise(len(k), pshapes[k]))
    return feats, _cameras(n, radius, aniso), sd, _mapper(F, dim_out), R, F, n_harm


def _mlp_pooler(cid, sd=None, **over):
    R, n, radius, shapes, F, dim_out, n_harm, aniso = MLP[cid]
    args = dict(exclude_target_view=False, exclude_target_view_mask_features=False, dim_out=dim_out,
                n_harmonic_functions_ray=n_harm)
    args.update(over)
    vp = ViewPooler(feature_aggregator_class_type="MLPMeanFeatureAggregator", feature_aggregator_MLPMeanFeatureAggregator_args=args)
    if sd is not None:
        vp.feature_aggregator.load_state_dict(sd)
    return vp.to(gu.DEV)


def _mlp_ref(cid):
    def make():
        feats, cams_d, sd, w, R, F, n_harm = _mlp_inputs(cid)
        g = torch.from_numpy(np_noise(321, (1, F, R, R, R)))
        leaves = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
        psd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        mw, mb = w["w"].clone().requires_grad_(True), w["b"].clone().requires_grad_(True)
        out = vo.voxel_features_from_views_mlp_mean(leaves, cams_d, psd, mw, mb, R, EXTENT, n_harmonic=n_harm)
        out.backward(g)
        return dict(out=out.detach(), g=g, maps={k: v.grad for k, v in leaves.items()}, agg={k: v.grad for k, v in psd.items()},
                    mw=mw.grad, mb=mb.grad)
    return _cached(("mlp", cid), make)


def _mlp_forward(vp, cid):
    feats, cams_d, sd, w, R, F, n_harm = _mlp_inputs(cid)
    return vp.pool_to_voxel_features(_dev(feats), _dev_cameras(cams_d), w["w"].to(gu.DEV), w["b"].to(gu.DEV), R, EXTENT)


def _mlp_backward(vp, cid, g):
    """-> (map gradients, d mapper weight, d mapper bias, aggregator parameter gradients)"""
    feats, cams_d, sd, w, R, F, n_harm = _mlp_inputs(cid)
    gf, gw, gb = vp.pool_to_voxel_features_backward(_dev(feats), _dev_cameras(cams_d), w["w"].to(gu.DEV), w["b"].to(gu.DEV), R,
                                                    EXTENT, g.to(gu.DEV))
    return gf, gw, gb, dict(vp.feature_aggregator.native_grads)


def _check_mlp_grads(what, got, ref):
    gf, gw, gb, ga = got
    errs = {"mapper.weight": _rel(gw, ref["mw"]), "mapper.bias": _rel(gb, ref["mb"])}
    assert set(ga) == set(ref["agg"]) and set(gf) == set(ref["maps"])
    for grp, refs in ((ga, ref["agg"]), (gf, ref["maps"])):
        for k, r in refs.items():
            assert grp[k].shape == r.shape, (what, k)
            assert float(r.abs().max()) > 0, (what, k)
            errs[k] = _rel(grp[k], r)
    print(f"[viewpool-shapes] {what}: worst gradient error {max(errs.values()):.2e} of scale ({max(errs, key=errs.get)})")
    for k, e in errs.items():
        assert e < GRAD_TOL, (what, k, e)


@pytest.mark.parametrize("cid", [c for c in MLP if c != "R6-chunk27"])  # (its forward is R6's, run with its backward below)
def test_mlp_mean_forward_vs_oracle(cid):
    """holo_mlp_mean_pool against the oracle at max|d| < 1e-4 on the 32-, 64-, 96- and 128-wide instantiations (tests/
    test_viewpool.py reaches 48 only), a partial 32-voxel MFMA tile (125, 216 and 8 voxels), 1 and 16 views, dim_out 1 and
    300, 0 and 8 harmonic functions, feature sizes 4, 5, 12 and 20."""
    ref = _mlp_ref(cid) if cid in MLP_BWD else None
    feats, cams_d, sd, w, R, F, n_harm = _mlp_inputs(cid)
    if ref is None:
        out = _cached(("mlp-fwd", cid),
                      lambda: vo.voxel_features_from_views_mlp_mean(feats, cams_d, sd, w["w"], w["b"], R, EXTENT, n_harmonic=n_harm))
    else:
        out = ref["out"]
    got = _mlp_forward(_mlp_pooler(cid, sd), cid)
    assert got.shape == out.shape
    err = float((got.cpu() - out).abs().max())
    print(f"[viewpool-shapes] mlp-mean {cid}: forward max|d| {err:.2e}")
    assert err < FWD_TOL, (cid, err)
    assert out.abs().max() <= 1.0 and out.std() > 0.02


@pytest.mark.parametrize("cid", [pytest.param(c, marks=_EMU_SKIPS_CHUNK) if c == "R6-chunk27" else c for c in MLP_BWD])
def test_mlp_mean_backward_vs_autograd_of_the_oracle(cid, monkeypatch):
    """holo_mlp_mean_backward against autograd through the oracle: every aggregator parameter, the mapper and the maps at 1e-3
    of each tensor's scale; the dp-dependent buffers and GEMM shapes follow the forward's width.  `R6-chunk27`: the grid in 8
    chunks of 27 voxels (unaligned p0, the parameter gradients adding up over the chunks), also within 1e-5 of scale of the
    unchunked call."""
    monkeypatch.delenv("HOLO_MLP_MEAN_BWD_CHUNK", raising=False)
    ref = _mlp_ref(cid)
    sd = _mlp_inputs(cid)[2]
    if cid == "R6-chunk27":
        whole = _mlp_pooler(cid, sd)  # (the knob is read when the native pooler is created: at its first call)
        base = _mlp_backward(whole, cid, ref["g"])
        monkeypatch.setenv("HOLO_MLP_MEAN_BWD_CHUNK", "27")
    vp = _mlp_pooler(cid, sd)
    if cid == "R6-chunk27":
        err = float((_mlp_forward(vp, cid).cpu() - ref["out"]).abs().max())
        print(f"[viewpool-shapes] mlp-mean {cid}: forward max|d| {err:.2e}")
        assert err < FWD_TOL
    got = _mlp_backward(vp, cid, ref["g"])
    _check_mlp_grads(f"mlp-mean {cid} backward", got, ref)
    if cid == "R6-chunk27":
        pairs = [("mapper.weight", got[1], base[1]), ("mapper.bias", got[2], base[2])]
        pairs += [(k, got[3][k], base[3][k]) for k in base[3]] + [(k, got[0][k], base[0][k]) for k in base[0]]
        worst = max(_rel(a, b.cpu()) for _, a, b in pairs)
        print(f"[viewpool-shapes] mlp-mean {cid}: 8 chunks against one, worst {worst:.2e} of scale")
        for k, a, b in pairs:
            assert _rel(a, b.cpu()) < 1e-5, (k, _rel(a, b.cpu()))


# ---- 3. the workspace's earlier contents -----------------------------------------------------------------------------
def _fill_workspace(vp, byte):
    held = vp.__dict__.get("_holo_ws")
    if held is not None and byte is not None:
        held[1].fill_(byte)


@pytest.mark.parametrize("kind,cid", [("angle", "odd-maps"), ("angle", "A512"), ("angle", "R5"), ("mlp", "dp32"), ("mlp", "dp128"),
                                      ("mlp", "R5-one-view"), ("mlp", "R2-tiny-maps")])
def test_results_do_not_depend_on_the_workspace_contents(kind, cid, monkeypatch):
    """Forward and backward once, then three more times with the pooler's cached workspace filled with 0xFF (NaN), 0x00 and
    0x7F (3.4e38) bytes before every call: the forward output, the mapper's and the aggregator's parameter gradients are
    bit-equal across the four runs and finite; so are, in the deterministic mode, the map gradients, which lie within 2e-5 of
    the default mode's.  In the default mode the map gradients are atomics: finite and within 1e-3 of the oracle's.  A padded
    channel, padding row or partial tile that is read before it is written shows as a NaN or a differing bit."""
    monkeypatch.delenv("HOLO_VIEWPOOL_BWD_V1", raising=False)
    monkeypatch.delenv("HOLO_MLP_MEAN_BWD_CHUNK", raising=False)
    if kind == "angle":
        ref = _angle_ref(cid)
        vp = _angle_pooler(_angle_inputs(cid)[5])
        fwd, bwd = (lambda: _angle_forward(vp, cid)), (lambda: _angle_backward(vp, cid, ref["g"]) + ({},))
    else:
        ref = _mlp_ref(cid)
        vp = _mlp_pooler(cid, _mlp_inputs(cid)[2])
        fwd, bwd = (lambda: _mlp_forward(vp, cid)), (lambda: _mlp_backward(vp, cid, ref["g"]))

    def run(byte):
        _fill_workspace(vp, byte)
        out = fwd().clone()
        _fill_workspace(vp, byte)
        gf, gw, gb, ga = bwd()
        fixed = {"out": out, "mapper.weight": gw.clone(), "mapper.bias": gb.clone()}
        fixed.update({k: v.clone() for k, v in ga.items()})
        return fixed, {k: v.clone() for k, v in gf.items()}

    maps = {}
    for det in (False, True):
        with runtime.deterministic(det, gu.DEV):
            runs = [run(b) for b in (None, 0xFF, 0x00, 0x7F)]
        for fixed, gf in runs:
            for k, v in list(fixed.items()) + list(gf.items()):
                assert torch.isfinite(v).all(), (cid, det, k)
            for k, v in fixed.items():
                assert torch.equal(v, runs[0][0][k]), (cid, det, k)
            for k, v in gf.items():
                if det:
                    assert torch.equal(v, runs[0][1][k]), (cid, det, k)
                else:
                    assert _rel(v, ref["maps"][k]) < GRAD_TOL, (cid, k, _rel(v, ref["maps"][k]))
        maps[det] = runs[0][1]
        assert float((runs[0][0]["out"].cpu() - ref["out"]).abs().max()) < FWD_TOL
    worst = max(_rel(maps[True][k], maps[False][k].cpu()) for k in maps[True])
    print(f"[viewpool-shapes] {kind} {cid}: four workspace fills bit-equal; deterministic against default mode {worst:.2e} of scale")
    for k in maps[True]:
        assert _rel(maps[True][k], maps[False][k].cpu()) < DET_TOL, (cid, k)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def _still_works():
    """After a refusal the same process pools normally (the smallest case, against its cached reference)."""
    got = _angle_forward(_angle_pooler(_angle_inputs("R2")[5]), "R2")
    assert float((got.cpu() - _angle_ref("R2")["out"]).abs().max()) < FWD_TOL


def _angle_call(n, shapes, F, R=8, backward=False):
    feats, cams_d = _dev(_maps(77, n, shapes)), _dev_cameras(_cameras(n, 6.0, False))
    w = _mapper(F, 2 * sum(s[0] for s in shapes))
    vp = _angle_pooler(dict(gamma=1.0, min_weight=0.1))
    args = (feats, cams_d, w["w"].to(gu.DEV), w["b"].to(gu.DEV), R, EXTENT)
    if backward:
        return vp.pool_to_voxel_features_backward(*args, torch.from_numpy(np_noise(5, (1, F, R, R, R))).to(gu.DEV))
    return vp.pool_to_voxel_features(*args)


_ANGLE_REFUSALS = [
    ("17 views", dict(n=17, shapes=USUAL, F=16), r"1\.\.16 source views"),
    ("9 maps", dict(n=2, shapes=((2, 3, 3),) * 9, F=16), r"1\.\.8 feature maps"),
    ("514 aggregated features", dict(n=2, shapes=((128, 4, 5), (129, 5, 4)), F=8), r"514 aggregated features \(at most 512\)"),
    ("R = 1", dict(n=2, shapes=USUAL, F=16, R=1), r"resol >= 2"),
    ("backward at F = 33", dict(n=2, shapes=USUAL, F=33, backward=True), r"feature_size <= 32"),
    ("backward at F = 64", dict(n=2, shapes=USUAL, F=64, backward=True), r"feature_size <= 32"),
]


@pytest.mark.parametrize("what,call,fragment", _ANGLE_REFUSALS, ids=[r[0].replace(" = ", "").replace(" ", "-") for r in _ANGLE_REFUSALS])
def test_angle_weighted_refusals(what, call, fragment):
    """Beyond MAX_VIEWS, MAX_FEATS, MAX_AGG, below a 2^3 grid and, for the backward, above 32 output features the entry raises
    HoloError naming the limit, and the next call works."""
    with pytest.raises(_lib.HoloError, match=fragment):
        _angle_call(**call)
    _still_works()


def _mlp_call(n, shapes, F, n_harm=3, backward=False):
    R = 4
    feats, cams_d = _dev(_maps(78, n, shapes)), _dev_cameras(_cameras(n, 6.0, False))
    w = _mapper(F, 24)
    vp = ViewPooler(feature_aggregator_class_type="MLPMeanFeatureAggregator",
                    feature_aggregator_MLPMeanFeatureAggregator_args=dict(
                        exclude_target_view=False, exclude_target_view_mask_features=False, dim_out=24,
                        n_harmonic_functions_ray=n_harm)).to(gu.DEV)  # (LazyLinear layers: Xavier weights at the first call)
    args = (feats, cams_d, w["w"].to(gu.DEV), w["b"].to(gu.DEV), R, EXTENT)
    out = vp.pool_to_voxel_features(*args)
    if backward:
        assert torch.isfinite(out).all()
        return vp.pool_to_voxel_features_backward(*args, torch.from_numpy(np_noise(5, (1, F, R, R, R))).to(gu.DEV))
    return out


_MLP_REFUSALS = [
    ("17 views", dict(n=17, shapes=USUAL, F=16), r"1\.\.16 source views"),
    ("F = 33", dict(n=2, shapes=USUAL, F=33), r"feature_size <= 32"),
    ("9 harmonics", dict(n=2, shapes=USUAL, F=16, n_harm=9), r"<= 8 harmonic functions"),
    ("padded width above 128", dict(n=2, shapes=((16, 4, 4),) * 7, F=16), r"exceed the kernel's 128"),
    ("backward at F = 5", dict(n=2, shapes=USUAL, F=5, backward=True), r"feature_size a multiple of 4"),
    ("9 maps", dict(n=2, shapes=((2, 3, 3),) * 9, F=16), r"9 feature maps \(at most 8\)"),
]


@pytest.mark.parametrize("what,call,fragment", _MLP_REFUSALS, ids=[r[0].replace(" = ", "").replace(" ", "-") for r in _MLP_REFUSALS])
def test_mlp_mean_refusals(what, call, fragment):
    """Beyond MAX_VIEWS, 32 output features, 8 harmonic functions, a padded input width of 128, 8 feature maps (refused before
    the 8-entry channel table of the native configuration is filled) and, for the backward, a feature size that is no multiple
    of 4, the entry raises HoloError naming the limit, and the next call works."""
    with pytest.raises(_lib.HoloError, match=fragment):
        _mlp_call(**call)
    _still_works()
