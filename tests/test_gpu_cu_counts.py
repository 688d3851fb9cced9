"""The GPU parity tests under small planner CU counts (HOLO_NUM_CUS = 8, 20, 32).

Every launch geometry of the library is a function of HoloCtx::num_cus: the convolution kernel conv_plan picks, its
split-K count and the persistent grids, the key splits of the attention kernels, the weight-gradient split, the workgroup
counts of the renderer and of the view-pooling kernels.  On an MI355X that number is 256 and the suite's small shapes never
fill the chip: grid-stride loops run one trip, split decisions sit in one narrow band.  Here the same references and bounds
as in the files named per test, with the context planning for 8 CUs (the smallest count the bf16 persistent kernel takes:
the most loop trips), 20 (neither a multiple of 8 nor a power of two: num_cus & ~7 = 16, the renderer's XCD tile order
switches itself off, work lists do not divide) and 32 (the chip in CPX partition mode).

No count above the device's own is used: the persistent kernels assume one resident workgroup per counted CU.

Every case runs on inputs no other test of the suite uses, with every torch.empty output and workspace of the wrappers
NaN-filled (a tile a kernel skipped must not find the right values an identical earlier call left in the block the
allocator hands back), and checks that its result is finite first.  The oracle runs once per case and is shared by the
CU counts."""
import contextlib
import ctypes as C
import gc
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, runtime  # noqa: E402
from holo_diffusion_amd.render import (HoloMultiPassEmissionAbsorptionRenderer, HoloVoxelGridImplicitFunction,  # noqa: E402
                                       RenderMLP)
from holo_diffusion_amd.unet import SimpleUnet3D  # noqa: E402
from holo_diffusion_amd.viewpool import MLPMeanFeatureAggregator  # noqa: E402
from oracle import render_oracle as ro  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle import viewpool_oracle as vo  # noqa: E402
from oracle.common import np_noise  # noqa: E402

from tests import gpu_utils as gu  # noqa: E402
from tests import test_viewpool as tvp  # noqa: E402

CU_COUNTS = (8, 20, 32)
_cu_id = lambda n: f"cu{n}"  # noqa: E731


# ---- the fixture -----------------------------------------------------------------------------------------------------------
# probe of the fixture's own check: holo_view_pool_backward_workspace_bytes launches nothing; for R = 16 (256 groups of 16
# voxels) its per-workgroup partials of d weight / d bias take min(256, 4 * num_cus) rows of 2 * sumC * F + F floats - one
# 4-channel map and F = 16: 576 bytes a row, so every row count used here is a whole number of the 256-byte units the
# library rounds to
_PROBE_ROW_BYTES = (2 * 4 * 16 + 16) * 4


def _probe_bytes(ctx) -> int:
    cfg = _lib.HoloViewPoolCfg(16, 8.0, 16, 1.0, 0.1, 1e-2)
    arr = (_lib.HoloViewFeature * 1)()
    arr[0].feats, arr[0].channels, arr[0].height, arr[0].width = None, 4, 8, 8
    return int(runtime.lib().holo_view_pool_backward_workspace_bytes(ctx, C.byref(cfg), arr, 1, 2))


def _device_cus() -> int:
    if gu.EMU:  # (the host emulation's pretended chip, tests/emu/emu_runtime.h)
        return int(os.environ.get("HOLO_EMU_CUS", "4"))
    return int(torch.cuda.get_device_properties(gu.DEV).multi_processor_count)


_NATIVE_OWNERS = (SimpleUnet3D, HoloMultiPassEmissionAbsorptionRenderer, HoloVoxelGridImplicitFunction, RenderMLP,
                  MLPMeanFeatureAggregator)  # the classes that create native handles (each on runtime.ctx() at that moment)


def _close_native(obj) -> None:
    """Destroys the native handles under a module tree NOW, through the owners' public close() (they hold the context
    pointer they were created with): what the objects' own __del__ would do once the last Python reference is gone - a
    failed test's traceback may keep one."""
    for m in (obj.modules() if isinstance(obj, torch.nn.Module) else [obj]):
        if isinstance(m, _NATIVE_OWNERS):
            m.close()


def _poison_empty(monkeypatch) -> None:
    """torch.empty / torch.empty_like hand out NaN (floating point) and 0xFF bytes (the byte workspaces: NaN as fp32 and as
    bf16) for the rest of the test.  The library's Python wrappers allocate every output and workspace with them, and the
    caching allocator likes to return the block an identical earlier call - the same case under another CU count, the
    default-context run next to it - has just freed: a tile that a kernel skipped must read as NaN, not as the right answer."""
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(0xFF)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(real_like(*a, **k)))


class _CuContext:
    def __init__(self, n, handle, default, idx):
        self.n, self.handle, self.default, self.idx = n, handle, default, idx
        self._owned = []

    def own(self, obj):
        """Registers a model / net built under this context: its native handles are destroyed before the context is."""
        self._owned.append(obj)
        return obj

    @contextlib.contextmanager
    def default_context(self):
        """The device's ordinary context for the block (the 256-CU plans on an MI355X): for the comparisons 'same bits as the
        default context's output' and 'another plan than the default context's'."""
        runtime._CTX[self.idx] = self.default
        try:
            yield
        finally:
            runtime._CTX[self.idx] = self.handle


@pytest.fixture
def cu(request, monkeypatch):
    """A context of the test's own that plans for ``request.param`` CUs.  HOLO_NUM_CUS is read once, in holo_ctx_create, and
    runtime.py caches one context per device: the knob is set, the device's entry taken out of the cache, and the next
    runtime.ctx() creates a fresh context under the knob.  Everything the test builds holds that context; at teardown the
    device is drained, the test's native handles are destroyed, then the temporary context, and monkeypatch puts the cached
    entry back."""
    n = int(request.param)
    dev_cus = _device_cus()
    if not gu.EMU:  # (the emulation has no residency to speak of, and its pretended chip has 4 CUs)
        assert n <= dev_cus, f"HOLO_NUM_CUS {n} above the device's {dev_cus} CUs: a persistent kernel may wait on a workgroup that is not resident"
    idx = 0
    default = runtime.ctx(gu.DEV)  # (created here if this file runs alone)
    assert runtime._CTX[idx] is default
    monkeypatch.setenv("HOLO_NUM_CUS", str(n))
    monkeypatch.delitem(runtime._CTX, idx)
    handle = runtime.ctx(gu.DEV)
    c = _CuContext(n, handle, default, idx)
    _poison_empty(monkeypatch)
    try:
        assert handle.value != default.value
        # the count took effect (a mistyped variable or a re-used context would leave this file on the default plans again)
        rows = lambda cus: min(256, 4 * cus)  # noqa: E731
        want = (rows(dev_cus) - rows(n)) * _PROBE_ROW_BYTES
        assert want != 0, (dev_cus, n)
        assert _probe_bytes(default) - _probe_bytes(handle) == want, (_probe_bytes(default), _probe_bytes(handle), want)
        yield c
    finally:
        torch.cuda.synchronize()
        for obj in c._owned:
            _close_native(obj)
        c._owned.clear()
        gc.collect()
        runtime._CTX[idx] = handle  # (a test that failed inside default_context(): monkeypatch restores the entry below)
        runtime.lib().holo_ctx_destroy(handle)


def _cu(*counts):
    return pytest.mark.parametrize("cu", list(counts), indirect=True, ids=_cu_id)


_REF = {}


def _cached(key, make):
    """One oracle run per case, shared by the CU counts (and left unchanged by them)."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _finite(t, what=""):
    assert torch.isfinite(t).all(), what


# ---- 5. view pooling, forward ------------------------------------------------------------------------------------------------
@_cu(8, 20)
@pytest.mark.parametrize("R,n_src,radius,gamma", [(16, 3, 6.0, 2.0), (12, 3, 10.0, 1.0)])
def test_view_pool_forward(cu, R, n_src, radius, gamma):
    """view_pool_kernel against the oracle of tests/test_viewpool.py::test_view_pool_kernel_vs_oracle at its 1e-4 bound.  Its
    grid does not depend on the CU count; every voxel's arithmetic is independent of its workgroup: bit-equal to the default
    context's output."""
    feats, cams_d, w, F = tvp._angle_inputs(R, n_src, radius, seed=700 + R)
    ref = _cached(("vp", R, n_src, radius, gamma),
                  lambda: vo.voxel_features_from_views(feats, cams_d, w["w"], w["b"], R, 8.0, gamma=gamma))
    dev_feats = {k: v.to(gu.DEV) for k, v in feats.items()}
    cams = tvp._dev_cameras(cams_d)
    got = cu.own(tvp._angle_model(R, F, gamma, w)).pool_views_to_voxel_features(dev_feats, cams).clone()
    assert got.shape == (1, F, R, R, R)
    _finite(got)
    assert (got.cpu() - ref).abs().max().item() < 1e-4
    assert ref.abs().max() <= 1.0 and ref.std() > 0.05
    with cu.default_context():
        base = cu.own(tvp._angle_model(R, F, gamma, w)).pool_views_to_voxel_features(dev_feats, cams)
    assert torch.equal(got, base)


_MLP_MEAN = dict(F=16, dim_out=24, n_harm=3)  # (the smallest aggregator of tests/test_viewpool.py)


@_cu(8, 20)
@pytest.mark.parametrize("R,n_src,radius", [(16, 3, 6.0), (12, 3, 10.0)])
def test_mlp_mean_pool_forward(cu, R, n_src, radius):
    """mlp_mean_pool_kernel against the oracle of test_mlp_mean_view_pool_kernel_vs_oracle at its 1e-4 bound.  The launcher
    takes min(ceil(tiles / 4), num_cus) workgroups of four waves, one 32-voxel tile per wave and trip (tile += gridDim.x * 4):
      R = 16: 128 tiles; 8 CUs -> 8 workgroups, four trips each; 20 CUs -> 20 workgroups, 80 tiles a trip: the second trip
              is ragged (48 tiles); the default context: 32 workgroups, one trip;
      R = 12: 1728 voxels = 54 tiles; 8 CUs -> 8 workgroups, the second trip ragged (22 of 32 waves); 20 CUs -> ceil(54 / 4)
              = 14 workgroups, one trip with two idle waves.
    Every voxel's arithmetic is independent of the workgroup that computes it: bit-equal to the default context's output."""
    F, dim_out, n_harm = _MLP_MEAN["F"], _MLP_MEAN["dim_out"], _MLP_MEAN["n_harm"]
    feats, cams_d, sd, shapes, w = tvp._mlp_mean_inputs(R, n_src, radius, F, dim_out, n_harm, seed=800 + R)
    ref = _cached(("mm", R, n_src, radius), lambda: vo.voxel_features_from_views_mlp_mean(
        feats, cams_d, sd, w["w"], w["b"], R, 8.0, n_harmonic=n_harm))
    dev_feats = {k: v.to(gu.DEV) for k, v in feats.items()}
    cams = tvp._dev_cameras(cams_d)
    got = cu.own(tvp._mlp_mean_model(R, F, dim_out, n_harm, sd, w)).pool_views_to_voxel_features(dev_feats, cams).clone()
    assert got.shape == (1, F, R, R, R)
    _finite(got)
    assert (got.cpu() - ref).abs().max().item() < 1e-4
    assert ref.abs().max() <= 1.0 and ref.std() > 0.02
    with cu.default_context():
        base = cu.own(tvp._mlp_mean_model(R, F, dim_out, n_harm, sd, w)).pool_views_to_voxel_features(dev_feats, cams)
    assert torch.equal(got, base)


# ---- 6. view pooling, backward -----------------------------------------------------------------------------------------------
# view_pool_bwd_kernel / view_pool_bwd2_kernel: min(ceil(R^3 / 16), 4 * num_cus) workgroups walk the groups of 16 voxels with
# stride gridDim.x; 8 CUs -> 32 workgroups:
#   R = 16: 256 groups, eight per workgroup (the default context: 256 workgroups, one each); coarse maps, so that segmented
#           sums cross a group boundary inside one workgroup
#   R = 12: 108 groups: three full trips and a ragged fourth (12 of 32 workgroups)
#   R = 6:  14 groups, the last one half empty, fewer groups than workgroups
_BWD_ROWS = [(16, 3, 6.0, 2.0, True), (12, 3, 10.0, 1.0, False), (6, 2, 7.0, 1.0, False)]


@_cu(8)
@pytest.mark.parametrize("v1", ["0", "1"])
@pytest.mark.parametrize("R,n_src,radius,gamma,coarse", _BWD_ROWS)
def test_view_pool_backward(cu, R, n_src, radius, gamma, coarse, v1, monkeypatch):
    """holo_view_pool_backward, both kernel forms, against autograd through the oracle as
    test_view_pool_backward_vs_autograd_of_the_oracle (rel < 1e-3); group counts above."""
    monkeypatch.setenv("HOLO_VIEWPOOL_BWD_V1", v1)
    feats, cams_d, w, F = tvp._angle_inputs(R, n_src, radius, seed=900 + R, coarse=coarse)
    g = torch.from_numpy(np_noise(923, (1, F, R, R, R)))
    leaves, mw, mb = _cached(("vpb", R, n_src, radius, gamma, coarse),
                             lambda: tvp._angle_oracle_grads(feats, cams_d, w, R, gamma, g))
    model = cu.own(tvp._angle_model(R, F, gamma, w))
    cams = tvp._dev_cameras(cams_d)
    dev_feats = {k: v.to(gu.DEV) for k, v in feats.items()}
    got = model.pool_views_backward(dev_feats, cams, g.to(gu.DEV))
    for k, v in got["image_features"].items():
        _finite(v, k)
    for k, v in got["pooled_feature_mapper"].items():
        _finite(v, k)
    tvp._check_angle_backward(got, feats, leaves, mw, mb)


@_cu(8)
@pytest.mark.parametrize("v1", ["0", "1"])
def test_view_pool_backward_deterministic_mode(cu, v1, monkeypatch):
    """The deterministic mode of holo_view_pool_backward as tests/test_viewpool.py::test_view_pool_backward_deterministic_mode,
    on the R = 16 coarse-map row (eight groups per workgroup): two calls bit-identical, feature-map gradients within 2e-5 of
    the atomic mode's, mapper gradients (fixed-order sums in both modes) bit-identical between the modes."""
    monkeypatch.setenv("HOLO_VIEWPOOL_BWD_V1", v1)
    R, n_src, radius, gamma, coarse = _BWD_ROWS[0]
    feats, cams_d, w, F = tvp._angle_inputs(R, n_src, radius, seed=940, coarse=coarse)
    g = torch.from_numpy(np_noise(941, (1, F, R, R, R))).to(gu.DEV)
    model = cu.own(tvp._angle_model(R, F, gamma, w))
    cams = tvp._dev_cameras(cams_d)
    dev_feats = {k: v.to(gu.DEV) for k, v in feats.items()}

    def run():
        out = model.pool_views_backward(dev_feats, cams, g)
        return ({k: v.clone() for k, v in out["image_features"].items()},
                {k: v.clone() for k, v in out["pooled_feature_mapper"].items()})

    with runtime.deterministic(True, gu.DEV):
        f1, m1 = run()
        f2, m2 = run()
    with runtime.deterministic(False, gu.DEV):
        fa, ma = run()
    for k in m1:
        _finite(m1[k], k)
        assert torch.equal(m1[k], m2[k]) and torch.equal(m1[k], ma[k]), k
    for k in feats:
        _finite(f1[k], k)
        scale = float(fa[k].abs().max())
        assert scale > 0 and torch.equal(f1[k], f2[k]), k
        assert float((f1[k] - fa[k]).abs().max()) < 2e-5 * scale, (k, float((f1[k] - fa[k]).abs().max()) / scale)


@_cu(8)
@pytest.mark.parametrize("R,n_src,radius,coarse", [(16, 3, 6.0, True), (12, 3, 10.0, False), (6, 2, 7.0, False)])
def test_mlp_mean_backward(cu, R, n_src, radius, coarse):
    """holo_mlp_mean_backward against autograd through the oracle as
    test_mlp_mean_view_pool_backward_vs_autograd_of_the_oracle (rel < 1e-3), at the grid sizes of the test above.  None of its
    launches is sized by the CU count (only the forward it follows, mlp_mean_pool_kernel, is): the same plan under every
    count - the case holds the entry to its bounds on a context that is not the device's default one."""
    F, dim_out, n_harm = _MLP_MEAN["F"], _MLP_MEAN["dim_out"], _MLP_MEAN["n_harm"]
    feats, cams_d, sd, shapes, w = tvp._mlp_mean_inputs(R, n_src, radius, F, dim_out, n_harm, seed=960 + R, coarse=coarse)
    g = torch.from_numpy(np_noise(961, (1, F, R, R, R)))
    leaves, psd, mw, mb = _cached(("mmb", R, n_src, radius, coarse),
                                  lambda: tvp._mlp_mean_oracle_grads(feats, cams_d, sd, w, R, n_harm, g))
    model = cu.own(tvp._mlp_mean_model(R, F, dim_out, n_harm, sd, w))
    cams = tvp._dev_cameras(cams_d)
    dev_feats = {k: v.to(gu.DEV) for k, v in feats.items()}
    model.pool_views_to_voxel_features(dev_feats, cams)
    got = model.pool_views_backward(dev_feats, cams, g.to(gu.DEV))
    for grp in ("image_features", "feature_aggregator", "pooled_feature_mapper"):
        for k, v in got[grp].items():
            _finite(v, (grp, k))
    tvp._check_mlp_mean_backward(got, feats, shapes, leaves, psd, mw, mb)


# ---- the denoiser ------------------------------------------------------------------------------------------------------------
_PLAN_CONV = re.compile(r"\[plan\] conv (?P<cin>\d+)->(?P<cout>\d+) k(?P<ksz>\d) s(?P<stride>\d) @(?P<dim>\d+)\^3 batch (?P<batch>\d+)"
                        r"(?P<skip> \+skip)?: (?P<kernel>\w+), tz \d+, split-K (?P<nsplit>\d+) x \d+ chunks \(skip \d+\), grid_x (?P<grid_x>\d+)")
_PLAN_ATTN = re.compile(r"\[plan\] attention (?P<tag>\S+): T=(?P<T>\d+) C=\d+ heads=\d+ -> (?P<form>\w+) flash kernel, (?P<splits>\d+) key splits")


def _plan_of(text, batch):
    """The HOLO_DEBUG_PLAN lines of the launches at ``batch``: (convolutions, attentions) as lists of dicts, duplicates
    (the plan is printed whenever it is made: workspace query, forward) dropped."""
    convs, attns = {}, {}
    for ln in text.splitlines():
        m = _PLAN_CONV.match(ln)
        if m and int(m["batch"]) == batch:
            d = {k: (v if k in ("kernel", "skip") else int(v)) for k, v in m.groupdict().items()}
            convs[ln] = d
        m = _PLAN_ATTN.match(ln)
        if m:
            attns[ln] = dict(tag=m["tag"], T=int(m["T"]), form=m["form"], splits=int(m["splits"]))
    return list(convs.values()), list(attns.values())


def _wino3_items(c):
    """work items of a conv_wino3_kernel launch: 2 x 8 x 8 tiles x 64-channel output blocks x splits"""
    return (c["batch"] * c["dim"] ** 3 // 128) * (c["cout"] // 64) * c["nsplit"]


def _unet_cfg(image, mc, mult, attn, nrb=2):
    return uo.UNetCfg(image_size=image, in_channels=16, out_channels=16, model_channels=mc, num_res_blocks=nrb,
                      channel_mult=mult, attention_resolutions=attn, num_heads=2)


def _unet_case(cfg_args, batch, seed):
    """Inputs and the oracle's trace of one net, made once and shared by the CU counts and the compute modes."""
    def make():
        cfg = _unet_cfg(*cfg_args)
        sd = gu.synth_state_dict(uo.unet_param_shapes(cfg), seed)
        x = torch.from_numpy(np_noise(seed + 1, (batch, 16) + (cfg.image_size,) * 3))
        t = torch.tensor([611, 29, 902][:batch], dtype=torch.int64)
        trace = {}
        ref = uo.unet_forward(sd, cfg, x, t, trace)
        return cfg, x, t, ref, trace
    return _cached(("unet", cfg_args, batch, seed), make)


def _plan_summary(convs):
    """(kernel, grid edge, split-K, grid_x[, work items of a conv_wino3_kernel launch])"""
    return sorted({(c["kernel"], c["dim"], c["nsplit"], c["grid_x"]) + ((_wino3_items(c),) if c["kernel"] == "conv_wino3_kernel" else ())
                   for c in convs})


# (image, mc, mult, attn), batch, weights seed
_NET_A = ((16, 64, (1, 2, 2), (4,)), 2, 1301)  # the second net of test_mid_size_unet_vs_oracle_blockwise
_NET_B = ((8, 64, (1, 2), (2,)), 1, 1311)      # its first


@_cu(*CU_COUNTS)
@pytest.mark.parametrize("compute", ["f32", "f32_bf16x3"])
@pytest.mark.parametrize("net_id", ["A16", "B8"])
def test_unet_forward_blockwise(cu, net_id, compute, monkeypatch, capfd):
    """Every block output against the pinned oracle as tests/test_gpu_unet.py::test_mid_size_unet_vs_oracle_blockwise
    (rel_err < 1e-4 per block) and, in the f32_bf16x3 mode, ::test_f32_bf16x3_mode_meets_the_fp32_tolerance (the same bound);
    no kernel-forcing knob.  What conv_plan decides for these nets in exact fp32 under 8 CUs (t3 = 128-voxel tiles x 64-channel
    output blocks of one launch; wino3_split = ceil(num_cus / t3) up to the 32-channel chunks; the kernel from num_cus / 2 = 4
    items on; grid_x = ceil(items / ceil(items / num_cus))):
      A16, batch 2: 16^3 level, 64 channels: t3 = 64 -> no split, 64 items on grid_x 8: eight items per workgroup (the
                    default context: split-K 2, 128 items, one each); 8^3 level, 128 channels: t3 = 16, grid_x 8;
      B8, batch 1:  8^3 level, 64 channels: t3 = 4 -> split-K 2, 8 items; into 128 channels at 8^3: does not occur (4^3)."""
    args, batch, seed = _NET_A if net_id == "A16" else _NET_B
    cfg, x, t, ref, trace = _unet_case(args, batch, seed)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    capfd.readouterr()
    net = cu.own(gu.make_unet(cfg, seed=seed, compute_dtype=compute)[0])
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    _finite(y)
    assert gu.rel_err(y, ref) < 1e-4
    gu.block_outputs_vs_oracle(net, trace, 1e-4, (net_id, compute, cu.n))
    convs, _ = _plan_of(capfd.readouterr().err, batch)
    assert convs
    if compute != "f32":
        return
    # the plan of the default context for the same net: another set of (kernel, split-K) pairs
    with cu.default_context():
        base = cu.own(gu.make_unet(cfg, seed=seed, compute_dtype=compute)[0])
        base.workspace_bytes(batch, gu.DEV)  # (plans; launches nothing)
    base_convs, _ = _plan_of(capfd.readouterr().err, batch)
    pairs = lambda cs: {(c["kernel"], c["cin"], c["cout"], c["dim"], c["nsplit"]) for c in cs}  # noqa: E731
    assert base_convs and pairs(base_convs) != pairs(convs), (_plan_summary(base_convs), _plan_summary(convs))
    if cu.n != 8:
        return
    w3 = [c for c in convs if c["kernel"] == "conv_wino3_kernel"]
    if net_id == "A16":
        assert {c["dim"] for c in w3} == {16, 8}, _plan_summary(convs)
        assert any(c["grid_x"] < _wino3_items(c) for c in w3 if c["dim"] == 16), _plan_summary(convs)
        assert all(c["grid_x"] <= 8 for c in w3)
    else:
        assert {c["dim"] for c in w3} == {8}, _plan_summary(convs)
        assert any(c["nsplit"] > 1 for c in w3), _plan_summary(convs)


# ---- 2. bf16 storage mode
@_cu(8, 20)
def test_bf16_storage_mode_blockwise(cu, monkeypatch, capfd):
    """The net and bounds of tests/test_gpu_unet.py::test_bf16_storage_mode_blockwise (every block output at 2e-2 of the fp32
    oracle) with no HOLO_CONV_BF16T / HOLO_CONV_BF16P / HOLO_CONV_S2T: the persistent wide-tile kernel (conv_bf16p_kernel) and
    the stride-2 halo kernel (conv_s2_bf16_kernel) by the planner's own choice.  The persistent form needs raw input, no
    split-K (t8 >= num_cus 8^3-tiles x 64-channel slices), t8 >= 2 * num_cus or a K extent of 192, and t8 >= (num_cus & ~7):
      8 CUs, batch 2:  the input convolution 16 -> 64 at 16^3: t8 = 16 on grid_x 8, two tiles per workgroup; the Upsample
                       convolution 128 -> 128 at 16^3: t8 = 32, four per workgroup;
      20 CUs, batch 3: (at batch 2 no raw-input launch reaches 2 * 20 tiles) the Upsample convolution: t8 = 48 >= 40 on
                       grid_x 16 = 20 & ~7, three tiles per workgroup; the input convolution (t8 = 24) stays on the halo kernel.
    The stride-2 kernel runs from num_cus / 4 tiles on: the Downsample 16^3 -> 8^3 has 8 (12) of them."""
    batch = 2 if cu.n == 8 else 3
    args, _, seed = _NET_A
    cfg, x, t, ref, trace = _unet_case(args, batch, seed + 40)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    for k in ("HOLO_CONV_BF16T", "HOLO_CONV_BF16P", "HOLO_CONV_S2T", "HOLO_CONV_BF16P_WGS"):
        monkeypatch.delenv(k, raising=False)
    capfd.readouterr()
    net = cu.own(gu.make_unet(cfg, seed=seed + 40, compute_dtype="bf16")[0])
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    _finite(y)
    assert 1e-5 < gu.rel_err(y, ref) < 2e-2
    gu.block_outputs_vs_oracle(net, trace, 2e-2, ("bf16", cu.n))
    convs, _ = _plan_of(capfd.readouterr().err, batch)
    pers = [c for c in convs if c["kernel"] == "conv_bf16p_kernel"]
    assert pers and any(c["kernel"] == "conv_s2_bf16_kernel" for c in convs), _plan_summary(convs)
    for c in pers:  # several tiles per persistent workgroup
        tiles = (c["batch"] * c["dim"] ** 3 // 512) * ((c["cout"] + 63) // 64)
        assert c["grid_x"] == (cu.n & ~7) and tiles >= 2 * c["grid_x"], c


@_cu(8, 20)
def test_bf16_attention_level_at_16_cubed(cu, monkeypatch, capfd):
    """One attention block at 16^3 (T = 4096) in the bf16 mode, as tests/test_gpu_unet.py::test_bf16_flash_attention_vs_oracle
    (output within 2e-2 of the fp32 oracle) without HOLO_BF16_FLASH_MIN_T: flash_attn_bf16v2_ksplit and
    conv1x1_qkv_bf16_plan size their grids from num_cus."""
    args, batch, seed = (16, 64, (1, 2), (1,), 1), 2, 1361
    cfg, x, t, ref, trace = _unet_case(args, batch, seed)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    capfd.readouterr()
    net = cu.own(gu.make_unet(cfg, seed=seed, compute_dtype="bf16")[0])
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    _finite(y)
    err = gu.rel_err(y, ref)
    assert 1e-5 < err < 2e-2, err
    gu.block_outputs_vs_oracle(net, trace, 2e-2, ("bf16 attention", cu.n))
    convs, attns = _plan_of(capfd.readouterr().err, batch)
    big = [a for a in attns if a["T"] == 4096]  # (the middle block's T = 512 stays on the fp32 kernel)
    assert big and all(a["form"] == "bf16" for a in big), attns
    assert any(c["kernel"] == "conv1x1_qkv_bf16_kernel" for c in convs), _plan_summary(convs)


# ---- 3. fp32 attention
@_cu(8, 32)
def test_fp32_attention(cu, monkeypatch, capfd):
    """tests/test_gpu_attention_fp32.py::CASES["T512_ch128"] with HOLO_FLASH_SPLIT unset, same oracle and bounds (1e-4, block by
    block).  flash_attn_splits: the un-split grid has 2 heads x 512 / 32 = 32 workgroups, a split only below num_cus of them:
    one key split under 8 and under 32 CUs (the default context: four)."""
    from tests import test_gpu_attention_fp32 as ta
    monkeypatch.delenv("HOLO_FLASH_SPLIT", raising=False)
    monkeypatch.setenv("HOLO_KEEP_INTERMEDIATES", "1")
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    c = ta.CASES["T512_ch128"]
    args, batch, seed = (c["image"], c["mc"], c["mult"], c["attn"], 1), c["batch"], 1371
    cfg, x, t, ref, trace = _unet_case(args, batch, seed)
    capfd.readouterr()
    net = cu.own(gu.make_unet(cfg, seed=seed)[0])
    with torch.no_grad():
        y = net(x.to(gu.DEV), t.to(gu.DEV))
    _finite(y)
    assert gu.rel_err(y, ref) < 1e-4
    gu.block_outputs_vs_oracle(net, trace, 1e-4, ("fp32 attention", cu.n))
    _, attns = _plan_of(capfd.readouterr().err, batch)
    assert attns and all(a["form"] == "fp32" and a["T"] == 512 and a["splits"] == 1 for a in attns), attns
    with torch.no_grad():  # the merge-free path is a fixed order too: a second forward is bit-identical
        y2 = net(x.to(gu.DEV), t.to(gu.DEV))
    assert torch.equal(y, y2)


# ---- 4. denoiser backward
_BWD_CACHE = {}


@_cu(8, 32)
@pytest.mark.parametrize("cfg_name", ["wide", "deep", "wide-tiled-reduce"])
def test_unet_backward(cu, cfg_name, monkeypatch):
    """tests/test_gpu_backward.py::test_unet_backward_vs_oracle_autograd (its body, its _check at rtol 1e-3) on the nets `wide`
    and `deep`.  wgrad_plan's row-staged kernel takes splits = ceil(2 * num_cus / pairs) slabs (pairs = 32 x 32 channel blocks
    of the weight), at most rows / 8 and 64: under 8 CUs that is ceil(16 / pairs) - 4 for a 64 x 64 weight, 2 for 128 x 64 and
    ONE from 128 x 128 on, the un-split launch and its reduce - where the default context (ceil(512 / pairs)) sits on the
    rows / 8 cap for all of them; `wide-tiled-reduce`: the reduce's tile form (HOLO_WGRAD_REDUCE_TILE_MIN=1) behind the same
    splits."""
    from tests import test_gpu_backward as tb
    if gu.EMU:
        pytest.skip("backward tests run on the device")
    name = cfg_name
    if cfg_name == "wide-tiled-reduce":
        monkeypatch.setenv("HOLO_WGRAD_REDUCE_TILE_MIN", "1")
        name = "wide"
    tb._backward_vs_oracle(gu, tb.BACKWARD_CFGS[name], 1, name, seeds=(1405, 1401, 1402), cache=_BWD_CACHE, own=cu.own)


# ---- 9. invariants
@_cu(8)
def test_batch_invariant_rows_equal_batch1(cu):
    """tests/test_gpu_batched_chains.py::test_batch_invariant_forward_rows_equal_batch1 on its 16^3 net: with the flag on every
    row of a batch-3 forward (both layouts) is bit-equal to its batch-1 forward."""
    from oracle.common import seeded_input
    from tests import test_gpu_batched_chains as tc
    cfg = tc.TINY_CFG if gu.EMU else tc.MID_CFG
    net = cu.own(gu.make_unet(cfg, seed=1501)[0])
    xs = torch.cat([seeded_input(cfg, 1510 + b) for b in range(3)]).to(gu.DEV)
    ts = torch.tensor([999, 500, 3], device=gu.DEV)
    y1_off = net(xs[:1], ts[:1])
    _finite(y1_off)
    net.set_batch_invariant(True)
    assert net.batch_invariant
    assert torch.equal(net(xs[:1], ts[:1]), y1_off)
    for cl in (False, True):
        assert all(tc._rows_vs_batch1(net, xs, ts, cl)), cl
    net.set_batch_invariant(False)
    assert torch.equal(net(xs[:1], ts[:1]), y1_off)


@_cu(8, 20)
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_forward_is_repeatable_on_any_workspace_contents(cu, compute):
    """tests/test_gpu_unet.py::test_repeated_forwards_are_bit_identical and ::test_forward_does_not_depend_on_workspace_contents
    on the second net of the latter: forwards on a workspace of zeros, of 0xFF and of 0x7F bytes and a repeat are finite
    and bit-identical, and right.  Smaller split counts leave more of the scratch untouched between ops: that is where stale
    memory would show."""
    args, batch, seed = (16, 64, (1, 2, 2), (1, 2)), 2, 1521
    cfg, x, t, ref, _ = _unet_case(args, batch, seed)
    net = cu.own(gu.make_unet(cfg, seed=seed, compute_dtype=compute)[0])
    x, t = x.to(gu.DEV), t.to(gu.DEV)
    outs = []
    for fill in (0, 0xFF, 0x7F, 0x7F):
        ws = runtime.workspace(net, gu.DEV, net.workspace_bytes(batch, gu.DEV))
        ws.fill_(fill)
        with torch.no_grad():
            outs.append(net(x, t).clone())
    for o in outs:
        _finite(o)
        assert torch.equal(outs[0], o)
    assert gu.rel_err(outs[1], ref) < (2e-2 if compute == "bf16" else 2e-3)


# ---- the renderer ------------------------------------------------------------------------------------------------------------
from tests.test_gpu_render import TINY_UNET  # noqa: E402


def _render_case(R, C, H, W, n_fine, n_cams, seed, bias, with_normals=False, oracle_frames=None):
    """Model arguments, grid, cameras and the oracle's frames (made once, shared by the CU counts)."""
    def make():
        rcfg = ro.RenderCfg(resol=R, feature_size=C, image_height=H, image_width=W, n_pts_fine=n_fine)
        msd = gu.synth_state_dict(ro.render_mlp_param_shapes(rcfg), 4321)
        msd["_density_net.mlp.3.0.bias"][-1] += bias
        grid = torch.tanh(torch.from_numpy(np_noise(seed, (1, C, R, R, R))))
        cams = hda.get_simple_360_camera_trajectory(2 * math.pi, n_cams, -30.0 * (2 * math.pi / 360), 10, (0.0, -1.0, 0.0), 3.2)
        frames = range(n_cams) if oracle_frames is None else oracle_frames
        refs = {i: ro.render(grid, msd, gu.cam_dict(cams, i), rcfg, with_normals=with_normals) for i in frames}
        return grid, cams, refs
    return _cached(("render", R, C, H, W, n_fine, n_cams, seed, bias, with_normals), make)


def _check_frames(out, refs, with_normals=False):
    """the bounds of tests/test_gpu_render.py::test_render_vs_oracle (and ::test_rendered_normals_vs_oracle for the normals)"""
    far = 14.0
    for k in ("images_render", "masks_render", "depths_render"):
        _finite(out[k], k)
    for i, ref in refs.items():
        for k, tol in (("images_render", 2e-4), ("masks_render", 2e-4), ("depths_render", 2e-4 * far)):
            err = (out[k][i].cpu() - ref[k][0]).abs().max().item()
            assert err < tol, (i, k, err)
        if with_normals:
            _finite(out["normals_render"])
            assert (out["normals_render"][i].cpu() - ref["normals_render"][0]).abs().max().item() < 5e-4, i


@_cu(8, 20)
@pytest.mark.parametrize("case", ["plain", "normals"])
def test_render_three_cameras_ragged_frame(cu, case):
    """holo_render, evaluation mode, against oracle.render_oracle at the bounds of test_render_vs_oracle: a 23 x 21 frame (483
    pixels: 121 tiles of four rays, the last one ragged) of an 8^3 grid for three cameras in one render_views call, on the
    (ray, depth)-tiled kernel.  Workgroups = min(ceil(tiles / waves per workgroup), num_cus); 363 tiles on 12-wave workgroups
    (`plain`: 32 features, 64 fine samples) ask for 31, on 10-wave ones (`normals`: 16 features, 16 fine samples, with the
    density field) for 37, so the count is the cap:
      8 CUs:  8 workgroups, a multiple of 8: the XCD-range tile order is on, the eight range boundaries 363 * k / 8 fall
              inside cameras (none is a multiple of 121), every range ends in single-ray tail items;
      20 CUs: 20 workgroups, not a multiple of 8: the plain dynamic hand-out.
    (The default context: 31 / 37 workgroups, below its cap: no XCD order, at most one tile per wave and a few.)"""
    C, n_fine = (16, 16) if case == "normals" else (32, 64)
    R, H, W, n_cams = 8, 23, 21, 3
    grid, cams, refs = _render_case(R, C, H, W, n_fine, n_cams, 1601, 0.05, with_normals=case == "normals")
    model = cu.own(gu.make_model(R, C, H, W, TINY_UNET, n_fine=n_fine, density_bias=0.05)[0])
    model.net_3d_enabled = False
    if case == "normals":
        model._implicit_functions[0]._fn.render_normals = True
    out = model.render_views(grid.to(gu.DEV), cams.to(gu.DEV))
    assert out["images_render"].shape == (n_cams, 3, H, W)
    _check_frames(out, refs, with_normals=case == "normals")
    assert min(float(r["masks_render"].min()) for r in refs.values()) < 0.5  # (partially transparent rays)
    again = model.render_views(grid.to(gu.DEV), cams.to(gu.DEV))
    assert torch.equal(again["images_render"], out["images_render"]) and torch.equal(again["depths_render"], out["depths_render"])


@_cu(8, 20)
def test_render_split_arithmetic_second_trip(cu):
    """holo_render in the f32_bf16x3 mode (32 features) at the bounds of test_render_vs_oracle: the ray-per-column kernel,
    tiles of 32 rays, a STATIC stride (tile += workgroups x 12 waves) and one 32 KB scratch slot per resident wave.  The
    23 x 21 frame has 16 tiles (the last one of 3 rays); workgroups = min(ceil(tiles / 12), num_cus):
      8 CUs:  7 cameras = 112 tiles -> ceil(112 / 12) = 10, capped to 8 workgroups = 96 waves: 16 waves take a second tile;
      20 CUs: 16 cameras = 256 tiles -> 22, capped to 20 workgroups = 240 waves: 16 waves take a second tile.
    (Three cameras would be 48 tiles on 4 workgroups under every count.)  The waves per workgroup are read back from the size
    of the scratch - the one place the renderer shows its workgroup count: num_cus workgroups' worth of slots behind the
    channels-last grid here, the device's in the default context - and the tile count is held against them."""
    R, C, H, W, n_fine = 8, 32, 23, 21, 64
    n_cams = {8: 7, 20: 16}[cu.n]
    grid, cams, refs = _render_case(R, C, H, W, n_fine, n_cams, 1621, 0.05)
    model = cu.own(gu.make_model(R, C, H, W, TINY_UNET, n_fine=n_fine, density_bias=0.05)[0])
    model.net_3d_enabled = False
    model.renderer.compute_dtype = "f32_bf16x3"
    out = model.render_views(grid.to(gu.DEV), cams.to(gu.DEV))
    assert out["images_render"].shape == (n_cams, 3, H, W)
    _check_frames(out, refs)
    assert min(float(r["masks_render"].min()) for r in refs.values()) < 0.5
    again = model.render_views(grid.to(gu.DEV), cams.to(gu.DEV))
    assert torch.equal(again["images_render"], out["images_render"]) and torch.equal(again["depths_render"], out["depths_render"])
    L = runtime.lib()
    slots = lambda m: int(L.holo_render_workspace_bytes(m.renderer._handle, n_cams, 0)) - R ** 3 * C * 4 - 256  # noqa: E731
    with cu.default_context():
        base = cu.own(gu.make_model(R, C, H, W, TINY_UNET, n_fine=n_fine, density_bias=0.05)[0])
        base.net_3d_enabled = False
        base.renderer.compute_dtype = "f32_bf16x3"
        base.render_views(grid.to(gu.DEV), cams[[0]].to(gu.DEV))
    assert slots(model) > 0 and slots(model) % (cu.n * 32768) == 0
    waves = slots(model) // (cu.n * 32768)
    assert waves == slots(base) // (_device_cus() * 32768) == 12, (slots(model), slots(base))
    n_tiles = n_cams * ((H * W + 31) // 32)
    assert cu.n * waves < n_tiles < 2 * cu.n * waves, (n_tiles, cu.n, waves)  # capped, and a ragged second trip


@_cu(8)
def test_render_34_cameras_in_two_launches(cu):
    """34 cameras of a 6 x 7 frame in one render_views call: two launches of 17 (the launch parameters hold 32 cameras, more
    are split evenly).  Every frame is bit-equal to the single-camera render of its camera, as
    test_batched_views_equal_single_views_and_are_deterministic asks of three; frames 0, 16, 17 and 33 against the oracle.
    17 x 11 tiles a launch on 8 workgroups."""
    R, C, H, W, n_fine, n_cams = 8, 32, 6, 7, 64, 34
    grid, cams, refs = _render_case(R, C, H, W, n_fine, n_cams, 1611, 0.05, oracle_frames=(0, 16, 17, 33))
    model = cu.own(gu.make_model(R, C, H, W, TINY_UNET, n_fine=n_fine, density_bias=0.05)[0])
    model.net_3d_enabled = False
    dgrid, dcams = grid.to(gu.DEV), cams.to(gu.DEV)
    allv = model.render_views(dgrid, dcams)
    assert allv["images_render"].shape == (n_cams, 3, H, W)
    _check_frames(allv, refs)
    for i in range(n_cams):
        one = model(camera=dcams[i], voxel_features=dgrid)
        for k in ("images_render", "depths_render", "masks_render"):
            assert torch.equal(one[k][0], allv[k][i]), (i, k)


# ---- 8. training mode and backward
@_cu(8)
def test_render_rays_backward(cu):
    """The row (P 12, Pf 10, C 16, R 8, 3 cameras x 13 rays) of
    tests/test_gpu_render_backward.py::test_render_rays_backward_vs_oracle_autograd, its body and bounds.  The training-mode
    forward launches min(ceil(tiles / 12), num_cus) workgroups of 12 waves for 3 x ceil(13 / 4) = 12 tiles of four rays: ONE
    workgroup, under 8 CUs as under 256 - this row's launches do not depend on the CU count; it holds the entry, its training
    handle and its workspace to their bounds on a context that is not the device's default one."""
    from tests import test_gpu_render_backward as trb
    trb._render_rays_backward_case(gu, 12, 10, 16, 8, 3, 13, "all", seed=1700, own=cu.own)
