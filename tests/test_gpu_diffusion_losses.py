"""GPU: the diffusion losses and the variational bound on the fused kernels (kernels_misc.hip: diffusion_loss_kernel,
vb_terms_kernel, loss_finalize_kernel; include/holo_abi.h: holo_diffusion_loss, holo_vb_terms) and what stands on them:
ImplicitronGaussianDiffusion.training_losses / calc_bpd_loop, HoloDiffusionModel.diffusion_training_step.

References: the float64 numpy restatement (tests/support/diffusion_loss_ref.py, checked against the reference's float64 run
when the fixture was written) on the kernel's own float32 inputs, and the reference's recorded results
(tests/golden/diffusion_losses.npz).  Bounds, per sample term: 2e-6 relative for mse, huber, xstart_mse, eps_mse and the KL
rows of vb (a handful of float32 roundings per element at 2^-24 each, sums in double); 1e-5 for the decoder rows (t == 0: a
device tanh within ~2 ulp near 1 is 1.2e-7 on a CDF difference that is >= 0.065 on the fixture's rows, 2e-6 per element
against a mean of ~1.4 nats); grad_out bit for bit against the float32 restatement.  Under HOLO_TEST_EMU=1 the kernel cases run
as they are and the cases that need the denoiser are skipped, as in test_gpu_inpaint.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, runtime  # noqa: E402
from tests import gpu_utils as gu  # noqa: E402
from tests.support import diffusion_loss_ref as ref  # noqa: E402
from tests.test_gpu_cu_counts import _cu, cu  # noqa: E402,F401  (the HOLO_NUM_CUS context fixture of that file)
from tests.test_gpu_inpaint import TINY_UNET  # noqa: E402

D = gu.DEV
CASES = [(si, ri) for si in range(len(ref.SHAPES)) for ri in range(len(ref.T_ROWS))]
TOL, TOL_DECODER = 2e-6, 1e-5
SEED = 0x1234567890ABCDEF
EMU_SKIP = pytest.mark.skipif(gu.EMU, reason="the UNet legs are too slow for the host emulation")
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(D)  # noqa: E731
bits32 = lambda a: np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)  # noqa: E731
bits64 = lambda a: np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint64)  # noqa: E731


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_losses.npz")))


@pytest.fixture(scope="module")
def diff():
    return hda.ImplicitronGaussianDiffusion(num_steps=1000)


_CASE = {}


def case(diff, si, ri):
    """One case's inputs and float64 references, computed once and shared by the tests."""
    if (si, ri) not in _CASE:
        c = ref.case_inputs(diff, si, ri)
        c["rows64"] = ref.schedule_rows(diff, c["t"])
        c["mse"], c["huber"] = ref.loss_terms(c["x_start"], c["model_out"])
        c["vb"] = {clip: ref.vb_terms(c["rows64"], c["x_start"], c["x_t"], c["noise"], c["model_out"], clip)
                   for clip in (True, False)}
        _CASE[(si, ri)] = c
    return _CASE[(si, ri)]


def check(what, got, want, tol):
    err = ref.rel(got, want)
    print(f"{what}: rel {np.array2string(np.atleast_1d(err), precision=3)} (bound {np.array2string(np.atleast_1d(tol), precision=3)})")
    assert (err <= tol).all(), (what, err, tol)
    return err


# ---- 1. holo_diffusion_loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si,ri", CASES)
def test_diffusion_loss_terms_and_grad(diff, si, ri):
    c = case(diff, si, ri)
    x0, mo = dev(c["x_start"]), dev(c["model_out"])
    B = x0.shape[0]
    w = np.array([0.7, 1.3, 0.25][:B])
    scale = dev((2.0 * w / x0[0].numel()).astype(np.float32))
    terms, none = diff._diffusion_loss(x0, mo)
    assert none is None and terms.dtype == torch.float64 and tuple(terms.shape) == (B, 2)
    check("mse", terms[:, 0].cpu().numpy(), c["mse"], TOL)
    check("huber", terms[:, 1].cpu().numpy(), c["huber"], TOL)
    none, grad = diff._diffusion_loss(x0, mo, row_scale=scale, want_terms=False, want_grad=True)
    both_t, both_g = diff._diffusion_loss(x0, mo, row_scale=scale, want_terms=True, want_grad=True)
    assert none is None
    # the three forms agree bit for bit; grad_out is the float32 restatement's bits
    assert np.array_equal(bits64(terms), bits64(both_t)) and np.array_equal(bits32(grad), bits32(both_g))
    assert np.array_equal(bits32(grad), bits32(ref.loss_grad32(c["x_start"], c["model_out"], w)))
    # row_scale NULL: every weight 1
    _, unit = diff._diffusion_loss(x0, mo, want_terms=False, want_grad=True)
    assert np.array_equal(bits32(unit), bits32(ref.loss_grad32(c["x_start"], c["model_out"], np.ones(B))))
    # torch autograd of ((x0 - y)**2).mean(dims) * w on CPU tensors: another rounding order
    y = torch.from_numpy(c["model_out"]).requires_grad_(True)
    ((torch.from_numpy(c["x_start"]) - y) ** 2).flatten(1).mean(1).mul(torch.from_numpy(w).float()).sum().backward()
    g, a = grad.cpu().numpy().astype(np.float64), y.grad.numpy().astype(np.float64)
    assert np.abs(g - a).max() <= 1e-6 * np.abs(a).max()
    # a channels-last permutation of the inputs: the same grad_out after permuting back, the double sums in another order
    perm, back = (0, 2, 3, 4, 1), (0, 4, 1, 2, 3)
    t_cl, g_cl = diff._diffusion_loss(x0.permute(perm).contiguous(), mo.permute(perm).contiguous(), row_scale=scale,
                                      want_terms=True, want_grad=True)
    assert np.array_equal(bits32(g_cl.permute(back).contiguous()), bits32(grad))
    assert ref.rel(t_cl.cpu().numpy(), terms.cpu().numpy()).max() <= 1e-12


# ---- 2. holo_vb_terms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("si,ri", CASES)
def test_vb_terms(diff, golden, si, ri, clip):
    c = case(diff, si, ri)
    x0, xt, nz, mo = (dev(c[k]) for k in ("x_start", "x_t", "noise", "model_out"))
    rows = diff.vb_coefs(c["t"]).to(D)
    got = diff._vb_terms(rows, x0, xt, nz, mo, clip)
    assert got.dtype == torch.float64 and tuple(got.shape) == (x0.shape[0], 3)
    g, want = got.cpu().numpy(), c["vb"][clip]
    t0 = c["t"] == 0
    err_vb = check("vb", g[:, 0], want[:, 0], np.where(t0, TOL_DECODER, TOL))
    check("xstart_mse", g[:, 1], want[:, 1], TOL)
    check("eps_mse", g[:, 2], want[:, 2], TOL)
    # the KL rows are no further from float64 than the reference's own float32 run (the kernel does not evaluate normal_kl's
    # -1 + lv2 - lv1 + exp(lv1 - lv2): its float32 residue is the reference's deviation at large t)
    f64 = golden[f"s{si}.r{ri}.clip{int(clip)}.vb.f64"]
    dev_ref = golden[f"s{si}.r{ri}.clip{int(clip)}.vb.dev"]
    assert (ref.rel(g[:, 0], f64)[~t0] <= dev_ref[~t0] + TOL).all(), (ref.rel(g[:, 0], f64), dev_ref)
    assert (err_vb[~t0] <= dev_ref[~t0] + TOL).all()
    # a null noise: the eps term is skipped, the other two keep their bits
    no_eps = diff._vb_terms(rows, x0, xt, None, mo, clip)
    assert np.array_equal(bits64(no_eps[:, :2]), bits64(got[:, :2])) and (no_eps[:, 2] == 0).all()
    # a row's result does not depend on the batch or the row it runs in
    b = x0.shape[0] - 1
    alone = diff._vb_terms(rows[b:b + 1].contiguous(), x0[b:b + 1], xt[b:b + 1], nz[b:b + 1], mo[b:b + 1], clip)
    assert np.array_equal(bits64(alone[0]), bits64(got[b]))
    if b > 0:
        alone_loss, _ = diff._diffusion_loss(x0[b:b + 1], mo[b:b + 1])
        assert np.array_equal(bits64(alone_loss[0]), bits64(diff._diffusion_loss(x0, mo)[0][b]))


# ---- 3. repeatability ---------------------------------------------------------------------------------------------------------
def _all_terms(diff, c):
    x0, xt, nz, mo = (dev(c[k]) for k in ("x_start", "x_t", "noise", "model_out"))
    rows = diff.vb_coefs(c["t"]).to(D)
    return torch.cat([diff._diffusion_loss(x0, mo)[0], diff._vb_terms(rows, x0, xt, nz, mo, True)], dim=1).cpu()


@pytest.mark.parametrize("si,ri", [(2, 1), (3, 2)])
def test_two_calls_are_bit_identical(diff, si, ri):
    c = case(diff, si, ri)
    first = _all_terms(diff, c)
    assert torch.isfinite(first).all() and np.array_equal(bits64(first), bits64(_all_terms(diff, c)))


@_cu(8)
@pytest.mark.parametrize("si,ri", [(2, 1), (3, 2)])
def test_bits_do_not_depend_on_the_cu_count(cu, diff, si, ri):
    """The number of partials is a function of (batch, elems_per_sample) alone: a context that plans for 8 CUs (HOLO_NUM_CUS)
    gives the default context's bits, with every output and workspace NaN-filled first."""
    c = case(diff, si, ri)
    got = _all_terms(diff, c)
    assert torch.isfinite(got).all()
    with cu.default_context():
        base = _all_terms(diff, c)
    assert np.array_equal(bits64(got), bits64(base))


# ---- 4. training_losses -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si,ri", [(0, 0), (1, 1), (2, 2), (3, 3)])
def test_training_losses_match_the_fixture(diff, golden, si, ri):
    c = case(diff, si, ri)
    key = f"s{si}.r{ri}"
    mo = dev(c["model_out"])
    seen = []

    def model(x, t, **kw):
        seen.append((x, t))
        return mo

    terms = diff.training_losses(model, dev(c["x_start"]), dev(c["t"]), noise=dev(c["noise"]), get_xstart=True,
                                 clip_denoised=True)
    assert set(terms) == {"x_t", "mse", "huber", "loss", "noise", "model_output", "pred_xstart"}
    # x_t is q_sample bit for bit, and what the model saw
    assert np.array_equal(bits32(terms["x_t"]), bits32(c["x_t"]))
    assert np.array_equal(bits32(terms["x_t"]), bits32(diff.q_sample(*(torch.from_numpy(c[k]) for k in ("x_start", "t", "noise")))))
    assert seen[0][0] is terms["x_t"] and torch.equal(seen[0][1].cpu(), torch.from_numpy(c["t"]))
    assert terms["mse"].dtype == torch.float32 and terms["loss"] is terms["mse"] and not terms["huber"].requires_grad
    for name in ("mse", "huber"):
        check(name + " vs the float64 reference", terms[name].cpu().numpy(), golden[f"{key}.{name}.f64"], TOL)
    assert terms["model_output"] is mo and torch.equal(terms["noise"].cpu(), torch.from_numpy(c["noise"]))
    assert torch.equal(terms["pred_xstart"], mo.clamp(-1, 1))
    # x_start_for_error changes the returned noise only (gaussian_diffusion.py:882-883)
    other = diff.training_losses(model, dev(c["x_start"]), dev(c["t"]), noise=dev(c["noise"]), x_start_for_error=mo)
    assert torch.equal(other["mse"], terms["mse"]) and not torch.equal(other["noise"], terms["noise"])
    assert "pred_xstart" not in other


def test_training_losses_with_device_noise(diff):
    c = case(diff, 2, 1)
    d = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=3)
    x0, t = dev(c["x_start"]), dev(c["t"])
    index = d.__dict__.get("training_draw_index", 0)
    terms = d.training_losses(lambda x, ts, **kw: x, x0, t)
    x_t, noise = d._q_sample_rows(x0, d.q_sample_coefs(c["t"]).to(D), timestep_index=index, want_noise=True)
    assert np.array_equal(bits32(terms["noise"]), bits32(noise)) and np.array_equal(bits32(terms["x_t"]), bits32(x_t))
    assert 0.9 < float(noise.std()) < 1.1
    again = d.training_losses(lambda x, ts, **kw: x, x0, t)  # the next call draws another block of the stream
    assert not torch.equal(again["noise"], terms["noise"])


# ---- 5. calc_bpd_loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("si", range(len(ref.SHAPES)))
def test_calc_bpd_loop_on_a_subset(diff, golden, si, clip):
    """timesteps = (999, 500, 1, 0) with the fixture's draws: column k is the recorded _vb_terms_bpd / xstart_mse / mse of the
    case whose sample 0 sits at that timestep."""
    shape = ref.SHAPES[si]
    where = {999: (0, 0), 500: (1, 0), 1: (2, 0), 0: (3, 0)}  # timestep -> (timestep row, sample) of the fixture
    # every case of a shape has its own x_start; run the loop once per timestep on that case's grid
    for ti in ref.SUBSET_TIMESTEPS:
        ri, b = where[ti]
        c = case(diff, si, ri)
        assert c["t"][b] == ti
        stub = lambda x, ts, **kw: dev(c["model_out"][b:b + 1])  # noqa: E731
        res = diff.calc_bpd_loop(stub, dev(c["x_start"][b:b + 1]), clip_denoised=clip, timesteps=(ti,),
                                 noise_sampler=lambda t_, shp, dv: dev(c["noise"][b:b + 1]))
        assert "total_bpd" not in res and set(res) == {"prior_bpd", "vb", "xstart_mse", "mse"}
        key = f"s{si}.r{ri}.clip{int(clip)}"
        for name, fix in (("vb", "vb"), ("xstart_mse", "xstart_mse"), ("mse", "eps_mse")):
            assert tuple(res[name].shape) == (1, 1) and res[name].dtype == torch.float32
            tol = TOL_DECODER if (ti == 0 and name == "vb") else TOL
            check(f"{name} t={ti}", res[name][0, 0].item(), golden[f"{key}.{fix}.f64"][b], tol)
    # several timesteps in one call: the columns follow them, each equal to its own one-timestep call's bits
    c = case(diff, si, 1)
    model = lambda x, ts, **kw: torch.tanh(x) * 0.9  # noqa: E731
    sampler = lambda t_, shp, dv: dev(ref.np_noise(77 + t_, shp))  # noqa: E731
    res = diff.calc_bpd_loop(model, dev(c["x_start"]), clip_denoised=clip, timesteps=ref.SUBSET_TIMESTEPS, noise_sampler=sampler)
    assert tuple(res["vb"].shape) == (shape[0], 4) and torch.isfinite(res["vb"]).all()
    one = diff.calc_bpd_loop(model, dev(c["x_start"]), clip_denoised=clip, timesteps=(500,), noise_sampler=sampler)
    for name in ("vb", "xstart_mse", "mse"):
        assert torch.equal(res[name][:, 1], one[name][:, 0]), name
    check("prior_bpd", res["prior_bpd"].cpu().numpy(), ref.prior_bpd(diff, c["x_start"]), TOL)


def test_calc_bpd_loop_full_at_20_steps(golden):
    """T = 20, every timestep: total_bpd = vb.sum(1) + prior_bpd, and the reference's recorded full loop.  (At T = 20 the
    linear schedule ends on beta = 1: sqrt_recip_alphas_cumprod[19] is infinite and the eps column is NaN there, in the
    reference as here.)

    The eps column of this loop has a bound of its own.  The recorded float64 loop forms x_t in float64; here x_t, the
    coefficient rows and the arithmetic are float32, and eps - noise = (x_start - pred) / sqrt_recipm1 is the small difference
    of two O(1) numbers: at t = 18 its rms is 1.4e-4.  Eight float32 roundings reach eps (three in q_sample, two coefficient
    casts, the product, the difference, the division), each at most 2^-24 of |eps| ~ |x_t| * sqrt_recip / sqrt_recipm1, so
    the absolute error of eps - noise is at most 8 * 2^-24 * |eps| per element, and by Cauchy-Schwarz the relative error of
    its mean square at most 2 * 8 * 2^-24 * rms(eps) / sqrt(mse).  That is 1e-6 where the term is O(1) and 7e-3 at t = 18
    (measured there: 4e-5; the reference's own float32 loop: 3e-5)."""
    d = hda.ImplicitronGaussianDiffusion(num_steps=ref.LOOP_STEPS)
    x0 = ref.make_x_start(ref.LOOP_SEED, ref.LOOP_SHAPE)
    ts = np.arange(ref.LOOP_STEPS)[::-1]
    with np.errstate(invalid="ignore"):
        ratio = d.sqrt_recip_alphas_cumprod[ts] / d.sqrt_recipm1_alphas_cumprod[ts]
    x_rms = np.array([np.sqrt(np.mean(ref.q_sample32(d, x0, [ti] * x0.shape[0], ref.loop_noise(x0.shape, ti)).astype(np.float64) ** 2))
                      for ti in ts])
    eps_conditioning = (16 * 2.0 ** -24 * np.nan_to_num(ratio) * x_rms)[None, :]
    calls = []

    def model(x, ts, **kw):
        calls.append(int(ts[0]))
        return dev(ref.loop_model_output(d, x0, calls[-1]))

    res = d.calc_bpd_loop(model, dev(x0), clip_denoised=True,
                          noise_sampler=lambda ti, shp, dv: dev(ref.loop_noise(shp, ti)))
    assert calls == list(range(ref.LOOP_STEPS))[::-1]
    assert set(res) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"}
    total = res["vb"].double().sum(1) + res["prior_bpd"].double()
    assert ref.rel(res["total_bpd"].cpu().numpy(), total.cpu().numpy()).max() <= 4 * 2.0 ** -24
    t0 = np.arange(ref.LOOP_STEPS)[::-1] == 0
    for name in ("vb", "xstart_mse", "mse"):
        got, want = res[name].cpu().numpy(), golden[f"loop.{name}.f64"]
        assert got.shape == want.shape == (ref.LOOP_SHAPE[0], ref.LOOP_STEPS)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and (np.isnan(want).sum() == 0 or name == "mse")
        ok = ~np.isnan(want)
        tol = np.where(t0[None, :] & (name == "vb"), TOL_DECODER, TOL)
        if name == "mse":
            tol = TOL + eps_conditioning / np.sqrt(np.where(ok, want, 1.0))
        err = ref.rel(got, want)
        print(name, "max rel", err[ok].max())
        assert (err[ok] <= np.broadcast_to(tol, err.shape)[ok]).all(), (name, err)
    check("prior_bpd", res["prior_bpd"].cpu().numpy(), golden["loop.prior_bpd.f64"], TOL)
    check("total_bpd", res["total_bpd"].cpu().numpy(), golden["loop.total_bpd.f64"], TOL)
    check("total_bpd vs float32 reference", res["total_bpd"].cpu().numpy(), golden["loop.total_bpd.f32"], 1e-5)


# ---- 6. the training step on the tiny denoiser ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    m, *_ = gu.make_model(8, 16, 16, 16, TINY_UNET, diffusion_args=dict(num_steps=1000))
    return m


@EMU_SKIP
def test_diffusion_training_step(model):
    B, shape = 2, (2, 16, 8, 8, 8)
    x0 = dev(ref.make_x_start(9001, shape))
    rs = {"timesteps": torch.tensor([700, 3]), "q_noise": torch.from_numpy(ref.np_noise(9002, shape))}
    out = model.diffusion_training_step(x0, rng_streams=rs)
    assert set(out) == {"loss", "terms", "unet"} and set(out["unet"]) == set(model.net_3d._param_names)
    tm = out["terms"]
    # by hand: the same x_t, the re-run forward, the kernel's grad_out
    x_t = model.diffusion.q_sample(x0.cpu(), rs["timesteps"], rs["q_noise"])
    assert np.array_equal(bits32(tm["x_t"]), bits32(x_t))
    y, _, grads = model.net_3d.backward(tm["x_t"], tm["timesteps"], tm["grad_output"])
    assert np.array_equal(bits32(y), bits32(tm["model_output"]))
    w = np.full(B, np.float32(1.0 / B), dtype=np.float64)
    assert np.array_equal(bits32(tm["grad_output"]), bits32(ref.loss_grad32(x0.cpu().numpy(), y.cpu().numpy(), w)))
    mse, _ = ref.loss_terms(x0.cpu().numpy(), y.cpu().numpy())
    check("mse", tm["mse"].cpu().numpy(), mse, TOL)
    check("loss", out["loss"].item(), mse.mean(), TOL)
    for k, g in out["unet"].items():
        assert torch.isfinite(g).all(), k
        scale = float(grads[k].abs().max())
        assert float((g - grads[k]).abs().max()) <= 1e-5 * scale + 1e-12, (k, float((g - grads[k]).abs().max()), scale)
    assert any(float(g.abs().max()) > 0 for g in out["unet"].values())
    # the autograd route: training_losses(...)["loss"].mean().backward() through the denoiser's own node
    net = model.net_3d
    net.requires_grad_(True)  # (the plugin's parameters are created frozen)
    for p in net.parameters():
        p.grad = None
    with torch.enable_grad():
        terms = model.diffusion.training_losses(net, x0, dev(rs["timesteps"].numpy()), noise=dev(rs["q_noise"].numpy()))
        assert terms["loss"].requires_grad and not terms["huber"].requires_grad
        terms["loss"].mean().backward()
    assert np.array_equal(bits32(terms["mse"].detach()), bits32(tm["mse"]))
    named = dict(net._net.named_parameters())
    for k, g in out["unet"].items():
        assert named[k].grad is not None, k
        scale = float(g.abs().max())
        assert float((named[k].grad - g).abs().max()) <= 1e-5 * scale + 1e-12, k
    # one HoloAdam step on the result changes the parameters and leaves the next forward finite
    before = {k: p.detach().clone() for k, p in named.items()}
    try:
        hda.HoloAdam(lr=1e-3).add_unet(net).step(out)
        assert any(not torch.equal(before[k], p.detach()) for k, p in named.items())
        with torch.no_grad():
            assert torch.isfinite(net(tm["x_t"], tm["timesteps"])).all()
        assert torch.isfinite(model.diffusion_training_step(x0, rng_streams=rs)["loss"])
    finally:
        with torch.no_grad():
            for k, p in named.items():
                p.copy_(before[k])
                p.grad = None
        net.requires_grad_(False)
        net.mark_parameters_changed()


@EMU_SKIP
def test_voxel_features_bpd(model):
    x0 = dev(ref.make_x_start(9003, (1, 16, 8, 8, 8)))
    sampler = lambda ti, shp, dv: dev(ref.np_noise(9100 + ti, shp))  # noqa: E731
    res = model.voxel_features_bpd(x0, timesteps=(999, 500, 0), noise_sampler=sampler)
    assert set(res) == {"prior_bpd", "vb", "xstart_mse", "mse"} and tuple(res["vb"].shape) == (1, 3)
    assert all(torch.isfinite(v).all() for v in res.values())
    direct = model.diffusion.calc_bpd_loop(model.net_3d, x0, timesteps=(999, 500, 0), noise_sampler=sampler)
    assert all(torch.equal(res[k], direct[k]) for k in res)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(diff):
    L = runtime.lib()
    x = torch.zeros(2, 4096, device=D)
    ws = torch.zeros(64, dtype=torch.float64, device=D)
    out = torch.zeros(8, dtype=torch.float64, device=D)
    P, ctx, st = runtime.ptr, runtime.ctx(D), runtime.stream_ptr(D)
    need = int(L.holo_diffusion_loss_workspace_bytes(2, 4096))
    assert L.holo_diffusion_loss(ctx, 2, 4094, P(x), P(x), None, P(out), None, P(ws), 512, st) == -1
    assert b"multiple of 4" in L.holo_last_error()
    assert L.holo_diffusion_loss(ctx, 2, 4096, P(x), P(x), None, P(out), None, P(ws), need - 8, st) == -3
    assert b"workspace" in L.holo_last_error()
    assert L.holo_diffusion_loss(ctx, 2, 4096, P(x), P(x), None, None, None, P(ws), need, st) == -1
    assert b"at least one of terms and grad_out" in L.holo_last_error()
    assert L.holo_vb_terms(ctx, P(x), 2, 4094, P(x), P(x), None, P(x), 1, P(out), P(ws), 512, st) == -1
    assert L.holo_vb_terms(ctx, P(x), 2, 4096, P(x), P(x), None, P(x), 1, P(out), P(ws), need - 8, st) == -3
    with pytest.raises(ValueError, match="does not match"):
        diff._diffusion_loss(x, x[:, :64])
    with pytest.raises(ValueError, match="timesteps must be in"):
        diff.calc_bpd_loop(lambda a, b: a, x.view(2, 4, 4, 16, 16), timesteps=(1000,))
    torch.cuda.synchronize()
    assert (out == 0).all()  # nothing ran


def test_training_step_refuses_the_bf16_mode():
    m = hda.HoloDiffusionModel(resol=8, feature_size=16, render_image_width=16, render_image_height=16,
                               net_3d_SimpleUnet3D_args=dict(TINY_UNET, compute_dtype="bf16")).to(D)
    with pytest.raises(_lib.HoloError, match="fp32 mode only"):
        m.diffusion_training_step(torch.zeros(1, 16, 8, 8, 8, device=D))
