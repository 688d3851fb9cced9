"""GPU: guided sampling - the guided step kernels (holo_ddpm_step_guided / holo_ddim_step_guided and their Philox forms)
against the float32 restatements (tests/support/guided_ref.py) and the reference's recorded steps
(tests/golden/guided_sampler.npz, scripts/make_golden_guided.py), ``cond_fn`` through the sampler loops, and
PhotometricGuidance against the training path.  Under HOLO_TEST_EMU=1 (host emulation) the kernel cases run as they are, the
loop cases run on a cheap stand-in for the denoiser (an emulated UNet call takes about a minute), and the two cases that
need the denoiser's backward are skipped, as the training-path tests of test_gpu_render_backward.py are."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import runtime  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.support.guided_ref import ddim_guided_step, ddpm_guided_step  # noqa: E402

STEP_TS = (999, 500, 1, 0)
SHAPES = ((2, 8, 4, 4, 4), (2, 8, 8, 8, 8))
TINY_UNET = dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
bits = lambda a: np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)  # noqa: E731


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "guided_sampler.npz"))


def _inputs(shape, dev):
    """x, model output (scaled so that the clamp acts), gradient, noise of a shape: np_noise draws, computed once."""
    x, mo, gr, nz = (torch.from_numpy(np_noise(s, shape)) for s in (1, 2, 5, 3))
    return x.to(dev), (mo * 1.5).to(dev), (gr * 0.1).to(dev), nz.to(dev)


def _ddpm_scalars(diff, t):
    """(c1, c2, v, sigma) of ddpm_guided_step from the tables the kernel reads; sigma with numpy's float32 exp."""
    t = np.asarray(t)
    tab = np.stack([diff.posterior_mean_coef1, diff.posterior_mean_coef2, diff.posterior_log_variance_clipped], 1).astype(np.float32)
    sigma = (t != 0).astype(np.float32) * np.exp(np.float32(0.5) * tab[t, 2])
    return tab[t, 0], tab[t, 1], diff.posterior_variance[t].astype(np.float32), sigma


def test_ddim_guided_step_bit_exact_vs_restatement_and_reference(gu, g):
    """holo_ddim_step_guided with injected noise: every recorded step (t in {999, 500, 1, 0}, eta in {0, 0.5, 1}, clip on /
    off) and the batch of 2 with different t equal the restatement and, through it, the reference bit for bit; so do the
    restatement and the kernel on the two full shapes.  pred_xstart may be null, and so may the noise where c4 = 0."""
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    D = gu.DEV
    x, gr = T(g["step.x"]), T(g["step.grad"])
    for ti in STEP_TS:
        mo, nz = T(g[f"step.t{ti}.model_out"]), T(g[f"step.t{ti}.noise"])
        for clip in (1, 0):
            for eta in (0.0, 0.5, 1.0):
                c = diff.ddim_guided_coefs([ti], [ti - 1], eta)
                s, p = diff._ddim_step(x.to(D), mo.to(D), c.to(D), nz.to(D), bool(clip), grad=gr.to(D))
                rs, rp = ddim_guided_step(x, mo, gr, c, nz, bool(clip))
                assert torch.equal(s.cpu(), rs) and torch.equal(p.cpu(), rp), (ti, clip, eta)
                assert torch.equal(s.cpu(), T(g[f"ddim.t{ti}.clip{clip}.eta{eta:g}.sample"])), (ti, clip, eta)
                assert torch.equal(p.cpu(), T(g[f"ddim.t{ti}.clip{clip}.pred_xstart"])), (ti, clip)
        # the public single step on the same inputs (model = the recorded output, cond_fn = the recorded gradient)
        out = diff.ddim_sample(lambda a, b: mo.to(D), x.to(D), torch.tensor([ti], device=D), eta=0.5,
                               cond_fn=lambda a, b: gr.to(D), noise_sampler=lambda t, shp, dev: nz.to(dev))
        assert torch.equal(out["sample"].cpu(), T(g[f"ddim.t{ti}.clip1.eta0.5.sample"])) and set(out) == {"sample", "pred_xstart"}
    t2 = T(g["b2.t"])
    mo2, n2, g2 = T(g["b2.model_out"]), T(g["b2.noise"]), T(g["b2.grad"])
    out = diff.ddim_sample(lambda a, b: mo2.to(D), T(g["b2.x"]).to(D), t2.to(D), eta=0.5, cond_fn=lambda a, b: g2.to(D),
                           noise_sampler=lambda t, shp, dev: n2.to(dev))
    assert torch.equal(out["sample"].cpu(), T(g["b2.ddim.sample"]))
    assert torch.equal(out["pred_xstart"].cpu(), T(g["b2.ddim.pred_xstart"]))
    for shape in SHAPES:
        xs, ms, gs, ns = _inputs(shape, D)
        for tt, eta in ((999, 1.0), (500, 0.5), (1, 1.0), (0, 1.0), (500, 0.0)):
            c = diff.ddim_guided_coefs([tt, max(tt - 1, 0)], [tt - 1, max(tt - 1, 0) - 1], eta)
            s, p = diff._ddim_step(xs, ms, c.to(D), ns, True, grad=gs)
            rs, rp = ddim_guided_step(xs.cpu(), ms.cpu(), gs.cpu(), c, ns.cpu(), True)
            assert torch.equal(s.cpu(), rs) and torch.equal(p.cpu(), rp), (shape, tt, eta)
            if eta == 0.0:  # c4 = 0: the noise is not read; pred_xstart is optional
                s0, p0 = diff._ddim_step(xs, ms, c.to(D), None, True, want_pred=False, grad=gs)
                assert p0 is None and torch.equal(s0, s)
    s, p = diff._ddim_step(x.to(D), mo.to(D), diff.ddim_guided_coefs([0], [-1], 1.0).to(D), None, True, want_pred=False,
                           grad=gr.to(D))
    assert p is None and torch.equal(s.cpu(), T(g["ddim.t0.clip1.eta1.sample"]))


def test_ddpm_guided_step_arithmetic_is_pinned(gu, g):
    """What holo_ddpm_step_guided computes, bit for bit: mean = fma(c2, x, c1*pred), mean_g = mean + v*grad (product
    rounded, sum rounded), sample = fma(sigma, noise, mean_g); pred_xstart = the clamp.  With zero noise the sigma term adds
    +0 and the device expf plays no part.  The restatement states the fma through float64 (exact unless an element sits on a
    double-rounding tie: none of the 73728 (shape, timestep, clip, element) cases here does - checked once on the CPU
    with fractions.Fraction).  A separately rounded c2*x changes the result in thousands of them (counted below), so the
    test tells the two orders apart.  With noise: within the fused DDPM update's tolerance of the reference's recorded
    steps (test_step_kernel_bit_exact_vs_oracle: rtol 3e-7, atol 1e-7)."""
    diff = hda.ImplicitronGaussianDiffusion()
    D = gu.DEV
    n_alt = 0
    for shape in SHAPES:
        x, mo, gr, _ = _inputs(shape, D)
        zero = torch.zeros(shape, device=D)
        for pair in ((999, 998), (500, 499), (1, 0), (0, 0)):
            c1, c2, v, sigma = _ddpm_scalars(diff, pair)
            for clip in (True, False):
                s, p = diff._step(x, torch.tensor(pair, device=D), mo, zero, clip, gr)
                ws, wp = ddpm_guided_step(x.cpu(), mo.cpu(), gr.cpu(), zero.cpu(), c1, c2, v, sigma, clip)
                n_pred, n_sample = int((bits(p) != bits(wp)).sum()), int((bits(s) != bits(ws)).sum())
                assert n_pred == 0 and n_sample == 0, (shape, pair, clip, n_pred, n_sample)
                col = lambda a: a.reshape(2, 1, 1, 1, 1)  # noqa: E731
                alt = (col(c2) * x.cpu().numpy() + col(c1) * wp.numpy()) + col(v) * gr.cpu().numpy()
                assert alt.dtype == np.float32
                n_alt += int((bits(alt) != bits(ws)).sum())
    print(f"separately rounded products differ from the fused mean in {n_alt} elements")
    assert n_alt > 1000
    x, gr = T(g["step.x"]), T(g["step.grad"])
    for ti in STEP_TS:
        mo, nz = T(g[f"step.t{ti}.model_out"]), T(g[f"step.t{ti}.noise"])
        for clip in (1, 0):
            out = diff.p_sample(lambda a, b: mo.to(D), x.to(D), torch.tensor([ti], device=D), clip_denoised=bool(clip),
                                cond_fn=lambda a, b: gr.to(D), noise_sampler=lambda t, shp, dev: nz.to(dev))
            torch.testing.assert_close(out["sample"].cpu(), T(g[f"ddpm.t{ti}.clip{clip}.sample"]), rtol=3e-7, atol=1e-7)
            assert torch.equal(out["pred_xstart"].cpu(), T(g[f"ddpm.t{ti}.clip{clip}.pred_xstart"]))
            assert torch.equal(out["noise"].cpu(), nz)
    out = diff.p_sample(lambda a, b: T(g["b2.model_out"]).to(D), T(g["b2.x"]).to(D), T(g["b2.t"]).to(D),
                        cond_fn=lambda a, b: T(g["b2.grad"]).to(D), noise_sampler=lambda t, shp, dev: T(g["b2.noise"]).to(dev))
    torch.testing.assert_close(out["sample"].cpu(), T(g["b2.ddpm.sample"]), rtol=3e-7, atol=1e-7)
    assert torch.equal(out["pred_xstart"].cpu(), T(g["b2.ddpm.pred_xstart"]))


def test_ddpm_guided_step_with_zero_gradient_is_the_ddpm_step(gu):
    """grad = 0: holo_ddpm_step_guided is holo_ddpm_step bit for bit, sample and pred_xstart, noise included."""
    diff = hda.ImplicitronGaussianDiffusion()
    for shape in SHAPES:
        x, mo, _, nz = _inputs(shape, gu.DEV)
        zero = torch.zeros_like(x)
        for tt in STEP_TS:
            t = torch.tensor([tt, max(tt - 1, 0)], device=gu.DEV)
            for clip in (True, False):
                s, p = diff._step(x, t, mo, nz, clip)
                sg, pg = diff._step(x, t, mo, nz, clip, zero)
                assert torch.equal(bits_t(sg), bits_t(s)) and torch.equal(bits_t(pg), bits_t(p)), (shape, tt, clip)


def bits_t(a):
    return a.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", SHAPES)
def test_guided_philox_steps(gu, shape):
    """The Philox forms of both guided steps: (1) the noise they report is the unguided kernels' draw at the same (seed,
    stream, t), bit for bit; (2) the sample is the plain guided entry fed that noise; (3) the NCDHW and the channels-last
    call agree; (4) the per-row form on streams (5, 9) equals two batch-1 offset calls."""
    seed, stream = 0x1234567890ABCDEF, 3
    D = gu.DEV
    diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=stream)
    rows = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=(5, 9))
    ones = [hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=s) for s in (5, 9)]
    x, mo, gr, _ = _inputs(shape, D)
    cl = lambda a: a.permute(0, 2, 3, 4, 1).contiguous()  # noqa: E731
    for tt, eta in ((999, 1.0), (500, 0.5), (1, 1.0), (0, 1.0)):
        t = torch.tensor([tt, tt], device=D)
        c = diff.ddim_guided_coefs([tt, tt], [tt - 1, tt - 1], eta).to(D)
        steps = {
            "ddpm": (lambda d, a, m, gg, tv, cc, **kw: d._step_device_noise(a, tv, m, tt, True, grad=gg, **kw),
                     lambda a, m, gg, e: diff._step(a, t, m, e, True, gg)),
            "ddim": (lambda d, a, m, gg, tv, cc, **kw: d._ddim_step_device_noise(a, m, cc, tt, True, grad=gg, **kw),
                     lambda a, m, gg, e: diff._ddim_step(a, m, c, e, True, grad=gg)),
        }
        e_plain = diff._step_device_noise(x, t, mo, tt, True, want_noise=True)[2]
        for name, (philox, plain) in steps.items():
            s1, p1, e1 = philox(diff, x, mo, gr, t, c, want_noise=True)
            assert torch.equal(e1, e_plain), (name, tt)
            s2, p2 = plain(x, mo, gr, e1)
            assert torch.equal(s1, s2) and torch.equal(p1, p2), (name, tt)
            s3, p3, e3 = philox(diff, cl(x), cl(mo), cl(gr), t, c, want_noise=True, channels_last=True)
            assert torch.equal(e3, cl(e1)) and torch.equal(s3, cl(s1)) and torch.equal(p3, cl(p1)), (name, tt)
            s4, p4, e4 = philox(diff, x, mo, gr, t, c, want_pred=False)
            assert torch.equal(s4, s1) and p4 is None and e4 is None
            sr, pr, er = philox(rows, x, mo, gr, t, c, want_noise=True)
            for b in (0, 1):
                sb, pb, eb = philox(ones[b], x[b:b + 1], mo[b:b + 1], gr[b:b + 1], t[b:b + 1], c[b:b + 1], want_noise=True)
                assert torch.equal(sr[b:b + 1], sb) and torch.equal(pr[b:b + 1], pb) and torch.equal(er[b:b + 1], eb), (name, tt, b)


def test_null_gradient_is_an_argument_error(gu):
    """The C entries refuse a null grad (HOLO_E_INVALID, through the shared argument check)."""
    diff = hda.ImplicitronGaussianDiffusion()
    x, mo, _, nz = _inputs(SHAPES[0], gu.DEV)
    t = torch.tensor([5, 5], device=gu.DEV)
    L = runtime.lib()
    out = torch.empty_like(x)
    rc = L.holo_ddpm_step_guided(runtime.ctx(x.device), *diff._ddpm_guided_head(x, t), 2, x[0].numel(), runtime.ptr(x),
                                 runtime.ptr(mo), None, runtime.ptr(nz), 1, runtime.ptr(out), None, runtime.stream_ptr(x.device))
    assert rc == -1 and b"holo_ddpm_step_guided" in L.holo_last_error()  # (HOLO_E_INVALID)
    c = diff.ddim_guided_coefs([5, 5], [4, 4]).to(gu.DEV)
    rc = L.holo_ddim_step_guided(runtime.ctx(x.device), runtime.ptr(c), 2, x[0].numel(), runtime.ptr(x), runtime.ptr(mo), None,
                                 None, 1, runtime.ptr(out), None, runtime.stream_ptr(x.device))
    assert rc == -1 and b"holo_ddim_step_guided" in L.holo_last_error()


# ---- the loops -------------------------------------------------------------------------------------------------------
class _StandIn:
    """HOLO_TEST_EMU=1 only: a denoiser-shaped callable for the loop plumbing (the loops only need model(x, t))."""

    def __call__(self, x, t, **kw):
        return torch.tanh(x) * (1.0 + 1e-4 * t.float().reshape(-1, 1, 1, 1, 1))


@pytest.fixture(scope="module")
def tiny_net(gu):
    if gu.EMU:
        return _StandIn(), (2, 8, 8, 8, 8)
    cfg = uo.UNetCfg(image_size=8, in_channels=8, out_channels=8, model_channels=32, num_res_blocks=2, channel_mult=(1, 2),
                     attention_resolutions=(1, 2), num_heads=2)
    net, _ = gu.make_unet(cfg)
    return net, (2, 8, 8, 8, 8)


def _noise_by_t(dev):
    return lambda t, shp, device=None: torch.from_numpy(np_noise(8000 + int(t), tuple(shp))).to(dev)


class Recorder:
    """cond_fn = -0.05 * x that writes down what it is called with."""

    def __init__(self):
        self.calls = []

    def __call__(self, x, t, **kw):
        self.calls.append((tuple(x.shape), x.is_contiguous(), t.dtype, tuple(t.shape), t.cpu().tolist(), torch.is_grad_enabled(), kw))
        return -0.05 * x


def test_guided_loops_equal_the_single_steps(gu, tiny_net):
    """ddim_sample_loop (ddim4, eta 0.5) and p_sample_loop (max_iter 4) with a cond_fn equal a chain stepped with the public
    single-step methods, bit for bit; the cond_fn sees the NCDHW x_t of the chain's shape, int64 t of shape (B,), one call per
    step under the loop's no_grad; dpm_sample_loop still refuses a cond_fn."""
    net, shape = tiny_net
    D = gu.DEV
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    ns = _noise_by_t(D)
    x_T = torch.from_numpy(np_noise(4243, shape)).to(D)
    # DDIM
    rec = Recorder()
    final = diff.ddim_sample_loop(net, shape, noise=x_T, device=D, ddim_steps=4, eta=0.5, noise_sampler=ns, cond_fn=rec)
    ts = diff.ddim_schedule(4)
    assert [c[4] for c in rec.calls] == [[t, t] for t in ts]
    assert all(c[:4] == (shape, True, torch.int64, (2,)) and c[5] is False and c[6] == {} for c in rec.calls)
    img = x_T
    for k, tt in enumerate(ts):
        img = diff.ddim_sample(net, img, torch.tensor([tt, tt], device=D), eta=0.5, t_prev=ts[k + 1] if k + 1 < 4 else -1,
                               noise_sampler=ns, cond_fn=lambda a, b: -0.05 * a)["sample"]
    assert torch.equal(final, img)
    # DDPM
    rec = Recorder()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        final = diff.p_sample_loop(net, shape, noise=x_T, device=D, max_iter=4, noise_sampler=ns, cond_fn=rec)
        ts = diff._indices(4)
    assert [c[4] for c in rec.calls] == [[t, t] for t in ts] and len(ts) == 4
    assert all(c[:4] == (shape, True, torch.int64, (2,)) and c[5] is False for c in rec.calls)
    img = x_T
    for tt in ts:
        img = diff.p_sample(net, img, torch.tensor([tt, tt], device=D), noise_sampler=ns, cond_fn=lambda a, b: -0.05 * a)["sample"]
    assert torch.equal(final, img)
    # the in-kernel draw (per-row streams): the loop still equals the single steps, and a guided chain runs NCDHW
    dn = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=77, device_noise_stream=(4, 6))
    rec = Recorder()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        final = dn.p_sample_loop(net, shape, noise=x_T, device=D, max_iter=4, cond_fn=rec)
    assert all(c[0] == shape and c[1] for c in rec.calls) and len(rec.calls) == 4
    img = x_T
    for tt in ts:
        img = dn.p_sample(net, img, torch.tensor([tt, tt], device=D), cond_fn=lambda a, b: -0.05 * a)["sample"]
    assert torch.equal(final, img)
    with pytest.raises(NotImplementedError):
        diff.dpm_sample_loop(net, shape, noise=x_T, device=D, steps=4, cond_fn=lambda a, b: -0.05 * a)


# ---- PhotometricGuidance ---------------------------------------------------------------------------------------------
R, C, HW, N_RAYS, SCALE = 8, 16, 16, 21, 2.5


@pytest.fixture(scope="module")
def scene(gu):
    model, *_ = gu.make_model(R, C, HW, HW, TINY_UNET, diffusion_args=dict(num_steps=1000))
    model.n_train_target_views = 2
    model.raysampler.n_pts_per_ray_training = 16
    model.renderer.n_pts_per_ray_fine_training = 16
    cams3 = hda.get_simple_360_camera_trajectory(2 * math.pi, 3, -0.5, 10, (0.0, -1.0, 0.0), 3.2).to(gu.DEV)
    rgb = torch.from_numpy(np_noise(51, (2, 3, HW, HW))).mul(0.3).add(0.5).clamp(0, 1).to(gu.DEV)
    fg = torch.from_numpy(np_noise(52, (2, 1, HW, HW))).mul(0.3).add(0.6).clamp(0, 1).to(gu.DEV)
    mask = torch.zeros(2, 1, HW, HW)
    mask[:, :, 3:13, 2:14] = 1
    return model, cams3, rgb, fg, mask.to(gu.DEV)


EMU_SKIP = pytest.mark.skipif(os.environ.get("HOLO_TEST_EMU") == "1", reason="the UNet legs are too slow for the host emulation")


@EMU_SKIP
def test_photometric_guidance_is_the_training_path_gradient(gu, scene):
    """PhotometricGuidance(x_t, t = 700) = -scale * d L / d x_t, where the training path (training_step given the same rays
    and renderer streams, timesteps = 700, no bootstrap, the same loss, and the (x_0, q_noise) that x_t = q_sample(x_0, 700,
    q_noise) was made from) returns d L / d x_0 = sqrt(abar_700) * d L / d x_t.  The same chain of kernels in the
    deterministic mode, so the two agree to the rounding of that one multiply and divide: rtol 1e-5.  Not tightened to
    equality: the first run on an MI355X gave max |d| 7.3e-12 of 9.5e-5 (8e-8 relative: the multiply and the divide round), and
    a loss equal to the eight digits printed (held to rtol 1e-6: the two routes sum the same per-ray tensors)."""
    model, cams3, rgb, fg, mask = scene
    D = gu.DEV
    guide = hda.PhotometricGuidance(model, cams3[[0, 1]], rgb, fg_probability=fg, mask_crop=mask, scale=SCALE,
                                    n_rays_per_view=N_RAYS, seed=11)
    x0 = torch.tanh(torch.from_numpy(np_noise(5, (1, C, R, R, R)))).to(D)
    q_noise = torch.from_numpy(np_noise(41, tuple(x0.shape))).to(D)
    t = torch.tensor([700], device=D)
    x_t = model.diffusion.q_sample(x0, t, noise=q_noise)
    with runtime.deterministic(True):
        got = guide(x_t, t)
        rs = dict(guide.last_rng_streams, timesteps=t, q_noise=q_noise, bootstrap=False)
        assert rs["xys"].shape == (2, N_RAYS, 2) and guide.last_loss.dim() == 0 and guide.last_loss.device.type == D.type
        out = model.training_step(camera=cams3, voxel_features=x0, rng_streams=rs,
                                  loss_fn=lambda p: guide.photometric_loss(p, rs["xys"]))
    assert got.shape == x_t.shape and torch.isfinite(got).all() and got.abs().max() > 0
    sqrt_ab = model.diffusion._extract(model.diffusion.sqrt_alphas_cumprod, t, x0.shape)
    want = -SCALE * out["voxel_features"] / sqrt_ab
    print(f"guidance vs training path: max |d| {(got - want).abs().max().item():.3e} of {want.abs().max().item():.3e}; "
          f"loss {float(guide.last_loss):.8f} vs {float(out['loss']):.8f}")
    torch.testing.assert_close(got, want, rtol=1e-5, atol=0)
    torch.testing.assert_close(guide.last_loss, out["loss"], rtol=1e-6, atol=0)
    # a second call draws new rays from the same generator; a fresh guidance with the same seed repeats the first
    guide(x_t, t)
    assert not torch.equal(guide.last_rng_streams["xys"], rs["xys"])
    again = hda.PhotometricGuidance(model, cams3[[0, 1]], rgb, fg_probability=fg, mask_crop=mask, scale=SCALE,
                                    n_rays_per_view=N_RAYS, seed=11)
    with runtime.deterministic(True):
        assert torch.equal(again(x_t, t), got) and torch.equal(again.last_rng_streams["xys"], rs["xys"])


def test_photometric_guidance_refuses_what_it_cannot_do(gu, scene):
    model, cams3, rgb, fg, mask = scene
    guide = hda.PhotometricGuidance(model, cams3[[0, 1]], rgb, n_rays_per_view=N_RAYS)
    x2 = torch.zeros(2, C, R, R, R, device=gu.DEV)
    with pytest.raises(ValueError, match="batch"):
        guide(x2, torch.tensor([5, 5], device=gu.DEV))
    prev = model.net_3d.compute_dtype
    model.net_3d.compute_dtype = "bf16"
    try:
        with pytest.raises(ValueError, match="fp32"):
            guide(x2[:1], torch.tensor([5], device=gu.DEV))
    finally:
        model.net_3d.compute_dtype = prev
    with pytest.raises(ValueError):
        hda.PhotometricGuidance(model, cams3[[0, 1]], rgb[:, :, :8])


@EMU_SKIP
def test_guided_sampling_through_the_model(gu, scene):
    """The product entry: sample_random_voxel_features(sampler="ddim", ddim_steps=3, cond_fn=PhotometricGuidance(...)) - a
    finite grid that differs from the unguided chain of the same x_T."""
    model, cams3, rgb, fg, mask = scene
    guide = hda.PhotometricGuidance(model, cams3[[0, 1]], rgb, mask_crop=mask, scale=50.0, n_rays_per_view=N_RAYS, seed=3)
    x_T = torch.from_numpy(np_noise(77, (1, C, R, R, R))).to(gu.DEV)
    a = model.sample_random_voxel_features(sampler="ddim", ddim_steps=3, cond_fn=guide, noise=x_T)
    b = model.sample_random_voxel_features(sampler="ddim", ddim_steps=3, noise=x_T)
    assert a.shape == (1, C, R, R, R) and torch.isfinite(a).all() and not torch.equal(a, b)
    assert guide.last_loss is not None and torch.isfinite(guide.last_loss)
