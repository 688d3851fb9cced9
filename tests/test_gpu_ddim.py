"""GPU: DDIM through ImplicitronGaussianDiffusion (holo_ddim_step / holo_ddim_step_philox, gaussian_diffusion.py:645-815)
against the float32 restatement (tests/support/ddim_ref.py) and the reference's recorded steps and trajectories
(tests/golden/ddim_sampler.npz, scripts/make_golden_ddim.py)."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.support.ddim_ref import ddim_step  # noqa: E402
from tests.test_gpu_diffusion import _philox_normals  # noqa: E402

STEP_TS = (999, 500, 1, 0)
TINY_UNET = dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2))


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "ddim_sampler.npz"))


def _ddim_cfg(g):
    R, C, mc, _ = (int(v) for v in g["cfg"])
    return uo.UNetCfg(image_size=R, in_channels=C, out_channels=C, model_channels=mc, num_res_blocks=2,
                      channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2)


def test_ddim_step_bit_exact_vs_restatement(gu, g):
    """holo_ddim_step with injected noise: every recorded single step (t in {999, 500, 1, 0}, eta in {0, 0.5, 1}, clip on /
    off), every reverse step and the batch of 2 with different t equal the restatement and the reference bit for bit."""
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    x = T(g["step.x"])
    for ti in STEP_TS:
        mo, nz = T(g[f"step.t{ti}.model_out"]), T(g[f"step.t{ti}.noise"])
        for clip in (1, 0):
            for eta in (0.0, 0.5, 1.0):
                c = diff.ddim_coefs([ti], [ti - 1], eta)
                s, p = diff._ddim_step(x.to(gu.DEV), mo.to(gu.DEV), c.to(gu.DEV), nz.to(gu.DEV), bool(clip))
                rs, rp = ddim_step(x, mo, c, nz, bool(clip))
                assert torch.equal(s.cpu(), rs) and torch.equal(p.cpu(), rp), (ti, clip, eta)
                assert torch.equal(s.cpu(), T(g[f"step.t{ti}.clip{clip}.eta{eta:g}.sample"])), (ti, clip, eta)
        # the public single-step methods on the same inputs (model = the recorded output)
        out = diff.ddim_sample(lambda a, b: mo.to(gu.DEV), x.to(gu.DEV), torch.tensor([ti], device=gu.DEV), eta=0.5,
                               noise_sampler=lambda t, shp, dev: nz.to(dev))
        assert torch.equal(out["sample"].cpu(), T(g[f"step.t{ti}.clip1.eta0.5.sample"])) and set(out) == {"sample", "pred_xstart"}
        rev = diff.ddim_reverse_sample(lambda a, b: mo.to(gu.DEV), x.to(gu.DEV), torch.tensor([ti], device=gu.DEV))
        assert torch.equal(rev["sample"].cpu(), T(g[f"rev.t{ti}.sample"])), ti
    t2 = torch.from_numpy(g["b2.t"])
    mo2, n2 = T(g["b2.model_out"]), T(g["b2.noise"])
    out = diff.ddim_sample(lambda a, b: mo2.to(gu.DEV), T(g["b2.x"]).to(gu.DEV), t2.to(gu.DEV), eta=0.5,
                           noise_sampler=lambda t, shp, dev: n2.to(dev))
    assert torch.equal(out["sample"].cpu(), T(g["b2.sample"])) and torch.equal(out["pred_xstart"].cpu(), T(g["b2.pred_xstart"]))
    # pred_xstart is optional; a null noise pointer is only legal where it is not read
    s, p = diff._ddim_step(x.to(gu.DEV), mo.to(gu.DEV), diff.ddim_coefs([0], [-1], 1.0).to(gu.DEV), None, True, want_pred=False)
    assert p is None and torch.equal(s.cpu(), T(g["step.t0.clip1.eta1.sample"]))


def test_ddim_philox_step(gu):
    """holo_ddim_step_philox: (1) the noise it reports is the documented Philox4x32-10 / Box-Muller draw, the one
    holo_ddpm_step_philox draws at the same (seed, stream, timestep); (2) its sample is holo_ddim_step of that noise bit for
    bit; (3) the NCDHW and the channels-last call draw the same noise; (4) eta = 0 needs no draw and gives the same sample."""
    seed, stream = 0x1234567890ABCDEF, 3
    diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=stream)
    shape = (2, 8, 8, 8, 8)
    per = int(np.prod(shape[1:]))
    x, mo = (torch.from_numpy(np_noise(s, shape)).to(gu.DEV) for s in (1, 2))
    cl = lambda a: a.permute(0, 2, 3, 4, 1).contiguous()  # noqa: E731
    for tt, eta in ((999, 1.0), (500, 0.5), (1, 1.0), (0, 1.0)):
        c = diff.ddim_coefs([tt, tt], [tt - 1, tt - 1], eta).to(gu.DEV)
        s1, p1, e1 = diff._ddim_step_device_noise(x, mo, c, tt, True, want_noise=True)
        want_cl = _philox_normals(seed, (stream << 32) | tt, shape[0], per).reshape(shape[0], *shape[2:], shape[1])
        assert np.abs(e1.cpu().numpy() - want_cl.transpose(0, 4, 1, 2, 3)).max() < 2e-5
        e_ddpm = diff._step_device_noise(x, torch.tensor([tt, tt], device=gu.DEV), mo, tt, True, want_noise=True)[2]
        assert torch.equal(e1, e_ddpm)
        s2, p2 = diff._ddim_step(x, mo, c, e1, True)
        assert torch.equal(s1, s2) and torch.equal(p1, p2)
        s4, p4, e4 = diff._ddim_step_device_noise(cl(x), cl(mo), c, tt, True, want_noise=True, channels_last=True)
        assert torch.equal(e4, cl(e1)) and torch.equal(s4, cl(s1)) and torch.equal(p4, cl(p1))
        s3, p3, e3 = diff._ddim_step_device_noise(x, mo, c, tt, True, want_pred=False)
        assert torch.equal(s3, s1) and p3 is None and e3 is None
    c0 = diff.ddim_coefs([500, 500], [499, 499], 0.0).to(gu.DEV)
    assert torch.equal(diff._ddim_step_device_noise(x, mo, c0, 500, True)[0], diff._ddim_step(x, mo, c0, None, True)[0])


def test_ddim_eta1_full_schedule_is_the_ddpm_step(gu):
    """With the full schedule and eta = 1, DDIM's update is DDPM's posterior step in exact arithmetic: with the same noise
    the two kernels agree to 1e-5 of the dynamic range (only the rounding of the two formulas differs) for t >= 20 and at
    t = 0.  Below t = 20 the reference's float32 order itself is ill-conditioned - sigma's 1 - abar / abar_prev is beta_t ~ 1e-4
    and 1 - abar_prev - sigma^2 cancels likewise, ~4 digits lost in the coefficients - and the gap grows to ~3e-4 at t = 1."""
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    shape = (2, 8, 4, 4, 4)
    x, mo, nz = (torch.from_numpy(np_noise(s, shape)).to(gu.DEV) for s in (11, 12, 13))
    mo = mo * 1.5
    for tt in (999, 700, 500, 100, 50, 20, 10, 2, 1, 0):
        t = torch.tensor([tt, tt], device=gu.DEV)
        s_ddpm, p_ddpm = diff._step(x, t, mo, nz, True)
        s_ddim, p_ddim = diff._ddim_step(x, mo, diff.ddim_coefs([tt, tt], [tt - 1, tt - 1], 1.0).to(gu.DEV), nz, True)
        assert torch.equal(p_ddim, p_ddpm)
        err = ((s_ddim - s_ddpm).abs().max() / s_ddpm.abs().max()).item()
        assert err < (1e-5 if tt >= 20 or tt == 0 else 1e-3), (tt, err)


def _noise_by_t(g, tag, dev):
    """The noise the reference drew at timestep t of the recorded chain: np_noise(noise_seed + step index)."""
    idx = {int(t): k for k, t in enumerate(g[f"{tag}.indices"])}
    seed = int(g[f"{tag}.noise_seed"])
    return lambda t, shp, device=None: torch.from_numpy(np_noise(seed + idx[int(t)], tuple(shp))).to(dev)


def _crop(a):
    """The block of a grid the fixture stores (scripts/make_golden_ddim.py, crop): channel 0, depth slices 0..3."""
    return a[..., :1, :4, :, :]


@pytest.mark.parametrize("tag,T,ddim_steps", [("T25_eta0", 25, None), ("T25_eta1", 25, None), ("T1000_ddim10", 1000, 10)])
def test_ddim_trajectory_vs_reference(gu, g, tag, T, ddim_steps):
    """The tiny UNet's DDIM chains recorded from the reference (full range at T = 25, eta 0 and 1; ddim10 at T = 1000,
    eta 0.5, built as a respaced GaussianDiffusion): every step's sample and pred_xstart within 5e-3 of the dynamic range,
    as test_sampler_trajectory_vs_reference.  The chains run on the whole grid; the fixture keeps one block of each step."""
    cfg = _ddim_cfg(g)
    net, _ = gu.make_unet(cfg, seed=int(g["cfg"][3]))
    diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
    shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
    eta = float(g[f"{tag}.eta"])
    x_T = torch.from_numpy(np_noise(int(g[f"{tag}.x_seed"]), shape)).to(gu.DEV)
    ns = _noise_by_t(g, tag, gu.DEV)
    steps = list(diff.ddim_sample_loop_progressive(net, shape, noise=x_T, eta=eta, ddim_steps=ddim_steps, noise_sampler=ns))
    assert len(steps) == g[f"{tag}.samples"].shape[0]
    for i, s in enumerate(steps):
        assert set(s) == {"sample", "pred_xstart"}
        assert gu.rel_err(_crop(s["sample"]), torch.from_numpy(g[f"{tag}.samples"][i])) < 5e-3, (tag, i)
        assert gu.rel_err(_crop(s["pred_xstart"]), torch.from_numpy(g[f"{tag}.pred_xstart"][i])) < 5e-3, (tag, i)
    final = diff.ddim_sample_loop(net, shape, noise=x_T, eta=eta, ddim_steps=ddim_steps, noise_sampler=ns)
    assert torch.equal(final, steps[-1]["sample"])
    if ddim_steps is not None:  # the same schedule as an explicit list
        again = diff.ddim_sample_loop(net, shape, noise=x_T, eta=eta, timesteps=diff.ddim_schedule(ddim_steps),
                                      noise_sampler=ns)
        assert torch.equal(again, final)


def test_north_star_ddim4_perf_chain_vs_oracle(gu):
    """The DDIM loop's perf chain (device_noise_seed: channels-last, forward_channels_last + holo_ddim_step_philox) on the
    64^3 x 32 net, ddim4 at eta = 0, against the pinned UNet oracle driving the float32 restatement: every step's sample and
    pred_xstart within 5e-3, as test_north_star_sampler_chain_vs_oracle."""
    from oracle.common import NORTH_CFG, TINY_CFG
    cfg = TINY_CFG if gu.EMU else NORTH_CFG
    net, sd = gu.make_unet(cfg)
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=77)
    shape = (1, cfg.in_channels) + (cfg.image_size,) * 3
    x_T = torch.from_numpy(np_noise(4243, shape))
    steps = [{k: v.cpu() for k, v in s.items()}
             for s in diff.ddim_sample_loop_progressive(net, shape, noise=x_T.to(gu.DEV), ddim_steps=4)]
    ts = diff.ddim_schedule(4)
    assert len(steps) == 4 and ts == [750, 500, 250, 0]
    torch.set_num_threads(min(32, torch.get_num_threads()))
    img, worst = x_T, 0.0
    for k, tt in enumerate(ts):
        y = uo.unet_forward(sd, cfg, img, torch.tensor([tt]))
        rs, rp = ddim_step(img, y, diff.ddim_coefs([tt], [ts[k + 1] if k + 1 < 4 else -1], 0.0))
        for got, ref in ((steps[k]["sample"], rs), (steps[k]["pred_xstart"], rp)):
            e = gu.rel_err(got, ref)
            worst = max(worst, e)
            assert e < 5e-3, (k, e)
        img = rs
    print(f"north-star ddim4 perf chain: worst relative error {worst:.2e}")


def test_model_ddim_sampling_and_inversion(gu):
    """HoloDiffusionModel.sample_random_voxel_features(sampler="ddim") and invert_voxel_features through the product:
    shapes, determinism for a fixed seed, the sampled grid in [-1, 1], a finite x_T; the progressive generator clips."""
    model, *_ = gu.make_model(8, 32, 8, 8, TINY_UNET, diffusion_args=dict(num_steps=1000))
    torch.manual_seed(3)
    a = model.sample_random_voxel_features(sampler="ddim", ddim_steps=4)
    torch.manual_seed(3)
    b = model.sample_random_voxel_features(sampler="ddim", ddim_steps=4)
    assert a.shape == (1, 32, 8, 8, 8) and torch.equal(a, b) and a.min() >= -1 and a.max() <= 1
    torch.manual_seed(3)
    c = model.sample_random_voxel_features(sampler="ddim", ddim_steps=4, eta=1.0)
    assert not torch.equal(a, c) and c.min() >= -1 and c.max() <= 1
    x_T = model.invert_voxel_features(a, ddim_steps=4)
    assert x_T.shape == a.shape and torch.isfinite(x_T).all() and torch.equal(x_T, model.invert_voxel_features(a, ddim_steps=4))
    torch.manual_seed(3)
    outs = list(model.sample_random_voxel_features_progressive(sampler="ddim", ddim_steps=3, eta=0.5))
    assert len(outs) == 3 and all(o.min() >= -1 and o.max() <= 1 for o in outs)
    with pytest.raises(ValueError):
        model.sample_random_voxel_features(ddim_steps=4)  # DDIM keys need sampler="ddim"


def test_generate_samples_with_ddim(gu):
    """generate_samples with sampler_kwargs={"sampler": "ddim", ...} end to end on a small model, with torch noise and with
    the in-kernel draw (device_noise): reproducible, finite frames."""
    from holo_diffusion_amd.generate import generate_samples
    model, *_ = gu.make_model(8, 32, 8, 8, TINY_UNET, diffusion_args=dict(num_steps=1000))
    kw = {"sampler": "ddim", "ddim_steps": 3, "eta": 0.5}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for device_noise in (False, True):
            r1 = generate_samples(model, num_samples=2, n_eval_cameras=2, seed=3, device=gu.DEV, sampler_kwargs=kw,
                                  device_noise=device_noise)
            r2 = generate_samples(model, num_samples=2, n_eval_cameras=2, seed=3, device=gu.DEV, sampler_kwargs=kw,
                                  device_noise=device_noise)
            img = r1["images_render"]
            assert img.shape == (2, 2, 3, 8, 8) and torch.isfinite(img).all() and torch.equal(img, r2["images_render"])
    assert model.diffusion.device_noise_seed is None
