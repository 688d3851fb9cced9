"""GPU parity: DDPM ancestral sampler through ImplicitronGaussianDiffusion (HIP UNet + fused step kernel)
vs trajectories recorded from the reference's GaussianDiffusion.p_sample_loop_progressive."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from oracle import diffusion_oracle as do  # noqa: E402
from oracle.common import TINY_CFG, np_noise  # noqa: E402


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _ns(dev):
    return lambda t, shp, device=None: torch.from_numpy(np_noise(900 * 100003 + t, tuple(shp))).to(dev)


@pytest.mark.parametrize("tag,T,max_iter", [("T1000_iter4", 1000, 4), ("T20_full", 20, None)])
def test_sampler_trajectory_vs_reference(gu, golden_dir, tag, T, max_iter):
    g = np.load(os.path.join(golden_dir, "tiny_sampler.npz"))
    net, _ = gu.make_unet(TINY_CFG)
    with np.errstate(divide="ignore"):
        diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
    shape = (1, TINY_CFG.in_channels) + (TINY_CFG.image_size,) * 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        steps = list(diff.p_sample_loop_progressive(net, shape, clip_denoised=True, noise_sampler=_ns(gu.DEV),
                                                    max_iter=max_iter))
    assert len(steps) == g[f"{tag}.samples"].shape[0]
    for i, s in enumerate(steps):
        assert set(s) == {"sample", "pred_xstart", "noise"}
        # errors compound along the chain; per-step tolerance 5e-3 of the dynamic range
        assert gu.rel_err(s["sample"], torch.from_numpy(g[f"{tag}.samples"][i])) < 5e-3, (tag, i)
        assert gu.rel_err(s["pred_xstart"], torch.from_numpy(g[f"{tag}.pred_xstart"][i])) < 5e-3, (tag, i)
    final = diff.p_sample_loop(net, shape, noise_sampler=_ns(gu.DEV), max_iter=max_iter)
    assert torch.equal(final, steps[-1]["sample"])
    assert final.min() >= -1 and final.max() <= 1  # t=0 step returns the clipped x0


def test_step_kernel_bit_exact_vs_oracle(gu):
    """The fused elementwise tail is a fixed sequence of fp32 mul/add: bit-exact vs the oracle
    (up to the device exp in sigma, hence 1-ulp tolerance on the noisy steps)."""
    diff = hda.ImplicitronGaussianDiffusion()
    orc = do.DiffusionOracle(1000)
    shape = (2, 8, 4, 4, 4)
    x, mo, nz = (torch.from_numpy(np_noise(s, shape)) for s in (1, 2, 3))
    mo = mo * 1.5
    for tt in (999, 500, 1, 0):
        t = torch.tensor([tt, max(tt - 1, 0)])
        ref = orc.p_sample(lambda a, b: mo, x, t, nz, True)
        out = diff.p_sample(lambda a, b: mo.to(gu.DEV), x.to(gu.DEV), t.to(gu.DEV),
                            noise_sampler=lambda ti, shp, dev: nz.to(dev))
        torch.testing.assert_close(out["sample"].cpu(), ref["sample"], rtol=3e-7, atol=1e-7)
        assert torch.equal(out["pred_xstart"].cpu(), ref["pred_xstart"])
    pmv = diff.p_mean_variance(lambda a, b: mo.to(gu.DEV), x.to(gu.DEV), torch.tensor([7, 7], device=gu.DEV))
    refm = orc.p_mean_variance(lambda a, b: mo, x, torch.tensor([7, 7]))
    for k in ("mean", "variance", "log_variance", "pred_xstart"):
        torch.testing.assert_close(pmv[k].cpu(), refm[k], rtol=1e-6, atol=1e-7)


def test_ddpm_step_arithmetic_is_pinned(gu):
    """What holo_ddpm_step computes, bit for bit: pred_xstart is the clamp (or the model output), and
    sample = fma(sigma, noise, fma(c2, x, c1 * pred)) - the product c1 * pred rounded, the other two fused into the sums
    (the reference rounds all three; DESIGN.md, "Sampling").  With zero noise the sigma term adds +0, so the device expf
    plays no part.  The inner fma is stated through float64: c2 * x is exact there, and one float64 sum rounded to float32
    equals the exactly rounded fma unless an element sits on a double-rounding tie.  No element of this fixture does:
    checked once on the CPU with fractions.Fraction, all 8192 (timestep, clip, element) cases; the separately rounded
    products differ from it in 1346 of them, so the test tells the two apart."""
    diff = hda.ImplicitronGaussianDiffusion()
    shape = (2, 8, 4, 4, 4)
    x, mo = (torch.from_numpy(np_noise(s, shape)) for s in (1, 2))
    mo = mo * 1.5  # (so that the clamp acts)
    tab = diff._tables_on(gu.DEV).cpu().numpy()
    assert tab.dtype == np.float32
    zero = torch.zeros(shape, device=gu.DEV)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    for pair in ((999, 998), (500, 499), (1, 0), (0, 0)):
        c1, c2 = (tab[list(pair), k].reshape(2, 1, 1, 1, 1) for k in (0, 1))
        for clip in (True, False):
            s, p = diff._step(x.to(gu.DEV), torch.tensor(pair, device=gu.DEV), mo.to(gu.DEV), zero, clip)
            m = np.clip(mo.numpy(), -1, 1) if clip else mo.numpy()
            want = (c2.astype(np.float64) * x.numpy().astype(np.float64) + (c1 * m).astype(np.float64)).astype(np.float32)
            want = want + np.float32(0)
            assert m.dtype == np.float32 and want.dtype == np.float32
            n_pred = int((bits(p.cpu().numpy()) != bits(m)).sum())
            n_sample = int((bits(s.cpu().numpy()) != bits(want)).sum())
            print(f"t={pair} clip={clip}: pred_xstart differs in {n_pred}, sample in {n_sample} of {want.size} elements")
            assert n_pred == 0 and n_sample == 0, (pair, clip, n_pred, n_sample)


def test_default_noise_path_runs_and_is_seeded(gu):
    net, _ = gu.make_unet(TINY_CFG)
    diff = hda.ImplicitronGaussianDiffusion()
    shape = (1, TINY_CFG.in_channels) + (TINY_CFG.image_size,) * 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(5)
        a = diff.p_sample_loop(net, shape, max_iter=3)
        torch.manual_seed(5)
        b = diff.p_sample_loop(net, shape, max_iter=3)
    assert torch.equal(a, b) and torch.isfinite(a).all()


def _philox4x32_10(ctr, key):
    """numpy statement of Philox4x32-10 (Salmon et al. 2011; the published constants): ctr (n,4) uint32, key (2,) -> (n,4)."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M0, M1, W0, W1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=1).astype(np.uint32)


def _philox_normals(seed, offset, batch, per):
    """The draw of holo_ddpm_step_philox (include/holo_abi.h): float64 Box-Muller of the same 24-bit uniforms."""
    out = np.empty((batch, per), dtype=np.float64)
    q = np.arange(per // 4, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF)
    for b in range(batch):
        ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, b), np.full_like(q, offset & 0xFFFFFFFF)], axis=1)
        r = _philox4x32_10(ctr.astype(np.uint32), key)
        u = ((r >> 8).astype(np.float64) + 0.5) / 16777216.0
        for j in (0, 2):
            rad, ang = np.sqrt(-2.0 * np.log(u[:, j])), 2.0 * np.pi * u[:, j + 1]
            out[b, j::4], out[b, j + 1::4] = rad * np.cos(ang), rad * np.sin(ang)
    return out


def test_philox_known_answer():
    """The numpy statement above against the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors)."""
    z = _philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = _philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    p = _philox4x32_10(np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], np.uint32), (0xa4093822, 0x299f31d0))[0]
    assert [int(v) for v in p] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_device_noise_step_kernel(gu):
    """holo_ddpm_step_philox (perf mode): (1) the noise it reports is the documented Philox4x32-10 / Box-Muller draw
    (numpy statement, pinned to the published known-answer vectors above) to float32 rounding of log / sin / cos; (2) the
    sample is holo_ddpm_step of that noise BIT for bit; (3) draws depend on (seed, stream, timestep, sample, LOGICAL element)
    and nothing else - in particular not on the layout: the (N, C, R, R, R) call and the channels-last call (the sampler's
    perf chain) draw the same value for the same (n, c, z, y, x), quads numbered in channels-last order; (4) mean / variance
    / lag-1 correlation / 4th moment of 2 M draws are those of a standard normal."""
    from holo_diffusion_amd import _lib, runtime
    L = runtime.lib()
    seed, stream = 0x1234567890ABCDEF, 3
    diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=stream)
    plain = hda.ImplicitronGaussianDiffusion()
    shape = (2, 8, 8, 8, 8)
    per = int(np.prod(shape[1:]))
    x, mo = (torch.from_numpy(np_noise(s, shape)).to(gu.DEV) for s in (1, 2))
    for tt in (999, 1, 0):
        t = torch.tensor([tt, tt], device=gu.DEV)
        s1, p1, e1 = diff._step_device_noise(x, t, mo, tt, True, want_noise=True)
        # (N, C, R, R, R) tensors: the documented draw lives in channels-last order
        want_cl = _philox_normals(seed, (stream << 32) | tt, shape[0], per).reshape(shape[0], *shape[2:], shape[1])
        assert np.abs(e1.cpu().numpy() - want_cl.transpose(0, 4, 1, 2, 3)).max() < 2e-5
        s2, p2 = plain._step(x, t, mo, e1, True)
        assert torch.equal(s1, s2) and torch.equal(p1, p2)
        # the channels-last call on the same logical tensors: the same noise, sample and pred_xstart, bit for bit
        cl = lambda a: a.permute(0, 2, 3, 4, 1).contiguous()  # noqa: E731
        s4, p4, e4 = diff._step_device_noise(cl(x), t, cl(mo), tt, True, want_noise=True, channels_last=True)
        assert torch.equal(e4, cl(e1)) and torch.equal(s4, cl(s1)) and torch.equal(p4, cl(p1))
        s3, p3, e3 = diff._step_device_noise(x, t, mo, tt, True, want_pred=False, want_noise=False)
        assert torch.equal(s3, s1) and p3 is None and e3 is None
    # independence of the draws: another timestep / stream / seed / sample gives another tensor
    t = torch.tensor([5, 5], device=gu.DEV)
    base = diff._step_device_noise(x, t, mo, 5, True, want_noise=True)[2]
    assert not torch.equal(base[0], base[1])
    assert not torch.equal(base, diff._step_device_noise(x, t, mo, 6, True, want_noise=True)[2])
    other = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=stream + 1)
    assert not torch.equal(base, other._step_device_noise(x, t, mo, 5, True, want_noise=True)[2])
    other = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed + 1, device_noise_stream=stream)
    assert not torch.equal(base, other._step_device_noise(x, t, mo, 5, True, want_noise=True)[2])
    # statistics
    n = (1, 16, 16, 16, 16) if gu.EMU else (1, 32, 64, 32, 32)
    big = torch.zeros(n, device=gu.DEV)
    e = diff._step_device_noise(big, torch.tensor([7], device=gu.DEV), big, 7, True, want_noise=True)[2].double().reshape(-1).cpu()
    N = e.numel()
    tol = 5.0 / N ** 0.5  # five standard errors
    assert abs(float(e.mean())) < tol and abs(float(e.var()) - 1.0) < 1.5 * tol
    assert abs(float((e[1:] * e[:-1]).mean())) < tol and abs(float((e[4:] * e[:-4]).mean())) < tol
    assert abs(float((e ** 4).mean()) - 3.0) < 10 * tol and float(e.abs().max()) < 5.95
    assert abs(float((e > 0).double().mean()) - 0.5) < tol


def test_device_noise_chain_is_reproducible(gu):
    """p_sample_loop in the perf mode: same seed -> the same grid bit for bit (no generator state anywhere), another stream
    -> another grid; torch's global generator plays no part in the per-step noise."""
    net, _ = gu.make_unet(TINY_CFG)
    shape = (1, TINY_CFG.in_channels) + (TINY_CFG.image_size,) * 3
    x_T = torch.from_numpy(np_noise(41, shape)).to(gu.DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d1 = hda.ImplicitronGaussianDiffusion(device_noise_seed=11)
        torch.manual_seed(1)
        a = list(d1.p_sample_loop_progressive(net, shape, noise=x_T, max_iter=4))
        torch.manual_seed(2)
        b = d1.p_sample_loop(net, shape, noise=x_T, max_iter=4)
        c = hda.ImplicitronGaussianDiffusion(device_noise_seed=11, device_noise_stream=1).p_sample_loop(net, shape, noise=x_T, max_iter=4)
    assert all(s["noise"] is None and set(s) == {"sample", "pred_xstart", "noise"} for s in a)
    assert torch.equal(a[-1]["sample"], b) and torch.isfinite(b).all() and not torch.equal(b, c)
    out = d1.p_sample(net, x_T, torch.tensor([500], device=gu.DEV))
    assert out["noise"] is None and torch.isfinite(out["sample"]).all()


@pytest.mark.parametrize("compute", ["f32", "f32_bf16x3"])
@pytest.mark.parametrize("T,max_iter", [(1000, 4), (20, None)])
def test_sampler_trajectory_wide_net_both_modes_vs_oracle(gu, compute, T, max_iter):
    """The recorded reference trajectories use the 32-channel tiny net, whose convolutions never reach the LDS-halo
    kernels the opt-in f32_bf16x3 mode replaces.  Here a 64-channel net (halo kernel, fused skip, split-K) is sampled
    in BOTH arithmetic modes against the pinned oracle's chain with the same injected noise: every step's sample and
    pred_xstart at the same 5e-3 tolerance as test_sampler_trajectory_vs_reference."""
    from oracle import unet_oracle as uo
    cfg = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2)
    net, sd = gu.make_unet(cfg, seed=99, compute_dtype=compute)
    with np.errstate(divide="ignore"):
        diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
    shape = (1, 16, 8, 8, 8)
    cpu_ns = lambda t, shp, device=None: torch.from_numpy(np_noise(900 * 100003 + t, tuple(shp)))  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        steps = list(diff.p_sample_loop_progressive(net, shape, clip_denoised=True, noise_sampler=_ns(gu.DEV),
                                                    max_iter=max_iter))
        ref = list(do.DiffusionOracle(T).p_sample_loop_progressive(lambda x, t: uo.unet_forward(sd, cfg, x, t), shape,
                                                                   cpu_ns, True, max_iter))
    assert len(steps) == len(ref) == (max_iter or T)
    for i, (s, r) in enumerate(zip(steps, ref)):
        assert gu.rel_err(s["sample"], r["sample"]) < 5e-3, (compute, i)
        assert gu.rel_err(s["pred_xstart"], r["pred_xstart"]) < 5e-3, (compute, i)


def _psnr(a, b):
    import math
    mse = ((a.double() - b.double()) ** 2).mean().item()
    return 10.0 * math.log10(1.0 / max(mse, 1e-20))


def _render_frame(gu, grid, resol, C, H=64, W=64):
    """One fp32 frame of tanh-range grid `grid` (device tensor) through the HIP renderer."""
    import math
    from oracle import render_oracle as ro
    fn = hda.HoloVoxelGridImplicitFunction(resol=resol, n_hidden=C, feature_dim=0)
    fn.render_mlp.load_state_dict(gu.synth_state_dict(ro.render_mlp_param_shapes(ro.RenderCfg(resol=resol, feature_size=C)), 4321))
    fn.to(gu.DEV)
    wrap = hda.render.ImplicitFunctionWrapper(fn)
    renderer = hda.HoloMultiPassEmissionAbsorptionRenderer(
        raymarcher_EmissionAbsorptionRaymarcher_args=dict(bg_color=(1.0, 1.0, 1.0)))
    cams = hda.get_simple_360_camera_trajectory(2 * math.pi, 4, -30.0 * (2 * math.pi / 360), 10, (0.0, -1.0, 0.0), 3.2)
    sampler = hda.render.AdaptiveRaySampler(image_width=W, image_height=H, scene_extent=4.0)
    wrap.bind_args(voxel_grid_features=grid)
    out = renderer(ray_bundle=sampler(cams[[1]], hda.render.EvaluationMode.EVALUATION), implicit_functions=[wrap, wrap])
    return out.features.clone()


class _Tap:
    """Wraps a denoiser and keeps its raw outputs (the sampler only returns the clamped pred_xstart)."""

    def __init__(self, fn):
        self.fn, self.outs, self.xs = fn, [], []

    def __call__(self, x, t, **kw):
        y = self.fn(x, t, **kw)
        self.xs.append(x.detach().cpu())
        self.outs.append(y.detach().cpu())
        return y

    def parameters(self):
        return self.fn.parameters()


def _chain_errors(out_bf, out_ref, s, r):
    """Per-step drift of a bf16 chain against the fp32 chain: the denoiser's raw output in the max norm relative to its
    dynamic range (the SAME measure as every single-forward bf16 test, tolerance 2e-2), pred_xstart (the
    raw output clamped to [-1, 1]) as relative RMS and max, and the next sample."""
    ob, orf = out_bf.float().cpu(), out_ref.float().cpu()
    e_raw = ((ob - orf).abs().max() / orf.abs().max()).item()
    px_b, px_r = s["pred_xstart"].float().cpu(), r["pred_xstart"].float().cpu()
    e_rms = ((px_b - px_r).pow(2).mean().sqrt() / px_r.pow(2).mean().sqrt()).item()
    e_max = (px_b - px_r).abs().max().item()
    sb, sr = s["sample"].float().cpu(), r["sample"].float().cpu()
    e_s = ((sb - sr).abs().max() / sr.abs().max()).item()
    return e_raw, e_rms, e_max, e_s, orf.abs().max().item()


@pytest.mark.parametrize("T,max_iter", [(20, None), (1000, 4)])
def test_bf16_mode_sampler_chain_vs_fp32_oracle_chain(gu, T, max_iter):
    """BASELINE configs[4] is a DDPM CHAIN in the bf16 storage mode: the rounding of every stored activation feeds back
    through x_{t-1}.  A 64-channel net (bf16 halo / row-tile kernels, attention) is sampled in the bf16 mode against the
    PINNED fp32 oracle's chain with the same injected noise.

    (1) PER STEP (the bf16 net is fed the ORACLE chain's x_t, so nothing compounds): the denoiser output within rtol 2e-2
        of its dynamic range in the max norm - the measure of every single-forward bf16 test, SURVEY.md 8c - and
        pred_xstart within 2e-2 relative RMS, on EVERY step of the chain.  (pred_xstart clamps the output to [-1, 1]; its
        max-norm error relative to 1 is the raw error times the raw range, ~3 for a random-weight net.)
    (2) FREE RUNNING, a contractive denoiser (the synthetic net with its output convolution scaled by 1/4, so that - like
        a trained denoiser near the data - it damps perturbations of x_t instead of amplifying them): nothing compounds
        beyond the per-step error - every step's output / pred_xstart / sample within 3e-2 (the last, noise-free steps
        hand the per-step 1.3e-2 straight to the sample) - and the rendered 64x64 frame of the final 8^3 grids agrees to
        PSNR >= 35 dB (a ray of this tiny grid crosses a handful of voxels; the 40 dB of SURVEY.md 8c is asserted at the
        configuration it is stated for, 128^3, in test_128_cubed_forward_vs_oracle and test_bf16_mode_chain_at_donut_size).
    (3) FREE RUNNING, the unit-scale random net: REPORTED only.  Such a net amplifies ANY perturbation of x_t ~2.5x per
        low-noise step (the fp32 HIP chain's own 1e-6 deviation from the oracle grows the same way, see
        test_sampler_trajectory_wide_net_both_modes_vs_oracle's 5e-3 budget), so the bf16-sized per-step error reaches
        ~1e-1 over the last four steps of a 20-step chain; that is the conditioning of the random net, not of the mode.
    The drift curves are printed (pytest -s) and recorded in DESIGN.md."""
    from oracle import unet_oracle as uo
    cfg = uo.UNetCfg(image_size=8, in_channels=16, out_channels=16, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2)
    shape = (1, 16, 8, 8, 8)
    cpu_ns = lambda t, shp, device=None: torch.from_numpy(np_noise(900 * 100003 + t, tuple(shp)))  # noqa: E731
    fmt = lambda dr: " ".join(f"{i}:{d[0]:.1e}/{d[1]:.1e}/{d[2]:.1e}/{d[3]:.1e};{d[4]:.1f}" for i, d in enumerate(dr))  # noqa: E731
    for out_scale in (1.0, 0.25):
        net, sd = gu.make_unet(cfg, seed=99, compute_dtype="bf16")
        if out_scale != 1.0:
            sd = dict(sd)
            sd["out.2.weight"] = sd["out.2.weight"] * out_scale
            net.load_state_dict({"_net." + k: v for k, v in sd.items()})
            net.to(gu.DEV)
        with np.errstate(divide="ignore"):
            diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
        tap_b, tap_r = _Tap(net), _Tap(lambda x, t: uo.unet_forward(sd, cfg, x, t))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            steps = list(diff.p_sample_loop_progressive(tap_b, shape, clip_denoised=True, noise_sampler=_ns(gu.DEV),
                                                        max_iter=max_iter))
            ref = list(do.DiffusionOracle(T).p_sample_loop_progressive(tap_r, shape, cpu_ns, True, max_iter))
        assert len(steps) == len(ref) == len(tap_b.outs) == len(tap_r.outs) == (max_iter or T)
        drift = [_chain_errors(tap_b.outs[i], tap_r.outs[i], s, r) for i, (s, r) in enumerate(zip(steps, ref))]
        print(f"bf16 FREE chain T={T} max_iter={max_iter} out_scale={out_scale} (step: raw-out max / pred_xstart rms / "
              f"pred_xstart max / sample; raw range):", fmt(drift))
        # (1) per step, teacher forced: x_t of the oracle chain (x_T, then the oracle's samples), the chain's own timesteps
        ts = diff._indices(max_iter)
        x_in = [None] * len(ts)
        x_in[0] = tap_r.xs[0]
        for i in range(1, len(ts)):
            x_in[i] = ref[i - 1]["sample"]
        forced = []
        with torch.no_grad():
            for i, ti in enumerate(ts):
                yb = net(x_in[i].to(gu.DEV), torch.tensor([ti], device=gu.DEV)).cpu()
                yr = tap_r.outs[i]
                e_raw = ((yb - yr).abs().max() / yr.abs().max()).item()
                pb, pr = yb.clamp(-1, 1), yr.clamp(-1, 1)
                e_rms = ((pb - pr).pow(2).mean().sqrt() / pr.pow(2).mean().sqrt()).item()
                forced.append((e_raw, e_rms))
                assert e_raw < 2e-2 and e_rms < 2e-2, ("bf16 per-step (teacher forced)", T, out_scale, i, e_raw, e_rms)
        print(f"bf16 PER-STEP T={T} out_scale={out_scale} (raw-out max / pred_xstart rms):",
              " ".join(f"{i}:{a:.1e}/{b:.1e}" for i, (a, b) in enumerate(forced)))
        assert max(f[0] for f in forced) > 1e-5  # bf16-sized, not an accidental fp32 run
        if out_scale != 1.0:  # (2) the contractive denoiser: the free-running chain stays inside the tolerance
            for i, d in enumerate(drift):
                assert d[0] < 3e-2 and d[1] < 3e-2 and d[3] < 3e-2, ("bf16 free chain, contractive net", T, i, d)
            f_bf = _render_frame(gu, steps[-1]["sample"].clamp(-1, 1), 8, 16)
            f_32 = _render_frame(gu, ref[-1]["sample"].clamp(-1, 1).to(gu.DEV), 8, 16)
            print(f"bf16 free chain T={T} out_scale={out_scale}: rendered-frame PSNR {_psnr(f_bf, f_32):.1f} dB")
            assert _psnr(f_bf, f_32) >= (35.0 if T == 1000 else 30.0), _psnr(f_bf, f_32)  # the 20-step schedule ends on four almost noise-free steps


def test_bf16_mode_chain_at_donut_size(gu):
    """BASELINE configs[4] at its own size: 8 consecutive DDPM steps (t = 999..992, injected noise) at 128^3 x 32 in the
    bf16 storage mode against the exact-fp32 chain of the same library, step by step, with the measures of the test above
    (denoiser output max norm / pred_xstart RMS / sample, each 2e-2); rendered frame of the two final pred_xstart grids at
    PSNR >= 40 dB.  The fp32 chain is tied to the PINNED oracle on its last step (one 128^3 forward on the host cores: the
    oracle evaluated on the fp32 chain's x_t reproduces that step's pred_xstart at the full-forward tolerance 2e-3), so
    bf16-vs-oracle follows by the triangle inequality without eight minute-long CPU forwards."""
    from oracle import unet_oracle as uo
    if os.environ.get("HOLO_TEST_EMU") == "1":
        pytest.skip("128^3 is not an emulation size")
    cfg = uo.UNetCfg(image_size=128, in_channels=32, out_channels=32, model_channels=64, num_res_blocks=2,
                     channel_mult=(1, 1, 2, 4, 8), attention_resolutions=(4, 8), num_heads=2)
    n32, sd = gu.make_unet(cfg, seed=1234)
    nbf, _ = gu.make_unet(cfg, seed=1234, compute_dtype="bf16")
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    shape = (1, 32, 128, 128, 128)
    n_steps = 8
    x32 = xbf = torch.from_numpy(np_noise(41, shape)).to(gu.DEV)
    drift = []
    last_in = None
    tap32, tapbf = _Tap(n32), _Tap(nbf)
    with torch.no_grad():
        for k in range(n_steps):
            t = torch.tensor([999 - k], device=gu.DEV)
            eps = torch.from_numpy(np_noise(5000 + k, shape)).to(gu.DEV)
            ns = lambda ti, shp, dev, e=eps: e  # noqa: E731
            last_in = x32
            o32 = diff.p_sample(tap32, x32, t, noise_sampler=ns)
            obf = diff.p_sample(tapbf, xbf, t, noise_sampler=ns)
            drift.append(_chain_errors(tapbf.outs.pop(), tap32.outs.pop(), obf, o32))
            x32, xbf = o32["sample"], obf["sample"]
    print("bf16 chain drift at 128^3 (step: raw-out max / pred_xstart rms / pred_xstart max / sample; raw range):",
          " ".join(f"{i}:{d[0]:.1e}/{d[1]:.1e}/{d[2]:.1e}/{d[3]:.1e};{d[4]:.1f}" for i, d in enumerate(drift)))
    for i, d in enumerate(drift):
        assert d[0] < 2e-2 and d[1] < 2e-2 and d[3] < 2e-2, ("bf16 chain 128^3", i, d)
    assert drift[0][0] > 1e-5
    f_bf = _render_frame(gu, obf["pred_xstart"], 128, 32, 100, 100)
    f_32 = _render_frame(gu, o32["pred_xstart"], 128, 32, 100, 100)
    assert _psnr(f_bf, f_32) >= 40.0, _psnr(f_bf, f_32)
    # the fp32 chain against the pinned oracle on its last step
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = uo.unet_forward(sd, cfg, last_in.cpu(), torch.tensor([999 - (n_steps - 1)])).clamp(-1, 1)
    assert (o32["pred_xstart"].cpu() - ref).abs().max() <= 2e-3 * ref.abs().max()
