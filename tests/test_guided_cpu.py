"""CPU: guided sampling host logic - the guided DDIM rows, the float32 restatements of the two guided steps
(tests/support/guided_ref.py) against the reference's recorded steps (tests/golden/guided_sampler.npz,
scripts/make_golden_guided.py) and the ray -> pixel lookup of PhotometricGuidance."""
import os

import numpy as np
import pytest
import torch

from holo_diffusion_amd.diffusion import ImplicitronGaussianDiffusion
from holo_diffusion_amd.guidance import xys_to_pixels
from tests.support.guided_ref import ddim_guided_step, ddpm_guided_step

STEP_TS = (999, 500, 1, 0)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "guided_sampler.npz"))


def ddpm_scalars(diff, t):
    """(c1, c2, v, sigma) of ddpm_guided_step: float32 casts of the float64 schedule, sigma with numpy's float32 exp."""
    t = np.asarray(t)
    f32 = lambda a: a[t].astype(np.float32)  # noqa: E731
    sigma = (t != 0).astype(np.float32) * np.exp(np.float32(0.5) * f32(diff.posterior_log_variance_clipped))
    return f32(diff.posterior_mean_coef1), f32(diff.posterior_mean_coef2), f32(diff.posterior_variance), sigma


def test_guided_rows_fill_slot_5_only():
    diff = ImplicitronGaussianDiffusion(num_steps=1000)
    for t, t_prev in (([999, 500, 1, 0], [998, 499, 0, -1]), ([980, 20, 0], [960, 0, -1])):
        for eta in (0.0, 0.5, 1.0):
            plain, rows = diff.ddim_coefs(t, t_prev, eta), diff.ddim_guided_coefs(t, t_prev, eta)
            assert rows.dtype == torch.float32 and rows.shape == (len(t), 8)
            assert (plain[:, 5:] == 0).all()  # ddim_coefs keeps its zeros
            assert torch.equal(rows[:, :5], plain[:, :5]) and (rows[:, 6:] == 0).all()
            want = np.sqrt(np.float32(1) - diff.alphas_cumprod[t].astype(np.float32))
            assert want.dtype == np.float32 and np.array_equal(rows[:, 5].numpy(), want)


def test_ddim_restatement_reproduces_reference_steps(g):
    """ddim_guided_step with the plugin's guided rows IS the reference's ddim_sample with cond_fn, bit for bit."""
    diff = ImplicitronGaussianDiffusion(num_steps=1000)
    T = torch.from_numpy
    x, gr = T(g["step.x"]), T(g["step.grad"])
    for ti in STEP_TS:
        mo, nz = T(g[f"step.t{ti}.model_out"]), T(g[f"step.t{ti}.noise"])
        for clip in (1, 0):
            for eta in (0.0, 0.5, 1.0):
                s, p = ddim_guided_step(x, mo, gr, diff.ddim_guided_coefs([ti], [ti - 1], eta), nz, bool(clip))
                assert torch.equal(s, T(g[f"ddim.t{ti}.clip{clip}.eta{eta:g}.sample"])), (ti, clip, eta)
                assert torch.equal(p, T(g[f"ddim.t{ti}.clip{clip}.pred_xstart"])), (ti, clip)
    t2 = g["b2.t"].tolist()
    s, p = ddim_guided_step(T(g["b2.x"]), T(g["b2.model_out"]), T(g["b2.grad"]),
                            diff.ddim_guided_coefs(t2, [t - 1 for t in t2], 0.5), T(g["b2.noise"]))
    assert torch.equal(s, T(g["b2.ddim.sample"])) and torch.equal(p, T(g["b2.ddim.pred_xstart"]))


def test_ddpm_restatement_reproduces_reference_steps(g):
    """ddpm_guided_step against the reference's p_sample with cond_fn: to the tolerance of the fused DDPM update
    (test_step_kernel_bit_exact_vs_oracle) - the reference rounds the mean's products separately and uses torch's exp;
    pred_xstart, which condition_mean leaves alone, bit for bit."""
    diff = ImplicitronGaussianDiffusion(num_steps=1000)
    T = torch.from_numpy
    x, gr = T(g["step.x"]), T(g["step.grad"])
    for ti in STEP_TS:
        mo, nz = T(g[f"step.t{ti}.model_out"]), T(g[f"step.t{ti}.noise"])
        for clip in (1, 0):
            s, p = ddpm_guided_step(x, mo, gr, nz, *ddpm_scalars(diff, [ti]), bool(clip))
            torch.testing.assert_close(s, T(g[f"ddpm.t{ti}.clip{clip}.sample"]), rtol=3e-7, atol=1e-7)
            assert torch.equal(p, T(g[f"ddpm.t{ti}.clip{clip}.pred_xstart"])), (ti, clip)
    t2 = g["b2.t"].tolist()
    s, p = ddpm_guided_step(T(g["b2.x"]), T(g["b2.model_out"]), T(g["b2.grad"]), T(g["b2.noise"]), *ddpm_scalars(diff, t2))
    torch.testing.assert_close(s, T(g["b2.ddpm.sample"]), rtol=3e-7, atol=1e-7)
    assert torch.equal(p, T(g["b2.ddpm.pred_xstart"]))


def test_guidance_moves_the_recorded_steps(g):
    """The fixture's gradient matters: the recorded guided steps are not the unguided ones of ddim_sampler.npz's inputs."""
    from tests.support.ddim_ref import ddim_step
    diff = ImplicitronGaussianDiffusion(num_steps=1000)
    T = torch.from_numpy
    s, _ = ddim_step(T(g["step.x"]), T(g["step.t500.model_out"]), diff.ddim_coefs([500], [499], 0.0))
    assert (s - T(g["ddim.t500.clip1.eta0.sample"])).abs().max() > 1e-3


@pytest.mark.parametrize("H,W", [(16, 16), (12, 16), (16, 12)])
def test_xys_pixel_lookup_round_trips(H, W):
    """The ray sampler's pixel centres (PyTorch3D NDC: the shorter side spans [-1, 1]) map back to their (row, column)."""
    rx, ry = (W / H, 1.0) if W >= H else (1.0, H / W)
    xs = torch.linspace(rx - rx / W, -rx + rx / W, W, dtype=torch.float32)
    ys = torch.linspace(ry - ry / H, -ry + ry / H, H, dtype=torch.float32)
    idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(1)).reshape(2, -1)
    row, col = xys_to_pixels(torch.stack([xs[idx % W], ys[idx // W]], dim=-1), H, W)
    assert torch.equal(row, idx // W) and torch.equal(col, idx % W)
    with pytest.raises(ValueError):
        xys_to_pixels(torch.tensor([[rx + 3 * rx / W, 0.0]]), H, W)


def test_ray_sampler_draws_pixel_centres_from_a_generator():
    """AdaptiveRaySampler's mask draw with ``n_rays`` / ``generator``: reproducible, inside the mask's support, and every
    xy is a pixel centre of the (non-square) frame."""
    import holo_diffusion_amd as hda
    from holo_diffusion_amd.render import RenderSamplingMode
    H, W = 12, 16
    rs = hda.AdaptiveRaySampler(image_height=H, image_width=W)
    cams = hda.get_simple_360_camera_trajectory(6.28, 2, -0.5, 10, (0.0, -1.0, 0.0), 3.2)
    mask = torch.zeros(2, 1, H, W)
    mask[:, :, 3:9, 4:13] = 1
    draw = lambda seed: rs(cams, hda.EvaluationMode.TRAINING, sampling_mode=RenderSamplingMode.MASK_SAMPLE, mask=mask,  # noqa: E731
                           n_rays=21, generator=torch.Generator().manual_seed(seed)).xys
    a, b, c = draw(3), draw(3), draw(4)
    assert a.shape == (2, 21, 1, 2) and torch.equal(a, b) and not torch.equal(a, c)
    row, col = xys_to_pixels(a.reshape(2, 21, 2), H, W)
    assert bool((mask[torch.arange(2)[:, None], 0, row, col] == 1).all())
