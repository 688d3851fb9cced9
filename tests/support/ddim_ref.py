"""Float32 CPU restatement of the DDIM step (gaussian_diffusion.py:677-693, :717-727) and a float64 statement of its
coefficient rows.  ``ddim_step`` is pinned to the reference by tests/golden/ddim_sampler.npz (tests/test_ddim_cpu.py); the
GPU tests compare holo_ddim_step against it bit for bit."""
import numpy as np


def ddim_step(x, model_out, coefs, noise=None, clip=True):
    """x, model_out, noise: (B, ...) float32; coefs: (B, 8) rows of holo_ddim_step.  Returns (sample, pred_xstart)."""
    shp = (-1,) + (1,) * (x.dim() - 1)
    c0, c1, c2, c3, c4 = (coefs[:, k].reshape(shp) for k in range(5))
    pred = model_out.clamp(-1, 1) if clip else model_out
    eps = (c0 * x - pred) / c1
    mean = pred * c2 + c3 * eps
    sample = mean + c4 * noise if noise is not None else mean
    return sample, pred


def ddim_coefs_f64(alphas_cumprod, t, t_other, eta=0.0, reverse=False):
    """The rows of ImplicitronGaussianDiffusion.ddim_coefs in float64 (numpy), not rounded.  c0 / c1 come from the float64
    schedule; the other slots start from abar cast to float32, as the reference's ``_extract_into_tensor`` hands them to
    its float32 arithmetic (1 - abar_prev at t = 1 cancels: the cast, not the arithmetic, decides its value)."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    T = ac.shape[0]
    t, t_other = np.asarray(t), np.asarray(t_other)
    rows = np.zeros((t.shape[0], 8))
    rows[:, 0] = np.sqrt(1.0 / ac[t])
    rows[:, 1] = np.sqrt(1.0 / ac[t] - 1)
    ac = ac.astype(np.float32).astype(np.float64)
    ab = ac[t]
    if reverse:
        ab_next = np.where(t_other < T, ac[np.minimum(t_other, T - 1)], 0.0)
        rows[:, 2], rows[:, 3] = np.sqrt(ab_next), np.sqrt(1 - ab_next)
        return rows
    ab_prev = np.where(t_other >= 0, ac[np.maximum(t_other, 0)], 1.0)
    sigma = eta * np.sqrt((1 - ab_prev) / (1 - ab)) * np.sqrt(1 - ab / ab_prev)
    rows[:, 2], rows[:, 3] = np.sqrt(ab_prev), np.sqrt(np.maximum(1 - ab_prev - sigma ** 2, 0.0))
    rows[:, 4] = (t != 0) * sigma
    return rows
