"""Float32 CPU restatements of the two guided sampler steps (include/holo_abi.h: holo_ddpm_step_guided - condition_mean,
gaussian_diffusion.py:429-433 inside p_sample :499-506 -, holo_ddim_step_guided - condition_score :445-453 followed by
ddim_sample :674-693).  Both are pinned to the reference by tests/golden/guided_sampler.npz (tests/test_guided_cpu.py); the
GPU tests compare the kernels against them bit for bit."""
import numpy as np
import torch


def _col(v, x):
    return np.asarray(v, dtype=np.float32).reshape((-1,) + (1,) * (x.ndim - 1))


def ddpm_guided_step(x, model_out, grad, noise, c1, c2, v, sigma, clip=True):
    """x, model_out, grad, noise: (B, ...) float32 tensors; c1, c2, v, sigma: (B,) float32 - posterior_mean_coef1/2,
    posterior_variance and [t != 0] * exp(0.5 * log_variance) of each sample's timestep.  The kernel's arithmetic:
      mean = fma(c2, x, c1*pred) ;  mean_g = mean + v*grad (product rounded, sum rounded) ;  sample = fma(sigma, noise, mean_g)
    Each fma is stated through float64: the product of two float32 is exact there, and the one float64 sum rounded to
    float32 is the exactly rounded fma unless an element sits on a double-rounding tie (tests/test_gpu_diffusion.py,
    test_ddpm_step_arithmetic_is_pinned).  Returns (sample, pred_xstart) as tensors."""
    x, m, g, e = (np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a, dtype=np.float32) for a in (x, model_out, grad, noise))
    c1, c2, v, sigma = (_col(a, x) for a in (c1, c2, v, sigma))
    pred = np.clip(m, np.float32(-1), np.float32(1)) if clip else m
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    mean = (f64(c2) * f64(x) + f64(c1 * pred)).astype(np.float32)
    mean_g = mean + v * g
    sample = (f64(sigma) * f64(e) + f64(mean_g)).astype(np.float32)
    assert pred.dtype == mean_g.dtype == np.float32
    return torch.from_numpy(sample), torch.from_numpy(pred)


def ddim_guided_step(x, model_out, grad, coefs, noise=None, clip=True):
    """x, model_out, grad, noise: (B, ...) float32 tensors; coefs: (B, 8) rows of holo_ddim_step_guided
    (ImplicitronGaussianDiffusion.ddim_guided_coefs).  Every operation rounded, in the reference's order.  Returns
    (sample, pred_xstart)."""
    shp = (-1,) + (1,) * (x.dim() - 1)
    c0, c1, c2, c3, c4, c5 = (coefs[:, k].reshape(shp) for k in range(6))
    pred = model_out.clamp(-1, 1) if clip else model_out
    eps0 = (c0 * x - pred) / c1
    eps1 = eps0 - c5 * grad
    predg = c0 * x - c1 * eps1  # (not clamped again)
    eps = (c0 * x - predg) / c1
    mean = predg * c2 + c3 * eps
    sample = mean + c4 * noise if noise is not None else mean
    return sample, predg
