"""Float64 numpy restatement of the diffusion losses and of the variational bound's terms (include/holo_abi.h:
holo_diffusion_loss, holo_vb_terms; START_X, FIXED_SMALL), the float32 restatement of the loss cotangent, and the cases,
inputs and stub model of tests/golden/diffusion_losses.npz.  scripts/make_golden_diffusion_losses.py checks the float64
functions against the reference code run on float64 tensors before it writes the fixture; the GPU tests compare the kernels
against them.  ``diff`` is anything that carries the float64 schedule tables under the reference's names (the reference's
GaussianDiffusion or ImplicitronGaussianDiffusion)."""
import numpy as np

SHAPES = ((2, 8, 4, 4, 4), (1, 6, 4, 4, 4), (2, 8, 8, 8, 8), (3, 4, 12, 12, 12))
T_ROWS = ((999, 998), (500, 1), (1, 0), (0, 0))
LOOP_SHAPE, LOOP_STEPS, LOOP_SEED = (2, 8, 4, 4, 4), 20, 4100
SUBSET_TIMESTEPS = (999, 500, 1, 0)
LN2 = float(np.log(2.0))


def np_noise(seed, shape):
    """oracle.common.np_noise (restated: the tests do not import the oracle package for a draw)."""
    g = np.random.Generator(np.random.Philox(key=int(seed) & 0xFFFFFFFFFFFFFFFF))
    return g.standard_normal(int(np.prod(shape)), dtype=np.float64).astype(np.float32).reshape(shape)


def np_uniform(seed, shape, lo, hi):
    g = np.random.Generator(np.random.Philox(key=int(seed) & 0xFFFFFFFFFFFFFFFF))
    return g.uniform(lo, hi, int(np.prod(shape))).reshape(shape)


def case_seed(shape_index, row_index):
    return 5000 + 100 * shape_index + 10 * row_index


def timesteps_of(row, batch):
    """A timestep row cut or extended to the batch: (1, 0) at batch 3 is (1, 0, 1)."""
    return np.array([row[i % len(row)] for i in range(batch)], dtype=np.int64)


def make_x_start(seed, shape):
    """tanh(1.5 * noise) with 24 elements per sample set to exactly +1 / -1 (both tail branches of the decoder term)."""
    x = np.tanh(1.5 * np_noise(seed, shape).astype(np.float64)).astype(np.float32)
    flat = x.reshape(shape[0], -1)
    idx = 5 + 13 * np.arange(24)
    flat[:, idx[0::2]] = 1.0
    flat[:, idx[1::2]] = -1.0
    return x


def sigma0(diff):
    return float(np.exp(0.5 * diff.posterior_log_variance_clipped[0]))


def stub_output(diff, x_start, t, seed):
    """The fixed 'model' of the fixture, a function of seeds only.  Rows with t > 0: 0.6 * x_start + 0.5 * noise(seed) (it
    leaves [-1, 1], so the clip matters).  Rows with t == 0: x_start + sigma_0 * u, u uniform in [-2, 2] - the decoder term's
    input condition (holo_abi.h): the clamped CDF difference stays far from underflow."""
    x64 = x_start.astype(np.float64)
    out = 0.6 * x64 + 0.5 * np_noise(seed, x_start.shape)
    near = x64 + sigma0(diff) * np_uniform(seed + 1, x_start.shape, -2.0, 2.0)
    t0 = (np.asarray(t).reshape(-1) == 0).reshape((-1,) + (1,) * (x_start.ndim - 1))
    return np.where(t0, near, out).astype(np.float32)


def q_sample32(diff, x_start, t, noise):
    """q_sample in float32: a*x + b*e, products rounded, sum rounded (gaussian_diffusion.py:209-227, holo_q_sample)."""
    t = np.asarray(t).reshape(-1)
    col = lambda v: v.astype(np.float32).reshape((-1,) + (1,) * (x_start.ndim - 1))  # noqa: E731
    out = col(diff.sqrt_alphas_cumprod[t]) * x_start + col(diff.sqrt_one_minus_alphas_cumprod[t]) * noise
    assert out.dtype == np.float32
    return out


def case_inputs(diff, shape_index, row_index):
    """x_start, noise, t, x_t (float32 q_sample) and the stub's output of one (shape, timestep row) case."""
    shape, seed = SHAPES[shape_index], case_seed(shape_index, row_index)
    t = timesteps_of(T_ROWS[row_index], shape[0])
    x_start, noise = make_x_start(seed, shape), np_noise(seed + 1, shape)
    return {"x_start": x_start, "noise": noise, "t": t, "x_t": q_sample32(diff, x_start, t, noise),
            "model_out": stub_output(diff, x_start, t, seed + 2)}


def loop_model_output(diff, x_start, timestep, seed=LOOP_SEED):
    """The stub as a model of calc_bpd_loop: its output at one (uniform) timestep."""
    return stub_output(diff, x_start, np.full(x_start.shape[0], timestep), seed + 10 * int(timestep))


def loop_noise(shape, timestep, seed=LOOP_SEED):
    return np_noise(seed + 10 * int(timestep) + 5, shape)


# ---- the restatement ---------------------------------------------------------------------------
def _flat_mean(a):
    return a.reshape(a.shape[0], -1).mean(axis=1)


def _col(v, x):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (x.ndim - 1))


def loss_terms(target, model_out):
    """(mse, huber) per sample in float64: mean_flat((target - model_out)**2) and mean_flat(_huber(.., scaling=0.001))."""
    sq = (np.asarray(target, np.float64) - np.asarray(model_out, np.float64)) ** 2
    s = 0.001
    huber = (np.sqrt(np.maximum(1 + sq / (s * s), 0.0) + 1e-4) - 1) * s
    return _flat_mean(sq), _flat_mean(huber)


def loss_grad32(target, model_out, weights):
    """holo_diffusion_loss's grad_out bit for bit: (model_out - target) * float32(2 * w_b / n), float32 operations."""
    target, model_out = np.asarray(target, np.float32), np.asarray(model_out, np.float32)
    n = target[0].size
    s = (2.0 * np.asarray(weights, np.float64) / n).astype(np.float32)
    out = (model_out - target) * s.reshape((-1,) + (1,) * (target.ndim - 1))
    assert out.dtype == np.float32
    return out


def schedule_rows(diff, t):
    """(n, 8) float64 rows of holo_vb_terms at timesteps t, from the float64 schedule (vb_coefs casts them to float32)."""
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    lv = diff.posterior_log_variance_clipped[t]
    return np.stack([diff.posterior_mean_coef1[t], diff.posterior_mean_coef2[t], lv, np.exp(-lv), np.exp(-0.5 * lv),
                     diff.sqrt_recip_alphas_cumprod[t], diff.sqrt_recipm1_alphas_cumprod[t], (t == 0).astype(np.float64)],
                    axis=1)


def _cdf(x):
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def decoder_clamp_args(x_start, mean, inv_std):
    """The argument of the clamp(min=1e-12) that discretized_gaussian_log_likelihood takes the log of, per element."""
    centered = x_start - mean
    cdf_plus = _cdf(inv_std * (centered + 1.0 / 255.0))
    cdf_min = _cdf(inv_std * (centered - 1.0 / 255.0))
    return np.where(x_start < -0.999, cdf_plus, np.where(x_start > 0.999, 1.0 - cdf_min, cdf_plus - cdf_min))


def vb_terms(rows, x_start, x_t, noise, model_out, clip, reference_residue=False, with_clamp_args=False):
    """(n, 3) float64 {vb in bits, xstart_mse, eps_mse} of holo_vb_terms on the (n, 8) ``rows``; ``noise`` None: eps_mse 0.
    ``reference_residue``: add normal_kl's -1 + lv2 - lv1 + exp(lv1 - lv2) in the reference's order - exactly 0 in real
    arithmetic, a rounding residue in floating point, which the kernel does not evaluate."""
    x0, xt, m = (np.asarray(v, np.float64) for v in (x_start, x_t, model_out))
    rows = np.asarray(rows, np.float64)
    c1, c2, lv, einv, istd, sr, srm1, t0 = (_col(rows[:, k], x0) for k in range(8))
    pred = np.clip(m, -1.0, 1.0) if clip else m
    mean_p, mean_q = c1 * pred + c2 * xt, c1 * x0 + c2 * xt
    residue = (-1.0 + lv - lv + np.exp(lv - lv)) if reference_residue else 0.0
    kl = 0.5 * (residue + (mean_q - mean_p) ** 2 * einv)
    args = decoder_clamp_args(x0, mean_p, istd)
    nll = -np.log(np.maximum(args, 1e-12))
    vb = _flat_mean(np.where(t0 != 0, nll, kl)) / LN2
    xs = _flat_mean((pred - x0) ** 2)
    with np.errstate(invalid="ignore", over="ignore"):
        eps = np.zeros_like(xs) if noise is None else _flat_mean(((sr * xt - pred) / srm1 - np.asarray(noise, np.float64)) ** 2)
    out = np.stack([vb, xs, eps], axis=1)
    return (out, args) if with_clamp_args else out


def prior_bpd(diff, x_start):
    """_prior_bpd (gaussian_diffusion.py:970-986): normal_kl(q(x_T | x_0) || N(0, 1)) in bits per dimension."""
    x0 = np.asarray(x_start, np.float64)
    T = len(diff.betas)
    mean = diff.sqrt_alphas_cumprod[T - 1] * x0
    lv = diff.log_one_minus_alphas_cumprod[T - 1]
    return _flat_mean(0.5 * (-1.0 + 0.0 - lv + np.exp(lv - 0.0) + mean ** 2 * np.exp(-0.0))) / LN2


def rel(a, b):
    """|a - b| / |b| elementwise (0 where both are 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))
