"""DPM-Solver++ multistep sampling (Lu et al. 2022), restated for the tests and independent of the product code:

  * float64: the log-SNR tables, the schedule, the effective orders and one step in the paper's D-form (differences of
    predictions), from which a step's four scalars are read off by applying it to unit inputs;
  * float32 numpy: the rounding order of holo_dpm_step, sample = ((a*x + b0*pred) + b1*hist1) + b2*hist2;
  * the closed-form Gaussian test problem of the convergence checks (optimal denoiser and probability-flow solution)."""
import numpy as np


def tables(alphas_cumprod):
    """(alpha, sigma, lambda) per timestep, float64: alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma)."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    alpha, sigma = np.sqrt(ac), np.sqrt(1.0 - ac)
    return alpha, sigma, np.log(alpha / sigma)


def logsnr_schedule(alphas_cumprod, steps):
    """For each of linspace(lambda_{T-1}, lambda_0, steps) the timestep with the nearest lambda (ties: the smaller t),
    duplicates removed; descending."""
    _, _, lam = tables(alphas_cumprod)
    picked = []
    for target in np.linspace(lam[-1], lam[0], steps):
        d = np.abs(lam - target)
        t = min(i for i in range(len(lam)) if d[i] == d.min())
        if t not in picked:
            picked.append(t)
    return picked


def effective_orders(n, order, lower_order_final=True):
    """Warm-up: step k uses min(order, k + 1).  The last step (past the end of the chain) is the order-1 one; with
    ``lower_order_final`` and order 3 the step before it is at most order 2."""
    out = [min(order, k + 1) for k in range(n)]
    out[-1] = 1
    if lower_order_final and order == 3 and n >= 2:
        out[-2] = min(out[-2], 2)
    return out


def step_f64(alphas_cumprod, order, s, t, x, m0, m1=None, m2=None, s1=None, s2=None):
    """One update s -> t (t < 0: past the end, the sample is the prediction) in the D-form; m1 / m2 are the predictions at
    the timesteps s1 / s2 visited before s."""
    if t < 0:
        return 1.0 * m0
    alpha, sigma, lam = tables(alphas_cumprod)
    h = lam[t] - lam[s]
    phi1 = np.expm1(-h)
    if order == 1:
        return (sigma[t] / sigma[s]) * x - alpha[t] * phi1 * m0
    r0 = (lam[s] - lam[s1]) / h
    if order == 2:
        D1 = (m0 - m1) / r0
        return (sigma[t] / sigma[s]) * x - alpha[t] * phi1 * m0 - 0.5 * alpha[t] * phi1 * D1
    r1 = (lam[s1] - lam[s2]) / h
    D1_0, D1_1 = (m0 - m1) / r0, (m1 - m2) / r1
    D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
    D2 = (D1_0 - D1_1) / (r0 + r1)
    phi2 = phi1 / h + 1.0
    phi3 = phi2 / h - 0.5
    return (sigma[t] / sigma[s]) * x - alpha[t] * phi1 * m0 + alpha[t] * phi2 * D1 - alpha[t] * phi3 * D2


def coefs_f64(alphas_cumprod, indices, order=2, lower_order_final=True):
    """((steps, 4) float64 rows (a, b0, b1, b2), effective orders): each scalar is the D-form step applied to a unit input."""
    n = len(indices)
    orders = effective_orders(n, order, lower_order_final)
    rows = np.zeros((n, 4))
    for k, s in enumerate(indices):
        t = indices[k + 1] if k + 1 < n else -1
        s1 = indices[k - 1] if k >= 1 else None
        s2 = indices[k - 2] if k >= 2 else None
        for j in range(4):
            e = [0.0, 0.0, 0.0, 0.0]
            e[j] = 1.0
            if j > orders[k] or (t < 0 and j > 1):
                continue  # the term does not exist at this order
            rows[k, j] = step_f64(alphas_cumprod, orders[k], s, t, e[0], e[1], e[2], e[3], s1, s2)
    return rows, orders


def dpm_step_f32(x, model_out, row, hist1=None, hist2=None, clip=True):
    """holo_dpm_step on numpy float32 arrays: x, model_out, hist*: (B, ...); row: (B, >= 4) float32.  Every product and every
    sum is rounded to float32, in the kernel's order; a None history term is not added.  Returns (sample, pred_xstart)."""
    x, model_out = np.asarray(x, dtype=np.float32), np.asarray(model_out, dtype=np.float32)
    row = np.asarray(row, dtype=np.float32)
    shp = (-1,) + (1,) * (x.ndim - 1)
    a, b0, b1, b2 = (row[:, k].reshape(shp) for k in range(4))
    pred = np.clip(model_out, np.float32(-1), np.float32(1)) if clip else model_out
    s = (a * x).astype(np.float32) + (b0 * pred).astype(np.float32)
    if hist1 is not None:
        s = s + (b1 * np.asarray(hist1, dtype=np.float32)).astype(np.float32)
    if hist2 is not None:
        s = s + (b2 * np.asarray(hist2, dtype=np.float32)).astype(np.float32)
    assert s.dtype == np.float32
    return s, pred


def chain_f32(x_T, outputs, rows, orders, clip=True):
    """The chain of ``dpm_step_f32`` driven by recorded model outputs: [(sample, pred_xstart) per step].  ``rows``:
    (steps, 8) float32, the same row for every sample of the batch."""
    x = np.asarray(x_T, dtype=np.float32)
    B = x.shape[0]
    h1 = h2 = None
    out = []
    for k, y in enumerate(outputs):
        row = np.repeat(np.asarray(rows[k], dtype=np.float32)[None], B, axis=0)
        s, p = dpm_step_f32(x, y, row, h1 if orders[k] >= 2 else None, h2 if orders[k] >= 3 else None, clip)
        out.append((s, p))
        x, h1, h2 = s, p, h1
    return out


# ---- the Gaussian test problem: data N(MU, SD^2) --------------------------------------------------------------------
MU, SD = 0.3, 0.5


def gaussian_denoiser(alphas_cumprod, x, t):
    """E[x_0 | x_t] for x_0 ~ N(MU, SD^2): the optimal x_0-prediction."""
    alpha, sigma, _ = tables(alphas_cumprod)
    a, s = alpha[t], sigma[t]
    return MU + a * SD * SD / (a * a * SD * SD + s * s) * (x - a * MU)


def gaussian_flow_solution(alphas_cumprod, x_T):
    """The exact probability-flow solution at abar = 1 of the chain that starts from x_T at t = T-1: the flow maps the
    marginal N(alpha*MU, alpha^2 SD^2 + sigma^2) onto N(MU, SD^2) quantile by quantile."""
    alpha, sigma, _ = tables(alphas_cumprod)
    a, s = alpha[-1], sigma[-1]
    return MU + SD / np.sqrt(a * a * SD * SD + s * s) * (x_T - a * MU)


def gaussian_chain_error(alphas_cumprod, indices, rows, orders, x_T):
    """max |final sample - exact solution| of a float64 loop driven by coefficient rows (a, b0, b1, b2), clip off."""
    x = np.asarray(x_T, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    m1 = m2 = None
    for k, s in enumerate(indices):
        m0 = gaussian_denoiser(alphas_cumprod, x, s)
        nxt = rows[k, 0] * x + rows[k, 1] * m0
        if orders[k] >= 2:
            nxt = nxt + rows[k, 2] * m1
        if orders[k] >= 3:
            nxt = nxt + rows[k, 3] * m2
        x, m1, m2 = nxt, m0, m1
    return float(np.abs(x - gaussian_flow_solution(alphas_cumprod, x_T)).max())
