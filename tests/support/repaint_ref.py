"""Float32 numpy restatements of the masked (inpainting) DDPM step and of the forward noising behind it
(include/holo_abi.h: holo_ddpm_step_inpaint, holo_q_sample), and the bookkeeping of a masked chain's noise requests.
tests/test_inpaint_cpu.py checks them against the plain DDPM restatement (tests/support/guided_ref.py, zero gradient) and
against ``ImplicitronGaussianDiffusion.q_sample``; the GPU tests compare the loops against them."""
import numpy as np
import torch

f32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)  # noqa: E731


def _col(v, x):
    return np.asarray(v, dtype=np.float32).reshape((-1,) + (1,) * (x.ndim - 1))


def step_scalars(diff, t):
    """(c1, c2, sigma) of each sample's timestep from the float32 table the DDPM kernels read; sigma with numpy's float32
    exp (the device's expf may differ in the last bit: the comparisons that involve it carry a tolerance)."""
    t = np.asarray(t).reshape(-1)
    tab = np.stack([diff.posterior_mean_coef1, diff.posterior_mean_coef2, diff.posterior_log_variance_clipped], 1).astype(np.float32)
    return tab[t, 0], tab[t, 1], (t != 0).astype(np.float32) * np.exp(np.float32(0.5) * tab[t, 2])


def q_lin(a, x, b, e):
    """a*x + b*e with the row (a, b) of each sample: both products rounded, the sum rounded (holo_q_sample)."""
    x, e = f32(x), f32(e)
    out = _col(a, x) * x + _col(b, x) * e
    assert out.dtype == np.float32
    return out


def inpaint_step(x, model_out, known, mask, noise, noise_known, c1, c2, sigma, a, b, clip=True):
    """The masked step on NCDHW arrays; mask (B, 1, R, R, R); c1, c2, sigma, a, b: (B,) float32.
      unk = fma(sigma, e_u, fma(c2, x, c1*pred))   (each fma through float64, as guided_ref.ddpm_guided_step states it)
      known = a*x0 + b*e_k ;  out = m*known + (1 - m)*unk   (every product and sum rounded)
    ``noise_known`` None: e_k = 0.  Returns (sample, pred_xstart) as float32 arrays."""
    x, m_out, k0, m, e = (f32(v) for v in (x, model_out, known, mask, noise))
    ek = np.zeros_like(x) if noise_known is None else f32(noise_known)
    c1, c2, sigma = (_col(v, x) for v in (c1, c2, sigma))
    pred = np.clip(m_out, np.float32(-1), np.float32(1)) if clip else m_out
    f64 = lambda v: v.astype(np.float64)  # noqa: E731
    mean = (f64(c2) * f64(x) + f64(c1 * pred)).astype(np.float32)
    unk = (f64(sigma) * f64(e) + f64(mean)).astype(np.float32)
    kn = q_lin(a, k0, b, ek)
    om = np.float32(1) - m
    out = m * kn + om * unk
    assert out.dtype == np.float32
    return out, pred


def walk(ops, T):
    """The reverse steps of a ``repaint_schedule`` with what the loop needs of each: [(t, visit, jump | None)], jump =
    (level_from, level_to, visit of the target) for a forward jump in front of the step.  visit counts the earlier visits of
    the timestep (of the jump's target level; the start of a chain below T counts as one)."""
    top = ops[0][1] + 1
    seen, fwd_seen, out, jump = {}, ({top: 1} if top < T else {}), [], None
    for op in ops:
        if op[0] == "forward":
            jump = (op[1], op[2], fwd_seen.get(op[2], 0))
            fwd_seen[op[2]] = jump[2] + 1
        else:
            out.append((op[1], seen.get(op[1], 0), jump))
            seen[op[1]] = seen.get(op[1], 0) + 1
            jump = None
    return out


def sampler_index(T, t, visit, d):
    """What the masked loop asks a ``noise_sampler`` for: d = 0 the step's noise, 1 the known part's, 2 a jump's or the
    start's (t = the target timestep)."""
    return t if (d == 0 and visit == 0) else t + (T + 1) * (3 * visit + d)
