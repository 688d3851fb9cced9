"""CPU: DPM-Solver++ host logic - the log-SNR schedule, the coefficient rows of holo_dpm_step against the float64
restatement (tests/support/dpm_ref.py), convergence orders on a Gaussian problem with a closed-form solution, the order-1
step against DDIM at eta 0, and the generate CLI / model keys."""
import numpy as np
import pytest
import torch

from holo_diffusion_amd.diffusion import ImplicitronGaussianDiffusion
from oracle.common import np_noise
from tests.support import dpm_ref
from tests.support.ddim_ref import ddim_step

STEPS = (1, 2, 3, 5, 20, 50)
EXPLICIT = [900, 640, 333, 100, 31, 7, 0]


@pytest.fixture(scope="module")
def diff():
    return ImplicitronGaussianDiffusion(num_steps=1000)


# ---- schedule ---------------------------------------------------------------------------------------------------------
def test_logsnr_schedule(diff):
    """log-SNR spacing: the documented lengths on the 1000-step table (duplicates removed: 50 -> 49, 100 -> 94), T-1 first
    and 0 last with more than one step, [T-1] alone for one step, strictly decreasing, equal to the restatement."""
    for steps, n in ((20, 20), (50, 49), (100, 94), (2, 2), (1, 1)):
        s = diff.dpm_schedule(steps)
        assert len(s) == n, (steps, len(s))
        assert s == dpm_ref.logsnr_schedule(diff.alphas_cumprod, steps)
        assert all(a > b for a, b in zip(s, s[1:]))
        assert s[0] == 999 and (s[-1] == 0 if steps > 1 else s == [999])
    assert diff.dpm_schedule(20, spacing="logsnr") == diff.dpm_schedule(20) == diff.dpm_schedule()  # (20 is the default)
    assert diff.dpm_schedule(4, spacing="time") == diff.ddim_schedule(4) == [750, 500, 250, 0]
    assert diff.dpm_schedule(timesteps=EXPLICIT) == EXPLICIT


def test_schedule_value_errors(diff):
    for bad in ([10, 10], [3, 7], [1000, 5], []):
        with pytest.raises(ValueError):
            diff.dpm_schedule(timesteps=bad)
    with pytest.raises(ValueError):
        diff.dpm_schedule(4, timesteps=[5, 0])  # steps together with timesteps
    for bad in (0, -3):
        with pytest.raises(ValueError):
            diff.dpm_schedule(bad)
    with pytest.raises(ValueError):
        diff.dpm_schedule(4, spacing="karras")
    with pytest.raises(ValueError):
        diff.dpm_schedule(999, spacing="time")  # (the "ddimS" rule: no integer stride gives 999 timesteps)


# ---- coefficient rows -------------------------------------------------------------------------------------------------
def _check_rows(diff, indices, order, lower_order_final=True):
    rows, orders = diff.dpm_coefs(indices, order, lower_order_final)
    want, want_orders = dpm_ref.coefs_f64(diff.alphas_cumprod, indices, order, lower_order_final)
    assert rows.dtype == torch.float32 and rows.shape == (len(indices), 8) and (rows[:, 4:] == 0).all()
    assert list(orders) == want_orders, (indices, order)
    # 1e-6 relative: the float64 formulas carry < 1e-10, the float32 rounding of a row 6e-8; a wrong coefficient is off by O(1)
    np.testing.assert_allclose(rows[:, :4].numpy().astype(np.float64), want, rtol=1e-6, atol=0)
    assert rows[-1].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]  # the step past the end: the sample is the prediction
    for k, o in enumerate(orders):  # terms above the effective order are exactly absent
        assert (rows[k, 1 + o:4] == 0).all(), (k, o)
    return orders


@pytest.mark.parametrize("spacing", ["logsnr", "time"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_coefficient_rows_vs_float64(diff, order, spacing):
    """dpm_coefs against the D-form restatement for steps in {1, 2, 3, 5, 20, 50}.  (spacing="time" is the "ddimS" stride, which
    has no one-step schedule on 1000 timesteps: that single combination must raise, as ddim_schedule(1) does.)"""
    for steps in STEPS:
        if spacing == "time" and steps == 1:
            with pytest.raises(ValueError):
                diff.dpm_schedule(steps, spacing)
            continue
        indices = diff.dpm_schedule(steps, spacing)
        orders = _check_rows(diff, indices, order)
        n = len(indices)
        # warm-up min(order, k + 1); the last step order 1; with order 3 the one before it at most 2
        want = [min(order, k + 1) for k in range(n)]
        want[-1] = 1
        if order == 3 and n >= 2:
            want[-2] = min(want[-2], 2)
        assert list(orders) == want, (steps, orders)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_coefficient_rows_explicit_list(diff, order):
    orders = _check_rows(diff, EXPLICIT, order)
    assert list(orders) == {1: [1] * 7, 2: [1, 2, 2, 2, 2, 2, 1], 3: [1, 2, 3, 3, 3, 2, 1]}[order]
    free = _check_rows(diff, EXPLICIT, order, lower_order_final=False)
    assert list(free) == {1: [1] * 7, 2: [1, 2, 2, 2, 2, 2, 1], 3: [1, 2, 3, 3, 3, 3, 1]}[order]
    _check_rows(diff, [0], order)  # a one-step chain is the prediction
    for bad in (0, 4):
        with pytest.raises(ValueError):
            diff.dpm_coefs(EXPLICIT, bad)


def test_order1_coefficients_are_ddim_eta0(diff):
    """In exact arithmetic the order-1 update is DDIM at eta 0: x_prev = sqrt(abar_prev) pred + sqrt(1 - abar_prev) eps with
    eps = (x - sqrt(abar) pred) / sqrt(1 - abar), i.e. a = sigma_t / sigma_s and b0 = alpha_t - a alpha_s."""
    ac = diff.alphas_cumprod
    idx = diff.dpm_schedule(50)
    rows, _ = dpm_ref.coefs_f64(ac, idx, 1)
    for k in range(len(idx) - 1):
        s, t = idx[k], idx[k + 1]
        a = np.sqrt(1 - ac[t]) / np.sqrt(1 - ac[s])
        assert abs(rows[k, 0] - a) < 1e-15 and abs(rows[k, 1] - (np.sqrt(ac[t]) - a * np.sqrt(ac[s]))) < 1e-14, k


# ---- convergence ------------------------------------------------------------------------------------------------------
def test_convergence_orders_on_gaussian_data(diff):
    """The product's rows drive a float64 loop with the optimal denoiser of N(0.3, 0.5^2) data (clip off, log-SNR spacing);
    the error is the max over 4096 chains against the exact probability-flow solution.  Deterministic float64 arithmetic:
    order 2 at 20 steps at most 1/4 of order 1's error; halving the step (40 -> 80) divides the error by ~2 at order 1, by
    >= 3 at order 2 and by >= 5 at order 3; order 3 below order 2 at 80 steps."""
    ac = diff.alphas_cumprod
    x_T = np.random.default_rng(0).standard_normal(4096)
    err = {}
    for order in (1, 2, 3):
        for steps in (20, 40, 80):
            idx = diff.dpm_schedule(steps)
            rows, orders = diff.dpm_coefs(idx, order)
            err[order, steps] = dpm_ref.gaussian_chain_error(ac, idx, rows.numpy(), orders, x_T)
    print("dpm convergence errors:", {k: f"{v:.2e}" for k, v in err.items()})
    assert err[2, 20] <= 0.25 * err[1, 20], err
    assert 1.7 <= err[1, 40] / err[1, 80] <= 2.3, err
    assert err[2, 40] / err[2, 80] >= 3, err
    assert err[3, 40] / err[3, 80] >= 5, err
    assert err[3, 80] < err[2, 80], err


# ---- order 1 is DDIM --------------------------------------------------------------------------------------------------
PAIRS = [(999, 998), (999, 946), (800, 600), (500, 499), (200, 0), (100, 80), (20, 19), (20, 0), (19, 18), (10, 5), (2, 1),
         (1, 0), (0, -1)]
CAST_LIMITED = (20, 0)  # the one pair with t >= 20 whose reference step is limited by the float32 cast of abar_prev (see the test)


@pytest.mark.parametrize("t,t_prev", PAIRS)
def test_order1_step_vs_ddim_restatement(diff, t, t_prev):
    """The float32 restatement of an order-1 step against tests/support/ddim_ref.ddim_step at eta 0 on the same inputs:
    within 1e-5 of the sample's range for t >= 20 and at the last step, 1e-3 below (the project's DDIM / DDPM thresholds,
    test_ddim_eta1_full_schedule_is_the_ddpm_step).  One named exception, (20, 0), the last stride of ddim50: it measures
    2.9e-5, and the error is the REFERENCE's.  Its c3 = sqrt(1 - abar_prev) starts from abar_0 = 0.9999 cast to float32
    (half an ulp, 2^-25, is 1.5e-4 of 1 - abar_0 after the square root), and t = 20 scales eps by 1 / c1 = 12.6.  That pair's
    bound is 1e-5 plus exactly this cast error carried through c3 * eps, computed below (about 5e-5 here), and the order-1
    step itself is within 4.2e-7 * (|a x| + |b0 pred|) of float64 at every pair (seven roundings of 2^-24 each)."""
    shape = (2, 8, 4, 4, 4)
    x, mo = np_noise(21, shape), np_noise(22, shape) * np.float32(1.5)
    indices = [t, t_prev] if t_prev >= 0 else [t]
    rows, _ = diff.dpm_coefs(indices, order=1)
    row = rows[:1].numpy().repeat(2, axis=0)
    s, p = dpm_ref.dpm_step_f32(x, mo, row)
    ds, dp = ddim_step(torch.from_numpy(x), torch.from_numpy(mo), diff.ddim_coefs([t, t], [t_prev, t_prev], 0.0))
    assert np.array_equal(p, dp.numpy())
    rel = float(np.abs(s - ds.numpy()).max() / np.abs(ds.numpy()).max())
    print(f"order-1 step vs DDIM at t={t} -> {t_prev}: {rel:.2e} of the range")
    bound = 1e-5 if t >= 20 or t_prev < 0 else 1e-3
    if (t, t_prev) == CAST_LIMITED:
        ac = diff.alphas_cumprod
        c3_rel = 2.0 ** -25 / (2 * (1 - ac[t_prev]))  # half an ulp of float32(abar_prev) through sqrt(1 - abar_prev)
        eps = (x.astype(np.float64) / np.sqrt(ac[t]) - p) / np.sqrt(1 / ac[t] - 1)
        bound += c3_rel * np.sqrt(1 - ac[t_prev]) * np.abs(eps).max() / np.abs(ds.numpy()).max()
        assert bound < 1e-4, bound
    assert rel <= bound, (t, t_prev, rel, bound)
    want, _ = dpm_ref.coefs_f64(diff.alphas_cumprod, indices, 1)
    a, b0 = want[0, 0], want[0, 1]
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    exact = a * x64 + b0 * p64
    bound = 4.2e-7 * (np.abs(a * x64) + np.abs(b0 * p64))
    assert (np.abs(s.astype(np.float64) - exact) <= bound).all(), (t, t_prev)


# ---- loop arguments (refused before the model or the device is touched) -------------------------------------------------
def test_loop_argument_errors(diff):
    shape = (1, 4, 2, 2, 2)
    for kw in (dict(order=0), dict(order=4), dict(steps=0), dict(steps=5, timesteps=[10, 0]), dict(spacing="plms")):
        with pytest.raises(ValueError):
            diff.dpm_sample_loop(None, shape, device="cpu", **kw)
        with pytest.raises(ValueError):
            next(diff.dpm_sample_loop_progressive(None, shape, device="cpu", **kw))
    with pytest.raises(NotImplementedError):
        diff.dpm_sample_loop(None, shape, device="cpu", cond_fn=lambda *a: None)


# ---- command line and model keys ----------------------------------------------------------------------------------------
def test_cli_accepts_dpmpp_keys():
    from holo_diffusion_amd.generate import cli_sampler_kwargs, parse_cli
    cfg = parse_cli(["exp_dir=/x", "sampler=dpmpp", "dpm_steps=20", "dpm_order=2", "dpm_spacing=logsnr"])
    assert cfg["sampler"] == "dpmpp" and cfg["dpm_steps"] == 20 and cfg["dpm_order"] == 2 and cfg["dpm_spacing"] == "logsnr"
    assert cli_sampler_kwargs(cfg) == {"sampler": "dpmpp", "dpm_steps": 20, "dpm_order": 2, "dpm_spacing": "logsnr"}
    assert cli_sampler_kwargs(parse_cli(["sampler=dpmpp", "dpm_order=3", "dpm_spacing=time", "chains_per_gpu=2"])) == \
        {"sampler": "dpmpp", "dpm_steps": None, "dpm_order": 3, "dpm_spacing": "time"}
    assert cli_sampler_kwargs(parse_cli(["exp_dir=/x"])) is None  # DDPM stays the default
    assert cli_sampler_kwargs(parse_cli(["sampler=ddim", "ddim_steps=50"])) == {"sampler": "ddim", "ddim_steps": 50, "eta": 0.0}
    for bad in (["dpm_steps=20"], ["dpm_order=3"], ["dpm_spacing=time"], ["sampler=ddim", "dpm_steps=20"],
                ["sampler=dpmpp", "ddim_steps=50"], ["sampler=dpmpp", "ddim_eta=1.0"], ["sampler=dpmpp", "dpm_order=4"],
                ["sampler=dpmpp", "dpm_spacing=karras"], ["sampler=dpmpp", "dpm_steps=0"], ["sampler=plms"]):
        with pytest.raises(SystemExit):
            parse_cli(bad)


def test_model_dpmpp_argument_checks():
    from holo_diffusion_amd.model import HoloDiffusionModel
    m = HoloDiffusionModel.__new__(HoloDiffusionModel)
    assert m._sampler_loop_kwargs("dpmpp", None, None, 0.0, {"noise": 1}, dpm_steps=7, dpm_order=3, dpm_spacing="time") == \
        {"noise": 1, "steps": 7, "order": 3, "spacing": "time", "timesteps": None}
    assert m._sampler_loop_kwargs("dpmpp", None, [9, 0], 0.0, {}) == \
        {"steps": None, "order": 2, "spacing": "logsnr", "timesteps": [9, 0]}
    for sampler in ("ddpm", "ddim"):
        for kw in (dict(dpm_steps=4), dict(dpm_order=3), dict(dpm_spacing="time")):
            with pytest.raises(ValueError):
                m._sampler_loop_kwargs(sampler, None, None, 0.0, {}, **kw)
    with pytest.raises(ValueError):
        m._sampler_loop_kwargs("dpmpp", 4, None, 0.0, {})  # ddim_steps
    with pytest.raises(ValueError):
        m._sampler_loop_kwargs("dpmpp", None, None, 0.5, {})  # eta
    with pytest.raises(ValueError):
        m._sampler_loop_kwargs("plms", None, None, 0.0, {})
