"""CPU: the host side of masked DDPM sampling - RePaint's jump schedule in level terms, the coefficient rows of the masked
step and of the forward jumps, the float32 restatements (tests/support/repaint_ref.py) against what they must reduce to, and
the refusals of the loop, which come before any device work."""
import math

import numpy as np
import pytest
import torch

import holo_diffusion_amd as hda
from oracle.common import np_noise
from tests.support import repaint_ref as rr
from tests.support.guided_ref import ddpm_guided_step

CASES = ((20, 5, 1), (20, 5, 3), (20, 7, 2), (1000, 10, 10))
bits = lambda a: np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a).view(np.uint32)  # noqa: E731


@pytest.mark.parametrize("T,j,r", CASES)
def test_repaint_schedule_properties(T, j, r):
    diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
    ops = diff.repaint_schedule(j, r)
    level, n_reverse = T, 0
    for op in ops:
        if op[0] == "reverse":
            assert op[1] == level - 1
            level -= 1
            n_reverse += 1
        else:
            assert op[0] == "forward" and op[1] == level and op[2] - op[1] == j
            level = op[2]
        assert 0 <= level <= T
    assert ops[-1] == ("reverse", 0) and level == 0
    assert n_reverse == T + (r - 1) * j * math.ceil((T - j) / j)
    left = {}
    for op in ops:
        if op[0] == "forward":
            left[op[1]] = left.get(op[1], 0) + 1
    assert left == ({L: r - 1 for L in range(0, T - j, j)} if r > 1 else {})
    if r == 1:
        assert [op[1] for op in ops] == diff._indices(None) and all(op[0] == "reverse" for op in ops)
    idx = [t + T * visit for t, visit, _ in rr.walk(ops, T)]
    assert len(set(idx)) == len(idx) == n_reverse and max(idx) < 2 ** 32


def test_repaint_schedule_start_level_and_refusals():
    diff = hda.ImplicitronGaussianDiffusion(num_steps=20)
    ops = diff.repaint_schedule(5, 2, start_level=12)
    assert ops[0] == ("reverse", 11) and ops[-1] == ("reverse", 0)
    level = 12
    for op in ops:
        level = level - 1 if op[0] == "reverse" else op[2]
        assert 0 <= level <= 12
    assert sorted(op[1] for op in ops if op[0] == "forward") == [0, 5]  # (10 -> 15 would leave the start level)
    assert diff.repaint_schedule(5, 1, start_level=3) == [("reverse", 2), ("reverse", 1), ("reverse", 0)]
    for kw, name in ((dict(jump_length=0), "jump_length"), (dict(n_resample=0), "n_resample"),
                     (dict(start_level=0), "start_level"), (dict(start_level=21), "start_level")):
        with pytest.raises(ValueError, match=name):
            diff.repaint_schedule(**kw)


def test_loop_refusals_name_the_argument():
    diff = hda.ImplicitronGaussianDiffusion(num_steps=20)
    shape = (2, 4, 4, 4, 4)
    known, mask = torch.zeros(shape), torch.zeros(2, 1, 4, 4, 4)
    model = lambda x, t: x  # noqa: E731
    loop = lambda **kw: diff.inpaint_sample_loop(model, shape, kw.pop("known", known), kw.pop("mask", mask),  # noqa: E731
                                                 device=torch.device("cpu"), **kw)
    for kw, name in ((dict(cond_fn=lambda x, t: x), "cond_fn"), (dict(max_iter=4), "max_iter"),
                     (dict(mask=torch.zeros(2, 4, 4, 4, 4)), "mask"), (dict(mask=torch.zeros(3, 1, 4, 4, 4)), "mask"),
                     (dict(mask=torch.zeros(1, 1, 4, 4, 2)), "mask"), (dict(jump_length=0), "jump_length"),
                     (dict(n_resample=0), "n_resample"), (dict(start_level=0), "start_level"),
                     (dict(start_level=21), "start_level"), (dict(known=torch.zeros(2, 3, 4, 4, 4)), "known")):
        with pytest.raises(ValueError, match=name):
            loop(**kw)


def test_coefficient_rows():
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    t = np.array([0, 1, 499, 500, 998, 999])
    rows = diff.known_coefs(t).numpy()
    assert rows.dtype == np.float32 and rows.shape == (6, 2)
    assert np.array_equal(rows[:, 0], np.sqrt(diff.alphas_cumprod_prev[t]).astype(np.float32))
    assert np.array_equal(rows[:, 1], np.sqrt(1.0 - diff.alphas_cumprod_prev[t]).astype(np.float32))
    assert rows[0, 0] == 1.0 and rows[0, 1] == 0.0
    # one level down: q_sample's own coefficients
    assert np.array_equal(rows[1:], diff.q_sample_coefs(t[1:] - 1).numpy())
    q = diff.q_sample_coefs(t).numpy()
    assert np.array_equal(q[:, 0], diff.sqrt_alphas_cumprod[t].astype(np.float32))
    assert np.array_equal(q[:, 1], diff.sqrt_one_minus_alphas_cumprod[t].astype(np.float32))
    # composed jumps: a^2 + b^2 = 1 to one float32 ulp; from level 0 the jump is q_sample at the target
    lo = np.array([0, 10, 500, 980, 1, 989])
    hi = np.array([10, 20, 510, 990, 1000, 999])
    j = diff.jump_coefs(lo, hi).numpy().astype(np.float64)
    assert np.all(np.abs(j[:, 0] ** 2 + j[:, 1] ** 2 - 1.0) <= 2.0 ** -23)
    abar = np.append(diff.alphas_cumprod, 1.0)
    assert np.array_equal(j[:, 0].astype(np.float32), np.sqrt(abar[hi - 1] / abar[lo - 1]).astype(np.float32))
    assert np.array_equal(diff.jump_coefs([0], [10]).numpy()[:, 0], diff.q_sample_coefs([9]).numpy()[:, 0])
    # ten single steps compose to the jump (in exact arithmetic; float64 here)
    a = np.prod(np.sqrt(1.0 - diff.betas[10:20]))
    assert abs(a - j[1, 0]) < 1e-7
    for bad in (([5], [5]), ([5], [1001]), ([-1], [3])):
        with pytest.raises(ValueError):
            diff.jump_coefs(*bad)


@pytest.mark.parametrize("shape", ((2, 8, 4, 4, 4), (1, 6, 4, 4, 4)))
def test_restatement_reduces_to_the_plain_step_and_to_q_sample(shape):
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    x, mo, known, nz, nzk = (torch.from_numpy(np_noise(s, shape)) for s in (1, 2, 6, 3, 7))
    mo = mo * 1.5
    mshape = (shape[0], 1) + shape[2:]
    zero, one = np.zeros(mshape, np.float32), np.ones(mshape, np.float32)
    for pair in ((999, 998), (500, 499), (1, 0), (0, 0)):
        t = np.array(pair[:shape[0]])
        c1, c2, sigma = rr.step_scalars(diff, t)
        ab = diff.known_coefs(t).numpy()
        for clip in (True, False):
            s0, p0 = rr.inpaint_step(x, mo, known, zero, nz, nzk, c1, c2, sigma, ab[:, 0], ab[:, 1], clip)
            ws, wp = ddpm_guided_step(x, mo, torch.zeros(shape), nz, c1, c2, np.zeros_like(c1), sigma, clip)
            assert np.array_equal(bits(s0), bits(ws)) and np.array_equal(bits(p0), bits(wp)), (pair, clip)
            s1, _ = rr.inpaint_step(x, mo, known, one, nz, nzk, c1, c2, sigma, ab[:, 0], ab[:, 1], clip)
            for b, tt in enumerate(t):
                want = known[b:b + 1] if tt == 0 else diff.q_sample(known[b:b + 1], torch.tensor([tt - 1]), nzk[b:b + 1])
                assert np.array_equal(bits(s1[b:b + 1]), bits(want)), (pair, clip, b)
    # q_lin on q_sample's rows is q_sample
    t = torch.tensor([700, 3][:shape[0]])
    ab = diff.q_sample_coefs(t.numpy()).numpy()
    assert np.array_equal(bits(rr.q_lin(ab[:, 0], known, ab[:, 1], nzk)), bits(diff.q_sample(known, t, nzk)))


def test_sampler_indices_of_a_chain_are_distinct():
    """The integers a masked chain hands its noise_sampler: pairwise distinct, distinct from x_T's (T), and a first visit's
    step noise asks for t, as p_sample_loop does."""
    T = 20
    diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
    for top in (20, 12):
        asked = [T] if top == T else [rr.sampler_index(T, top - 1, 0, 2)]
        for t, visit, jump in rr.walk(diff.repaint_schedule(5, 3, start_level=top), T):
            if jump is not None:
                asked.append(rr.sampler_index(T, jump[1] - 1, jump[2], 2))
            asked += [rr.sampler_index(T, t, visit, 0), rr.sampler_index(T, t, visit, 1)]
            if visit == 0:
                assert asked[-2] == t
        assert len(set(asked)) == len(asked)
