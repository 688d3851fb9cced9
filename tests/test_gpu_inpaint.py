"""GPU: masked DDPM sampling - the masked step kernels (holo_ddpm_step_inpaint and its Philox form), holo_q_sample*, the
masked loop with its resampling jumps, completion / editing through the model, and the frustum coverage kernel.  The kernels
are compared with what they are made of: the existing DDPM step kernel (pinned by its own tests) and ``q_sample`` on CPU
tensors, blended in numpy float32.  Under HOLO_TEST_EMU=1 (host emulation) the kernel cases run as they are, the loop cases
run on a cheap stand-in for the denoiser, and the cases that need the denoiser itself are skipped, as in test_gpu_guided.py."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle import viewpool_oracle as vo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.support import repaint_ref as rr  # noqa: E402

SHAPES = ((2, 8, 4, 4, 4), (2, 8, 8, 8, 8), (1, 6, 4, 4, 4))
PAIRS = ((999, 998), (500, 499), (1, 0), (0, 0))
TINY_UNET = dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2))
SEED = 0x1234567890ABCDEF
bits = lambda a: np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)  # noqa: E731
same = lambda a, b: np.array_equal(bits(a), bits(b))  # noqa: E731
cl = lambda a: a.permute(0, 2, 3, 4, 1).contiguous()  # noqa: E731
EMU_SKIP = pytest.mark.skipif(os.environ.get("HOLO_TEST_EMU") == "1", reason="the UNet legs are too slow for the host emulation")


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _inputs(shape, dev):
    """x, model output (scaled so that the clamp acts), known grid, the two noises: np_noise draws, computed once."""
    x, mo, kn, nz, nzk = (torch.from_numpy(np_noise(s, shape)) for s in (1, 2, 6, 3, 7))
    return x.to(dev), (mo * 1.5).to(dev), torch.tanh(kn).to(dev), nz.to(dev), nzk.to(dev)


def _masks(shape, dev):
    ms = (shape[0], 1) + tuple(shape[2:])
    u = torch.from_numpy(np_noise(9, ms))
    return {"zero": torch.zeros(ms, device=dev), "one": torch.ones(ms, device=dev), "binary": (u > 0).float().to(dev),
            "soft": (0.5 * (torch.tanh(u) + 1)).clamp(0, 1).to(dev)}


def _known_at(diff, known, t, noise_known):
    """The known part at each row's level t - 1 on CPU tensors: q_sample there, the grid itself at t = 0."""
    rows = [known[b:b + 1] if tt == 0 else diff.q_sample(known[b:b + 1], torch.tensor([tt - 1]), noise_known[b:b + 1])
            for b, tt in enumerate(t)]
    return torch.cat(rows).numpy()


def _blend(mask, known, unk):
    m = mask.cpu().numpy()
    out = m * known + (np.float32(1) - m) * unk
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_inpaint_step_with_injected_noise(gu, shape):
    """holo_ddpm_step_inpaint = numpy float32 blend of holo_ddpm_step's sample and q_sample(known, t - 1) on CPU, bit for bit,
    for four masks, four timestep pairs, clip on and off; an all-zero mask is the plain step, an all-one mask q_sample (the
    known grid at t = 0); pred_xstart and (at t = 0) the known part's noise may be null; the channels-last call agrees."""
    D = gu.DEV
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000)
    x, mo, known, nz, nzk = _inputs(shape, D)
    masks = _masks(shape, D)
    for pair in PAIRS:
        tl = list(pair[:shape[0]])
        t = torch.tensor(tl, device=D)
        coefs = diff.known_coefs(tl).to(D)
        kn_cpu = _known_at(diff, known.cpu(), tl, nzk.cpu())
        for clip in (True, False):
            s0, p0 = diff._step(x, t, mo, nz, clip)
            for name, m in masks.items():
                s, p = diff._step_inpaint(x, t, mo, known, m, coefs, nz, nzk, clip)
                assert same(s, _blend(m, kn_cpu, s0.cpu().numpy())) and same(p, p0), (pair, clip, name)
                if name == "zero":
                    assert same(s, s0), (pair, clip)
                if name == "one":
                    assert same(s, kn_cpu), (pair, clip)
                    if pair == (0, 0):
                        assert same(s, known)
            s2, p2 = diff._step_inpaint(x, t, mo, known, masks["soft"], coefs, nz, nzk, clip, want_pred=False)
            assert p2 is None and same(s2, diff._step_inpaint(x, t, mo, known, masks["soft"], coefs, nz, nzk, clip)[0])
            s3, p3 = diff._step_inpaint(cl(x), t, cl(mo), cl(known), masks["soft"], coefs, cl(nz), cl(nzk), clip,
                                        channels_last=True)
            assert same(s3, cl(s2)) and same(p3, cl(p0)), (pair, clip)
    # every row at t = 0: the known part's noise is not needed
    t = torch.tensor([0] * shape[0], device=D)
    coefs = diff.known_coefs([0] * shape[0]).to(D)
    a = diff._step_inpaint(x, t, mo, known, masks["soft"], coefs, nz, None, True)[0]
    assert same(a, diff._step_inpaint(x, t, mo, known, masks["soft"], coefs, nz, nzk, True)[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_inpaint_step_philox(gu, shape):
    """holo_ddpm_step_inpaint_philox: (1) all-zero mask - sample and noise_out are holo_ddpm_step_philox's / _rows' for the
    same seed, stream and index, with and without the noise outputs; (2) the sample is the injected-noise entry fed the two
    reported noises, also where the draws a mask makes useless are skipped; (3) channels-last and NCDHW inputs agree;
    (4) row b of a launch with per-row streams equals the batch-1 launch with that stream."""
    D = gu.DEV
    B = shape[0]
    streams = (5, 9)[:B]
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=3)
    rows = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=streams)
    ones = [hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=s) for s in streams]
    x, mo, known, _, _ = _inputs(shape, D)
    masks = _masks(shape, D)
    for tt in (999, 500, 1, 0):
        t = torch.tensor([tt] * B, device=D)
        coefs = diff.known_coefs([tt] * B).to(D)
        for d in (diff, rows):
            ws, wp, we = d._step_device_noise(x, t, mo, tt, True, want_noise=True)
            s, p, eu, ek = d._step_inpaint(x, t, mo, known, masks["zero"], coefs, None, None, True, timestep_index=tt,
                                           want_noise=True)
            assert same(s, ws) and same(p, wp) and same(eu, we), tt
            s, p, eu, ek = d._step_inpaint(x, t, mo, known, masks["zero"], coefs, None, None, True, timestep_index=tt)
            assert same(s, ws) and eu is None and ek is None, tt
        for name in ("soft", "binary", "one"):
            m = masks[name]
            s, p, eu, ek = diff._step_inpaint(x, t, mo, known, m, coefs, None, None, True, timestep_index=tt, want_noise=True)
            s2, p2 = diff._step_inpaint(x, t, mo, known, m, coefs, eu, ek, True)
            assert same(s, s2) and same(p, p2), (tt, name)
            s3 = diff._step_inpaint(x, t, mo, known, m, coefs, None, None, True, timestep_index=tt, want_pred=False)
            assert s3[1] is None and same(s3[0], s), (tt, name)  # (without the outputs: the skipped draws change nothing)
            c = diff._step_inpaint(cl(x), t, cl(mo), cl(known), m, coefs, None, None, True, channels_last=True,
                                   timestep_index=tt, want_noise=True)
            if shape[1] % 4 == 0:  # the draws are keyed on the logical element: the layouts agree
                assert same(c[0], cl(s)) and same(c[1], cl(p)) and same(c[2], cl(eu)) and same(c[3], cl(ek)), (tt, name)
            else:  # the memory order is the key: another draw, the same arithmetic on it
                c2 = diff._step_inpaint(cl(x), t, cl(mo), cl(known), m, coefs, c[2], c[3], True, channels_last=True)
                assert same(c[0], c2[0]) and same(c[1], cl(p)) and not same(c[2], cl(eu)), (tt, name)
        m = masks["soft"]
        sr, pr, ur, kr = rows._step_inpaint(x, t, mo, known, m, coefs, None, None, True, timestep_index=tt, want_noise=True)
        for b in range(B):
            r1 = slice(b, b + 1)
            sb, pb, ub, kb = ones[b]._step_inpaint(x[r1], t[r1], mo[r1], known[r1], m[r1], coefs[r1], None, None, True,
                                                   timestep_index=tt, want_noise=True)
            assert same(sr[r1], sb) and same(pr[r1], pb) and same(ur[r1], ub) and same(kr[r1], kb), (tt, b)


def _stats_ok(a, others, n):
    """Mean, variance and correlations of a draw at five standard deviations of the estimators over n elements."""
    a = a.double().flatten().cpu()
    assert a.numel() == n
    mean, var = a.mean().item(), a.var(unbiased=False).item()
    assert abs(mean) < 5 / math.sqrt(n), mean
    assert abs(var - 1) < 5 * math.sqrt(2 / n), var
    for o in others:
        o = o.double().flatten().cpu()
        corr = (((a - a.mean()) * (o - o.mean())).mean() / (a.std(unbiased=False) * o.std(unbiased=False))).item()
        assert abs(corr) < 5 / math.sqrt(n), corr


def test_draw_domains_are_standard_normal_and_uncorrelated(gu):
    """Over the 8192 elements of the 8^3 shape: the known part's noise and holo_q_sample_philox's noise are standard normal,
    uncorrelated with the step's noise, with each other, and with their own draw at the next visit of the timestep."""
    D = gu.DEV
    shape, T, tt = SHAPES[1], 1000, 500
    n = int(np.prod(shape))
    assert n == 8192
    diff = hda.ImplicitronGaussianDiffusion(num_steps=T, device_noise_seed=SEED, device_noise_stream=3)
    x, mo, known, _, _ = _inputs(shape, D)
    m = _masks(shape, D)["soft"]
    t = torch.tensor([tt, tt], device=D)
    coefs = diff.known_coefs([tt, tt]).to(D)
    draw = lambda idx: diff._step_inpaint(x, t, mo, known, m, coefs, None, None, True, timestep_index=idx,  # noqa: E731
                                          want_noise=True)[2:]
    eu0, ek0 = draw(tt)
    eu1, ek1 = draw(tt + T)
    qrow = diff.q_sample_coefs([tt, tt]).to(D)
    eq0 = diff._q_sample_rows(x, qrow, timestep_index=tt, want_noise=True)[1]
    eq1 = diff._q_sample_rows(x, qrow, timestep_index=tt + T, want_noise=True)[1]
    _stats_ok(ek0, (eu0, ek1), n)
    _stats_ok(eq0, (eu0, ek0, eq1), n)
    _stats_ok(eu1, (eu0,), n)  # (a revisit's step noise is fresh too)


@pytest.mark.parametrize("shape", SHAPES)
def test_q_sample_kernels(gu, shape):
    """holo_q_sample on q_sample's rows is ``q_sample`` on CPU tensors, bit for bit; on the composed jump rows it is a*x + b*e
    as stated; the Philox form is the injected form fed the noise it reports, the same in both layouts and per row."""
    D = gu.DEV
    B = shape[0]
    streams = (5, 9)[:B]
    diff = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=3)
    rows = hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=streams)
    ones = [hda.ImplicitronGaussianDiffusion(num_steps=1000, device_noise_seed=SEED, device_noise_stream=s) for s in streams]
    x, _, _, nz, _ = _inputs(shape, D)
    for pair in PAIRS:
        tl = list(pair[:B])
        got = diff._q_sample_rows(x, diff.q_sample_coefs(tl).to(D), nz)
        assert same(got, diff.q_sample(x.cpu(), torch.tensor(tl), nz.cpu())), pair
    for lo, hi in (((0, 10)[:B], (10, 20)[:B]), ((500, 989)[:B], (510, 999)[:B]), ((990, 3)[:B], (1000, 700)[:B])):
        j = diff.jump_coefs(lo, hi)
        got = diff._q_sample_rows(x, j.to(D), nz)
        assert same(got, rr.q_lin(j[:, 0].numpy(), x, j[:, 1].numpy(), nz)), (lo, hi)
    q = diff.q_sample_coefs([500] * B).to(D)
    out, e = diff._q_sample_rows(x, q, timestep_index=500, want_noise=True)
    assert same(out, diff._q_sample_rows(x, q, e)) and same(diff._q_sample_rows(x, q, timestep_index=500)[0], out)
    oc, ec = diff._q_sample_rows(cl(x), q, channels_last=True, timestep_index=500, want_noise=True)
    if shape[1] % 4 == 0:
        assert same(oc, cl(out)) and same(ec, cl(e))
    else:  # (the memory order is the key)
        assert same(oc, diff._q_sample_rows(cl(x), q, ec))
    orow, erow = rows._q_sample_rows(x, q, timestep_index=500, want_noise=True)
    for b in range(B):
        ob, eb = ones[b]._q_sample_rows(x[b:b + 1], q[b:b + 1], timestep_index=500, want_noise=True)
        assert same(orow[b:b + 1], ob) and same(erow[b:b + 1], eb), b


# ---- the loop --------------------------------------------------------------------------------------------------------
class _StandIn:
    """HOLO_TEST_EMU=1 only: a denoiser-shaped callable for the loop plumbing (the loops only need model(x, t))."""

    def __call__(self, x, t, **kw):
        return torch.tanh(x) * (1.0 + 1e-4 * t.float().reshape(-1, 1, 1, 1, 1))


@pytest.fixture(scope="module")
def tiny_net(gu):
    if gu.EMU:
        return _StandIn()
    cfg = uo.UNetCfg(image_size=8, in_channels=8, out_channels=8, model_channels=32, num_res_blocks=2, channel_mult=(1, 2),
                     attention_resolutions=(1, 2), num_heads=2)
    return gu.make_unet(cfg)[0]


class Recording:
    """The denoiser behind a callable that writes down every output (and so counts the calls)."""

    def __init__(self, net):
        self.net, self.outputs = net, []

    def __call__(self, x, t, **kw):
        self.outputs.append(self.net(x, t))
        return self.outputs[-1]


LOOP_SHAPE = (2, 8, 8, 8, 8)


def _noise_by_index(dev):
    return lambda i, shp, device=None: torch.from_numpy(np_noise(8000 + int(i), tuple(shp))).to(dev)


def _half_mask(dev, batch=1):
    m = torch.zeros(batch, 1, 8, 8, 8, device=dev)
    m[:, :, :, :, :4] = 1
    return m


def _device_sigma(diff, t, dev):
    """[t != 0] * exp(0.5 * log variance) as the DDPM kernels form it, read off the existing step kernel (x = model output =
    0, noise = 1: sample = fma(sigma, 1, 0) = sigma).  The device's expf and numpy's float32 exp may differ in the last bit;
    on the 20-step schedule sigma * noise reaches 4, where that bit is 2.4e-7 - more than the tolerance below where the step's
    terms cancel.  The restatement is about the arithmetic around sigma, so it takes the kernel's own."""
    z = torch.zeros(len(t), 4, device=dev)
    return diff._step(z, torch.tensor(t, device=dev), z, torch.ones_like(z), False)[0][:, 0].cpu().numpy()


def test_masked_loop_walks_the_schedule(gu, tiny_net):
    """num_steps = 20, (j, r) = (5, 2), injected noise: one denoiser call per reverse operation of the schedule; each yielded
    sample is the restatement's step (a jump in front of it restated too) of the previous one within the fused DDPM update's
    tolerance (test_step_kernel_bit_exact_vs_oracle: rtol 3e-7, atol 1e-7); the last sample is the known grid, bit for bit,
    where the mask is 1."""
    D = gu.DEV
    T = 20
    diff = hda.ImplicitronGaussianDiffusion(num_steps=T)
    ns = _noise_by_index(D)
    x_T = torch.from_numpy(np_noise(4243, LOOP_SHAPE)).to(D)
    known = torch.tanh(torch.from_numpy(np_noise(6, (1,) + LOOP_SHAPE[1:]))).to(D)
    mask = _half_mask(D)
    rec = Recording(tiny_net)
    outs = list(diff.inpaint_sample_loop_progressive(rec, LOOP_SHAPE, known, mask, jump_length=5, n_resample=2, noise=x_T,
                                                     device=D, noise_sampler=ns))
    steps = rr.walk(diff.repaint_schedule(5, 2), T)
    assert len(rec.outputs) == len(outs) == len(steps) == 20 + 5 * 3
    assert sum(1 for s in steps if s[2] is not None) == 3
    kn, mk = known.expand(LOOP_SHAPE).cpu(), mask.expand(2, -1, -1, -1, -1).cpu()
    prev = x_T.cpu().numpy()
    for (t, visit, jump), out, mo in zip(steps, outs, rec.outputs):
        assert set(out) == {"sample", "pred_xstart", "noise"}
        if jump is not None:
            j = diff.jump_coefs([jump[0]] * 2, [jump[1]] * 2).numpy()
            prev = rr.q_lin(j[:, 0], prev, j[:, 1], ns(rr.sampler_index(T, jump[1] - 1, jump[2], 2), LOOP_SHAPE).cpu())
        c1, c2, _ = rr.step_scalars(diff, [t, t])
        sigma = _device_sigma(diff, [t, t], D)
        ab = diff.known_coefs([t, t]).numpy()
        e_u = ns(rr.sampler_index(T, t, visit, 0), LOOP_SHAPE).cpu()
        e_k = ns(rr.sampler_index(T, t, visit, 1), LOOP_SHAPE).cpu() if t != 0 else None
        assert torch.equal(out["noise"].cpu(), e_u)
        want, wpred = rr.inpaint_step(prev, mo.cpu(), kn, mk, e_u, e_k, c1, c2, sigma, ab[:, 0], ab[:, 1], True)
        torch.testing.assert_close(out["sample"].cpu(), torch.from_numpy(want), rtol=3e-7, atol=1e-7)
        assert same(out["pred_xstart"], wpred)
        prev = out["sample"].cpu().numpy()
    final = outs[-1]["sample"].cpu()
    keep = mk.expand(LOOP_SHAPE) == 1
    assert same(final[keep], kn[keep]) and not torch.equal(final[~keep], kn[~keep])
    assert same(diff.inpaint_sample_loop(tiny_net, LOOP_SHAPE, known, mask, jump_length=5, n_resample=2, noise=x_T, device=D,
                                         noise_sampler=ns), final)


def test_unmasked_loop_is_p_sample_loop(gu, tiny_net):
    """r = 1 with an all-zero mask is p_sample_loop bit for bit: with an injected noise sampler, and in perf mode (in-kernel
    noise; the denoiser's channels-last chain on the GPU), single stream and per-row streams."""
    D = gu.DEV
    x_T = torch.from_numpy(np_noise(4243, LOOP_SHAPE)).to(D)
    known = torch.tanh(torch.from_numpy(np_noise(6, LOOP_SHAPE))).to(D)
    zero = torch.zeros(1, 1, 8, 8, 8, device=D)
    ns = _noise_by_index(D)
    diff = hda.ImplicitronGaussianDiffusion(num_steps=20)
    want = diff.p_sample_loop(tiny_net, LOOP_SHAPE, noise=x_T, device=D, noise_sampler=ns)
    assert same(diff.inpaint_sample_loop(tiny_net, LOOP_SHAPE, known, zero, noise=x_T, device=D, noise_sampler=ns), want)
    for stream in (3, (4, 6)):
        perf = hda.ImplicitronGaussianDiffusion(num_steps=20, device_noise_seed=77, device_noise_stream=stream)
        want = perf.p_sample_loop(tiny_net, LOOP_SHAPE, noise=x_T, device=D)
        got = perf.inpaint_sample_loop(tiny_net, LOOP_SHAPE, known, zero, noise=x_T, device=D)
        assert same(got, want), stream
        # jumps in perf mode: finite, and the kept half survives the channels-last chain
        got = perf.inpaint_sample_loop(tiny_net, LOOP_SHAPE, known, _half_mask(D), jump_length=5, n_resample=2, noise=x_T, device=D)
        assert torch.isfinite(got).all() and same(got[..., :4], known[..., :4]) and not torch.equal(got[..., 4:], known[..., 4:])


# ---- the model -------------------------------------------------------------------------------------------------------
R, C, HW = 8, 16, 16


@pytest.fixture(scope="module")
def model(gu):
    m, *_ = gu.make_model(R, C, HW, HW, TINY_UNET, diffusion_args=dict(num_steps=20, device_noise_seed=11))
    return m


@EMU_SKIP
def test_complete_voxel_features(gu, model):
    """Half-grid mask, in-kernel noise: finite; the kept half is the known grid bit for bit and the generated half is not; two
    runs agree bit for bit; a batch of two chains on streams (4, 6) equals the two batch-1 chains."""
    D = gu.DEV
    known = torch.tanh(torch.from_numpy(np_noise(6, (1, C, R, R, R)))).to(D)
    mask = _half_mask(D)
    x_T = torch.from_numpy(np_noise(4243, (2, C, R, R, R))).to(D)
    diff = model.diffusion
    a = model.complete_voxel_features(known, mask, jump_length=5, n_resample=2, noise=x_T[:1])
    assert a.shape == (1, C, R, R, R) and a.is_contiguous() and torch.isfinite(a).all()
    assert same(a[..., :4], known[..., :4]) and not torch.equal(a[..., 4:], known[..., 4:])
    assert same(model.complete_voxel_features(known, mask, jump_length=5, n_resample=2, noise=x_T[:1]), a)
    net = model.net_3d
    net.set_batch_invariant(True)
    try:
        diff.device_noise_stream = (4, 6)
        both = model.complete_voxel_features(known, mask, jump_length=5, n_resample=2, noise=x_T, batch_size=2)
        assert both.shape == (2, C, R, R, R)
        for b, s in enumerate((4, 6)):
            diff.device_noise_stream = s
            one = model.complete_voxel_features(known, mask, jump_length=5, n_resample=2, noise=x_T[b:b + 1])
            assert same(both[b:b + 1], one), b
    finally:
        diff.device_noise_stream = 0
        net.set_batch_invariant(False)


@EMU_SKIP
def test_edit_voxel_features(gu, model):
    """strength = 1.0 starts from noise: the input grid's values outside the mask play no part in the generated part; a call
    makes start_level = clamp(round(strength * T), 1, T) denoiser calls; mask None regenerates everything."""
    D = gu.DEV
    grid = torch.tanh(torch.from_numpy(np_noise(6, (1, C, R, R, R)))).to(D)
    mask = _half_mask(D)
    x_T = torch.from_numpy(np_noise(4243, (1, C, R, R, R))).to(D)
    a = model.edit_voxel_features(grid, 1.0, mask=mask, noise=x_T)
    other = grid.clone()
    other[..., 4:] = torch.tanh(torch.from_numpy(np_noise(12, (1, C, R, R, 4)))).to(D)
    b = model.edit_voxel_features(other, 1.0, mask=mask, noise=x_T)
    assert same(a[..., :4], grid[..., :4]) and same(b[..., 4:], a[..., 4:])
    calls = []
    net = model.net_3d
    hook = net.register_forward_pre_hook(lambda mod, args: calls.append(1))
    inner = net.forward_channels_last  # (the perf chain calls the channels-last forward directly)
    net.forward_channels_last = lambda x, t: (calls.append(1), inner(x, t))[1]
    try:
        for strength, want in ((0.5, 10), (0.26, 5), (0.0, 1), (1.0, 20)):
            del calls[:]
            out = model.edit_voxel_features(grid, strength, mask=mask)
            assert len(calls) == want and same(out[..., :4], grid[..., :4]), strength
        free = model.edit_voxel_features(grid, 0.25)
        assert torch.isfinite(free).all() and not torch.equal(free[..., :4], grid[..., :4])
    finally:
        hook.remove()
        del net.forward_channels_last


# ---- coverage --------------------------------------------------------------------------------------------------------
def _coverage_cameras(kind):
    """(cameras, per-view (H, W)) of a coverage case.  The grid spans +-3.5 (extent 8, R = 8) / +-3.67 (R = 12)."""
    if kind == "one_view":  # a narrow frustum from outside the volume
        cams = hda.get_simple_360_camera_trajectory(2 * math.pi, 1, -0.5, 10, (0.0, -1.0, 0.0), 3.2)
        return cams, [(16, 16)]
    if kind == "three_views_non_square":  # a non-square map: the long axis is divided by the aspect ratio
        cams = hda.get_simple_360_camera_trajectory(2 * math.pi, 3, -0.5, 9, (0.0, -1.0, 0.0), 4.5)
        return cams, [(12, 20), (16, 16), (20, 12)]
    if kind == "off_axis":  # principal point off the centre, two different focal lengths
        base = hda.get_simple_360_camera_trajectory(2 * math.pi, 3, -0.3, 9, (0.0, -1.0, 0.0), 3.0)
        cams = hda.PerspectiveCameras(R=base.R, T=base.T, focal_length=torch.tensor([[3.0, 3.6]]).expand(3, 2),
                                      principal_point=torch.tensor([[0.3, -0.2], [0.0, 0.0], [-0.25, 0.1]]))
        return cams, [(16, 16)] * 3
    assert kind == "inside"  # a camera inside the volume: some voxels lie behind it or within projection_eps of its plane
    Rm, Tm = hda.look_at_view_transform(dist=1.3, elev=20.0, azim=30.0, up=((0.0, -1.0, 0.0),))
    return hda.PerspectiveCameras(R=Rm, T=Tm, focal_length=torch.tensor([[1.1]]), principal_point=torch.zeros(1, 2)), [(16, 24)]


def _coverage_f64(cams, sizes, resol, extent, eps=1e-2):
    """(count of seeing views, voxels too close to a boundary to call, (voxel, view) pairs with z <= eps) from the oracle's coord_grid / project_ndc and the g of
    ndc_grid_sample, in float64."""
    pts = vo.coord_grid(resol, extent, torch.float64)
    count = torch.zeros(pts.shape[0], dtype=torch.float64)
    unsure = torch.zeros(pts.shape[0], dtype=torch.bool)
    behind = 0
    Rc, Tc, fc, pc = (t.double() for t in cams.host())
    for v, (H, W) in enumerate(sizes):
        z = (pts @ Rc[v] + Tc[v][None])[:, 2]
        g = -vo.project_ndc(pts, Rc[v], Tc[v], fc[v], pc[v], eps)
        if W >= H:
            g[:, 0] = g[:, 0] / (W / H)
        else:
            g[:, 1] = g[:, 1] / (H / W)
        edge = g.abs().max(dim=1).values
        count += ((z > eps) & (edge <= 1)).double()
        unsure |= ((edge - 1).abs() < 1e-4) | ((z - eps).abs() < 1e-4)
        behind += int((z <= eps).sum())
    return count.reshape(1, 1, resol, resol, resol), unsure.reshape(1, 1, resol, resol, resol), behind


@pytest.mark.parametrize("kind,resol", (("one_view", 8), ("three_views_non_square", 12), ("off_axis", 8), ("inside", 12)))
def test_view_coverage(gu, kind, resol):
    """holo_view_coverage against the float64 evaluation of the oracle's projection: equal exactly, except voxels within 1e-4
    of a frustum boundary in float64 (at most 1 % of a case); every case has at least 10 % seen and 10 % unseen voxels."""
    cams, sizes = _coverage_cameras(kind)
    got = hda.view_coverage(cams.to(gu.DEV), sizes, resol, 8.0, device=gu.DEV)
    want, unsure, behind = _coverage_f64(cams, sizes, resol, 8.0)
    assert (behind > 0) == (kind == "inside")  # (only that camera has voxels at or behind its projection_eps plane)
    assert got.shape == (1, 1, resol, resol, resol) and got.dtype == torch.float32
    seen = (want > 0).double().mean().item()
    print(f"{kind}: {seen:.3f} seen, {unsure.double().mean().item():.4f} left out, max count {int(want.max())}")
    assert unsure.double().mean().item() <= 0.01
    assert 0.1 <= seen <= 0.9
    assert torch.equal(got.cpu().double()[~unsure], want[~unsure])
    if len(sizes) > 1 and len(set(sizes)) == 1:  # one size for all views
        assert torch.equal(hda.view_coverage(cams.to(gu.DEV), sizes[0], resol, 8.0, device=gu.DEV), got)


@EMU_SKIP
def test_reconstruct_from_views(gu):
    """known = pool_views_to_voxel_features, mask = coverage >= min_views, voxel_features = complete_voxel_features(known,
    mask) under the same seed - each bit for bit."""
    D = gu.DEV
    m = hda.HoloDiffusionModel(resol=R, feature_size=C, render_image_width=HW, render_image_height=HW,
                               net_3d_SimpleUnet3D_args=TINY_UNET, diffusion_args=dict(num_steps=20, device_noise_seed=11),
                               view_pooler_enabled=True)
    src, *_ = gu.make_model(R, C, HW, HW, TINY_UNET)
    m.load_state_dict(src.state_dict(), strict=False)
    m = m.to(D)
    cams = hda.get_simple_360_camera_trajectory(2 * math.pi, 3, -0.5, 9, (0.0, -1.0, 0.0), 3.6).to(D)
    feats = {"a": torch.from_numpy(np_noise(31, (3, 5, 12, 20))).to(D)}
    torch.manual_seed(5)
    pm = m.pool_views_to_voxel_features(feats, cams)  # (materialises the mapper)
    x_T = torch.from_numpy(np_noise(4243, (1, C, R, R, R))).to(D)
    for min_views in (1, 2):
        out = m.reconstruct_from_views(feats, cams, min_views=min_views, noise=x_T)
        assert set(out) == {"voxel_features", "known", "mask", "coverage"}
        cov = hda.view_coverage(cams, (12, 20), R, m.volume_extent, device=D)
        assert same(out["known"], pm) and same(out["coverage"], cov) and same(out["mask"], (cov >= min_views).float())
        assert 0 < out["mask"].mean().item() < 1
        assert same(out["voxel_features"], m.complete_voxel_features(pm, out["mask"], noise=x_T))
        keep = out["mask"].expand_as(pm) == 1
        assert same(out["voxel_features"][keep], pm[keep])
