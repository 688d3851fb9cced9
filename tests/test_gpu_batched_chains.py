"""GPU: batched sampling chains.  Several chains share one UNet call per step, and every row stays bit-equal to its chain
run alone: the per-row Philox step kernels (holo_ddpm_step_philox_rows / holo_ddim_step_philox_rows), the batch-invariant
forward plan (holo_unet_set_batch_invariant), the sampler's per-row streams and generate_samples(chains_per_gpu=B).
The small cases also run under HOLO_TEST_EMU=1 (host emulation of the kernels)."""
import re
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib, runtime  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import NORTH_CFG, TINY_CFG, np_noise, seeded_input  # noqa: E402

TINY_UNET = dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2))
# 16^3: its 8^3 level runs split-K convolutions and a key-split attention (T = 512); 32 channels at both ends keep the first
# and last convolution un-split at batch 1 (split-K ends: forward_channels_last in test_gpu_unet_grid_sizes.py)
MID_CFG = uo.UNetCfg(image_size=16, in_channels=32, out_channels=32, model_channels=32, num_res_blocks=1,
                     channel_mult=(1, 2), attention_resolutions=(2,), num_heads=2)
STREAMS = [5, 0, 9]


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


def _unet_cases(gu):
    return [TINY_CFG] if gu.EMU else [TINY_CFG, MID_CFG, NORTH_CFG]


# ---- 1. the per-row Philox step kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
def test_rows_step_kernels_match_batch1_launches(gu, channels_last):
    """Streams [5, 0, 9] in one launch: each row's sample, pred_xstart and noise equal a batch-1 holo_ddpm_step_philox /
    holo_ddim_step_philox launch on that row with stream_offset = (stream << 32) | timestep, bit for bit, in both layouts."""
    seed = 0x0123456789ABCDEF
    shape = (3, 8, 8, 8, 8)
    x, mo = (torch.from_numpy(np_noise(s, shape)).to(gu.DEV) for s in (31, 32))
    mo = mo * 1.5
    if channels_last:
        x, mo = (a.permute(0, 2, 3, 4, 1).contiguous() for a in (x, mo))
    batched = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=list(STREAMS))
    for ti, ts in ((999, [999, 500, 1]), (0, [0, 0, 0]), (417, [417, 3, 0])):
        t = torch.tensor(ts, device=gu.DEV)
        got = batched._step_device_noise(x, t, mo, ti, True, want_noise=True, channels_last=channels_last)
        coefs = batched.ddim_coefs(ts, [v - 1 for v in ts], 1.0).to(gu.DEV)
        got_ddim = batched._ddim_step_device_noise(x, mo, coefs, ti, True, want_noise=True, channels_last=channels_last)
        for b, s in enumerate(STREAMS):
            alone = hda.ImplicitronGaussianDiffusion(device_noise_seed=seed, device_noise_stream=s)
            r = slice(b, b + 1)
            want = alone._step_device_noise(x[r], t[r], mo[r], ti, True, want_noise=True, channels_last=channels_last)
            for g_, w_ in zip(got, want):
                assert torch.equal(g_[r], w_), (ti, b)
            want_ddim = alone._ddim_step_device_noise(x[r], mo[r], coefs[r], ti, True, want_noise=True,
                                                      channels_last=channels_last)
            for g_, w_ in zip(got_ddim, want_ddim):
                assert torch.equal(g_[r], w_), (ti, b)
        assert not torch.equal(got[2][0], got[2][2])  # (distinct streams draw distinct noise)
    # optional outputs stay optional; a stream list of the wrong length is an error
    t5 = torch.tensor([5, 5, 5], device=gu.DEV)
    s, p, e = batched._step_device_noise(x, t5, mo, 5, True, want_pred=False, channels_last=channels_last)
    assert p is None and e is None
    assert torch.equal(s, batched._step_device_noise(x, t5, mo, 5, True, channels_last=channels_last)[0])
    with pytest.raises(ValueError):
        batched._step_device_noise(x[:2], t5[:2], mo[:2], 5, True)


def test_rows_entries_reject_null_streams(gu):
    L = runtime.lib()
    rc = L.holo_ddpm_step_philox_rows(None, None, 1000, None, 1, 4, None, None, 1, None, 0, 1, None, None, None, 0, None)
    assert rc < 0 and b"null" in L.holo_last_error()
    rc = L.holo_ddim_step_philox_rows(None, None, 1, 4, None, None, 1, None, 0, 1, None, None, None, 0, None)
    assert rc < 0 and b"null" in L.holo_last_error()


# ---- 2. the batch-invariant forward plan ------------------------------------------------------------------------------
def _rows_vs_batch1(net, xs, ts, channels_last):
    fwd = net.forward_channels_last if channels_last else net
    prep = (lambda a: a.permute(0, 2, 3, 4, 1).contiguous()) if channels_last else (lambda a: a)
    yb = fwd(prep(xs), ts)
    return [torch.equal(yb[b:b + 1], fwd(prep(xs[b:b + 1]), ts[b:b + 1])) for b in range(xs.shape[0])]


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_batch_invariant_forward_rows_equal_batch1(gu, idx):
    """B = 3 with per-row timesteps: with the flag on, every row of forward and forward_channels_last is bit-equal to its
    batch-1 forward; with the flag on, the batch-1 output is the flag-off output bit for bit."""
    cases = _unet_cases(gu)
    if idx >= len(cases):
        pytest.skip("the 16^3 and north-star nets run on the GPU only (host emulation: too slow)")
    cfg = cases[idx]
    net, _ = gu.make_unet(cfg)
    xs = torch.cat([seeded_input(cfg, 40 + b) for b in range(3)]).to(gu.DEV)
    ts = torch.tensor([999, 500, 3], device=gu.DEV)
    y1_off = net(xs[:1], ts[:1])
    y1_off_cl = net.forward_channels_last(xs[:1].permute(0, 2, 3, 4, 1).contiguous(), ts[:1])
    net.set_batch_invariant(True)
    assert net.batch_invariant
    assert torch.equal(net(xs[:1], ts[:1]), y1_off)
    assert torch.equal(net.forward_channels_last(xs[:1].permute(0, 2, 3, 4, 1).contiguous(), ts[:1]), y1_off_cl)
    for cl in (False, True):
        assert all(_rows_vs_batch1(net, xs, ts, cl)), (cfg, cl)
    net.set_batch_invariant(False)
    assert torch.equal(net(xs[:1], ts[:1]), y1_off)


def _plan_lines(text):
    """HOLO_DEBUG_PLAN lines with the batch-dependent parts (batch, grid, scratch) taken out."""
    out = set()
    for ln in text.splitlines():
        if not ln.startswith("[plan]"):
            continue
        ln = re.sub(r"batch \d+", "batch -", ln)
        ln = re.sub(r"grid_x \d+", "grid_x -", ln)
        out.add(re.sub(r"scratch \d+ bytes", "scratch -", ln))
    return out


def test_batch_invariant_plan_lines_match_batch1(gu, capfd, monkeypatch):
    """HOLO_DEBUG_PLAN: at batch 3 with the flag on every convolution and attention shows the kernel, tile depth, split-K
    and key splits of batch 1; with the flag off the batch-3 plan of this net differs (it fills the chip differently)."""
    monkeypatch.setenv("HOLO_DEBUG_PLAN", "1")
    cfg = TINY_CFG if gu.EMU else MID_CFG
    net, _ = gu.make_unet(cfg)
    xs = torch.cat([seeded_input(cfg, 50 + b) for b in range(3)]).to(gu.DEV)
    ts = torch.tensor([10, 20, 30], device=gu.DEV)
    capfd.readouterr()
    net(xs[:1], ts[:1])
    one = _plan_lines(capfd.readouterr().err)
    net(xs, ts)
    free = _plan_lines(capfd.readouterr().err)
    net.set_batch_invariant(True)
    net(xs, ts)
    inv = _plan_lines(capfd.readouterr().err)
    assert one and inv == one
    if not gu.EMU:  # (the emulated 4-CU "chip" is filled at batch 1 already)
        assert free != one  # (else this net would not exercise the invariant plan)


def test_batch_invariant_refused_in_bf16_modes(gu):
    """The flag is exact-fp32 only: SimpleUnet3D refuses it for the bf16 modes, and the library refuses a bf16 mode while
    the flag is on (HOLO_E_UNSUPPORTED)."""
    net, _ = gu.make_unet(TINY_CFG, compute_dtype="bf16")
    with pytest.raises(_lib.HoloError, match="exact-fp32"):
        net.set_batch_invariant(True)
    net32, _ = gu.make_unet(TINY_CFG)
    x = seeded_input(TINY_CFG, 1).to(gu.DEV)
    net32(x, torch.tensor([1], device=gu.DEV))
    net32.set_batch_invariant(True)
    net32.compute_dtype = "bf16"
    with pytest.raises(_lib.HoloError, match="exact-fp32"):
        net32(x, torch.tensor([1], device=gu.DEV))


# ---- 3. batched chains ------------------------------------------------------------------------------------------------
CHAINS = [0, 2, 4, 6]
SEED = 11


def _chain_setup(gu):
    cfg = TINY_CFG if gu.EMU else NORTH_CFG
    net, _ = gu.make_unet(cfg)
    shape1 = (1, cfg.in_channels) + (cfg.image_size,) * 3
    gens = [torch.Generator(device=gu.DEV).manual_seed(SEED + i) for i in CHAINS]
    x_T = torch.cat([torch.randn(shape1, generator=g, device=gu.DEV) for g in gens])
    return net, shape1, x_T


def _loop(diff, sampler, net, shape, x_T, **kw):
    if sampler == "ddpm":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the subsampling notice of max_iter)
            return diff.p_sample_loop(net, shape, noise=x_T, max_iter=4, **kw)
    return diff.ddim_sample_loop(net, shape, noise=x_T, eta=1.0, ddim_steps=4, **kw)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_device_noise_chains_rows_equal_chains_alone(gu, sampler):
    """North-star net (host emulation: the tiny one), 4 steps, chains {0, 2, 4, 6} in one batch with per-row Philox
    streams and a batch-invariant net: every row is bit-equal to that chain run alone at batch 1 (flag off)."""
    net, shape1, x_T = _chain_setup(gu)
    diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=SEED, device_noise_stream=list(CHAINS))
    net.set_batch_invariant(True)
    batched = _loop(diff, sampler, net, (len(CHAINS),) + shape1[1:], x_T)
    net.set_batch_invariant(False)
    for b, i in enumerate(CHAINS):
        alone_diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=SEED, device_noise_stream=i)
        alone = _loop(alone_diff, sampler, net, shape1, x_T[b:b + 1].clone())
        assert torch.equal(batched[b:b + 1], alone), (sampler, i)


def test_torch_noise_chains_rows_equal_chains_alone(gu):
    """The default torch-noise mode: each row's step noise from its chain's own generator (seed + i) equals the
    randn_like sequence of the batch-1 chain after torch.manual_seed(seed + i); rows bit-equal to the chains alone."""
    net, shape1, x_T = _chain_setup(gu)
    gens = [torch.Generator(device=gu.DEV).manual_seed(SEED + i) for i in CHAINS]
    for g in gens:  # (past the x_T draw, as in _chain_setup)
        torch.randn(shape1, generator=g, device=gu.DEV)
    ns = lambda t, shape, dev: torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=dev)  # noqa: E731
                                          for g in gens])
    diff = hda.ImplicitronGaussianDiffusion()
    net.set_batch_invariant(True)
    batched = _loop(diff, "ddpm", net, (len(CHAINS),) + shape1[1:], x_T, noise_sampler=ns)
    net.set_batch_invariant(False)
    for b, i in enumerate(CHAINS):
        torch.manual_seed(SEED + i)
        x = torch.randn(shape1, device=gu.DEV)
        assert torch.equal(x, x_T[b:b + 1])  # a fresh generator reproduces torch.manual_seed on this build
        alone = _loop(diff, "ddpm", net, shape1, x)
        assert torch.equal(batched[b:b + 1], alone), i


# ---- 4. the product driver --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_noise", [False, True])
def test_generate_samples_chains_per_gpu_bit_equal(gu, device_noise):
    """generate_samples(num_samples=3, chains_per_gpu=2) - groups [0, 1] and [2] - gives the images, depths and masks of
    chains_per_gpu=1 bit for bit, and leaves the net's flag and the sampler's noise settings as they were."""
    from holo_diffusion_amd.generate import generate_samples
    model, *_ = gu.make_model(8, 32, 8, 12, TINY_UNET)
    kw = dict(num_samples=3, n_eval_cameras=2, seed=5, device=gu.DEV, sampler_kwargs={"max_iter": 3},
              device_noise=device_noise)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = generate_samples(model, chains_per_gpu=1, **kw)
        two = generate_samples(model, chains_per_gpu=2, **kw)
    for k in ("images_render", "depths_render", "masks_render"):
        assert torch.equal(one[k], two[k]), k
    assert not model.net_3d.batch_invariant
    assert model.diffusion.device_noise_seed is None and model.diffusion.device_noise_stream == 0
