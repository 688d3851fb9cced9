"""GPU: DPM-Solver++ through ImplicitronGaussianDiffusion (holo_dpm_step) against the float32 restatement of the kernel's
rounding order (tests/support/dpm_ref.py): single steps, chains on the tiny UNet in both layouts, the order-1 chain against
DDIM, batched chains and the product drivers.  Everything here also runs under HOLO_TEST_EMU=1 (host emulation)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd import _lib  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from tests.support import dpm_ref  # noqa: E402
from tests.test_gpu_ddim import TINY_UNET  # noqa: E402

# image_size 8, 8 channels, the widths of TINY_UNET
TINY8_CFG = uo.UNetCfg(image_size=8, in_channels=8, out_channels=8, model_channels=TINY_UNET["model_channels"],
                       num_res_blocks=2, channel_mult=TINY_UNET["channel_mult"],
                       attention_resolutions=TINY_UNET["attention_resolutions"], num_heads=2)
SHAPE8 = (1, 8, 8, 8, 8)


@pytest.fixture(scope="module")
def gu():
    import tests.gpu_utils as g
    return g


@pytest.fixture(scope="module")
def diff():
    return hda.ImplicitronGaussianDiffusion(num_steps=1000)


@pytest.fixture(scope="module")
def net(gu):
    return gu.make_unet(TINY8_CFG)[0]


class _Tap:
    """A model without ``forward_channels_last`` (so the loop takes the NCDHW route) that records every output."""

    def __init__(self, net):
        self.net, self.outs = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, x, t, **kwargs):
        y = self.net(x, t)
        self.outs.append(y.detach().cpu().numpy().copy())
        return y


# ---- the step kernel ----------------------------------------------------------------------------------------------------
# per-sample sizes 512, 108, 4096: fewer elements than one workgroup (1024), a ragged last workgroup, several workgroups
@pytest.mark.parametrize("shape", [(2, 8, 4, 4, 4), (2, 4, 3, 3, 3), (2, 8, 8, 8, 8)])
def test_dpm_step_bit_exact_vs_restatement(gu, diff, shape):
    """holo_dpm_step equals the float32 restatement bit for bit: orders 1, 2, 3 (rows of a real schedule, a different row
    per sample), clip on and off, with the history pointers null where the order does not use them, and without pred_xstart."""
    x, mo, h1, h2 = (np_noise(s, shape) for s in (41, 42, 43, 44))
    mo = mo * np.float32(1.5)
    h1, h2 = np.clip(h1, -1, 1), np.clip(h2, -1, 1)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(gu.DEV)  # noqa: E731
    idx = diff.dpm_schedule(10)
    for order in (1, 2, 3):
        rows, orders = diff.dpm_coefs(idx, order)
        ks = [k for k, o in enumerate(orders) if o == order and k < len(idx) - 1]
        row = torch.stack([rows[ks[0]], rows[ks[-1]]])  # batch 2 with different rows
        assert not torch.equal(row[0], row[1])
        for clip in (True, False):
            for g1, g2 in ((h1, h2), (h1, None), (None, None)):
                s, p = diff._dpm_step(dev(x), dev(mo), row.to(gu.DEV), dev(g1), dev(g2), clip)
                rs, rp = dpm_ref.dpm_step_f32(x, mo, row.numpy(), g1, g2, clip)
                assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(p.cpu().numpy(), rp), (order, clip)
        s, p = diff._dpm_step(dev(x), dev(mo), row.to(gu.DEV), dev(h1), dev(h2), True, want_pred=False)
        assert p is None and np.array_equal(s.cpu().numpy(), dpm_ref.dpm_step_f32(x, mo, row.numpy(), h1, h2)[0])
    # the step past the end: the sample is the clipped prediction
    last = diff.dpm_coefs(idx, 2)[0][-1:].repeat(2, 1)
    s, p = diff._dpm_step(dev(x), dev(mo), last.to(gu.DEV), None, None, True)
    assert torch.equal(s, p) and np.array_equal(p.cpu().numpy(), np.clip(mo, -1, 1))


def test_dpm_step_rejects_ragged_sample(gu, diff):
    """elems_per_sample = 27 is no multiple of 4: HoloError from the launcher, before any launch."""
    shape = (2, 1, 3, 3, 3)
    x = torch.from_numpy(np_noise(45, shape)).to(gu.DEV)
    row = diff.dpm_coefs([500, 0], 1)[0][:1].repeat(2, 1).to(gu.DEV)
    with pytest.raises(_lib.HoloError, match="multiple of 4"):
        diff._dpm_step(x, x, row, None, None, True)


# ---- chains on the tiny UNet ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
def test_dpm_chain_vs_restatement_both_layouts(gu, diff, net, order):
    """6 steps: every yielded sample / pred_xstart of the NCDHW route (a recording wrapper model) equals the restatement
    applied to the recorded outputs and histories bit for bit; the net itself (channels-last route) gives the same chain
    bit for bit; dpm_sample_loop returns the last progressive sample."""
    x_T = torch.from_numpy(np_noise(4243 + order, SHAPE8)).to(gu.DEV)
    tap = _Tap(net)
    steps = list(diff.dpm_sample_loop_progressive(tap, SHAPE8, noise=x_T, steps=6, order=order, device=gu.DEV))
    idx = diff.dpm_schedule(6)
    rows, orders = diff.dpm_coefs(idx, order)
    assert len(steps) == len(idx) == len(tap.outs) == 6 and max(orders) == order
    want = dpm_ref.chain_f32(x_T.cpu().numpy(), tap.outs, rows.numpy(), orders)
    for k, (s, (ws, wp)) in enumerate(zip(steps, want)):
        assert set(s) == {"sample", "pred_xstart"}
        assert np.array_equal(s["sample"].cpu().numpy(), ws) and np.array_equal(s["pred_xstart"].cpu().numpy(), wp), k
    direct = list(diff.dpm_sample_loop_progressive(net, SHAPE8, noise=x_T, steps=6, order=order))
    assert len(direct) == 6
    for k, (a, b) in enumerate(zip(direct, steps)):
        assert a["sample"].is_contiguous() and a["sample"].shape == SHAPE8
        assert torch.equal(a["sample"], b["sample"]) and torch.equal(a["pred_xstart"], b["pred_xstart"]), k
    final = diff.dpm_sample_loop(net, SHAPE8, noise=x_T, steps=6, order=order)
    assert final.is_contiguous() and torch.equal(final, steps[-1]["sample"])
    assert torch.equal(diff.dpm_sample_loop(net, SHAPE8, noise=x_T, timesteps=idx, order=order), final)
    # noise_sampler is asked for x_T only
    calls = []
    ns = lambda t, shp, dev: (calls.append(t), x_T)[1]  # noqa: E731
    assert torch.equal(diff.dpm_sample_loop(net, SHAPE8, noise_sampler=ns, steps=6, order=order), final)
    assert calls == [diff.num_timesteps]


def _single_step_bound(t):
    """The order-1 step against the DDIM step (tests/test_dpm_cpu.py): 1e-5 of the range for t >= 20, 1e-3 below."""
    return 1e-5 if t >= 20 else 1e-3


def test_order1_chain_vs_ddim(gu, diff, net):
    """dpm_sample_loop(order=1, spacing="time", steps=5) and ddim_sample_loop(eta=0, ddim_steps=5) from the same x_T: the same
    update in exact arithmetic, two float32 formulas.  Bound: 10x the single-step figure of the chain's smallest non-zero
    timestep (200 -> 1e-4 of the grid's range); the UNet carries differences from step to step by an unmeasured factor."""
    S = 5
    x_T = torch.from_numpy(np_noise(77, SHAPE8)).to(gu.DEV)
    a = diff.dpm_sample_loop(net, SHAPE8, noise=x_T, order=1, spacing="time", steps=S)
    b = diff.ddim_sample_loop(net, SHAPE8, noise=x_T, eta=0.0, ddim_steps=S)
    idx = diff.dpm_schedule(S, "time")
    assert idx == diff.ddim_schedule(S)
    bound = 10 * _single_step_bound(min(t for t in idx if t > 0))
    rel = ((a - b).abs().max() / b.abs().max()).item()
    print(f"order-1 dpmpp chain vs ddim{S}: max difference {rel:.2e} of the grid's range (bound {bound:.0e})")
    assert rel <= bound, f"order-1 chain vs DDIM: {rel:.3e} of the grid's range, bound {bound:.0e}"


def test_batched_chains_rows_equal_chains_alone(gu, diff, net):
    """Three chains with different x_T in one call under set_batch_invariant(True): every row equals its batch-1 chain
    (flag off) bit for bit.  Order 3, so both history terms are in play."""
    x_T = torch.cat([torch.from_numpy(np_noise(90 + b, SHAPE8)) for b in range(3)]).to(gu.DEV)
    net.set_batch_invariant(True)
    try:
        batched = diff.dpm_sample_loop(net, (3,) + SHAPE8[1:], noise=x_T, steps=5, order=3)
    finally:
        net.set_batch_invariant(False)
    for b in range(3):
        alone = diff.dpm_sample_loop(net, SHAPE8, noise=x_T[b:b + 1].clone(), steps=5, order=3)
        assert torch.equal(batched[b:b + 1], alone), b
    assert not torch.equal(batched[0], batched[1])


# ---- the product ---------------------------------------------------------------------------------------------------------
def test_model_dpmpp_sampling(gu):
    """sample_random_voxel_features(sampler="dpmpp"): deterministic for a fixed torch seed, within [-1, 1]; the progressive
    form yields one clipped grid per schedule entry; keys of other samplers are refused."""
    model, *_ = gu.make_model(8, 32, 8, 8, TINY_UNET, diffusion_args=dict(num_steps=1000))
    torch.manual_seed(3)
    a = model.sample_random_voxel_features(sampler="dpmpp", dpm_steps=4)
    torch.manual_seed(3)
    b = model.sample_random_voxel_features(sampler="dpmpp", dpm_steps=4)
    assert a.shape == (1, 32, 8, 8, 8) and torch.equal(a, b) and a.min() >= -1 and a.max() <= 1
    torch.manual_seed(3)
    c = model.sample_random_voxel_features(sampler="dpmpp", dpm_steps=4, dpm_order=3, dpm_spacing="time")
    assert c.shape == a.shape and not torch.equal(a, c)
    for kw in (dict(dpm_steps=50), dict(dpm_steps=3, dpm_order=1)):
        torch.manual_seed(3)
        outs = list(model.sample_random_voxel_features_progressive(sampler="dpmpp", **kw))
        assert len(outs) == len(model.diffusion.dpm_schedule(kw["dpm_steps"])) and len(outs) in (49, 3)
        assert all(o.min() >= -1 and o.max() <= 1 for o in outs)
    with pytest.raises(ValueError):
        model.sample_random_voxel_features(sampler="dpmpp", ddim_steps=4)
    with pytest.raises(ValueError):
        model.sample_random_voxel_features(sampler="ddim", dpm_steps=4)
    with pytest.raises(ValueError):
        model.sample_random_voxel_features(sampler="dpmpp", dpm_order=4)


def test_generate_samples_with_dpmpp(gu):
    """generate_samples(sampler_kwargs={"sampler": "dpmpp", "dpm_steps": 3}) end to end on a small model, one chain at a time
    and with chains_per_gpu=2 (which hands the loop a noise_sampler): finite frames, equal between the two."""
    from holo_diffusion_amd.generate import generate_samples
    model, *_ = gu.make_model(8, 32, 8, 8, TINY_UNET, diffusion_args=dict(num_steps=1000))
    kw = dict(num_samples=3, n_eval_cameras=2, seed=3, device=gu.DEV, sampler_kwargs={"sampler": "dpmpp", "dpm_steps": 3})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = generate_samples(model, **kw)
        two = generate_samples(model, chains_per_gpu=2, **kw)
    img = one["images_render"]
    assert img.shape == (3, 2, 3, 8, 8) and torch.isfinite(img).all()
    for k in ("images_render", "depths_render", "masks_render"):
        assert torch.equal(one[k], two[k]), k
    assert not model.net_3d.batch_invariant and model.diffusion.device_noise_seed is None
