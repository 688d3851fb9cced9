#!/usr/bin/env python3
"""Development only: writes tests/golden/guided_sampler.npz from the REAL reference's guided steps - GaussianDiffusion.p_sample
(condition_mean) and ddim_sample (condition_score) with ``cond_fn = lambda x, t: g`` - on the tiny reference UNet of
scripts/make_golden_ddim.py.  Needs the reference checkout that oracle/make_golden.py uses; the fixture holds numeric arrays
only, cropped as ddim_sampler.npz is (channel 0, depth slices 0..3 of every tensor: the arithmetic is elementwise).

g = 0.1 * np_noise(GRAD_SEED); single steps at t in {999, 500, 1, 0}, clip on and off, eta in {0, 0.5, 1} for DDIM; one
batch of 2 with different t.  p_sample takes its noise through ``noise_sampler``; ddim_sample draws ``th.randn_like``, which
is replayed from the seeded CPU generator as in make_golden_ddim.py.

The reference runs with a correctly rounded float32 sqrt (make_golden_ddim.py, ``ieee_sqrt``), here also for the
``Tensor.sqrt`` method that condition_score calls.  Before writing, the script checks that the float32 restatements
(tests/support/guided_ref.py) with the plugin's tables and rows reproduce every recorded step: DDIM bit for bit, DDPM to the
tolerance of the fused DDPM update (the kernel fuses two of the reference's separately rounded products).

Usage:  python scripts/make_golden_guided.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import build_reference, load_synth, ref_diffusion  # noqa: E402  (imports the reference)
from oracle.common import np_noise  # noqa: E402
from holo_diffusion_amd.diffusion import ImplicitronGaussianDiffusion  # noqa: E402
from scripts.make_golden_ddim import DDIM_CFG, ETAS, STEP_TS, WEIGHT_SEED, Tap, check_equal, crop, eta_tag, ieee_sqrt  # noqa: E402
from tests.support.guided_ref import ddim_guided_step, ddpm_guided_step  # noqa: E402

GRAD_SEED = 77
OUT = os.path.join(REPO, "tests", "golden", "guided_sampler.npz")


def ddpm_scalars(plug, t):
    """(c1, c2, v, sigma) of the guided DDPM restatement for timesteps ``t``: the float32 casts of the float64 schedule."""
    t = np.asarray(t)
    f32 = lambda a: a[t].astype(np.float32)  # noqa: E731
    sigma = (t != 0).astype(np.float32) * np.exp(np.float32(0.5) * f32(plug.posterior_log_variance_clipped))
    return f32(plug.posterior_mean_coef1), f32(plug.posterior_mean_coef2), f32(plug.posterior_variance), sigma


def check_close(a, b, what):
    torch.testing.assert_close(a, b, rtol=3e-7, atol=1e-7, msg=lambda m: f"{what}: {m}")


@torch.no_grad()
def main():
    torch.sqrt = ieee_sqrt  # (the reference calls th.sqrt and Tensor.sqrt: see the module docstring)
    torch.Tensor.sqrt = lambda self: ieee_sqrt(self)
    net = build_reference(DDIM_CFG)
    load_synth(net, DDIM_CFG, WEIGHT_SEED)
    shape = (1, DDIM_CFG.in_channels) + (DDIM_CFG.image_size,) * 3
    out = {"cfg": np.array([DDIM_CFG.image_size, DDIM_CFG.in_channels, DDIM_CFG.model_channels, WEIGHT_SEED])}
    gd, plug = ref_diffusion(1000), ImplicitronGaussianDiffusion(num_steps=1000)

    x = torch.from_numpy(np_noise(31, shape))
    g = 0.1 * torch.from_numpy(np_noise(GRAD_SEED, shape))
    out["step.x"], out["step.grad"] = crop(x), crop(g)
    cond_fn = lambda xx, tt: g  # noqa: E731
    for ti in STEP_TS:
        t = torch.tensor([ti])
        torch.manual_seed(7000 + ti)
        noise = torch.randn(shape)
        out[f"step.t{ti}.noise"] = crop(noise)
        for clip in (1, 0):
            tap = Tap(net)
            r = gd.p_sample(tap, x, t, clip_denoised=bool(clip), cond_fn=cond_fn, model_kwargs={},
                            noise_sampler=lambda tt, shp, dev: noise)
            out[f"step.t{ti}.model_out"] = crop(tap.outs[0])
            out[f"ddpm.t{ti}.clip{clip}.sample"] = crop(r["sample"])
            out[f"ddpm.t{ti}.clip{clip}.pred_xstart"] = crop(r["pred_xstart"])
            s, p = ddpm_guided_step(x, tap.outs[0], g, noise, *ddpm_scalars(plug, [ti]), bool(clip))
            check_close(s, r["sample"], f"ddpm step t={ti} clip={clip}")
            check_equal(p, r["pred_xstart"], f"ddpm pred t={ti} clip={clip}")
            for eta in ETAS:
                tap = Tap(net)
                torch.manual_seed(7000 + ti)
                r = gd.ddim_sample(tap, x, t, clip_denoised=bool(clip), cond_fn=cond_fn, model_kwargs={}, eta=eta)
                out[f"ddim.t{ti}.clip{clip}.pred_xstart"] = crop(r["pred_xstart"])
                out[f"ddim.t{ti}.clip{clip}.eta{eta_tag(eta)}.sample"] = crop(r["sample"])
                s, p = ddim_guided_step(x, tap.outs[0], g, plug.ddim_guided_coefs([ti], [ti - 1], eta), noise, bool(clip))
                check_equal(s, r["sample"], f"ddim step t={ti} eta={eta} clip={clip}")
                check_equal(p, r["pred_xstart"], f"ddim pred t={ti} clip={clip}")

    # one batch of 2 with different timesteps
    x2 = torch.from_numpy(np_noise(32, (2,) + shape[1:]))
    g2 = 0.1 * torch.from_numpy(np_noise(GRAD_SEED + 1, tuple(x2.shape)))
    t2 = torch.tensor([700, 3])
    torch.manual_seed(7777)
    n2 = torch.randn(x2.shape)
    tap = Tap(net)
    r = gd.p_sample(tap, x2, t2, clip_denoised=True, cond_fn=lambda xx, tt: g2, model_kwargs={},
                    noise_sampler=lambda tt, shp, dev: n2)
    out.update({"b2.x": crop(x2), "b2.grad": crop(g2), "b2.t": t2.numpy(), "b2.model_out": crop(tap.outs[0]),
                "b2.noise": crop(n2), "b2.ddpm.sample": crop(r["sample"]), "b2.ddpm.pred_xstart": crop(r["pred_xstart"])})
    s, p = ddpm_guided_step(x2, tap.outs[0], g2, n2, *ddpm_scalars(plug, [700, 3]))
    check_close(s, r["sample"], "ddpm batch of 2")
    torch.manual_seed(7777)
    r = gd.ddim_sample(net, x2, t2, clip_denoised=True, cond_fn=lambda xx, tt: g2, model_kwargs={}, eta=0.5)
    out.update({"b2.ddim.sample": crop(r["sample"]), "b2.ddim.pred_xstart": crop(r["pred_xstart"])})
    s, p = ddim_guided_step(x2, tap.outs[0], g2, plug.ddim_guided_coefs([700, 3], [699, 2], 0.5), n2)
    check_equal(s, r["sample"], "ddim batch of 2")
    check_equal(p, r["pred_xstart"], "ddim batch of 2, pred")
    np.savez_compressed(OUT, **out)
    print(f"{OUT} written ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
