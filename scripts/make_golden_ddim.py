#!/usr/bin/env python3
"""Development only: writes tests/golden/ddim_sampler.npz from the REAL reference's DDIM (GaussianDiffusion.ddim_sample,
ddim_reverse_sample, ddim_sample_loop_progressive) on a tiny reference UNet with synthetic weights.  Needs the reference
checkout that oracle/make_golden.py uses; the fixture holds numeric arrays only.

The reference draws its DDIM noise with ``th.randn_like`` inside ``ddim_sample``.  For the single steps the script seeds
torch's CPU generator before each call and replays ``torch.randn`` of the same shape to recover it.  For the trajectories it
hands the reference ``oracle.common.np_noise`` draws instead (``th.randn_like`` replaced during the loop: step k of a chain
draws np_noise(noise_seed + k)), so the tests regenerate the noise from one stored seed.  Before writing, it checks that the
float32 restatement (tests/support/ddim_ref.py) with the plugin's coefficient rows reproduces every recorded step.

The fixture stays small (``crop``): the step arithmetic is elementwise, so the single steps keep one block of every tensor
(channel 0, depth slices 0..3: 256 values per sample), and the trajectories keep the same block of every step's sample and
pred_xstart; x_T and the noise are np_noise draws regenerated from their seeds.

torch's CPU sqrt is not correctly rounded on every host: its last bit can depend on the CPU's vector math path, so the
reference's own float32 result differs between machines by an ulp.  The script therefore runs the reference with a
correctly rounded float32 ``torch.sqrt`` (``ieee_sqrt``): the recorded steps are the reference's formula in IEEE float32,
which the plugin's rows and the kernel reproduce on any machine.

The strided trajectory is built the guided-diffusion way (respace.py): a GaussianDiffusion on the betas
1 - abar[t_i] / abar[t_{i-1}] of the kept timesteps, and a model wrapper that maps the spaced index back to the original t.

Usage:  python scripts/make_golden_ddim.py
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
from oracle import unet_oracle as uo  # noqa: E402
from oracle.common import np_noise  # noqa: E402
from holo_diffusion.guided_diffusion.gaussian_diffusion import (  # noqa: E402
    GaussianDiffusion, LossType, ModelMeanType, ModelVarType)
from holo_diffusion_amd.diffusion import ImplicitronGaussianDiffusion  # noqa: E402
from tests.support.ddim_ref import ddim_step  # noqa: E402

# the tiny net of the fixture (8 channels keep the file small); the GPU tests build the same net from these numbers
DDIM_CFG = uo.UNetCfg(image_size=8, in_channels=8, out_channels=8, model_channels=32, num_res_blocks=2,
                      channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2)
WEIGHT_SEED = 1234
STEP_TS = (999, 500, 1, 0)
ETAS = (0.0, 0.5, 1.0)
OUT = os.path.join(REPO, "tests", "golden", "ddim_sampler.npz")


def crop(a: torch.Tensor) -> np.ndarray:
    """The part of a (..., C, R, R, R) tensor the fixture stores: channel 0, depth slices 0..3 (256 values of an 8^3 grid)."""
    return np.ascontiguousarray(a[..., :1, :4, :, :].numpy())


_torch_sqrt = torch.sqrt


def ieee_sqrt(a, *args, **kwargs):
    if isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.device.type == "cpu" and not args and not kwargs:
        return torch.from_numpy(np.sqrt(a.numpy()))
    return _torch_sqrt(a, *args, **kwargs)


class Tap:
    def __init__(self, fn):
        self.fn, self.outs = fn, []

    def __call__(self, x, t, **kw):
        y = self.fn(x, t, **kw)
        self.outs.append(y.detach().clone())
        return y


def eta_tag(eta):
    return f"{eta:g}"


def check_equal(a, b, what):
    assert torch.equal(a, b), f"{what}: restatement != reference (max |d| {(a - b).abs().max().item():.3e})"


@torch.no_grad()
def main():
    torch.sqrt = ieee_sqrt  # (the reference calls th.sqrt: see the module docstring)
    net = build_reference(DDIM_CFG)
    load_synth(net, DDIM_CFG, WEIGHT_SEED)
    shape = (1, DDIM_CFG.in_channels) + (DDIM_CFG.image_size,) * 3
    out = {"cfg": np.array([DDIM_CFG.image_size, DDIM_CFG.in_channels, DDIM_CFG.model_channels, WEIGHT_SEED])}
    gd, plug = ref_diffusion(1000), ImplicitronGaussianDiffusion(num_steps=1000)

    # single steps, batch 1
    x = torch.from_numpy(np_noise(31, shape))
    out["step.x"] = crop(x)
    for ti in STEP_TS:
        t = torch.tensor([ti])
        torch.manual_seed(7000 + ti)
        noise = torch.randn(shape)
        out[f"step.t{ti}.noise"] = crop(noise)
        for clip in (1, 0):
            for eta in ETAS:
                tap = Tap(net)
                torch.manual_seed(7000 + ti)
                r = gd.ddim_sample(tap, x, t, clip_denoised=bool(clip), eta=eta)
                out[f"step.t{ti}.model_out"] = crop(tap.outs[0])
                out[f"step.t{ti}.clip{clip}.pred_xstart"] = crop(r["pred_xstart"])
                out[f"step.t{ti}.clip{clip}.eta{eta_tag(eta)}.sample"] = crop(r["sample"])
                s, p = ddim_step(x, tap.outs[0], plug.ddim_coefs([ti], [ti - 1], eta), noise, bool(clip))
                check_equal(s, r["sample"], f"step t={ti} eta={eta} clip={clip}")
                check_equal(p, r["pred_xstart"], f"pred t={ti} clip={clip}")
        r = gd.ddim_reverse_sample(net, x, t, clip_denoised=True)
        out[f"rev.t{ti}.sample"] = crop(r["sample"])
        s, _ = ddim_step(x, net(x, t), plug.ddim_coefs([ti], [ti + 1], reverse=True))
        check_equal(s, r["sample"], f"reverse step t={ti}")

    # one batch of 2 with different timesteps
    x2 = torch.from_numpy(np_noise(32, (2,) + shape[1:]))
    t2 = torch.tensor([700, 3])
    tap = Tap(net)
    torch.manual_seed(7777)
    r = gd.ddim_sample(tap, x2, t2, clip_denoised=True, eta=0.5)
    torch.manual_seed(7777)
    n2 = torch.randn(x2.shape)
    out.update({"b2.x": crop(x2), "b2.t": t2.numpy(), "b2.model_out": crop(tap.outs[0]), "b2.noise": crop(n2),
                "b2.sample": crop(r["sample"]), "b2.pred_xstart": crop(r["pred_xstart"])})
    s, _ = ddim_step(x2, tap.outs[0], plug.ddim_coefs([700, 3], [699, 2], 0.5), n2)
    check_equal(s, r["sample"], "batch of 2")

    # trajectories: full range at T = 25 (eta 0, 1) and ddim10 at T = 1000 (eta 0.5).  (At T = 20 the linear schedule ends
    # on beta = 1, abar = 0, where the reference's DDIM divides by zero: its whole chain is NaN.)
    for tag, T, S, eta in (("T25_eta0", 25, None, 0.0), ("T25_eta1", 25, None, 1.0), ("T1000_ddim10", 1000, 10, 0.5)):
        plug = ImplicitronGaussianDiffusion(num_steps=T)
        kept = plug.ddim_schedule(S)
        if S is None:
            gdt, model = ref_diffusion(T), net
        else:
            ac, last, betas = plug.alphas_cumprod, 1.0, []
            for i in sorted(kept):
                betas.append(1 - ac[i] / last)
                last = ac[i]
            gdt = GaussianDiffusion(betas=np.array(betas), model_mean_type=ModelMeanType.START_X,
                                    model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE,
                                    rescale_timesteps=False)
            orig = torch.tensor(sorted(kept))
            model = lambda xx, ts: net(xx, orig[ts])  # noqa: E731
        x_seed, noise_seed = 900 + T, 8000 * 1000 + T * 1000
        x_T = torch.from_numpy(np_noise(x_seed, shape))
        noises = torch.stack([torch.from_numpy(np_noise(noise_seed + k, shape)) for k in range(len(kept))])
        drawn = iter(noises)
        randn_like = torch.randn_like
        torch.randn_like = lambda a: next(drawn).clone()  # (the reference's draw in ddim_sample: see the docstring)
        try:
            steps = list(gdt.ddim_sample_loop_progressive(model, shape, noise=x_T, clip_denoised=True, eta=eta,
                                                          device=torch.device("cpu")))
        finally:
            torch.randn_like = randn_like
        assert len(steps) == len(kept) and next(drawn, None) is None
        out[f"{tag}.indices"] = np.array(kept)
        out[f"{tag}.eta"] = np.array(eta)
        out[f"{tag}.x_seed"] = np.array(x_seed)
        out[f"{tag}.noise_seed"] = np.array(noise_seed)
        out[f"{tag}.samples"] = np.stack([crop(s_["sample"]) for s_ in steps])
        out[f"{tag}.pred_xstart"] = np.stack([crop(s_["pred_xstart"]) for s_ in steps])
        # the restatement replays the chain (the strided one to rounding: its abar comes from a re-accumulated cumprod)
        img = x_T
        for k, ti in enumerate(kept):
            y = net(img, torch.tensor([ti]))
            s, _ = ddim_step(img, y, plug.ddim_coefs([ti], [kept[k + 1] if k + 1 < len(kept) else -1], eta), noises[k])
            err = (s - steps[k]["sample"]).abs().max().item()
            assert err <= (0.0 if S is None else 1e-4) * max(1.0, s.abs().max().item()), (tag, k, err)
            img = steps[k]["sample"]
        print(f"{tag}: {len(kept)} steps, timesteps {kept[:3]}...{kept[-1]}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT} written ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
