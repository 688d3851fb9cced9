#!/usr/bin/env python3
"""Development only: writes tests/golden/diffusion_losses.npz from the REAL reference's GaussianDiffusion (START_X,
FIXED_SMALL, MSE): training_losses, _vb_terms_bpd, the xstart_mse / mse of calc_bpd_loop's body, _prior_bpd and one full
calc_bpd_loop at T = 20.  Needs the reference checkout that oracle/make_golden.py uses; the fixture holds numeric arrays only.

The model is a stub, a fixed function of numpy Philox seeds (tests/support/diffusion_loss_ref.py: stub_output), so no weights
are stored and the tests regenerate every input.  Each quantity is recorded twice: ``.f32`` from the reference as it runs,
in float32, and ``.f64`` from the same reference code fed float64 tensors, with ``_extract_into_tensor`` handing out the
float64 schedule entries instead of their float32 casts (the one substitution: otherwise the "float64" run would still round
every coefficient to float32).  Both runs get the SAME float32 inputs (x_start, noise, x_t, stub output), so ``.dev`` =
|f32 - f64| / |f64| is the reference's own float32 arithmetic error per case.

Before anything is written the script checks that
  - the float64 numpy restatement reproduces the float64 reference run to 1e-12 relative (with normal_kl's rounding residue
    restated; without it, the KL rows agree to the residue's size, which is printed),
  - on every t == 0 row the argument of the decoder term's clamp, in float64, is >= 1e-3 for every element (the input
    condition of holo_vb_terms: see include/holo_abi.h), with both tail branches taken.

Usage:  python scripts/make_golden_diffusion_losses.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.make_golden import ref_diffusion  # noqa: E402  (imports the reference)
from oracle.common import np_noise  # noqa: E402
import holo_diffusion.guided_diffusion.gaussian_diffusion as gdm  # noqa: E402
from holo_diffusion.guided_diffusion.nn import mean_flat  # noqa: E402
from tests.support import diffusion_loss_ref as ref  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "diffusion_losses.npz")
_extract32 = gdm._extract_into_tensor


def _extract64(arr, timesteps, broadcast_shape):
    """The schedule entries of a batch as float64, one per sample, broadcast over the sample's elements."""
    vals = torch.as_tensor(np.asarray(arr, dtype=np.float64)[timesteps.cpu().numpy()])
    return vals.reshape((-1,) + (1,) * (len(broadcast_shape) - 1)).expand(broadcast_shape)


class precision:
    """Runs the reference in float32 as it is, or in float64 (tensors and schedule entries)."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        gdm._extract_into_tensor = _extract64 if self.dtype == torch.float64 else _extract32
        return lambda a: torch.from_numpy(np.asarray(a)).to(self.dtype)

    def __exit__(self, *exc):
        gdm._extract_into_tensor = _extract32


def close(a, b, tol, what):
    err = float(np.max(ref.rel(a, b)))
    assert err <= tol, f"{what}: restatement vs reference {err:.3e} > {tol:g}"
    return err


@torch.no_grad()
def main():
    assert np.array_equal(ref.np_noise(3, (5, 7)), np_noise(3, (5, 7)))
    gd = ref_diffusion(1000)
    out = {}
    worst_clamp, tails = np.inf, [0, 0]
    for si, shape in enumerate(ref.SHAPES):
        for ri in range(len(ref.T_ROWS)):
            c = ref.case_inputs(gd, si, ri)
            t = torch.from_numpy(c["t"])
            key = f"s{si}.r{ri}"
            rows = ref.schedule_rows(gd, c["t"])
            for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                with precision(dtype) as T:
                    x0, nz, xt, mo = T(c["x_start"]), T(c["noise"]), T(c["x_t"]), T(c["model_out"])
                    model = lambda x, ts, r=mo, **kw: r  # noqa: E731
                    terms = gd.training_losses(model, x0, t, noise=nz)
                    if dtype == torch.float32:  # the float32 restatement of q_sample is the reference's, bit for bit
                        assert torch.equal(terms["x_t"], xt), key
                    out[f"{key}.mse.{tag}"] = terms["mse"].numpy()
                    out[f"{key}.huber.{tag}"] = terms["huber"].numpy()
                    for clip in (1, 0):
                        vb = gd._vb_terms_bpd(model, x_start=x0, x_t=xt, t=t, clip_denoised=bool(clip))
                        xs = mean_flat((vb["pred_xstart"] - x0) ** 2)
                        eps = gd._predict_eps_from_xstart(xt, t, vb["pred_xstart"])
                        out[f"{key}.clip{clip}.vb.{tag}"] = vb["output"].numpy()
                        out[f"{key}.clip{clip}.xstart_mse.{tag}"] = xs.numpy()
                        out[f"{key}.clip{clip}.eps_mse.{tag}"] = mean_flat((eps - nz) ** 2).numpy()
            # the restatement against the float64 run; the clamp condition of the t == 0 rows
            mse, huber = ref.loss_terms(c["x_start"], c["model_out"])
            close(mse, out[f"{key}.mse.f64"], 1e-12, key + " mse")
            close(huber, out[f"{key}.huber.f64"], 1e-12, key + " huber")
            for clip in (1, 0):
                got, args = ref.vb_terms(rows, c["x_start"], c["x_t"], c["noise"], c["model_out"], bool(clip),
                                         reference_residue=True, with_clamp_args=True)
                for k, name in enumerate(("vb", "xstart_mse", "eps_mse")):
                    close(got[:, k], out[f"{key}.clip{clip}.{name}.f64"], 1e-12, f"{key} clip{clip} {name}")
                plain = ref.vb_terms(rows, c["x_start"], c["x_t"], c["noise"], c["model_out"], bool(clip))
                resid = float(np.max(ref.rel(plain[:, 0], out[f"{key}.clip{clip}.vb.f64"])))
                assert resid <= 1e-7, (key, clip, resid)
                for b in np.nonzero(c["t"] == 0)[0]:
                    worst_clamp = min(worst_clamp, float(args[b].min()))
                    tails[0] += int((c["x_start"][b] > 0.999).sum())
                    tails[1] += int((c["x_start"][b] < -0.999).sum())
            for name in ("mse", "huber") + tuple(f"clip{cl}.{n}" for cl in (1, 0) for n in ("vb", "xstart_mse", "eps_mse")):
                out[f"{key}.{name}.dev"] = ref.rel(out[f"{key}.{name}.f32"], out[f"{key}.{name}.f64"])
            print(key, shape, c["t"].tolist(), "dev vb", out[f"{key}.clip1.vb.dev"], "eps", out[f"{key}.clip1.eps_mse.dev"])
        x0 = ref.make_x_start(ref.case_seed(si, 0), shape)
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            with precision(dtype) as T:
                out[f"s{si}.prior_bpd.{tag}"] = gd._prior_bpd(T(x0)).numpy()
        close(ref.prior_bpd(gd, x0), out[f"s{si}.prior_bpd.f64"], 1e-12, f"s{si} prior")
    assert worst_clamp >= 1e-3 and min(tails) > 0, (worst_clamp, tails)
    print(f"t == 0 rows: smallest clamp argument {worst_clamp:.4f}; {tails[0]} upper-tail, {tails[1]} lower-tail elements")

    # one full calc_bpd_loop at T = 20 (th.randn_like replaced by the loop's seeded draws, as make_golden_ddim.py does)
    gl = ref_diffusion(ref.LOOP_STEPS)
    x0 = ref.make_x_start(ref.LOOP_SEED, ref.LOOP_SHAPE)
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        with precision(dtype) as T:
            drawn = iter([T(ref.loop_noise(ref.LOOP_SHAPE, ti)) for ti in range(ref.LOOP_STEPS)[::-1]])
            model = lambda x, ts, **kw: T(ref.loop_model_output(gl, x0, int(ts[0])))  # noqa: E731
            randn_like = torch.randn_like
            torch.randn_like = lambda a: next(drawn).clone()
            try:
                res = gl.calc_bpd_loop(model, T(x0), clip_denoised=True)
            finally:
                torch.randn_like = randn_like
            assert next(drawn, None) is None
            for k, v in res.items():
                out[f"loop.{k}.{tag}"] = v.numpy()
    for b in range(ref.LOOP_SHAPE[0]):  # the loop's t == 0 term meets the clamp condition too
        mo = ref.loop_model_output(gl, x0, 0)
        rows = ref.schedule_rows(gl, [0] * ref.LOOP_SHAPE[0])
        xt = ref.q_sample32(gl, x0, [0] * ref.LOOP_SHAPE[0], ref.loop_noise(ref.LOOP_SHAPE, 0))
        _, args = ref.vb_terms(rows, x0, xt, None, mo, True, with_clamp_args=True)
        assert args.min() >= 1e-3, args.min()
    print("loop total_bpd", out["loop.total_bpd.f32"], out["loop.total_bpd.f64"])
    np.savez_compressed(OUT, **out)
    print(f"{OUT} written ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
