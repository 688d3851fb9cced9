"""CPU: the host side of the diffusion losses and of the variational bound (include/holo_abi.h: holo_diffusion_loss,
holo_vb_terms; ImplicitronGaussianDiffusion.training_losses / vb_coefs / calc_bpd_loop).  The float64 restatement
(tests/support/diffusion_loss_ref.py) against the reference's recorded results (tests/golden/diffusion_losses.npz, written by
scripts/make_golden_diffusion_losses.py), the coefficient rows, the binding, the argument checks that launch nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from holo_diffusion_amd import _lib
from holo_diffusion_amd.diffusion import ImplicitronGaussianDiffusion
from tests.support import diffusion_loss_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(si, ri) for si in range(len(ref.SHAPES)) for ri in range(len(ref.T_ROWS))]
VB_NAMES = ("vb", "xstart_mse", "eps_mse")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "diffusion_losses.npz")))


@pytest.fixture(scope="module")
def diff():
    return ImplicitronGaussianDiffusion(num_steps=1000)


@pytest.fixture(scope="module")
def lib():
    from holo_diffusion_amd import runtime
    return runtime.lib()


@pytest.mark.parametrize("si,ri", CASES)
def test_restatement_matches_the_recorded_reference(golden, diff, si, ri):
    """Float64 column: 1e-12 with normal_kl's rounding residue restated, and the residue-free KL within 1e-7 of it.  Float32
    column: within the reference's own recorded deviation (plus the 1e-12)."""
    c = ref.case_inputs(diff, si, ri)
    key = f"s{si}.r{ri}"
    rows = ref.schedule_rows(diff, c["t"])
    mse, huber = ref.loss_terms(c["x_start"], c["model_out"])
    for name, got in (("mse", mse), ("huber", huber)):
        assert ref.rel(got, golden[f"{key}.{name}.f64"]).max() <= 1e-12, name
        assert (ref.rel(golden[f"{key}.{name}.f32"], got) <= golden[f"{key}.{name}.dev"] + 1e-12).all(), name
        assert golden[f"{key}.{name}.dev"].max() < 2e-6, name  # (a well-conditioned mean: the reference's float32 is close)
    for clip in (1, 0):
        with_res = ref.vb_terms(rows, c["x_start"], c["x_t"], c["noise"], c["model_out"], bool(clip), reference_residue=True)
        plain = ref.vb_terms(rows, c["x_start"], c["x_t"], c["noise"], c["model_out"], bool(clip))
        for k, name in enumerate(VB_NAMES):
            f64, f32, dev = (golden[f"{key}.clip{clip}.{name}.{tag}"] for tag in ("f64", "f32", "dev"))
            assert ref.rel(with_res[:, k], f64).max() <= 1e-12, (clip, name)
            assert (ref.rel(f32, with_res[:, k]) <= dev + 1e-12).all(), (clip, name)
            assert ref.rel(plain[:, k], f64).max() <= 1e-7, (clip, name)
    if ri == 0:
        x0 = ref.make_x_start(ref.case_seed(si, 0), ref.SHAPES[si])
        assert ref.rel(ref.prior_bpd(diff, x0), golden[f"s{si}.prior_bpd.f64"]).max() <= 1e-12
        f32, f64 = golden[f"s{si}.prior_bpd.f32"], golden[f"s{si}.prior_bpd.f64"]  # (-1 - lv + exp(lv) cancels: ~4e-5 in float32)
        assert (ref.rel(f32, ref.prior_bpd(diff, x0)) <= ref.rel(f32, f64) + 1e-12).all() and ref.rel(f32, f64).max() < 1e-4


def test_the_float32_residue_is_what_the_kernel_drops(golden):
    """At t = 999 / 998 the KL is ~1e-7 nats and the reference's float32 value is dominated by the rounding residue of
    -1 + lv2 - lv1 + exp(lv1 - lv2) (exactly 0 in real arithmetic); at t <= 500 its float32 deviation is small."""
    assert golden["s0.r0.clip1.vb.dev"].min() > 1e-3
    for si in range(len(ref.SHAPES)):
        for ri in (1, 2, 3):
            assert golden[f"s{si}.r{ri}.clip1.vb.dev"].max() < 1e-5, (si, ri)


def test_decoder_rows_meet_the_clamp_condition(diff):
    """On every t == 0 row of the fixture the clamp argument of the decoder term is >= 1e-3 in float64, both tails occur."""
    lo, tails = np.inf, [0, 0]
    for si, ri in CASES:
        c = ref.case_inputs(diff, si, ri)
        rows = ref.schedule_rows(diff, c["t"])
        for clip in (True, False):
            _, args = ref.vb_terms(rows, c["x_start"], c["x_t"], None, c["model_out"], clip, with_clamp_args=True)
            for b in np.nonzero(c["t"] == 0)[0]:
                lo = min(lo, float(args[b].min()))
                tails[0] += int((c["x_start"][b] > 0.999).sum())
                tails[1] += int((c["x_start"][b] < -0.999).sum())
    assert lo >= 1e-3 and min(tails) > 0, (lo, tails)


def test_vb_coefs_rows(diff):
    t = np.array([0, 1, 2, 500, 998, 999])
    rows = diff.vb_coefs(t)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (6, 8)
    want = ref.schedule_rows(diff, t)
    assert np.array_equal(rows.numpy(), want.astype(np.float32))
    assert rows[:, 7].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert rows[0, 2] == rows[1, 2]  # posterior_log_variance_clipped[0] = [1]
    lv = diff.posterior_log_variance_clipped[t]
    assert np.allclose(want[:, 3] * np.exp(lv), 1.0, rtol=1e-14) and np.allclose(want[:, 4] ** 2, want[:, 3], rtol=1e-14)
    # the posterior of q_posterior_mean_variance: at t = 0 the mean is x_start itself
    assert rows[0, 0] == 1.0 and rows[0, 1] == 0.0
    every = diff.vb_coefs(np.arange(1000)).numpy()
    assert np.isfinite(every).all()


def test_header_and_binding():
    hdr = open(os.path.join(REPO, "include", "holo_abi.h")).read()
    for name in ("holo_diffusion_loss_workspace_bytes", "holo_diffusion_loss", "holo_vb_terms"):
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), name
        assert name in _lib.SIGNATURES
    assert "#define HOLO_ABI_VERSION 6" in hdr
    assert "normal_kl" in hdr and "INPUT CONDITION" in hdr  # the dropped residue term and the t == 0 condition are stated
    assert len(_lib.SIGNATURES["holo_diffusion_loss"][1]) == 11 and len(_lib.SIGNATURES["holo_vb_terms"][1]) == 13


@pytest.mark.parametrize("batch,per,partials", [(1, 4, 1), (2, 512, 1), (2, 2048, 1), (1, 2052, 2), (2, 4096, 2),
                                                (3, 6912, 4), (1, 8388608, 4096), (65535, 4, 1)])
def test_workspace_bytes(lib, batch, per, partials):
    """batch x 3 terms x ceil(elems / 2048) doubles: a function of the shapes alone."""
    assert lib.holo_diffusion_loss_workspace_bytes(batch, per) == batch * 3 * partials * 8


@pytest.mark.parametrize("batch,per", [(0, 64), (-1, 64), (65536, 64), (1, 0), (1, -4), (1, 6), (2, 2049)])
def test_invalid_shapes_are_refused_without_a_launch(lib, batch, per):
    assert lib.holo_diffusion_loss_workspace_bytes(batch, per) == 0
    assert b"multiple of 4" in lib.holo_last_error()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    rc = lib.holo_diffusion_loss(None, batch, per, p, p, None, p, None, p, 512, None)
    assert rc == -1
    assert b"holo_diffusion_loss" in lib.holo_last_error() and b"multiple of 4" in lib.holo_last_error()
    rc = lib.holo_vb_terms(None, p, batch, per, p, p, None, p, 1, p, p, 512, None)
    assert rc == -1 and b"holo_vb_terms" in lib.holo_last_error()


def test_null_arguments_and_short_workspace_are_refused_without_a_launch(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    need = lib.holo_diffusion_loss_workspace_bytes(2, 4096)
    assert need == 2 * 3 * 2 * 8
    assert lib.holo_diffusion_loss(None, 2, 4096, None, p, None, p, None, p, need, None) == -1
    assert b"null" in lib.holo_last_error()
    assert lib.holo_diffusion_loss(None, 2, 4096, p, p, None, None, None, p, need, None) == -1
    assert b"at least one of terms and grad_out" in lib.holo_last_error()
    assert lib.holo_diffusion_loss(None, 2, 4096, p, p, None, p, None, p, need - 8, None) == -3
    assert b"workspace" in lib.holo_last_error()
    assert lib.holo_diffusion_loss(None, 2, 4096, p, p, None, p, None, None, need, None) == -3
    assert lib.holo_vb_terms(None, None, 2, 4096, p, p, None, p, 1, p, p, need, None) == -1
    assert lib.holo_vb_terms(None, p, 2, 4096, p, p, None, p, 1, None, p, need, None) == -1
    assert lib.holo_vb_terms(None, p, 2, 4096, p, p, None, p, 1, p, p, need - 1, None) == -3


@pytest.mark.skipif(os.environ.get("HOLO_TEST_EMU") == "1", reason="the emulation lets CPU tensors through on purpose")
def test_cpu_tensors_are_refused(diff):
    x = torch.zeros(1, 4, 4, 4, 4)
    t = torch.tensor([5])
    model = lambda a, b, **kw: a  # noqa: E731
    with pytest.raises(_lib.HoloError, match="no CPU fallback"):
        diff.training_losses(model, x, t)
    with pytest.raises(_lib.HoloError, match="no CPU fallback"):
        diff.calc_bpd_loop(model, x)
    with pytest.raises(_lib.HoloError, match="no CPU fallback"):
        diff._vb_terms_bpd(model, x, x, t)
