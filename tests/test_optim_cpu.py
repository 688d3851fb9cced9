"""CPU: the host side of the fused Adam step (include/holo_abi.h: holo_adam_step, holo_grad_norm, holo_unet_adam_step;
holo_diffusion_amd/optim.py) - struct layouts, error paths, the host scalars, and the checkpoint layout shared with
torch.optim.Adam.  No kernel runs here."""
import ctypes

import pytest
import torch

from holo_diffusion_amd import _lib
from holo_diffusion_amd.optim import HoloAdam, bias_corrections


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_lib.HoloAdamTensor) == 40  # four pointers + int64
    assert ctypes.sizeof(_lib.HoloAdamCfg) == 28     # five floats + two int32


@pytest.mark.parametrize("name", ["holo_adam_step", "holo_unet_adam_step", "holo_grad_norm"])
def test_null_arguments_are_refused(lib, name):
    if name == "holo_grad_norm":
        rc = lib.holo_grad_norm(None, None, 0, 1.0, None, 0, None, None, None)
    else:
        rc = getattr(lib, name)(None, None, 0, None, None, None)
    assert rc < 0 and name.encode() in lib.holo_last_error()


def test_a_bad_configuration_is_refused(lib):
    t = (_lib.HoloAdamTensor * 1)()
    cfg = _lib.HoloAdamCfg(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=0, adamw=0)
    assert lib.holo_adam_step(None, t, 0, ctypes.byref(cfg), None, None) == -1 and b"step" in lib.holo_last_error()
    assert lib.holo_grad_norm_workspace_bytes(t, 0) == 0


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_bias_corrections_equal_torchs(step):
    """torch forms them in double from the Python floats (torch/optim/adam.py: 1 - beta ** step); the configuration carries
    floats, which the library widens back to the doubles the caller wrote."""
    for b1, b2 in ((0.9, 0.999), (0.5, 0.95), (0.0, 0.99)):
        assert bias_corrections(b1, b2, step) == (1 - b1 ** step, 1 - b2 ** step)


def test_host_scalars(lib):
    cfg = _lib.HoloAdamCfg(lr=4e-5, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=3, adamw=0)
    out = (ctypes.c_double * 6)()
    assert lib.holo_adam_scalars(ctypes.byref(cfg), out) == 0
    bc1, bc2 = 1 - 0.9 ** 3, 1 - 0.999 ** 3
    assert list(out) == [bc1, bc2, 4e-5 / bc1, bc2 ** 0.5, 1 - 0.9, 1 - 0.999]


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return {"a.weight": torch.randn(4, 3, generator=g), "a.bias": torch.randn(4, generator=g), "b": torch.randn(7, generator=g)}


def test_state_dict_round_trip_with_torch_adam():
    """HoloAdam -> torch.optim.Adam -> HoloAdam: steps and moments survive, and torch can take a step on what it loaded."""
    named = _tensors(0)
    opt = HoloAdam(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01).add_tensors(named, "g")
    grp = opt._groups[0]
    gen = torch.Generator().manual_seed(1)
    for j, p in enumerate(grp.params):  # a state as three steps would have left it
        grp.exp_avg[j], grp.exp_avg_sq[j], grp.steps[j] = torch.randn(p.shape, generator=gen), torch.rand(p.shape, generator=gen), 3
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2] and sd["param_groups"][0]["params"] == [0, 1, 2]
    tparams = [torch.nn.Parameter(v.clone()) for v in named.values()]
    topt = torch.optim.Adam(tparams, lr=1.0)
    topt.load_state_dict(sd)
    pg = topt.param_groups[0]
    assert (pg["lr"], tuple(pg["betas"]), pg["eps"], pg["weight_decay"]) == (3e-4, (0.8, 0.99), 1e-7, 0.01)
    for j, p in enumerate(tparams):
        st = topt.state[p]
        assert int(st["step"]) == 3
        assert torch.equal(st["exp_avg"], grp.exp_avg[j]) and torch.equal(st["exp_avg_sq"], grp.exp_avg_sq[j])
        p.grad = torch.ones_like(p)
    topt.step()  # every key torch's step reads is there
    back = HoloAdam(lr=1.0).add_tensors(_tensors(0), "g")
    back.load_state_dict(topt.state_dict())
    assert (back.lr, back.betas, back.eps, back.weight_decay) == (3e-4, (0.8, 0.99), 1e-7, 0.01)
    for j, p in enumerate(tparams):
        assert back._groups[0].steps[j] == 4
        assert torch.equal(back._groups[0].exp_avg[j], topt.state[p]["exp_avg"])
        assert torch.equal(back._groups[0].exp_avg_sq[j], topt.state[p]["exp_avg_sq"])


def test_state_dict_before_the_first_step_and_a_size_mismatch():
    opt = HoloAdam(lr=1e-3).add_tensors(_tensors(0))
    assert opt.state_dict()["state"] == {}
    other = HoloAdam(lr=1e-3).add_tensors({"x": torch.zeros(3)})
    with pytest.raises(ValueError):
        other.load_state_dict(opt.state_dict())
