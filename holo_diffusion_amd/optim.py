"""``HoloAdam``: the parameter update of a training step on the HIP path.

Replaces ``torch.optim.Adam(foreach=True)`` + ``clip_grad_norm_`` of the reference's training loop
(trainer/optimizer_factory.py:78-149, trainer/training_loop.py:544-556; configs/apple.yaml:254-285: Adam, lr 4e-5, no weight
decay) for the gradients this package produces as plain tensors (``HoloDiffusionModel.training_step`` /
``training_backward`` / ``pool_views_backward``, after ``ddp.allreduce_training_gradients``)::

    opt = HoloAdam.from_model(model, lr=4e-5)
    out = model.training_step(camera=cams, voxel_features=grid, rng_streams=rs, loss_fn=loss_fn)
    ddp.allreduce_training_gradients(out)
    opt.step(out)

One multi-tensor kernel (``holo_adam_step``) updates parameters and moments; for a denoiser ``holo_unet_adam_step`` also
re-packs the library's private weight copies in stream order, so the next forward neither re-binds ~400 parameters nor drains
the queue.  Arithmetic: ``torch/optim/adam.py::_single_tensor_adam``.

Not covered: SGD / Adagrad, amsgrad, LR schedulers (``lr`` is a plain attribute: set it between steps), the bf16 modes (the
backward is fp32-only), skipping a step on non-finite gradients, and reading gradients straight out of the backward's
workspace (bootstrap rounds and the DDP exchange need them as tensors first).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, runtime

ADAM_CHUNK = 65536      # kAdamChunk (csrc/holo_kernels.h): elements per (tensor, chunk) entry of a launch
ADAM_TABLE_TENSORS = 40  # kAdamTensors: tensors per launch
ADAM_TABLE_ENTRIES = 320  # kAdamBlocks: (tensor, chunk) entries per launch


def bias_corrections(beta1: float, beta2: float, step: int) -> Tuple[float, float]:
    """``(1 - beta1**step, 1 - beta2**step)`` as the library forms them on the host (``holo_adam_scalars``): in double, from
    the doubles the caller wrote."""
    cfg = _lib.HoloAdamCfg(lr=0.0, beta1=beta1, beta2=beta2, eps=0.0, weight_decay=0.0, step=int(step), adamw=0)
    out = (C.c_double * 6)()
    L = runtime.lib()
    _lib.check(L, L.holo_adam_scalars(C.byref(cfg), out), "holo_adam_scalars")
    return out[0], out[1]


class _Group:
    def __init__(self, name: str, named: Dict[str, torch.Tensor], net=None):
        self.name, self.net = name, net
        self.names: List[str] = list(named)
        self.params: List[torch.Tensor] = [named[k] for k in self.names]
        n = len(self.names)
        self.exp_avg: List[Optional[torch.Tensor]] = [None] * n
        self.exp_avg_sq: List[Optional[torch.Tensor]] = [None] * n
        self.steps: List[int] = [0] * n
        self.cache = None  # (key, order, ctypes array)

    def ensure_state(self, j: int) -> None:
        if self.exp_avg[j] is None:
            p = self.params[j]
            self.exp_avg[j] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self.exp_avg_sq[j] = torch.zeros_like(p, memory_format=torch.contiguous_format)


class HoloAdam:
    def __init__(self, lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 adamw: bool = False, max_grad_norm: float = 0.0):
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.adamw, self.max_grad_norm = float(weight_decay), bool(adamw), float(max_grad_norm)
        self._groups: List[_Group] = []
        self._norm_out: Optional[torch.Tensor] = None  # (total_norm, clip_coef) on the device
        self._norm_ws: Optional[torch.Tensor] = None
        self._clipped = False

    # ---- wiring -------------------------------------------------------------------------------
    def add_unet(self, net, name: str = "unet") -> "HoloAdam":
        """A ``SimpleUnet3D``: its step also refreshes the library's packed copies (``holo_unet_adam_step``).  Gradients are
        looked up under ``grads[name]`` by the parameter names of ``net.backward`` (no ``_net.`` prefix)."""
        self._groups.append(_Group(name, dict(net._net.named_parameters()), net=net))
        return self

    def add_tensors(self, named: Dict[str, torch.Tensor], name: Optional[str] = None) -> "HoloAdam":
        """Any other tensors (RenderMLP, ``pooled_feature_mapper``, the learnt aggregator).  Their owners notice the update
        through the tensors' version counters and re-bind as after an in-place torch op."""
        self._groups.append(_Group(name if name is not None else f"group{len(self._groups)}", dict(named)))
        return self

    @classmethod
    def from_model(cls, model, **hyper) -> "HoloAdam":
        """The groups whose gradients ``training_backward`` ("unet", "render_mlp") and ``pool_views_backward``
        ("pooled_feature_mapper", "feature_aggregator") return.  The mapper is a LazyLinear: it is wired once it has been
        materialised by a pooling forward."""
        opt = cls(**hyper)
        if getattr(model, "net_3d", None) is not None:
            opt.add_unet(model.net_3d)
        opt.add_tensors(dict(model._implicit_functions[0]._fn.render_mlp.named_parameters()), "render_mlp")
        if getattr(model, "view_pooler", None) is not None:
            pm = model.pooled_feature_mapper
            if not isinstance(pm.weight, torch.nn.parameter.UninitializedParameter):
                opt.add_tensors(dict(pm.named_parameters()), "pooled_feature_mapper")
            agg = dict(model.view_pooler.feature_aggregator.named_parameters())
            if agg:
                opt.add_tensors(agg, "feature_aggregator")
        return opt

    # ---- the step ------------------------------------------------------------------------------
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Global gradient norm of the last step with ``max_grad_norm > 0``: a device scalar (no synchronisation until read)."""
        return self._norm_out[0] if self._norm_out is not None and self._clipped else None

    def _cfg(self, step: int) -> _lib.HoloAdamCfg:
        return _lib.HoloAdamCfg(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                weight_decay=self.weight_decay, step=int(step), adamw=1 if self.adamw else 0)

    def _unet_order(self, g: _Group, h) -> List[int]:
        """Indices into the group's tensors in ``holo_unet_param_info`` order."""
        L = runtime.lib()
        name, pos = C.create_string_buffer(256), {k: j for j, k in enumerate(g.names)}
        order = []
        for i in range(L.holo_unet_num_params(h)):
            _lib.check(L, L.holo_unet_param_info(h, i, name, 256, None, None), "holo_unet_param_info")
            order.append(pos[name.value.decode()])
        return order

    def _descriptors(self, g: _Group, gd: Dict[str, torch.Tensor], dev):
        """``(order, HoloAdamTensor array over order, gradient tensors kept alive)`` with this step's gradients filled in."""
        if g.net is not None:
            h = g.net._ensure_handle(dev)
            key = (g.net.__dict__.get("_handle_generation", 0),) + tuple(p.data_ptr() for p in g.params)
        else:
            h, key = None, tuple(p.data_ptr() for p in g.params)
        have = tuple(j for j, k in enumerate(g.names) if gd.get(k) is not None)
        key = (key, have)
        if g.cache is None or g.cache[0] != key:
            order = self._unet_order(g, h) if g.net is not None else list(have)
            if g.net is not None and len(have) != len(g.names):
                missing = [k for k in g.names if gd.get(k) is None]
                raise _lib.HoloError(f"HoloAdam.step: the denoiser's step needs every gradient; missing {missing[:3]} ...")
            arr = (_lib.HoloAdamTensor * max(len(order), 1))()
            for i, j in enumerate(order):
                p = g.params[j]
                runtime.require_device(p, "HoloAdam.step")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.HoloError(f"HoloAdam.step: '{g.name}.{g.names[j]}' must be a contiguous float32 tensor")
                g.ensure_state(j)
                arr[i].param, arr[i].exp_avg, arr[i].exp_avg_sq = p.data_ptr(), g.exp_avg[j].data_ptr(), g.exp_avg_sq[j].data_ptr()
                arr[i].numel = p.numel()
            g.cache = (key, order, arr)
        _, order, arr = g.cache
        held = []
        for i, j in enumerate(order):
            p, t = g.params[j], gd[g.names[j]]
            if t.numel() != p.numel() or t.device != p.device:
                raise _lib.HoloError(f"HoloAdam.step: gradient of '{g.name}.{g.names[j]}' is {tuple(t.shape)} on {t.device}, "
                                     f"the parameter {tuple(p.shape)} on {p.device}")
            t = t.detach().to(torch.float32).contiguous()
            held.append(t)
            arr[i].grad = t.data_ptr()
        return order, arr, held

    @torch.no_grad()
    def step(self, grads: Dict) -> None:
        """``grads``: ``{group name: {parameter name: gradient}}`` - the dict of ``training_step`` / ``training_backward``,
        other entries ignored - or, for an optimiser with ONE group, that group's flat ``{name: gradient}``.  A group that is
        absent and a ``None`` gradient are skipped, like a parameter whose ``.grad`` is None (the denoiser takes all or none)."""
        flat = len(self._groups) == 1 and self._groups[0].name not in grads
        work = []
        for g in self._groups:
            gd = grads if flat else grads.get(g.name)
            if not gd or not any(gd.get(k) is not None for k in g.names):
                continue
            dev = g.params[0].device
            order, arr, held = self._descriptors(g, gd, dev)
            work.append((g, dev, order, arr, held))
        if not work:
            raise _lib.HoloError(f"HoloAdam.step: no gradient for any of the groups {[g.name for g in self._groups]}")
        L = runtime.lib()
        dev = work[0][1]
        st = runtime.stream_ptr(dev)
        clip = None
        self._clipped = self.max_grad_norm > 0.0
        if self._clipped:  # ONE norm over every gradient of the step; the coefficient stays on the device
            n = sum(len(w[2]) for w in work)
            alln = (_lib.HoloAdamTensor * n)()
            i = 0
            for _, _, order, arr, _ in work:
                for k in range(len(order)):
                    alln[i].grad, alln[i].numel = arr[k].grad, arr[k].numel
                    i += 1
            nbytes = int(L.holo_grad_norm_workspace_bytes(alln, n))
            if self._norm_out is None or self._norm_out.device != dev:
                self._norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
            if self._norm_ws is None or self._norm_ws.device != dev or self._norm_ws.numel() * 8 < nbytes:
                self._norm_ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
            clip = C.c_void_p(self._norm_out.data_ptr() + 4)
            _lib.check(L, L.holo_grad_norm(runtime.ctx(dev), alln, n, self.max_grad_norm, runtime.ptr(self._norm_ws),
                                           self._norm_ws.numel() * 8, runtime.ptr(self._norm_out), clip, st), "holo_grad_norm")
        for g, dev, order, arr, _ in work:
            for j in order:
                g.steps[j] += 1
            if g.net is not None:
                steps = {g.steps[j] for j in order}
                if len(steps) != 1:
                    raise _lib.HoloError("HoloAdam.step: the denoiser's parameters must share one step count")
                cfg = self._cfg(steps.pop())
                _lib.check(L, L.holo_unet_adam_step(g.net._handle, arr, len(order), C.byref(cfg), clip, st), "holo_unet_adam_step")
            else:
                by_step: Dict[int, List[int]] = {}
                for i, j in enumerate(order):
                    by_step.setdefault(g.steps[j], []).append(i)
                for s, idx in by_step.items():  # (one call unless tensors joined the updates at different times)
                    sub = arr
                    if len(idx) != len(order):
                        sub = (_lib.HoloAdamTensor * len(idx))(*[arr[i] for i in idx])
                    cfg = self._cfg(s)
                    _lib.check(L, L.holo_adam_step(runtime.ctx(dev), sub, len(idx), C.byref(cfg), clip, st), "holo_adam_step")
            # the tensors changed behind torch's back: version counters as after an in-place op
            for j in order:
                torch.autograd.graph.increment_version(g.params[j])
            if g.net is not None:
                g.net._adopt_native_update()

    # ---- checkpoints: torch.optim.Adam's layout ----------------------------------------------------
    def _param_group(self) -> dict:
        # the key set of the installed torch's Adam, so that the dict loads into one (and its step finds every key)
        pg = dict(torch.optim.Adam([torch.zeros(0)], lr=self.lr, betas=self.betas, eps=self.eps,
                                   weight_decay=self.weight_decay).param_groups[0])
        if "decoupled_weight_decay" in pg:
            pg["decoupled_weight_decay"] = self.adamw
        pg["params"] = list(range(sum(len(g.names) for g in self._groups)))
        return pg

    def state_dict(self) -> dict:
        """``{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]}`` as ``torch.optim.Adam.state_dict()``
        writes it: ONE parameter group, the tensors numbered in the order they were added (the denoiser's in its
        ``named_parameters`` order).  Loads into a ``torch.optim.Adam`` built over the same tensors in that order."""
        state, i = {}, 0
        for g in self._groups:
            for j in range(len(g.names)):
                if g.exp_avg[j] is not None:
                    state[i] = {"step": torch.tensor(float(g.steps[j])), "exp_avg": g.exp_avg[j].clone(),
                                "exp_avg_sq": g.exp_avg_sq[j].clone()}
                i += 1
        return {"state": state, "param_groups": [self._param_group()]}

    def load_state_dict(self, sd: dict) -> None:
        """Accepts ``torch.optim.Adam.state_dict()`` (any number of parameter groups: as in torch, tensors are matched by
        POSITION over the concatenated groups) - e.g. the reference's optimiser checkpoint - or ``HoloAdam.state_dict()``.
        Hyper-parameters come from the first group."""
        ids = [i for pg in sd["param_groups"] for i in pg["params"]]
        slots = [(g, j) for g in self._groups for j in range(len(g.names))]
        if len(ids) != len(slots):
            raise ValueError(f"HoloAdam.load_state_dict: {len(ids)} parameters in the checkpoint, {len(slots)} here")
        for pid, (g, j) in zip(ids, slots):
            st = sd["state"].get(pid)
            p = g.params[j]
            g.cache = None
            if st is None:
                g.exp_avg[j] = g.exp_avg_sq[j] = None
                g.steps[j] = 0
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"HoloAdam.load_state_dict: '{g.name}.{g.names[j]}' is {tuple(p.shape)}, the checkpoint's "
                                 f"moment {tuple(st['exp_avg'].shape)}")
            g.exp_avg[j] = st["exp_avg"].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
            g.exp_avg_sq[j] = st["exp_avg_sq"].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
            g.steps[j] = int(st["step"])
        pg = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(pg["lr"]), (float(pg["betas"][0]), float(pg["betas"][1])), float(pg["eps"])
        self.weight_decay = float(pg["weight_decay"])
        self.adamw = bool(pg.get("decoupled_weight_decay", self.adamw))
