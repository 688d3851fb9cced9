"""DDPM ancestral sampler plugin backed by the HIP library.

Mirrors ``ImplicitronGaussianDiffusion`` (/root/reference/holo_diffusion/utils/diffusion_utils.py:89-140),
a Configurable wrapper around ``GaussianDiffusion`` (guided_diffusion/gaussian_diffusion.py):
same config fields (:90-97), same method names and arguments (``q_sample``, ``p_mean_variance``,
``p_sample``, ``p_sample_loop``, ``p_sample_loop_progressive``, ``sample_timesteps``), same
returned dict keys.  Only START_X / FIXED_SMALL (what HoloDiffusion configures, :95-96) is built.

The float64 schedule tables follow gaussian_diffusion.py:25-51,129-187 and are cast to float32 at
gather time like ``_extract_into_tensor`` (:1046-1059).  The per-step elementwise tail
(clamp, posterior mean, noise add; :314-343,237-240,499-506) is one fused HIP kernel
(``holo_ddpm_step``) reading the coefficients by timestep index from a device table, so the
sampling loop never synchronises with the host.

DDIM (``ddim_sample``, ``ddim_reverse_sample``, ``ddim_sample_loop*``; gaussian_diffusion.py:645-815) runs on a second
fused kernel (``holo_ddim_step``) that reads one float32 coefficient row per sample, built on the host in the reference's
order; a chain's rows are uploaded once.  Build-side extensions: strided "ddimS" schedules (``ddim_steps``), explicit
``timesteps`` and ``ddim_reverse_sample_loop`` (inversion x_0 -> x_T).

DPM-Solver++ (``dpm_schedule``, ``dpm_coefs``, ``dpm_sample_loop*``; build-side extension, no reference counterpart) is the
multistep exponential integrator in log-SNR on the clipped x_0 prediction, orders 1-3, one model call per step.  Each step's
update is expanded on the host, in float64, into four scalars per sample; a third fused kernel (``holo_dpm_step``) applies
them to x_t, the model output and the previous two predictions.

What the samplers share is written once.  ``_chain`` is the chain loop: x_T, the one upload of the chain's timesteps and rows,
the choice of the channels-last layout, then model call, step, yield.  A sampler is its schedule, its host rows and a step
callback; ``_last_sample`` finishes the non-progressive loops.  ``_launch`` and ``_launch_device_noise`` are the two ways into
the library's step entries (plain, and with the noise drawn in the kernel: offset or per-row streams); ``_step``,
``_step_device_noise``, ``_ddim_step``, ``_ddim_step_device_noise`` and ``_dpm_step`` name the entry and its leading arguments.

Guidance (``cond_fn``; gaussian_diffusion.py:420-457, used at :502-505 and :669-670): ``p_sample*`` and ``ddim_sample*`` take the
reference's ``cond_fn(x, t, **model_kwargs)``, called once per step after the model, and hand its gradient to the guided forms
of the two step kernels (``holo_ddpm_step_guided``: condition_mean; ``holo_ddim_step_guided``: condition_score on
``ddim_guided_coefs`` rows).  A guided chain runs NCDHW.  Without ``cond_fn`` every path is the unguided one above.

Masked sampling (``repaint_schedule``, ``inpaint_sample_loop*``; build-side extension after RePaint, no reference counterpart):
a per-voxel mask holds part of a clean grid fixed while the DDPM chain generates the rest, with resampling jumps, and
``start_level`` starts the chain from a partly noised grid.  The step is ``holo_ddpm_step_inpaint`` (the DDPM update blended
with the known grid noised one level down), a forward jump one ``holo_q_sample`` launch on ``jump_coefs`` rows; ``_chain``
runs it through its ``pre`` hook.

Losses and the variational bound (``training_losses``, ``_vb_terms_bpd``, ``_prior_bpd``, ``calc_bpd_loop``;
gaussian_diffusion.py:817-1043 for START_X / FIXED_SMALL / MSE): x_t is a ``holo_q_sample`` launch on rows gathered on the
device, the per-sample means are double sums in a fixed order (``holo_diffusion_loss``: mse, huber and the cotangent of the
mse in one pass; ``holo_vb_terms``: the bound's term, xstart_mse and eps_mse on ``vb_coefs`` rows).  ``training_losses``
carries an autograd node, so ``terms["loss"].mean().backward()`` reaches the denoiser through its own node.
"""
from __future__ import annotations

import enum
import warnings
from typing import Callable, Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, runtime
from .registry import Configurable, apply_config


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


def get_named_beta_schedule(name: str, num_steps: int, beta_start_unscaled: float, beta_end_unscaled: float) -> np.ndarray:
    if name != "linear":
        raise NotImplementedError(f"unknown/unsupported beta schedule: {name}")
    scale = 1000 / num_steps
    return np.linspace(scale * beta_start_unscaled, scale * beta_end_unscaled, num_steps, dtype=np.float64)


def ddim_timesteps(num_timesteps: int, ddim_steps: int) -> List[int]:
    """guided-diffusion's "ddimS" spacing (respace.py ``space_timesteps``): ``range(0, T, k)`` for the smallest stride k that
    gives exactly S timesteps, in the descending order a sampling loop walks them."""
    S = int(ddim_steps)
    for k in range(1, max(num_timesteps, 2)):
        if len(range(0, num_timesteps, k)) == S:
            return list(range(0, num_timesteps, k))[::-1]
    raise ValueError(f"cannot create exactly {S} DDIM steps out of {num_timesteps} timesteps with an integer stride")


DPM_DEFAULT_STEPS = 20  # ``steps=None`` of the DPM-Solver++ schedule and loops


class UniformSampler:
    """guided_diffusion/timestep_sampler.py:67-73 + ScheduleSampler.sample (:40-62)."""

    def __init__(self, num_timesteps: int):
        self._weights = np.ones([num_timesteps])

    def sample(self, batch_size: int, device):
        w = self._weights
        p = w / np.sum(w)
        idx = np.random.choice(len(p), size=(batch_size,), p=p)
        indices = torch.from_numpy(idx).long().to(device)
        weights = torch.from_numpy(1 / (len(p) * p[idx])).float().to(device)
        return indices, weights


class ImplicitronGaussianDiffusion(Configurable):
    beta_schedule_type: str = "linear"
    num_steps: int = 1000
    beta_start_unscaled: float = 0.0001
    beta_end_unscaled: float = 0.02
    model_mean_type: ModelMeanType = ModelMeanType.START_X
    model_var_type: ModelVarType = ModelVarType.FIXED_SMALL
    schedule_sampler_type: str = "uniform"
    # build-side extension (not a reference field).  None (default): the per-step noise is ``torch.randn_like`` / the
    # caller's ``noise_sampler`` - the reference's draw, the parity path.  An integer: PERF MODE - ``p_sample`` /
    # ``p_sample_loop*`` draw the noise inside the step kernel (``holo_ddpm_step_philox``: Philox4x32-10 keyed on this
    # seed, counter = (element, sample, timestep); no randn launch, the noise never crosses HBM).  Statistically
    # equivalent to, not bit-equal with, torch's generator; the initial x_T still comes from torch.  ``device_noise_stream``
    # separates chains that share a seed (generate.py passes the sample index).  A sequence of ints: one stream per batch
    # row (batched chains, ``holo_*_step_philox_rows``) - row b draws what a batch-1 chain of stream ``device_noise_stream[b]``
    # draws, whatever batch and row it runs in.
    device_noise_seed: Optional[int] = None
    device_noise_stream: int = 0

    def __init__(self, **kwargs):
        apply_config(self, kwargs)
        if isinstance(self.model_mean_type, str):
            self.model_mean_type = ModelMeanType[self.model_mean_type]
        if isinstance(self.model_var_type, str):
            self.model_var_type = ModelVarType[self.model_var_type]
        if self.model_mean_type != ModelMeanType.START_X or self.model_var_type != ModelVarType.FIXED_SMALL:
            raise NotImplementedError("only model_mean_type=START_X / model_var_type=FIXED_SMALL are on the hot path")
        if self.schedule_sampler_type != "uniform":
            raise NotImplementedError("only the 'uniform' schedule sampler is supported")
        betas = get_named_beta_schedule(self.beta_schedule_type, self.num_steps, self.beta_start_unscaled,
                                        self.beta_end_unscaled)
        self._build_tables(betas)
        self._schedule_sampler = UniformSampler(self.num_timesteps)
        self._dev_tables: Dict[int, torch.Tensor] = {}
        self._dev_variances: Dict[int, torch.Tensor] = {}
        self._row_stream_tables: Dict[tuple, torch.Tensor] = {}

    # gaussian_diffusion.py:149-187
    def _build_tables(self, betas: np.ndarray) -> None:
        betas = np.array(betas, dtype=np.float64)
        assert betas.ndim == 1 and (betas > 0).all() and (betas <= 1).all()
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)

    def _tables_on(self, device: torch.device) -> torch.Tensor:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        t = self._dev_tables.get(idx)
        if t is None:
            tab = np.stack([self.posterior_mean_coef1, self.posterior_mean_coef2, self.posterior_log_variance_clipped,
                            np.zeros_like(self.betas)], axis=1).astype(np.float32)
            t = torch.from_numpy(tab).to(device).contiguous()
            self._dev_tables[idx] = t
        return t

    def _variances_on(self, device: torch.device) -> torch.Tensor:
        """posterior_variance as a (T,) float32 table on ``device`` (holo_ddpm_step_guided), uploaded once like ``_tables_on``."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        v = self._dev_variances.get(idx)
        if v is None:
            v = self._dev_variances[idx] = torch.from_numpy(self.posterior_variance.astype(np.float32)).to(device).contiguous()
        return v

    @staticmethod
    def _extract(arr: np.ndarray, timesteps: torch.Tensor, shape) -> torch.Tensor:
        res = torch.from_numpy(arr).to(device=timesteps.device)[timesteps].float()
        while res.dim() < len(shape):
            res = res[..., None]
        return res.expand(shape)

    # ---- forward process (training-side helper; plain torch ops, not on the sampling path) ----
    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        assert noise.shape == x_start.shape
        return (self._extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + self._extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    # ---- reverse process -----------------------------------------------------------------------
    def _launch(self, entry: str, head, x, model_output, extras, clip_denoised, want_pred=True):
        """One plain step kernel, ``entry`` of the library: (sample, pred_xstart | None).  ``head`` are the entry's arguments
        between the context and the batch (its table or rows), ``extras`` its optional input tensors after the model output
        (guidance gradient, noise, history): None goes in as a null pointer."""
        runtime.require_device(x, "ImplicitronGaussianDiffusion")
        L = runtime.lib()
        dev = x.device
        x, model_output = x.contiguous(), model_output.contiguous()
        extras = [None if e is None else e.contiguous() for e in extras]
        sample = torch.empty_like(x)
        pred = torch.empty_like(x) if want_pred else None
        _lib.check(L, getattr(L, entry)(runtime.ctx(dev), *head, x.shape[0], x[0].numel(), runtime.ptr(x),
                                        runtime.ptr(model_output), *[None if e is None else runtime.ptr(e) for e in extras],
                                        1 if clip_denoised else 0, runtime.ptr(sample), runtime.ptr(pred) if want_pred else None,
                                        runtime.stream_ptr(dev)), entry)
        return sample, pred

    def _launch_device_noise(self, entry: str, head, x, model_output, timestep_index: int, clip_denoised, want_pred, want_noise,
                             channels_last: bool, grad=None):
        """One step kernel with in-kernel Philox noise (perf mode): (sample, pred_xstart | None, noise | None).  ``entry`` is the
        offset form (``holo_*_step_philox``); per-row streams go to its ``_rows`` form.  A draw is keyed on the LOGICAL element
        (seed, stream, timestep, sample, channel, voxel): ``channels_last`` says which layout ``x`` is in - an (N, R, R, R, C)
        chain and an (N, C, R, R, R) chain of the same seed draw the same noise (C a multiple of 4; otherwise the NCDHW
        tensor's memory order is the key).  With ``grad`` (a guided entry, ``holo_*_step_guided_philox``) the gradient follows
        the model output and the one entry takes both stream forms."""
        runtime.require_device(x, "ImplicitronGaussianDiffusion")
        L = runtime.lib()
        dev = x.device
        x, model_output = x.contiguous(), model_output.contiguous()
        inputs = [runtime.ptr(x), runtime.ptr(model_output)]
        if grad is not None:
            grad = grad.contiguous()
            inputs.append(runtime.ptr(grad))
        sample = torch.empty_like(x)
        pred = torch.empty_like(x) if want_pred else None
        noise = torch.empty_like(x) if want_noise else None
        ncdhw = 0 if (channels_last or x.dim() < 3 or x.shape[1] % 4) else int(x.shape[1])
        rows = self._row_streams(x.shape[0], dev)
        tidx = int(timestep_index) & 0xFFFFFFFF
        # one stream per row: each row draws its batch-1 chain's noise; else the stream offset (chain id, timestep) - distinct
        # for every step of every chain that shares the seed
        offset = 0 if rows is not None else (int(self.device_noise_stream) << 32) | tidx
        if grad is not None:  # one guided entry for both forms: (stream_offset, row_streams | NULL, timestep_index)
            key = (offset, None if rows is None else runtime.ptr(rows), tidx)
        elif rows is not None:
            entry += "_rows"
            key = (runtime.ptr(rows), tidx)
        else:
            key = (offset,)
        _lib.check(L, getattr(L, entry)(runtime.ctx(dev), *head, x.shape[0], x[0].numel(), *inputs,
                                        int(self.device_noise_seed) & 0xFFFFFFFFFFFFFFFF, *key,
                                        1 if clip_denoised else 0, runtime.ptr(sample), runtime.ptr(pred) if want_pred else None,
                                        runtime.ptr(noise) if want_noise else None, ncdhw, runtime.stream_ptr(dev)), entry)
        return sample, pred, noise

    def _ddpm_head(self, x, t):
        runtime.require_device(x, "ImplicitronGaussianDiffusion")  # (before the table is looked up on x's device)
        return runtime.ptr(self._tables_on(x.device)), self.num_timesteps, runtime.ptr(t)

    def _ddpm_guided_head(self, x, t):
        return (*self._ddpm_head(x, t), runtime.ptr(self._variances_on(x.device)))

    def _step(self, x, t, model_output, noise, clip_denoised, grad=None):
        """Fused HIP tail of p_sample: returns (sample, pred_xstart).  ``grad`` (a cond_fn's gradient): holo_ddpm_step_guided."""
        if grad is not None:
            return self._launch("holo_ddpm_step_guided", self._ddpm_guided_head(x, t), x, model_output, [grad, noise],
                                clip_denoised)
        return self._launch("holo_ddpm_step", self._ddpm_head(x, t), x, model_output, [noise], clip_denoised)

    @staticmethod
    def _guidance(cond_fn, x, t, model_kwargs):
        """The gradient of a step: ``cond_fn(x, t, **model_kwargs).float()`` (gaussian_diffusion.py:429-431, :449), x's shape."""
        grad = cond_fn(x, t, **(model_kwargs or {})).float()
        if grad.shape != x.shape:
            raise ValueError(f"cond_fn returned shape {tuple(grad.shape)} for x of shape {tuple(x.shape)}")
        return grad

    def _row_streams(self, batch: int, device: torch.device) -> Optional[torch.Tensor]:
        """``device_noise_stream`` as a (batch,) uint32 table on ``device`` (held as int32) when it is a sequence - the per-row
        streams of the ``_rows`` step kernels, uploaded once per (streams, device) -, None for a plain int."""
        s = self.device_noise_stream
        if isinstance(s, (int, np.integer)):
            return None
        ids = tuple(int(v) for v in s)
        if len(ids) != batch:
            raise ValueError(f"device_noise_stream has {len(ids)} streams for a batch of {batch}")
        if any(v < 0 or v > 0xFFFFFFFF for v in ids):
            raise ValueError(f"device_noise_stream: stream ids must be in [0, 2^32): {ids}")
        key = (ids, str(device))
        cache = self._row_stream_tables
        t = cache.get(key)
        if t is None:
            cache.clear()
            t = cache[key] = torch.from_numpy(np.asarray(ids, dtype=np.uint32).view(np.int32)).to(device)
        return t

    def _step_device_noise(self, x, t, model_output, timestep_index: int, clip_denoised, want_pred=True, want_noise=False,
                           channels_last: bool = False, grad=None):
        """holo_ddpm_step_philox: the step with in-kernel noise, (sample, pred_xstart | None, noise | None).  ``grad``:
        holo_ddpm_step_guided_philox, the same draw."""
        if grad is not None:
            return self._launch_device_noise("holo_ddpm_step_guided_philox", self._ddpm_guided_head(x, t), x, model_output,
                                             timestep_index, clip_denoised, want_pred, want_noise, channels_last, grad)
        return self._launch_device_noise("holo_ddpm_step_philox", self._ddpm_head(x, t), x, model_output,
                                         timestep_index, clip_denoised, want_pred, want_noise, channels_last)

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        if model_kwargs is None:
            model_kwargs = {}
        B = x.shape[0]
        assert t.shape == (B,)
        model_output = model(x, t, **model_kwargs)
        if denoised_fn is not None:
            model_output = denoised_fn(model_output)
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        # mean/pred_xstart from the fused kernel with zero noise: sample == mean
        mean, pred = self._step(x, t, model_output, torch.zeros_like(x), clip_denoised)
        return {
            "mean": mean,
            "variance": self._extract(self.posterior_variance, t, x.shape),
            "log_variance": self._extract(self.posterior_log_variance_clipped, t, x.shape),
            "pred_xstart": pred,
        }

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                 noise_sampler=None):
        """``cond_fn(x, t, **model_kwargs)`` (gaussian_diffusion.py:429-433, condition_mean): the gradient of a conditional
        log-probability with respect to x; the posterior mean moves by variance * gradient, pred_xstart does not."""
        if model_kwargs is None:
            model_kwargs = {}
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        model_output = model(x, t, **model_kwargs)
        if denoised_fn is not None:
            model_output = denoised_fn(model_output)
        grad = None if cond_fn is None else self._guidance(cond_fn, x, t, model_kwargs)
        if noise_sampler is None and self.device_noise_seed is not None:  # perf mode: noise drawn inside the kernel
            sample, pred, noise = self._step_device_noise(x, t, model_output, int(t[0].item()), clip_denoised, grad=grad)
            return {"sample": sample, "pred_xstart": pred, "noise": noise}  # ("noise": None - it never left the kernel)
        if noise_sampler is not None:
            noise = noise_sampler(int(t[0].item()), x.shape, x.device)  # same host sync as the reference (:495-496)
        else:
            noise = torch.randn_like(x)
        sample, pred = self._step(x, t, model_output, noise, clip_denoised, grad)
        return {"sample": sample, "pred_xstart": pred, "noise": noise}

    def _indices(self, max_iter: Optional[int]):
        indices = list(range(self.num_timesteps))[::-1]
        if max_iter is not None and len(indices) > max_iter:
            warnings.warn(f"Subsampling diffusion steps from {len(indices)} -> {max_iter}")
            if max_iter == 1:
                indices = [indices[0]]
            else:
                indices = [indices[int(i)] for i in torch.round(torch.linspace(0, len(indices) - 1, max_iter)).long()]
        return indices

    def _chain(self, model, shape, indices, rows, step, *, noise=None, noise_sampler=None, device=None, progress=False,
               denoised_fn=None, model_kwargs=None, channels_last_ok=True, materialize=True, pre=None) -> Iterator[dict]:
        """The chain loop of every sampler.  Starts from ``noise``, else ``noise_sampler(T, shape, device)``, else
        ``torch.randn``; uploads the timesteps ``indices`` and the sampler's host ``rows`` ((steps, batch, 8), or None) once, so
        that no step talks to the host; then per step k calls the model and ``step(k, x, t, model_output, rows[k] on the
        device, channels_last)``, which returns the step's dict (its "sample" is the next x; None values stay None).
        With ``channels_last_ok`` and a plain ``forward_channels_last`` model the chain stays in the library's channels-last
        layout - the step kernels are elementwise, hence layout-agnostic, and the model runs without its two layout passes -
        and the dicts are yielded in NCDHW all the same: contiguous copies, or with ``materialize`` off (the non-progressive
        loops, which convert the last sample only) views of the channels-last buffers.  ``pre(k, x, channels_last)`` (the
        masked loop's forward jumps) may replace x in front of step k's model call; nothing is yielded for it."""
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        if noise is not None:
            img = noise
        elif noise_sampler is not None:
            img = noise_sampler(self.num_timesteps, shape, device)
        else:
            img = torch.randn(*shape, device=device)
        ts_all = torch.tensor(indices, dtype=torch.int64, device=device)[:, None].expand(-1, shape[0]).contiguous()
        rows_all = rows.to(device) if rows is not None else [None] * len(indices)
        it = range(len(indices))
        if progress:
            try:
                from tqdm.auto import tqdm
                it = tqdm(it)
            except Exception:
                pass
        use_cl = (channels_last_ok and denoised_fn is None and not model_kwargs and hasattr(model, "forward_channels_last")
                  and getattr(model, "in_channels", None) == shape[1] and img.is_cuda)
        as_ncdhw = lambda a: a  # noqa: E731
        if use_cl:
            as_ncdhw = (lambda a: a.permute(0, 4, 1, 2, 3).contiguous()) if materialize else (lambda a: a.permute(0, 4, 1, 2, 3))
            img = img.float().permute(0, 2, 3, 4, 1).contiguous()
        with torch.no_grad():
            for k in it:
                t = ts_all[k]
                if pre is not None:
                    img = pre(k, img, use_cl)
                if use_cl:
                    model_output = model.forward_channels_last(img, t)
                else:
                    model_output = self._model_output(model, img, t, denoised_fn, model_kwargs)
                out = step(k, img, t, model_output, rows_all[k], use_cl)
                yield {name: None if v is None else as_ncdhw(v) for name, v in out.items()}
                img = out["sample"]

    @staticmethod
    def _last_sample(steps: Iterator[dict], keep: Optional[list] = None):
        """Runs a progressive loop to its end (collecting its dicts in ``keep``): the last sample, made contiguous - the
        channels-last chain's one conversion at the end."""
        final = None
        for out in steps:
            if keep is not None:
                keep.append(out)
            final = out["sample"]
        if final is not None and not final.is_contiguous():
            final = final.contiguous()
        return final

    def _device_noise(self, noise_sampler) -> bool:
        """Perf mode: the steps draw their noise in the kernel, and the chain may run channels-last."""
        return noise_sampler is None and self.device_noise_seed is not None

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, max_iter=None,
                                  noise_sampler=None, _materialize_every_step: bool = True) -> Iterator[dict]:
        """``_materialize_every_step`` (internal, used by ``p_sample_loop``): see ``_chain``.  ``cond_fn`` as in ``p_sample``: called
        once per step after the model, on the NCDHW x_t, under the loop's ``torch.no_grad()`` (gaussian_diffusion.py:551)."""
        indices = self._indices(max_iter)
        device_noise = self._device_noise(noise_sampler)

        def step(k, img, t, model_output, _, channels_last):
            grad = None if cond_fn is None else self._guidance(cond_fn, img, t, model_kwargs)
            if device_noise:  # (no host sync: indices[k] is host-side; "noise": None - it never leaves the kernel)
                sample, pred, eps = self._step_device_noise(img, t, model_output, indices[k], clip_denoised,
                                                            channels_last=channels_last, grad=grad)
            else:
                eps = noise_sampler(indices[k], img.shape, img.device) if noise_sampler is not None else torch.randn_like(img)
                sample, pred = self._step(img, t, model_output, eps, clip_denoised, grad)
            return {"sample": sample, "pred_xstart": pred, "noise": eps}

        yield from self._chain(model, shape, indices, None, step, noise=noise, noise_sampler=noise_sampler, device=device,
                               progress=progress, denoised_fn=denoised_fn, model_kwargs=model_kwargs,
                               channels_last_ok=device_noise and cond_fn is None, materialize=_materialize_every_step)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False, return_all_samples=False, max_iter=None,
                      noise_sampler=None):
        samples = [] if return_all_samples else None
        final = self._last_sample(self.p_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, max_iter=max_iter, noise_sampler=noise_sampler,
            _materialize_every_step=return_all_samples), samples)
        return (final, samples) if return_all_samples else final

    # ---- masked ancestral sampling (build-side extension; RePaint, Lugmayr et al. 2022, arXiv:2201.09865) -----------------
    def repaint_schedule(self, jump_length: int = 10, n_resample: int = 1, start_level: Optional[int] = None) -> list:
        """RePaint's jump schedule in LEVEL terms: level L runs from T (noise) to 0 (clean); ``("reverse", t)`` is the step at
        timestep index t = L - 1 that takes level L to L - 1, ``("forward", L, L + j)`` the jump of ``jump_length`` back up.
        Every level in ``range(0, T - j, j)`` is left ``n_resample - 1`` times by a forward jump, so ``n_resample == 1`` is the
        plain descending list; the schedule ends with ``("reverse", 0)``.  ``start_level`` (None: T) starts the walk there and
        drops the jumps that would go above it."""
        T, j, r = self.num_timesteps, int(jump_length), int(n_resample)
        if j < 1:
            raise ValueError(f"jump_length must be >= 1, got {jump_length}")
        if r < 1:
            raise ValueError(f"n_resample must be >= 1, got {n_resample}")
        top = T if start_level is None else int(start_level)
        if not 1 <= top <= T:
            raise ValueError(f"start_level must be in [1, {T}], got {start_level}")
        jumps = {L: r - 1 for L in range(0, T - j, j) if L + j <= top}
        ops, L = [], top
        while L >= 1:
            ops.append(("reverse", L - 1))
            L -= 1
            if jumps.get(L, 0) > 0:
                jumps[L] -= 1
                ops.append(("forward", L, L + j))
                L += j
        return ops

    @staticmethod
    def _ab_rows(a: np.ndarray, b: np.ndarray) -> torch.Tensor:
        """(n, 2) float32 rows {a, b} of holo_ddpm_step_inpaint / holo_q_sample: float64 values cast once."""
        return torch.from_numpy(np.stack([np.asarray(a, np.float64), np.asarray(b, np.float64)], axis=-1).astype(np.float32))

    def known_coefs(self, t: Sequence[int]) -> torch.Tensor:
        """The rows of the masked step's known part at timesteps ``t``: q_sample's coefficients one level down,
        (sqrt(alphas_cumprod_prev[t]), sqrt(1 - alphas_cumprod_prev[t])) - (1, 0) at t = 0."""
        t = np.asarray(t, dtype=np.int64).reshape(-1)
        return self._ab_rows(np.sqrt(self.alphas_cumprod_prev[t]), np.sqrt(1.0 - self.alphas_cumprod_prev[t]))

    def q_sample_coefs(self, t: Sequence[int]) -> torch.Tensor:
        """The rows with which holo_q_sample is ``q_sample`` at timesteps ``t``."""
        t = np.asarray(t, dtype=np.int64).reshape(-1)
        return self._ab_rows(self.sqrt_alphas_cumprod[t], self.sqrt_one_minus_alphas_cumprod[t])

    def jump_coefs(self, level_from: Sequence[int], level_to: Sequence[int]) -> torch.Tensor:
        """The rows of the composed forward jump from level L to a higher level L': a = sqrt(abar[L' - 1] / abar[L - 1]) with
        abar[-1] = 1, b = sqrt(1 - a^2), in float64 - in distribution the L' - L single q steps between the two levels."""
        lo = np.asarray(level_from, dtype=np.int64).reshape(-1)
        hi = np.asarray(level_to, dtype=np.int64).reshape(-1)
        if lo.shape != hi.shape or (lo < 0).any() or (hi <= lo).any() or (hi > self.num_timesteps).any():
            raise ValueError(f"invalid forward jump levels {lo.tolist()} -> {hi.tolist()}")
        abar = np.append(self.alphas_cumprod, 1.0)  # (abar[-1] = 1: level 0 is the clean grid)
        a = np.sqrt(abar[hi - 1] / abar[lo - 1])
        return self._ab_rows(a, np.sqrt(1.0 - a * a))

    def _philox_key(self, batch: int, device, timestep_index: int):
        """(stream_offset, row_streams pointer | None, timestep_index) of the entries that take both stream forms, as
        ``_launch_device_noise`` forms them; the table is returned too, to keep it alive over the launch."""
        rows = self._row_streams(batch, device)
        tidx = int(timestep_index) & 0xFFFFFFFF
        offset = 0 if rows is not None else (int(self.device_noise_stream) << 32) | tidx
        return (offset, None if rows is None else runtime.ptr(rows), tidx), rows

    def _step_inpaint(self, x, t, model_output, known, mask, coefs_dev, noise, noise_known, clip_denoised, want_pred=True,
                      channels_last: bool = False, timestep_index: Optional[int] = None, want_noise: bool = False):
        """holo_ddpm_step_inpaint: (sample, pred_xstart | None) from the injected ``noise`` / ``noise_known`` (None where every
        row is at t = 0).  With ``timestep_index`` instead: holo_ddpm_step_inpaint_philox, both noises drawn in the kernel,
        (sample, pred_xstart | None, noise | None, noise_known | None).  ``known`` in x's layout (``channels_last``), ``mask``
        (N, 1, R, R, R), ``coefs_dev`` the (N, 2) ``known_coefs`` rows on the device."""
        runtime.require_device(x, "ImplicitronGaussianDiffusion")
        L = runtime.lib()
        dev = x.device
        x, model_output, known, mask = x.contiguous(), model_output.contiguous(), known.contiguous(), mask.contiguous()
        if known.shape != x.shape or mask.numel() * (x.shape[-1] if channels_last else x.shape[1]) != x.numel():
            raise ValueError(f"known {tuple(known.shape)} / mask {tuple(mask.shape)} do not belong to x {tuple(x.shape)}")
        sample = torch.empty_like(x)
        pred = torch.empty_like(x) if want_pred else None
        opt = lambda a: None if a is None else runtime.ptr(a)  # noqa: E731
        head = (runtime.ctx(dev), *self._ddpm_head(x, t), runtime.ptr(coefs_dev), x.shape[0], x[0].numel(),
                int(x.shape[-1] if channels_last else x.shape[1]), 0 if channels_last else 1, runtime.ptr(x),
                runtime.ptr(model_output), runtime.ptr(known), runtime.ptr(mask))
        if timestep_index is None:
            noise, noise_known = noise.contiguous(), None if noise_known is None else noise_known.contiguous()
            _lib.check(L, L.holo_ddpm_step_inpaint(*head, runtime.ptr(noise), opt(noise_known), 1 if clip_denoised else 0,
                                                   runtime.ptr(sample), opt(pred), runtime.stream_ptr(dev)),
                       "holo_ddpm_step_inpaint")
            return sample, pred
        e_u = torch.empty_like(x) if want_noise else None
        e_k = torch.empty_like(x) if want_noise else None
        key, _rows = self._philox_key(x.shape[0], dev, timestep_index)
        _lib.check(L, L.holo_ddpm_step_inpaint_philox(*head, int(self.device_noise_seed) & 0xFFFFFFFFFFFFFFFF, *key,
                                                      1 if clip_denoised else 0, runtime.ptr(sample), opt(pred), opt(e_u),
                                                      opt(e_k), runtime.stream_ptr(dev)), "holo_ddpm_step_inpaint_philox")
        return sample, pred, e_u, e_k

    def _q_sample_rows(self, x, coefs_dev, noise=None, channels_last: bool = False, timestep_index: Optional[int] = None,
                       want_noise: bool = False):
        """holo_q_sample: a*x + b*noise on the (N, 2) rows ``coefs_dev``.  With ``timestep_index`` instead of ``noise``:
        holo_q_sample_philox, (out, noise | None), the draw keyed on the logical element as in ``_launch_device_noise``."""
        runtime.require_device(x, "ImplicitronGaussianDiffusion")
        L = runtime.lib()
        dev = x.device
        x = x.contiguous()
        out = torch.empty_like(x)
        if timestep_index is None:
            noise = noise.contiguous()
            _lib.check(L, L.holo_q_sample(runtime.ctx(dev), runtime.ptr(coefs_dev), x.shape[0], x[0].numel(), runtime.ptr(x),
                                          runtime.ptr(noise), runtime.ptr(out), runtime.stream_ptr(dev)), "holo_q_sample")
            return out
        e = torch.empty_like(x) if want_noise else None
        ncdhw = 0 if (channels_last or x.dim() < 3 or x.shape[1] % 4) else int(x.shape[1])
        key, _rows = self._philox_key(x.shape[0], dev, timestep_index)
        _lib.check(L, L.holo_q_sample_philox(runtime.ctx(dev), runtime.ptr(coefs_dev), x.shape[0], x[0].numel(), runtime.ptr(x),
                                             int(self.device_noise_seed) & 0xFFFFFFFFFFFFFFFF, *key, runtime.ptr(out),
                                             None if e is None else runtime.ptr(e), ncdhw, runtime.stream_ptr(dev)),
                   "holo_q_sample_philox")
        return out, e

    def inpaint_sample_loop_progressive(self, model, shape, known, mask, jump_length=10, n_resample=1, start_level=None,
                                        init=None, noise=None, clip_denoised=True, denoised_fn=None, model_kwargs=None,
                                        device=None, progress=False, noise_sampler=None, cond_fn=None, max_iter=None,
                                        _materialize_every_step: bool = True) -> Iterator[dict]:
        """Masked DDPM sampling: where ``mask`` ((N, 1, R, R, R) or (1, 1, R, R, R), float in [0, 1], broadcast over the
        channels) is 1 the chain carries the clean grid ``known`` ((N | 1, C, R, R, R)) noised to the step's level, where it
        is 0 the diffusion prior generates - one ``holo_ddpm_step_inpaint*`` launch per step beside the model call.  The walk
        is ``repaint_schedule(jump_length, n_resample, start_level)``; a forward jump is ONE composed ``holo_q_sample*``
        launch (``jump_coefs``).  ``start_level = L0 < T`` starts from ``q_sample(init, L0 - 1)`` (``init`` None: ``known``)
        instead of from noise: editing.  One dict per reverse step, as ``p_sample_loop_progressive``.
        Noise: with ``device_noise_seed`` (perf mode; the chain runs channels-last) everything is drawn in the kernels, at
        Philox timestep index t + T * visit, visit = the earlier visits of timestep t in the schedule (forward jumps: of
        their target level, the start counting as one) - a first visit draws what the unmasked chain draws.  Otherwise
        ``noise_sampler(i, shape, device)``, else ``torch.randn_like``; i = t for a first visit's step noise (as
        ``p_sample_loop`` asks) and t + (T + 1) * (3 * visit + d) for the known part's (d = 1), a jump's or the start's
        (d = 2) and any revisit's noise; ``noise`` is x_T, or the start's noise when ``start_level < T``.
        Refused (ValueError): ``cond_fn``, ``max_iter``, a mask of another shape, ``jump_length`` / ``n_resample`` < 1,
        ``start_level`` outside [1, T].  Whether ``jump_length=10, n_resample=1`` (or RePaint's 10 / 10) suits a trained
        checkpoint is not measured: there is no checkpoint to measure it on."""
        if cond_fn is not None:
            raise ValueError("cond_fn: guidance is not supported by the masked loops; use p_sample_loop or ddim_sample_loop")
        if max_iter is not None:
            raise ValueError("max_iter: the masked loops walk the full schedule; shorten the chain with start_level")
        T = self.num_timesteps
        ops = self.repaint_schedule(jump_length, n_resample, start_level)
        shape = tuple(int(s) for s in shape)
        B = shape[0]
        if len(shape) != 5 or mask.dim() != 5 or tuple(mask.shape[1:]) != (1, *shape[2:]) or mask.shape[0] not in (1, B):
            raise ValueError(f"mask must be ({B}, 1, R, R, R) or (1, 1, R, R, R) for shape {shape}, got {tuple(mask.shape)}")
        if known.dim() != 5 or tuple(known.shape[1:]) != shape[1:] or known.shape[0] not in (1, B):
            raise ValueError(f"known must be ({B} | 1, C, R, R, R) for shape {shape}, got {tuple(known.shape)}")
        if device is None:
            device = next(model.parameters()).device
        known = known.to(device=device, dtype=torch.float32).expand(shape).contiguous()
        mask = mask.to(device=device, dtype=torch.float32).expand(B, *mask.shape[1:]).contiguous()
        device_noise = self._device_noise(noise_sampler)

        # the reverse steps are the chain's steps; a forward jump rides in front of the step that follows it
        indices, visits, jump_before, seen = [], [], {}, {}
        top = ops[0][1] + 1
        fwd_seen = {top: 1} if top < T else {}
        for op in ops:
            if op[0] == "reverse":
                indices.append(op[1])
                visits.append(seen.get(op[1], 0))
                seen[op[1]] = visits[-1] + 1
            else:
                jump_before[len(indices)] = (len(jump_before), op[2] - 1, fwd_seen.get(op[2], 0))
                fwd_seen[op[2]] = fwd_seen.get(op[2], 0) + 1
        rows = torch.stack([self.known_coefs([t] * B) for t in indices])  # (steps, B, 2)
        jumps = [op for op in ops if op[0] == "forward"]
        jump_rows = torch.stack([self.jump_coefs([op[1]] * B, [op[2]] * B) for op in jumps]).to(device) if jumps else None

        def draw(d, t, visit, like):
            if noise_sampler is None:
                return torch.randn_like(like)
            i = t if (d == 0 and visit == 0) else t + (T + 1) * (3 * visit + d)
            return noise_sampler(i, like.shape, like.device)

        def forward_noised(x, coefs, t, visit, channels_last, given=None):
            if given is not None:
                return self._q_sample_rows(x, coefs, given)
            if device_noise:
                return self._q_sample_rows(x, coefs, channels_last=channels_last, timestep_index=t + T * visit)[0]
            return self._q_sample_rows(x, coefs, draw(2, t, visit, x))

        if top < T:  # editing: the chain starts from the partly noised grid
            start = known if init is None else init.to(device=device, dtype=torch.float32).expand(shape)
            noise = forward_noised(start.contiguous(), self.q_sample_coefs([top - 1] * B).to(device), top - 1, 0, False, noise)
        known_by_layout = {False: known}

        def pre(k, img, channels_last):
            jump = jump_before.get(k)
            if jump is None:
                return img
            return forward_noised(img, jump_rows[jump[0]], jump[1], jump[2], channels_last)

        def step(k, img, t, model_output, coefs, channels_last):
            kn = known_by_layout.get(channels_last)
            if kn is None:  # (the one conversion of the known grid; the mask is per voxel: the same memory in both layouts)
                kn = known_by_layout[channels_last] = known.permute(0, 2, 3, 4, 1).contiguous()
            tt, visit = indices[k], visits[k]
            if device_noise:  # ("noise": None - it never leaves the kernel)
                sample, pred, eps, _ = self._step_inpaint(img, t, model_output, kn, mask, coefs, None, None, clip_denoised,
                                                          channels_last=channels_last, timestep_index=tt + T * visit)
            else:
                eps = draw(0, tt, visit, img)
                sample, pred = self._step_inpaint(img, t, model_output, kn, mask, coefs, eps,
                                                  draw(1, tt, visit, img) if tt != 0 else None, clip_denoised)
            return {"sample": sample, "pred_xstart": pred, "noise": eps}

        yield from self._chain(model, shape, indices, rows, step, noise=noise, noise_sampler=noise_sampler, device=device,
                               progress=progress, denoised_fn=denoised_fn, model_kwargs=model_kwargs,
                               channels_last_ok=device_noise, materialize=_materialize_every_step, pre=pre)

    def inpaint_sample_loop(self, model, shape, known, mask, jump_length=10, n_resample=1, start_level=None, init=None,
                            noise=None, clip_denoised=True, denoised_fn=None, model_kwargs=None, device=None, progress=False,
                            noise_sampler=None, cond_fn=None, max_iter=None):
        """The last sample of ``inpaint_sample_loop_progressive``: ``known`` where the mask is 1, generated where it is 0."""
        return self._last_sample(self.inpaint_sample_loop_progressive(
            model, shape, known, mask, jump_length=jump_length, n_resample=n_resample, start_level=start_level, init=init,
            noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, model_kwargs=model_kwargs, device=device,
            progress=progress, noise_sampler=noise_sampler, cond_fn=cond_fn, max_iter=max_iter,
            _materialize_every_step=False))

    # ---- DDIM (gaussian_diffusion.py:645-815) ----------------------------------------------------
    def ddim_schedule(self, ddim_steps: Optional[int] = None, timesteps: Optional[Sequence[int]] = None) -> List[int]:
        """The timesteps a DDIM loop visits, descending: all T (None), guided-diffusion's "ddimS" spacing (``ddim_steps``),
        or an explicit strictly decreasing list (``timesteps``)."""
        T = self.num_timesteps
        if timesteps is not None:
            if ddim_steps is not None:
                raise ValueError("give ddim_steps or timesteps, not both")
            ts = [int(t) for t in timesteps]
            if not ts or any(a <= b for a, b in zip(ts, ts[1:])) or ts[0] >= T or ts[-1] < 0:
                raise ValueError(f"timesteps must be a non-empty strictly decreasing list in [0, {T}): {ts}")
            return ts
        if ddim_steps is None:
            return list(range(T))[::-1]
        return ddim_timesteps(T, ddim_steps)

    def ddim_coefs(self, t: Sequence[int], t_other: Sequence[int], eta: float = 0.0, reverse: bool = False) -> torch.Tensor:
        """(batch, 8) float32 rows of holo_ddim_step (include/holo_abi.h), on the host, in float32 with torch ops in the
        reference's order (gaussian_diffusion.py:677-689, :717-724).  ``t_other`` is the timestep stepped to: t_prev for a
        sampling step (< 0: past the end of the chain, abar = 1), t_next for a reverse step (>= T: abar = 0)."""
        t = np.asarray(t, dtype=np.int64).reshape(-1)
        t_other = np.asarray(t_other, dtype=np.int64).reshape(-1)
        if t.shape != t_other.shape or (t < 0).any() or (t >= self.num_timesteps).any():
            raise ValueError(f"invalid DDIM step timesteps {t.tolist()} -> {t_other.tolist()}")
        ac = self.alphas_cumprod
        f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).float()  # noqa: E731  (_extract_into_tensor's cast)
        # float32 sqrt, correctly rounded: torch's CPU sqrt may go through a vector math library whose last bit depends on
        # the host CPU, which would make the rows (and the sampled grids) differ between machines
        sqrt = lambda a: torch.from_numpy(np.sqrt(a.numpy()))  # noqa: E731
        row = torch.zeros((t.shape[0], 8), dtype=torch.float32)
        row[:, 0] = f32(self.sqrt_recip_alphas_cumprod[t])
        row[:, 1] = f32(self.sqrt_recipm1_alphas_cumprod[t])
        if reverse:
            assert eta == 0.0, "Reverse ODE only for deterministic path"
            alpha_bar_next = f32(np.where(t_other < self.num_timesteps, ac[np.minimum(t_other, self.num_timesteps - 1)], 0.0))
            row[:, 2] = sqrt(alpha_bar_next)
            row[:, 3] = sqrt(1 - alpha_bar_next)
            return row
        alpha_bar = f32(ac[t])
        alpha_bar_prev = f32(np.where(t_other >= 0, ac[np.maximum(t_other, 0)], 1.0))
        sigma = eta * sqrt((1 - alpha_bar_prev) / (1 - alpha_bar)) * sqrt(1 - alpha_bar / alpha_bar_prev)
        row[:, 2] = sqrt(alpha_bar_prev)
        row[:, 3] = sqrt(1 - alpha_bar_prev - sigma ** 2)
        row[:, 4] = torch.from_numpy(t != 0).float() * sigma
        return row

    def ddim_guided_coefs(self, t: Sequence[int], t_prev: Sequence[int], eta: float = 0.0) -> torch.Tensor:
        """The rows of holo_ddim_step_guided: ``ddim_coefs`` with slot 5 = sqrt(1 - abar_t), the factor of the gradient in
        condition_score (gaussian_diffusion.py:445-451): float32, from the float32 cast of alphas_cumprod[t]."""
        row = self.ddim_coefs(t, t_prev, eta)
        alpha_bar = torch.from_numpy(self.alphas_cumprod[np.asarray(t, dtype=np.int64).reshape(-1)]).float()
        row[:, 5] = torch.from_numpy(np.sqrt((1 - alpha_bar).numpy()))  # (correctly rounded, as ddim_coefs' sqrt)
        return row

    def _ddim_step(self, x, model_output, coefs_dev, noise, clip_denoised, want_pred=True, grad=None):
        """holo_ddim_step: (sample, pred_xstart | None).  ``coefs_dev`` is the (batch, 8) row block on the device.  ``grad`` (a
        cond_fn's gradient): holo_ddim_step_guided on ``ddim_guided_coefs`` rows."""
        if grad is not None:
            return self._launch("holo_ddim_step_guided", [runtime.ptr(coefs_dev)], x, model_output, [grad, noise],
                                clip_denoised, want_pred)
        return self._launch("holo_ddim_step", [runtime.ptr(coefs_dev)], x, model_output, [noise], clip_denoised, want_pred)

    def _ddim_step_device_noise(self, x, model_output, coefs_dev, timestep_index: int, clip_denoised, want_pred=True,
                                want_noise=False, channels_last: bool = False, grad=None):
        """holo_ddim_step_philox: (sample, pred_xstart | None, noise | None), the draw of ``_step_device_noise`` at the same
        (seed, stream, timestep).  ``grad``: holo_ddim_step_guided_philox."""
        entry = "holo_ddim_step_philox" if grad is None else "holo_ddim_step_guided_philox"
        return self._launch_device_noise(entry, [runtime.ptr(coefs_dev)], x, model_output, timestep_index,
                                         clip_denoised, want_pred, want_noise, channels_last, grad)

    @staticmethod
    def _per_sample(v, t: torch.Tensor) -> np.ndarray:
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        return np.broadcast_to(np.asarray(v, dtype=np.int64), (t.shape[0],)).copy()

    def _model_output(self, model, x, t, denoised_fn, model_kwargs):
        model_output = model(x, t, **(model_kwargs or {}))
        if denoised_fn is not None:
            model_output = denoised_fn(model_output)
        return model_output

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0,
                    t_prev=None, noise_sampler=None):
        """One DDIM step t -> t_prev (default t - 1; < 0: the end of the chain).  The noise: ``noise_sampler(t, shape,
        device)``, else the in-kernel draw with ``device_noise_seed``, else ``torch.randn_like``; none is drawn when every
        sample's sigma is 0 (eta = 0, or t = 0).  ``cond_fn(x, t, **model_kwargs)`` (gaussian_diffusion.py:445-453,
        condition_score): the score moves by sqrt(1 - abar_t) * gradient, and pred_xstart is re-derived from it."""
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        t_host = t.cpu().numpy()
        t_prev = t_host - 1 if t_prev is None else self._per_sample(t_prev, t)
        coefs = (self.ddim_coefs if cond_fn is None else self.ddim_guided_coefs)(t_host, t_prev, eta)
        model_output = self._model_output(model, x, t, denoised_fn, model_kwargs)
        grad = None if cond_fn is None else self._guidance(cond_fn, x, t, model_kwargs)
        coefs_dev = coefs.to(x.device)
        if noise_sampler is None and self.device_noise_seed is not None:
            sample, pred, _ = self._ddim_step_device_noise(x, model_output, coefs_dev, int(t_host[0]), clip_denoised,
                                                           grad=grad)
            return {"sample": sample, "pred_xstart": pred}
        noise = None
        if bool((coefs[:, 4] != 0).any()):
            noise = noise_sampler(int(t_host[0]), x.shape, x.device) if noise_sampler is not None else torch.randn_like(x)
        sample, pred = self._ddim_step(x, model_output, coefs_dev, noise, clip_denoised, grad=grad)
        return {"sample": sample, "pred_xstart": pred}

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0,
                            t_next=None):
        """One reverse-ODE step t -> t_next (default t + 1; >= T: abar_next = 0)."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        t = t.to(device=x.device, dtype=torch.int64).contiguous()
        t_host = t.cpu().numpy()
        t_next = t_host + 1 if t_next is None else self._per_sample(t_next, t)
        coefs = self.ddim_coefs(t_host, t_next, reverse=True)
        model_output = self._model_output(model, x, t, denoised_fn, model_kwargs)
        sample, pred = self._ddim_step(x, model_output, coefs.to(x.device), None, clip_denoised)
        return {"sample": sample, "pred_xstart": pred}

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, ddim_steps=None,
                                     timesteps=None, noise_sampler=None, _materialize_every_step: bool = True
                                     ) -> Iterator[dict]:
        """DDIM over ``ddim_schedule(ddim_steps, timesteps)``.  Noise and the perf mode as ``p_sample_loop_progressive``:
        with ``device_noise_seed`` the chain runs channels-last through ``holo_ddim_step_philox``.  The coefficient rows of
        the whole chain are built on the host and uploaded once.  ``cond_fn`` as in ``ddim_sample``: called once per step after
        the model, on the NCDHW x_t, under the loop's ``torch.no_grad()``; the chain then runs NCDHW on the guided rows."""
        indices = self.ddim_schedule(ddim_steps, timesteps)
        B = shape[0]
        coefs_of = self.ddim_coefs if cond_fn is None else self.ddim_guided_coefs
        rows = torch.stack([coefs_of([t] * B, [t_prev] * B, eta)
                            for t, t_prev in zip(indices, indices[1:] + [-1])])  # (steps, B, 8)
        noisy = (rows[:, :, 4] != 0).any(dim=1).tolist()
        device_noise = self._device_noise(noise_sampler)

        def step(k, img, t, model_output, coefs, channels_last):
            grad = None if cond_fn is None else self._guidance(cond_fn, img, t, model_kwargs)
            if device_noise:
                sample, pred, _ = self._ddim_step_device_noise(img, model_output, coefs, indices[k], clip_denoised,
                                                               channels_last=channels_last, grad=grad)
            else:
                eps = None
                if noisy[k]:
                    eps = noise_sampler(indices[k], img.shape, img.device) if noise_sampler is not None else \
                        torch.randn_like(img)
                sample, pred = self._ddim_step(img, model_output, coefs, eps, clip_denoised, grad=grad)
            return {"sample": sample, "pred_xstart": pred}

        yield from self._chain(model, shape, indices, rows, step, noise=noise, noise_sampler=noise_sampler, device=device,
                               progress=progress, denoised_fn=denoised_fn, model_kwargs=model_kwargs,
                               channels_last_ok=device_noise and cond_fn is None, materialize=_materialize_every_step)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, ddim_steps=None, timesteps=None,
                         noise_sampler=None):
        return self._last_sample(self.ddim_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, eta=eta, ddim_steps=ddim_steps, timesteps=timesteps,
            noise_sampler=noise_sampler, _materialize_every_step=False))

    def ddim_reverse_sample_loop(self, model, x0, ddim_steps=None, timesteps=None, clip_denoised=True, denoised_fn=None,
                                 model_kwargs=None) -> torch.Tensor:
        """DDIM inversion (build-side extension): the reverse ODE from x0 over the schedule of ``ddim_sample_loop`` walked in
        ascending order; each step goes to the next kept timestep, the last one to abar = 0.  Returns x_T."""
        indices = self.ddim_schedule(ddim_steps, timesteps)[::-1]
        B = x0.shape[0]
        rows = torch.stack([self.ddim_coefs([t] * B, [t_next] * B, reverse=True)
                            for t, t_next in zip(indices, indices[1:] + [self.num_timesteps])])

        def step(k, img, t, model_output, coefs, channels_last):
            return {"sample": self._ddim_step(img, model_output, coefs, None, clip_denoised, want_pred=False)[0]}

        return self._last_sample(self._chain(model, tuple(x0.shape), indices, rows, step, noise=x0, device=x0.device,
                                             denoised_fn=denoised_fn, model_kwargs=model_kwargs, channels_last_ok=False))

    # ---- DPM-Solver++ multistep (build-side extension; Lu et al. 2022, arXiv:2211.01095, Algorithm 2 and its order-3 form) ----
    def log_snr(self) -> np.ndarray:
        """lambda_t = log(alpha_t / sigma_t), alpha = sqrt(abar), sigma = sqrt(1 - abar): float64, decreasing in t."""
        return np.log(self.sqrt_alphas_cumprod / self.sqrt_one_minus_alphas_cumprod)

    def dpm_schedule(self, steps: Optional[int] = None, spacing: str = "logsnr",
                     timesteps: Optional[Sequence[int]] = None) -> List[int]:
        """The timesteps a DPM-Solver++ loop visits, descending.  ``steps`` (None: 20) with ``spacing``:
          "logsnr"  for each of ``linspace(lambda_{T-1}, lambda_0, steps)`` the timestep of the nearest log-SNR (ties: the
                    smaller t), duplicates removed - so the list may be SHORTER than ``steps`` where the table's timesteps are
                    coarser than the targets (T = 1000: 20 -> 20, 50 -> 49, 100 -> 94).  More than one step: from T-1 to 0
          "time"    ``ddim_schedule(steps)``, the "ddimS" stride
        or an explicit strictly decreasing list (``timesteps``, validated as in ``ddim_schedule``)."""
        if timesteps is not None:
            if steps is not None:
                raise ValueError("give steps or timesteps, not both")
            return self.ddim_schedule(timesteps=timesteps)
        steps = DPM_DEFAULT_STEPS if steps is None else int(steps)
        if steps < 1:
            raise ValueError(f"dpm_schedule: steps must be >= 1, got {steps}")
        if spacing == "time":
            return self.ddim_schedule(steps)
        if spacing != "logsnr":
            raise ValueError(f"dpm_schedule: spacing must be 'logsnr' or 'time', not {spacing!r}")
        lam = self.log_snr()
        out: List[int] = []
        for target in np.linspace(lam[-1], lam[0], steps):
            t = int(np.argmin(np.abs(lam - target)))  # (the first minimum: ties go to the smaller t)
            if not out or t < out[-1]:
                out.append(t)
        return out

    def dpm_coefs(self, indices: Sequence[int], order: int = 2, lower_order_final: bool = True):
        """The chain over ``indices`` (descending timesteps; the last step goes past the end, abar = 1) as the rows of
        holo_dpm_step (include/holo_abi.h): ((steps, 8) float32 rows {a, b0, b1, b2, 0, 0, 0, 0}, [effective order per step]).
        Step k (s = indices[k] -> t = indices[k + 1], h = lambda_t - lambda_s) is the multistep DPM-Solver++ update of order
        min(order, k + 1) on the predictions m0, m1, m2 at s and the two timesteps before it, expanded into
        x_t = a*x + b0*m0 + b1*m1 + b2*m2 in float64 and rounded once.  The step past the end is (0, 1, 0, 0): the sample is
        the prediction.  ``lower_order_final``: that last step counts as the order-1 one, and with order 3 the step before it
        is at most order 2 (the high-order extrapolation is unstable over the large final log-SNR steps)."""
        order = int(order)
        if order not in (1, 2, 3):
            raise ValueError(f"dpm_coefs: order must be 1, 2 or 3, got {order}")
        idx = self.ddim_schedule(timesteps=indices)
        n = len(idx)
        alpha, sigma, lam = self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, self.log_snr()
        rows = np.zeros((n, 8), dtype=np.float64)
        orders: List[int] = []
        for k, s in enumerate(idx):
            if k == n - 1:  # t = -1: sigma_t = 0, alpha_t = 1, h = inf
                rows[k, 1] = 1.0
                orders.append(1)
                continue
            t = idx[k + 1]
            eff = min(order, k + 1)
            if lower_order_final and order == 3 and k == n - 2:  # (the only step the flag changes: the last is order 1 anyway)
                eff = min(eff, 2)
            h = lam[t] - lam[s]
            phi1 = np.expm1(-h)
            a, b0, b1, b2 = sigma[t] / sigma[s], -alpha[t] * phi1, 0.0, 0.0
            if eff == 2:
                r0 = (lam[s] - lam[idx[k - 1]]) / h
                d = -0.5 * alpha[t] * phi1 / r0  # the weight of m0 - m1
                b0, b1 = b0 + d, -d
            elif eff == 3:
                r0, r1 = (lam[s] - lam[idx[k - 1]]) / h, (lam[idx[k - 1]] - lam[idx[k - 2]]) / h
                phi2 = phi1 / h + 1.0
                phi3 = phi2 / h - 0.5
                c = r0 / (r0 + r1)
                p = alpha[t] * (phi2 * (1.0 + c) - phi3 / (r0 + r1)) / r0  # the weight of m0 - m1
                q = alpha[t] * (phi3 / (r0 + r1) - phi2 * c) / r1          # the weight of m1 - m2
                b0, b1, b2 = b0 + p, q - p, -q
            rows[k, :4] = (a, b0, b1, b2)
            orders.append(eff)
        return torch.from_numpy(rows.astype(np.float32)), orders

    def _dpm_step(self, x, model_output, coefs_dev, hist1, hist2, clip_denoised, want_pred=True):
        """holo_dpm_step: (sample, pred_xstart | None).  ``coefs_dev`` is the (batch, 8) row block on the device; ``hist1`` /
        ``hist2`` (the previous two steps' pred_xstart) may be None: the term is dropped."""
        return self._launch("holo_dpm_step", [runtime.ptr(coefs_dev)], x, model_output, [hist1, hist2], clip_denoised, want_pred)

    def dpm_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, model_kwargs=None,
                                    device=None, progress=False, steps=None, order=2, spacing="logsnr", timesteps=None,
                                    lower_order_final=True, noise_sampler=None, cond_fn=None,
                                    _materialize_every_step: bool = True) -> Iterator[dict]:
        """DPM-Solver++ multistep sampling over ``dpm_schedule(steps, spacing, timesteps)`` (``steps`` None: 20): one model call
        per step, like DDIM, on ``holo_dpm_step``.  Deterministic: ``noise_sampler`` is asked for x_T only (when ``noise`` is
        None), no step draws anything, and ``device_noise_seed`` plays no part.  The chain's rows and timesteps are uploaded
        once; a step reads the one or two previous predictions the order needs.  With a ``forward_channels_last`` model the
        chain stays channels-last (the step kernel is elementwise) under the DDIM loop's conditions minus the noise ones."""
        if cond_fn is not None:
            raise NotImplementedError("cond_fn guidance is not supported by the DPM-Solver++ loops: guidance on the multistep "
                                      "history is a separate piece of work; use p_sample_loop or ddim_sample_loop")
        indices = self.dpm_schedule(steps, spacing, timesteps)
        rows, orders = self.dpm_coefs(indices, order, lower_order_final)
        hist = [None, None]  # the predictions of the previous two steps, in the chain's layout

        def step(k, img, t, model_output, coefs, channels_last):
            sample, pred = self._dpm_step(img, model_output, coefs, hist[0] if orders[k] >= 2 else None,
                                          hist[1] if orders[k] >= 3 else None, clip_denoised)
            hist[:] = pred, hist[0]
            return {"sample": sample, "pred_xstart": pred}

        yield from self._chain(model, shape, indices, rows[:, None, :].expand(-1, shape[0], -1).contiguous(), step, noise=noise,
                               noise_sampler=noise_sampler, device=device, progress=progress, denoised_fn=denoised_fn,
                               model_kwargs=model_kwargs, materialize=_materialize_every_step)

    def dpm_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, model_kwargs=None, device=None,
                        progress=False, steps=None, order=2, spacing="logsnr", timesteps=None, lower_order_final=True,
                        noise_sampler=None, cond_fn=None):
        return self._last_sample(self.dpm_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, model_kwargs=model_kwargs,
            device=device, progress=progress, steps=steps, order=order, spacing=spacing, timesteps=timesteps,
            lower_order_final=lower_order_final, noise_sampler=noise_sampler, cond_fn=cond_fn, _materialize_every_step=False))

    # ---- losses and the variational bound (gaussian_diffusion.py:817-1043) ---------------------------------------------
    def vb_coefs(self, t: Sequence[int]) -> torch.Tensor:
        """(n, 8) float32 rows of holo_vb_terms at timesteps ``t``, float64 values cast once: {posterior_mean_coef1,
        posterior_mean_coef2, lv, exp(-lv), exp(-0.5*lv), sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, [t == 0]}
        with lv = posterior_log_variance_clipped[t] - every transcendental of a per-row scalar is taken here."""
        t = np.asarray(t, dtype=np.int64).reshape(-1)
        lv = self.posterior_log_variance_clipped[t]
        rows = np.stack([self.posterior_mean_coef1[t], self.posterior_mean_coef2[t], lv, np.exp(-lv), np.exp(-0.5 * lv),
                         self.sqrt_recip_alphas_cumprod[t], self.sqrt_recipm1_alphas_cumprod[t], (t == 0).astype(np.float64)],
                        axis=1)
        return torch.from_numpy(rows.astype(np.float32))

    def _loss_tables_on(self, device: torch.device):
        """((T, 2) q_sample rows, (T, 8) vb rows) on ``device``, uploaded once: a batch's rows are gathered by its device
        timesteps, so ``training_losses`` needs no host copy of ``t``."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        cache = self.__dict__.setdefault("_dev_loss_tables", {})
        tabs = cache.get(idx)
        if tabs is None:
            every = np.arange(self.num_timesteps)
            tabs = cache[idx] = (self.q_sample_coefs(every).to(device), self.vb_coefs(every).to(device))
        return tabs

    @staticmethod
    def _loss_workspace(x: torch.Tensor) -> torch.Tensor:
        nbytes = int(runtime.lib().holo_diffusion_loss_workspace_bytes(x.shape[0], x[0].numel()))
        if nbytes == 0:
            raise _lib.HoloError("holo_diffusion_loss_workspace_bytes: " + (runtime.lib().holo_last_error() or b"").decode())
        return torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)

    def _diffusion_loss(self, target, model_out, row_scale=None, want_terms=True, want_grad=False):
        """holo_diffusion_loss: ((N, 2) float64 {mse, huber} | None, grad_out | None) in one launch.  ``row_scale`` (N,) float32
        on the device: float(2 * w_b / n) of the cotangent of sum_b w_b * mse_b (None: every w_b is 1)."""
        runtime.require_device(target, "ImplicitronGaussianDiffusion")
        L = runtime.lib()
        dev = target.device
        target, model_out = target.contiguous().float(), model_out.contiguous().float()
        if target.shape != model_out.shape:
            raise ValueError(f"model output {tuple(model_out.shape)} does not match the target {tuple(target.shape)}")
        ws = self._loss_workspace(target)
        terms = torch.empty((target.shape[0], 2), dtype=torch.float64, device=dev) if want_terms else None
        grad = torch.empty_like(model_out) if want_grad else None
        opt = lambda a: None if a is None else runtime.ptr(a)  # noqa: E731
        row_scale = None if row_scale is None else row_scale.contiguous()
        _lib.check(L, L.holo_diffusion_loss(runtime.ctx(dev), target.shape[0], target[0].numel(), runtime.ptr(target),
                                            runtime.ptr(model_out), opt(row_scale), opt(terms), opt(grad), runtime.ptr(ws),
                                            ws.numel() * 8, runtime.stream_ptr(dev)), "holo_diffusion_loss")
        return terms, grad

    def _vb_terms(self, coefs_dev, x_start, x_t, noise, model_out, clip_denoised, out=None):
        """holo_vb_terms on the (N, 8) ``vb_coefs`` rows ``coefs_dev``: (N, 3) float64 {vb in bits, xstart_mse, eps_mse}
        (into ``out`` when given); ``noise`` None: no eps term."""
        runtime.require_device(x_start, "ImplicitronGaussianDiffusion")
        L = runtime.lib()
        dev = x_start.device
        x_start, x_t, model_out = x_start.contiguous().float(), x_t.contiguous().float(), model_out.contiguous().float()
        noise = None if noise is None else noise.contiguous().float()
        if not (x_start.shape == x_t.shape == model_out.shape) or (noise is not None and noise.shape != x_start.shape):
            raise ValueError(f"x_t {tuple(x_t.shape)}, the noise and the model output {tuple(model_out.shape)} must have "
                             f"x_start's shape {tuple(x_start.shape)}")
        ws = self._loss_workspace(x_start)
        if out is None:
            out = torch.empty((x_start.shape[0], 3), dtype=torch.float64, device=dev)
        _lib.check(L, L.holo_vb_terms(runtime.ctx(dev), runtime.ptr(coefs_dev), x_start.shape[0], x_start[0].numel(),
                                      runtime.ptr(x_start), runtime.ptr(x_t), None if noise is None else runtime.ptr(noise),
                                      runtime.ptr(model_out), 1 if clip_denoised else 0, runtime.ptr(out), runtime.ptr(ws),
                                      ws.numel() * 8, runtime.stream_ptr(dev)), "holo_vb_terms")
        return out

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """One term of the variational bound in bits per dimension (gaussian_diffusion.py:817-850): the KL between the true
        and the model's posterior at t > 0, the decoder's negative log-likelihood at t == 0.  ``{"output": (N,),
        "pred_xstart"}``."""
        runtime.require_device(x_start, "ImplicitronGaussianDiffusion._vb_terms_bpd")
        t = t.to(device=x_start.device, dtype=torch.int64)
        with torch.no_grad():
            model_output = model(x_t, t, **(model_kwargs or {}))
            terms = self._vb_terms(self._loss_tables_on(x_start.device)[1][t], x_start, x_t, None, model_output, clip_denoised)
            pred = model_output.clamp(-1, 1) if clip_denoised else model_output
        return {"output": terms[:, 0].float(), "pred_xstart": pred}

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, get_xstart=False, clip_denoised=False,
                        denoised_fn=None, x_start_for_error=None):
        """The training losses of one timestep batch (gaussian_diffusion.py:852-968; START_X, MSE): ``{"x_t", "mse", "huber",
        "loss" (= mse), "noise", "model_output"}`` and ``"pred_xstart"`` with ``get_xstart``.  x_t is one ``holo_q_sample``
        launch - with ``device_noise_seed`` and no ``noise`` one ``holo_q_sample_philox`` launch that also reports its draw
        (stream index ``training_draw_index``, which then advances) -, the two losses one ``holo_diffusion_loss`` launch.  With
        autograd enabled and a model output that requires grad, ``mse`` / ``loss`` carry an autograd node whose backward is the
        kernel's ``grad_out`` form with the upstream gradient as row weights: ``terms["loss"].mean().backward()`` reaches the
        denoiser's parameters through its own node.  ``huber`` is detached."""
        runtime.require_device(x_start, "ImplicitronGaussianDiffusion.training_losses")
        dev = x_start.device
        t = t.to(device=dev, dtype=torch.int64)
        x_start = x_start.contiguous().float()
        q_rows = self._loss_tables_on(dev)[0][t]
        if noise is None and self.device_noise_seed is not None:
            index = self.__dict__.get("training_draw_index", 0)
            self.__dict__["training_draw_index"] = index + 1
            x_t, noise = self._q_sample_rows(x_start, q_rows, timestep_index=index, want_noise=True)
        else:
            if noise is None:
                noise = torch.randn_like(x_start)
            if noise.shape != x_start.shape:
                raise ValueError(f"noise {tuple(noise.shape)} does not match x_start {tuple(x_start.shape)}")
            x_t = self._q_sample_rows(x_start, q_rows, noise.to(dev).float())
        if x_start_for_error is not None:  # (gaussian_diffusion.py:882-883: only the returned noise changes under START_X)
            noise = ((self._extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - x_start_for_error)
                     / self._extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape))
        terms = {"x_t": x_t}
        model_output = model(x_t, t, **(model_kwargs or {}))
        if get_xstart:
            pred = model_output if denoised_fn is None else denoised_fn(model_output)
            terms["pred_xstart"] = pred.clamp(-1, 1) if clip_denoised else pred
        if model_output.shape != x_start.shape:
            raise ValueError(f"model output {tuple(model_output.shape)} does not match x_start {tuple(x_start.shape)}")
        if torch.is_grad_enabled() and model_output.requires_grad:
            terms["mse"], terms["huber"] = _DiffusionLossFn.apply(self, x_start, model_output)
        else:
            both, _ = self._diffusion_loss(x_start, model_output)
            terms["mse"], terms["huber"] = both[:, 0].float(), both[:, 1].float()
        terms["loss"] = terms["mse"]
        terms["noise"] = noise
        terms["model_output"] = model_output
        return terms

    def _prior_bpd(self, x_start):
        """The prior term of the bound in bits per dimension (gaussian_diffusion.py:970-986): KL(q(x_T | x_0) || N(0, 1)), a
        per-row scalar formula on mean(x_0^2) - the loss kernel's mse against a zero target.  (N,) float32."""
        m2 = self._diffusion_loss(torch.zeros_like(x_start), x_start)[0][:, 0]
        a = float(self.sqrt_alphas_cumprod[-1])
        lv = float(self.log_one_minus_alphas_cumprod[-1])
        return ((0.5 * (-1.0 - lv + float(np.exp(lv))) + (0.5 * a * a) * m2) / float(np.log(2.0))).float()

    @torch.no_grad()
    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, noise_sampler=None, timesteps=None):
        """The variational bound in bits per dimension and its parts (gaussian_diffusion.py:988-1043): ``{"total_bpd",
        "prior_bpd", "vb", "xstart_mse", "mse"}``, the last three (N, T) with the reference's column order (t = T - 1 first).
        Build-side extensions: ``noise_sampler(t, shape, device)`` supplies the draws (else the in-kernel draw with
        ``device_noise_seed``, else ``torch.randn_like``); ``timesteps`` restricts the loop to these timesteps, in this order -
        then the columns follow them and ``total_bpd`` is left out.  Per timestep: one q_sample launch, one model call, one
        ``holo_vb_terms`` launch; the rows of the whole loop are uploaded once, the results stay on the device, and nothing
        synchronises."""
        runtime.require_device(x_start, "ImplicitronGaussianDiffusion.calc_bpd_loop")
        dev = x_start.device
        x_start = x_start.contiguous().float()
        B, T = x_start.shape[0], self.num_timesteps
        ts = list(range(T))[::-1] if timesteps is None else [int(v) for v in timesteps]
        if not ts or min(ts) < 0 or max(ts) >= T:
            raise ValueError(f"calc_bpd_loop: timesteps must be in [0, {T}), got {ts}")
        rep = np.repeat(np.asarray(ts, dtype=np.int64), B)
        t_all = torch.from_numpy(rep).to(dev).view(len(ts), B)
        q_rows = self.q_sample_coefs(rep).to(dev).view(len(ts), B, 2)
        vb_rows = self.vb_coefs(rep).to(dev).view(len(ts), B, 8)
        out = torch.empty((len(ts), B, 3), dtype=torch.float64, device=dev)
        for k, ti in enumerate(ts):
            if noise_sampler is not None:
                noise = noise_sampler(ti, tuple(x_start.shape), dev)
                x_t = self._q_sample_rows(x_start, q_rows[k], noise.to(dev).float())
            elif self.device_noise_seed is not None:
                x_t, noise = self._q_sample_rows(x_start, q_rows[k], timestep_index=ti, want_noise=True)
            else:
                noise = torch.randn_like(x_start)
                x_t = self._q_sample_rows(x_start, q_rows[k], noise)
            model_output = model(x_t, t_all[k], **(model_kwargs or {}))
            self._vb_terms(vb_rows[k], x_start, x_t, noise, model_output, clip_denoised, out=out[k])
        prior = self._prior_bpd(x_start)
        res = {"prior_bpd": prior, "vb": out[:, :, 0].t().float(), "xstart_mse": out[:, :, 1].t().float(),
               "mse": out[:, :, 2].t().float()}
        if timesteps is None:
            res["total_bpd"] = (out[:, :, 0].sum(dim=0) + prior.double()).float()
        return res

    def sample_timesteps(self, *args, **kwargs):
        return self._schedule_sampler.sample(*args, **kwargs)


class _DiffusionLossFn(torch.autograd.Function):
    """Autograd node of ``training_losses``: forward = the terms form of holo_diffusion_loss, (mse, huber) per sample;
    backward = its grad_out form, (model_out - target) * float(2 * g_b / n) with g_b the upstream gradient of mse_b, formed
    in double on the device and rounded once.  ``huber`` is not differentiable; the target gets no gradient."""

    @staticmethod
    def forward(ctx, diffusion, target, model_out):
        ctx.diffusion = diffusion
        target, model_out = target.detach(), model_out.detach()
        ctx.save_for_backward(target, model_out)
        terms, _ = diffusion._diffusion_loss(target, model_out)
        mse, huber = terms[:, 0].float(), terms[:, 1].float()
        ctx.mark_non_differentiable(huber)
        return mse, huber

    @staticmethod
    def backward(ctx, g_mse, _g_huber):
        target, model_out = ctx.saved_tensors
        scale = (g_mse.double() * 2.0 / target[0].numel()).float()
        _, grad = ctx.diffusion._diffusion_loss(target, model_out, row_scale=scale, want_terms=False, want_grad=True)
        return None, None, grad
