"""View guidance for the samplers: a ready-made ``cond_fn`` that pulls a sampled grid towards posed photographs.

``PhotometricGuidance`` is the ``cond_fn`` of ``ImplicitronGaussianDiffusion.p_sample*`` / ``ddim_sample*``
(gaussian_diffusion.py:420-457): for the chain's x_t it returns the gradient, with respect to x_t, of ``-scale * L`` where L is
the photometric loss of the TRAINING branch's render of the denoised grid against the observed views.  Every expensive part
is an existing HIP entry point: the taped denoiser forward and its backward to the input (``SimpleUnet3D.forward_train`` /
``backward_taped``), the training-mode renderer on explicit rays and its backward to the grid (``holo_render_rays`` /
``holo_render_rays_backward``).  The loss itself is a few torch ops on the per-ray tensors, as in ``training_step``.

Cost per step (not optimised here): one taped forward + backward of the denoiser next to the loop's own forward, one render
forward and backward (the latter also forms the RenderMLP's parameter gradients and synchronises the stream).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .render import EvaluationMode, RenderSamplingMode


def xys_to_pixels(xys: torch.Tensor, height: int, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (row, column) pixel indices of ray-sampler ``xys`` (..., 2) that are pixel centres of a ``height`` x ``width`` frame
    in PyTorch3D's NDC - the shorter side spans [-1, 1], x and y decrease with the column / row index:
    ``x_j = rx - (2j + 1) * rx / W`` (``linspace(rx - rx/W, -rx + rx/W, W)``), rx = max(W / H, 1), and likewise for y."""
    H, W = int(height), int(width)
    rx, ry = (W / H, 1.0) if W >= H else (1.0, H / W)
    col = torch.round(((rx - xys[..., 0].double()) * (W / rx) - 1.0) * 0.5).long()
    row = torch.round(((ry - xys[..., 1].double()) * (H / ry) - 1.0) * 0.5).long()
    if bool(((col < 0) | (col >= W) | (row < 0) | (row >= H)).any()):
        raise ValueError(f"xys outside the {H} x {W} frame")
    return row, col


class PhotometricGuidance:
    """``cond_fn(x_t, t)`` for one grid (batch 1) observed in ``len(camera)`` posed views.

      model          : HoloDiffusionModel with the two-pass renderer and the denoiser in the fp32 mode (the backward is fp32)
      camera         : the views' cameras
      image_rgb      : (n_views, 3, H, W) at the ray sampler's frame size - a ray's target colour is an exact pixel lookup
      fg_probability : (n_views, 1, H, W) or None - the per-pixel weight w of the loss (None: 1)
      mask_crop      : (n_views, 1, H, W) or None - the rays are drawn from its support (None: the whole frame)
      scale          : the guidance strength s: the return value is d(-s * L) / d x_t
      n_rays_per_view: rays per view and call (None: the ray sampler's ``n_rays_per_image_sampled_from_mask``)
      seed           : of the generator all draws of all calls come from (rays, stratified depths, density noise), created
                       on the first call: a chain is reproducible

    L = mean_{views, rays, channels} w * (rgb - target)^2 of the fine pass + the same of the coarse pass (the reference's
    ``loss_rgb_mse`` and ``loss_prev_stage_rgb_mse``, weight 1.0 each).  ``last_loss`` holds L of the last call as a device
    scalar (no synchronisation), ``last_rng_streams`` its draws (``xys`` and the renderer's streams: what
    ``training_step`` needs to repeat the call)."""

    def __init__(self, model, camera, image_rgb: torch.Tensor, fg_probability: Optional[torch.Tensor] = None,
                 mask_crop: Optional[torch.Tensor] = None, scale: float = 1.0, n_rays_per_view: Optional[int] = None,
                 seed: int = 0):
        n = len(camera)
        H, W = int(model.raysampler.image_height), int(model.raysampler.image_width)
        if tuple(image_rgb.shape) != (n, 3, H, W):
            raise ValueError(f"image_rgb must be {(n, 3, H, W)} (one frame per camera at the ray sampler's size), "
                             f"got {tuple(image_rgb.shape)}")
        for name, m in (("fg_probability", fg_probability), ("mask_crop", mask_crop)):
            if m is not None and tuple(m.shape) != (n, 1, H, W):
                raise ValueError(f"{name} must be {(n, 1, H, W)}, got {tuple(m.shape)}")
        self.model, self.camera = model, camera
        self.image_rgb = image_rgb.float()
        self.fg_probability = None if fg_probability is None else fg_probability.float()
        self.mask_crop = mask_crop
        self.scale = float(scale)
        self.n_rays_per_view = None if n_rays_per_view is None else int(n_rays_per_view)
        self.seed = int(seed)
        self._generator: Optional[torch.Generator] = None
        self.last_loss: Optional[torch.Tensor] = None
        self.last_rng_streams: Optional[Dict[str, torch.Tensor]] = None

    def _gen(self, device: torch.device) -> torch.Generator:
        g = self._generator
        if g is None or g.device.type != device.type:
            g = self._generator = torch.Generator(device=device)
            g.manual_seed(self.seed)
        return g

    def photometric_loss(self, preds: Dict[str, torch.Tensor], xys: torch.Tensor) -> torch.Tensor:
        """L for the rays ``xys`` (n_views, n_rays, 2): ``preds["images_render"]`` and ``preds["images_render_coarse"]`` are
        (n_views, 3, n_rays, 1), as ``training_step`` hands them to its ``loss_fn``."""
        dev = preds["images_render"].device
        n = xys.shape[0]
        row, col = xys_to_pixels(xys.reshape(n, -1, 2), *self.image_rgb.shape[2:])
        view = torch.arange(n, device=row.device)[:, None]
        target = self.image_rgb.to(dev)[view, :, row, col].permute(0, 2, 1)[..., None]  # (n_views, 3, n_rays, 1)
        w = 1.0 if self.fg_probability is None else self.fg_probability.to(dev)[view, :, row, col].permute(0, 2, 1)[..., None]
        return sum((w * (preds[k] - target) ** 2).mean() for k in ("images_render", "images_render_coarse"))

    def _render_streams(self, bundle, n_passes: int, device, gen) -> Dict[str, torch.Tensor]:
        """The renderer's training draws (HoloMultiPassEmissionAbsorptionRenderer._forward_training) from this generator."""
        r = self.model.renderer
        n_cam, n_rays = int(bundle.xys.shape[0]), int(bundle.xys.shape[1])
        P, Pf, noisy, two_pass = int(bundle.n_pts_per_ray), int(r.n_pts_per_ray_fine_training), \
            float(r.density_noise_std_train) > 0.0, n_passes > 1
        rs = {}
        if bundle.stratified:
            rs["u_coarse"] = torch.rand((n_cam, n_rays, P), device=device, generator=gen)
        if two_pass and r.stratified_sampling_coarse_training:
            rs["u_fine"] = torch.rand((n_cam, n_rays, Pf), device=device, generator=gen)
        if noisy:
            rs["noise_coarse"] = torch.randn((n_cam, n_rays, P), device=device, generator=gen)
        if noisy and two_pass:
            rs["noise_fine"] = torch.randn((n_cam, n_rays, P + Pf), device=device, generator=gen)
        return rs

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, t: torch.Tensor, **model_kwargs) -> torch.Tensor:
        model = self.model
        net = model.net_3d
        if x.shape[0] != 1:
            raise ValueError(f"PhotometricGuidance guides one grid (the renderer takes one): got a batch of {x.shape[0]}")
        if getattr(net, "compute_dtype", "f32") != "f32":
            raise ValueError(f"PhotometricGuidance needs the denoiser's fp32 mode (its backward is fp32 only), "
                             f"not {net.compute_dtype!r}")
        dev = x.device
        gen = self._gen(dev)
        cams = self.camera.to(dev)
        y = net.forward_train(x, t)
        grid = y.clamp(-1.0, 1.0)  # (the grid the training branch renders)
        H, W = self.image_rgb.shape[2:]
        mask = self.mask_crop.to(dev) if self.mask_crop is not None else torch.ones((len(cams), 1, H, W), device=dev)
        fns = list(model._implicit_functions)
        for func in fns:
            func.bind_args(voxel_grid_features=grid)
        try:
            bundle = model.raysampler(cams, EvaluationMode.TRAINING, sampling_mode=RenderSamplingMode.MASK_SAMPLE, mask=mask,
                                      n_rays=self.n_rays_per_view, generator=gen)
            xys = bundle.xys.reshape(len(cams), -1, 2)
            rs = self._render_streams(bundle, len(fns), dev, gen)
            rend = model.renderer(ray_bundle=bundle, implicit_functions=fns, evaluation_mode=EvaluationMode.TRAINING,
                                  rng_streams=rs)
            if rend.prev_stage is None:
                raise NotImplementedError("PhotometricGuidance: the two-pass renderer (coarse + fine implicit function)")
            leaves = {"images_render": rend.features, "images_render_coarse": rend.prev_stage.features}
            leaves = {k: v.permute(0, 3, 1, 2).detach().clone().requires_grad_(True) for k, v in leaves.items()}
            with torch.enable_grad():
                loss = self.photometric_loss(leaves, xys)
                cots = torch.autograd.grad(loss, list(leaves.values()))
            grads = {k: g.permute(0, 2, 3, 1).contiguous() for k, g in zip(("features", "features_coarse"), cots)}
            g_grid, _ = model.renderer.backward_training(bundle, fns, rs, grads)
        finally:
            for func in fns:
                func.unbind_args()
        g_y = g_grid * ((y >= -1.0) & (y <= 1.0)).to(g_grid.dtype)  # torch.clamp passes the gradient inside [min, max]
        g_x, _ = net.backward_taped(g_y, params=[])
        self.last_loss = loss.detach()
        self.last_rng_streams = dict(rs, xys=xys)
        return -self.scale * g_x
