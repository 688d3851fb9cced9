// render_exec.cpp — host side of the fused renderer: RenderMLP parameter binding, the float64 fold of
// the activation-free density net, per-camera depth bounds and the frame launch.
//
// Reference interfaces replaced (relative to /root/reference/holo_diffusion):
//   RenderMLP / MLPWithInputSkips parameters   holo_voxel_grid_implicit_function.py:73-92,
//                                              custom_modules.py:94-113 (state_dict names `mlp.<i>.0.*`)
//   AdaptiveRaySampler depth bounds            configs/apple.yaml:135-146 (PyTorch3D get_min_max_depth_bounds)
//   HoloDiffusionModel.forward render section  holo_diffusion_model.py:431-457,515-523
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/holo_abi.h"
#include "holo_common.h"
#include "holo_kernels.h"
#include "host_params.h"
#include "mlp_folds.h"

using namespace holo;

struct HoloRenderer {
  HoloCtx* ctx;
  HoloRenderCfg cfg;
  Knobs knobs;  // snapshot of holo_renderer_create (holo_knobs.h): the render family shapes the scratch and every launch
  HostParams params;        // raw parameters (host copies)
  float* packed = nullptr;  // device: w_feat | b_feat | w_dens | w_rad | w_dir | u_rad | w_fnet [Fd][Hd] | b_fnet [Fd]
  size_t fnet_off = 0;      // offset (floats) of w_fnet inside `packed`
  float k_rad[3] = {0, 0, 0};
  float b_dens = 0.f;
  float b_rad[3] = {0, 0, 0};
  bool committed = false;
  int split3 = 0;  // holo_renderer_set_compute_dtype
  // backward of the training-mode renderer: the float64 stages of the density-net fold (kept by holo_renderer_commit),
  // device copies of the folded weights in the GEMM layouts, the parameter gradients of the last backward
  DensityFold fold;
  float* bwd_pack = nullptr;  // WeP [Hp][C] | WeT [C][Hp] | be [Hp]
  bool bwd_pack_valid = false;
  HostGrads grads{"holo_render_rays_backward"};
  float* stage = nullptr;  // staging buffer of upload_via_stage (commit / backward re-packs)
  size_t stage_floats = 0;
};

static int dir_emb(const HoloRenderCfg& c) { return 3 * (2 * c.dir_emb_dims + 1); }

extern "C" {

int holo_renderer_create(HoloCtx* ctx, const HoloRenderCfg* cfg, HoloRenderer** out) {
  if (!ctx || !cfg || !out) {
    set_error("holo_renderer_create: null argument");
    return HOLO_E_INVALID;
  }
  if (cfg->dnet_hidden_dim != 256 || cfg->dir_emb_dims != 4 ||
      !(cfg->feature_size == 16 || cfg->feature_size == 32 || cfg->feature_size == 64 || cfg->feature_size == 128) ||
      cfg->n_pts_coarse < 3 || cfg->n_pts_coarse > 64 || cfg->n_pts_fine < 2 || cfg->resol < 2 || cfg->feature_dim < 0 ||
      (cfg->feature_dim & 3)) {
    set_error("holo_renderer_create: unsupported configuration (hidden 256, dir_emb 4, feature_size 16/32/64/128, "
              "3<=n_pts_coarse<=64, n_pts_fine>=2, feature_dim a multiple of 4)");
    return HOLO_E_UNSUPPORTED;
  }
  // the scene: each of these reaches the kernels as a divisor, a depth bound or a compositing constant
  const char* bad = nullptr;
  if (!(isfinite(cfg->volume_extent) && cfg->volume_extent > 0.f)) bad = "volume_extent must be finite and > 0";
  else if (!(isfinite(cfg->scene_extent) && cfg->scene_extent > 0.f)) bad = "scene_extent must be finite and > 0";
  else if (!(isfinite(cfg->background_opacity) && cfg->background_opacity >= 0.f)) bad = "background_opacity must be finite and >= 0";
  for (int k = 0; k < 3 && !bad; ++k) {
    if (!isfinite(cfg->scene_center[k])) bad = "scene_center must be finite";
    else if (!isfinite(cfg->bg_color[k])) bad = "bg_color must be finite";
  }
  if (bad) {
    set_error("holo_renderer_create: %s", bad);
    return HOLO_E_INVALID;
  }
  HoloRenderer* r = new HoloRenderer;
  r->ctx = ctx;
  r->cfg = *cfg;
  r->knobs = Knobs::from_env();
  const int64_t C = cfg->feature_size, Hd = cfg->dnet_hidden_dim, De = dir_emb(*cfg);
  r->params.declare("_density_net.mlp.0.0.weight", {Hd, C});
  r->params.declare("_density_net.mlp.0.0.bias", {Hd});
  r->params.declare("_density_net.mlp.1.0.weight", {Hd, Hd});
  r->params.declare("_density_net.mlp.1.0.bias", {Hd});
  r->params.declare("_density_net.mlp.2.0.weight", {Hd, Hd + C});
  r->params.declare("_density_net.mlp.2.0.bias", {Hd});
  r->params.declare("_density_net.mlp.3.0.weight", {Hd + 1, Hd});
  r->params.declare("_density_net.mlp.3.0.bias", {Hd + 1});
  r->params.declare("_radiance_net.mlp.0.0.weight", {3, Hd + De});
  r->params.declare("_radiance_net.mlp.0.0.bias", {3});
  const int64_t Fd = cfg->feature_dim;
  if (Fd > 0) {  // the view-point independent feature head (holo_voxel_grid_implicit_function.py:94-105,125-129)
    r->params.declare("_feature_net.mlp.0.0.weight", {Fd, Hd});
    r->params.declare("_feature_net.mlp.0.0.bias", {Fd});
  }
  r->fnet_off = (size_t)(Hd * C + Hd + C + 3 * Hd + 3 * De + 3 * C + 64);
  const size_t n = r->fnet_off + (size_t)(Fd * Hd + Fd);
  if (hipMalloc((void**)&r->packed, n * sizeof(float)) != hipSuccess) {
    set_error("holo_renderer_create: hipMalloc failed");
    delete r;
    return HOLO_E_HIP;
  }
  *out = r;
  return 0;
}

int holo_renderer_destroy(HoloRenderer* r) {
  if (!r) return 0;
  if (r->packed) (void)hipFree(r->packed);
  if (r->bwd_pack) (void)hipFree(r->bwd_pack);
  if (r->stage) (void)hipFree(r->stage);
  r->grads.release();
  delete r;
  return 0;
}

int holo_renderer_set_param(HoloRenderer* r, const char* name, const void* dev_ptr, int dtype, int ndim,
                            const int64_t* shape, void* stream) {
  if (!r || !name || !dev_ptr) {
    set_error("holo_renderer_set_param: null argument");
    return HOLO_E_INVALID;
  }
  if (dtype != HOLO_DTYPE_F32) {
    set_error("holo_renderer_set_param: only fp32 parameters are supported");
    return HOLO_E_UNSUPPORTED;
  }
  const int rc = r->params.set("holo_renderer_set_param", name, dev_ptr, ndim, shape, stream);
  if (!rc) r->committed = false;
  return rc;
}

// Folds the activation-free density net (mlp_folds.h) and uploads the forward kernels' image of the RenderMLP.
int holo_renderer_commit(HoloRenderer* r, void* stream) {
  if (!r) {
    set_error("holo_renderer_commit: null");
    return HOLO_E_INVALID;
  }
  if (const char* missing = r->params.first_missing()) {
    set_error("holo_renderer_commit: parameter '%s' has not been set", missing);
    return HOLO_E_STATE;
  }
  const int C = r->cfg.feature_size, Hd = r->cfg.dnet_hidden_dim, De = dir_emb(r->cfg);
  const HostParams& P = r->params;
  r->fold = fold_density_net(P["_density_net.mlp.0.0.weight"], P["_density_net.mlp.0.0.bias"], P["_density_net.mlp.1.0.weight"],
                             P["_density_net.mlp.1.0.bias"], P["_density_net.mlp.2.0.weight"], P["_density_net.mlp.2.0.bias"],
                             P["_density_net.mlp.3.0.weight"], P["_density_net.mlp.3.0.bias"], C, Hd);
  RenderMlpPack pk = pack_render_mlp(r->fold, P["_radiance_net.mlp.0.0.weight"], P["_radiance_net.mlp.0.0.bias"], C, Hd, De);
  r->b_dens = pk.b_dens;
  for (int c = 0; c < 3; ++c) r->k_rad[c] = pk.k_rad[c], r->b_rad[c] = pk.b_rad[c];
  r->bwd_pack_valid = false;
  r->grads.clear();
  if (r->cfg.feature_dim > 0) {  // the feature head's weights and bias follow the folded pack at fnet_off
    const auto &Wf = P["_feature_net.mlp.0.0.weight"], &bf = P["_feature_net.mlp.0.0.bias"];
    pk.image.resize(r->fnet_off + Wf.size() + bf.size(), 0.f);
    memcpy(pk.image.data() + r->fnet_off, Wf.data(), Wf.size() * sizeof(float));
    memcpy(pk.image.data() + r->fnet_off + Wf.size(), bf.data(), bf.size() * sizeof(float));
  }
  if (upload_via_stage(&r->stage, &r->stage_floats, r->packed, pk.image.data(), pk.image.size(), stream)) {
    set_error("holo_renderer_commit: upload of the packed RenderMLP failed");
    return HOLO_E_HIP;
  }
  r->committed = true;
  return 0;
}

}  // extern "C"

static void fill_mlp(const HoloRenderer* r, MlpParams& m) {
  const int C = r->cfg.feature_size, Hd = r->cfg.dnet_hidden_dim, De = dir_emb(r->cfg);
  m.w_feat = r->packed;
  m.b_feat = m.w_feat + (size_t)Hd * C;
  m.w_dens = m.b_feat + Hd;
  m.w_rad = m.w_dens + C;
  m.w_dir = m.w_rad + 3 * Hd;
  m.u_rad = m.w_dir + 3 * De;
  m.b_dens = r->b_dens;
  for (int k = 0; k < 3; ++k) {
    m.b_rad[k] = r->b_rad[k];
    m.k_rad[k] = r->k_rad[k];
  }
  m.Hd = Hd;
}

static size_t grid_cl_bytes(const HoloRenderer* r) {
  const size_t R = r->cfg.resol;
  return align256(R * R * R * (size_t)r->cfg.feature_size * sizeof(float));
}
static int64_t grid_voxels(const HoloRenderer* r) { return (int64_t)r->cfg.resol * r->cfg.resol * r->cfg.resol; }
// the caller's NCDHW grid as channels-last voxels at the head of the workspace (null: the launcher refused)
static float* grid_to_channels_last(const HoloRenderer* r, const float* grid, void* workspace, void* stream) {
  float* grid_cl = (float*)workspace;
  return ncdhw_to_ndhwc_launch(grid, grid_cl, 1, r->cfg.feature_size, grid_voxels(r), 0, stream) ? nullptr : grid_cl;
}
// the state checks of the entries that evaluate the RenderMLP
enum Needs { COMMITTED, COLOURS, COLOURS_UP_TO_64 };
static int ready(const char* entry, const HoloRenderer* r, Needs needs) {
  if (!r->committed) {
    set_error("%s: call holo_renderer_commit after setting the RenderMLP parameters", entry);
    return HOLO_E_STATE;
  }
  if (needs == COLOURS && r->cfg.feature_dim != 0) {
    set_error("%s: rendered view-point independent features are not on this path (HoloDiffusionModel builds its "
              "implicit function with feature_dim = 0, holo_diffusion_model.py:156)", entry);
    return HOLO_E_UNSUPPORTED;
  }
  if (needs == COLOURS_UP_TO_64 && (r->cfg.feature_dim != 0 || r->cfg.feature_size > 64)) {
    set_error("%s: colours only, feature_size 16/32/64", entry);
    return HOLO_E_UNSUPPORTED;
  }
  return 0;
}
// The plan of this handle's frames (holo_render) or ray lists (holo_render_rays: exact fp32, no normals): kernel, waves,
// workgroup cap, workspace layout (render_plan.h).  From the handle's own snapshot of the knobs, so the size query, the
// binding and the launch see one value.
static RenderPlan frame_plan(const HoloRenderer* r, bool normals) {
  const HoloRenderCfg& c = r->cfg;
  const bool split3 = r->split3 && c.feature_size == 32;
  return render_plan({c.feature_size, c.n_pts_coarse, c.n_pts_fine, normals, split3, false, c.resol, c.dnet_hidden_dim},
                     r->ctx->num_cus, r->knobs, EMU_BUILD);
}
static RenderPlan rays_plan(const HoloRenderer* r) {
  const HoloRenderCfg& c = r->cfg;
  return render_plan({c.feature_size, c.n_pts_coarse, c.n_pts_fine, false, false, true, c.resol, c.dnet_hidden_dim},
                     r->ctx->num_cus, r->knobs, EMU_BUILD);
}

static void fill_cam(const HoloRenderCfg& c, const HoloCamera& cam, RenderKernelParams::Cam& pc) {
  for (int k = 0; k < 9; ++k) pc.Rm[k] = cam.R[k];
  for (int k = 0; k < 3; ++k) pc.T[k] = cam.T[k];
  for (int k = 0; k < 2; ++k) {
    pc.focal[k] = cam.focal[k];
    pc.pp[k] = cam.principal_point[k];
  }
  // AdaptiveRaySampler: near/far from the camera centre C = -T R^T (fp32, as torch computes it)
  float d2 = 0.f;
  for (int j = 0; j < 3; ++j) {
    float cj = -(cam.T[0] * cam.R[j * 3 + 0] + cam.T[1] * cam.R[j * 3 + 1] + cam.T[2] * cam.R[j * 3 + 2]);
    const float d = cj - c.scene_center[j];
    d2 += d * d;
  }
  if (d2 < 0.001f) d2 = 0.001f;
  float dist = sqrtf(d2);
  if (dist < c.scene_extent + 1e-3f) dist = c.scene_extent + 1e-3f;
  pc.zmin = dist - c.scene_extent;
  pc.zmax = dist + c.scene_extent;
}

// Launch parameters are zeroed as a whole (padding included: the structs stay deterministic), then filled.  The fields every
// renderer kernel reads: the grid and its scale ...
template <class Params>
static void base_params(const HoloRenderer* r, const float* grid_cl, Params& p) {
  memset(&p, 0, sizeof p);
  p.grid_cl = grid_cl;
  p.R = r->cfg.resol;
  p.C = r->cfg.feature_size;
  p.half_extent = grid_half_extent(r->cfg.resol, r->cfg.volume_extent);
}
// ... with the RenderMLP (RenderKernelParams, ImplicitEvalParams) ...
template <class Params>
static void mlp_params(const HoloRenderer* r, const float* grid_cl, Params& p) {
  base_params(r, grid_cl, p);
  fill_mlp(r, p.mlp);
}
// ... and with one launch's cameras, the frame and the compositing constants (holo_render, render_rays_impl)
static void frame_params(const HoloRenderer* r, const float* grid_cl, const HoloCamera* cameras, int n, RenderKernelParams& p) {
  const HoloRenderCfg& c = r->cfg;
  mlp_params(r, grid_cl, p);
  p.n_cams = n;
  for (int g = 0; g < n; ++g) fill_cam(c, cameras[g], p.cams[g]);
  p.H = c.image_height;
  p.W = c.image_width;
  p.n_coarse = c.n_pts_coarse;
  p.n_fine = c.n_pts_fine;
  for (int k = 0; k < 3; ++k) p.bg[k] = c.bg_color[k];
  p.background_opacity = c.background_opacity;
  p.pdf_eps = c.sample_pdf_eps;
}

// HOLO_RENDER_TIMELINE=1, a development probe (synchronises!).  Before the launch it hangs zeroed per-slot phase clocks on
// p.dbg; called again after the launch it prints their per-tile means and frees them.
static int timeline_probe(RenderKernelParams& p, int nslots, int rays_per_tile, void* stream) {
#ifndef HOLO_EMU
  if (!p.dbg) {
    HIP_TRY(hipMalloc((void**)&p.dbg, (size_t)nslots * 64));
    HIP_TRY(hipMemsetAsync(p.dbg, 0, (size_t)nslots * 64, (hipStream_t)stream));
    return 0;
  }
  std::vector<unsigned long long> d((size_t)nslots * 8);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipMemcpy(d.data(), p.dbg, d.size() * 8, hipMemcpyDeviceToHost));
  (void)hipFree(p.dbg);
  double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tiles = 0;
  for (int w = 0; w < nslots; ++w) {
    for (int k = 0; k < 8; ++k) ph[k] += (double)d[w * 8 + k];
    tiles += (double)d[w * 8 + 4];
  }
  if (tiles < 1) tiles = 1;
  if (rays_per_tile == 4)
    fprintf(stderr, "[render timeline] frames %d slots %d 4-ray tiles %.0f | per tile (us): setup %.2f  coarse eval %.2f  "
            "coarse composite+cdf+inverse-cdf %.2f  new-sample eval %.2f  merged composite %.2f\n", p.n_cams, nslots, tiles,
            ph[0] / tiles * 0.01, ph[1] / tiles * 0.01, ph[2] / tiles * 0.01, ph[3] / tiles * 0.01, ph[5] / tiles * 0.01);
  else
    fprintf(stderr, "[render timeline] frames %d slots %d tiles %.0f | per tile: setup %.1f  coarse %.1f  cdf+inverse-cdf %.1f  "
            "fine+composite %.1f us\n", p.n_cams, nslots, tiles, ph[0] / tiles * 0.01, ph[1] / tiles * 0.01,
            (ph[2] - ph[1]) / tiles * 0.01, (ph[3] - ph[2]) / tiles * 0.01);
#endif
  return 0;
}

extern "C" {

int holo_renderer_set_compute_dtype(HoloRenderer* r, int dtype) {
  if (!r || (dtype != HOLO_DTYPE_F32 && dtype != HOLO_DTYPE_F32_BF16X3)) {
    set_error("holo_renderer_set_compute_dtype: HOLO_DTYPE_F32 or HOLO_DTYPE_F32_BF16X3");
    return HOLO_E_INVALID;
  }
  r->split3 = dtype == HOLO_DTYPE_F32_BF16X3 ? 1 : 0;
  return 0;
}

size_t holo_render_workspace_bytes(const HoloRenderer* r, int n_cameras, int with_normals) {
  (void)n_cameras;  // the scratch is per resident wave: any number of cameras renders out of the same buffer
  if (!r) return 0;
  return frame_plan(r, with_normals != 0).layout.total;
}

int holo_render(HoloRenderer* r, const float* grid, const HoloCamera* cameras, int n_cameras, float* images,
                float* depths, float* masks, float* images_coarse, float* depths_coarse, float* masks_coarse,
                float* normals, float* normals_coarse, void* workspace, size_t workspace_bytes, void* stream) {
  if (!r || !grid || !cameras || n_cameras < 1 || !images || !depths || !masks || !workspace) {
    set_error("holo_render: null/invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ready("holo_render", r, COLOURS);
  if (rc) return rc;
  const bool want_nrm = normals != nullptr || normals_coarse != nullptr;
  const RenderPlan plan = frame_plan(r, want_nrm);
  const RenderLayout& L = plan.layout;
  if (workspace_bytes < L.total) {
    set_error("holo_render: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  const bool have_coarse = images_coarse && depths_coarse && masks_coarse;
  // Two statements of "normals" that disagree, kept as they were: workspace, tiles and workgroups follow want_nrm; the
  // instantiation follows the outputs the launch can write, and normals_coarse without the coarse planes leaves both null.
  // Such a call runs the kernel without normals on the geometry planned with them (no caller in this repository makes it).
  const bool launch_nrm = normals != nullptr || (normals_coarse != nullptr && have_coarse);
  const RenderPlan kernel_plan = launch_nrm == want_nrm ? plan : frame_plan(r, launch_nrm);
  const HoloRenderCfg& c = r->cfg;
  auto at = [&](const RenderRegion& g) { return g.bytes ? (char*)workspace + g.off : nullptr; };
  const float* grid_cl = grid_to_channels_last(r, grid, workspace, stream);
  if (!grid_cl) return HOLO_E_INVALID;
  const int H = c.image_height, Wd = c.image_width;
  const int64_t npix = (int64_t)H * Wd;
  float* dens_field = nullptr;
  if (want_nrm && plan.family == RenderFamily::Tiled) {
    MlpParams mp;
    fill_mlp(r, mp);
    dens_field = (float*)at(L.dens_field);
    if (density_field_launch(grid_cl, mp.w_dens, c.feature_size, grid_voxels(r), dens_field, stream)) return HOLO_E_INVALID;
  }
  const bool timeline = r->knobs.render_timeline;  // development probe (synchronises!)
  for (const RenderLaunch& l : render_launches(plan, n_cameras, npix)) {
    const int c0 = l.cam0;
    RenderKernelParams p;
    frame_params(r, grid_cl, cameras + c0, l.n_cams, p);
    if (Wd >= H) {
      p.range_x = (float)Wd / (float)H;
      p.range_y = 1.f;
    } else {
      p.range_x = 1.f;
      p.range_y = (float)H / (float)Wd;
    }
    p.split3 = plan.sp ? 1 : 0;
    p.val_ws = (float*)at(L.val_ws);
    p.nrm_ws = (float*)at(L.nrm_ws);
    p.dens_field = dens_field;
    p.rgb = images + (size_t)c0 * 3 * npix;  // the kernel adds the per-frame offsets
    p.depth = depths + (size_t)c0 * npix;
    p.mask = masks + (size_t)c0 * npix;
    if (have_coarse) {
      p.rgb_c = images_coarse + (size_t)c0 * 3 * npix;
      p.depth_c = depths_coarse + (size_t)c0 * npix;
      p.mask_c = masks_coarse + (size_t)c0 * npix;
    }
    p.nrm = normals ? normals + (size_t)c0 * 3 * npix : nullptr;
    p.nrm_c = (normals_coarse && p.rgb_c) ? normals_coarse + (size_t)c0 * 3 * npix : nullptr;
    p.n_tiles = l.n_tiles;
    p.xcd = l.xcd;
    if (l.dynamic) {  // every launch starts from zeroed counters
      p.tile_ctr = (int*)at(L.tile_ctr);
      HIP_TRY(hipMemsetAsync(p.tile_ctr, 0, 8 * sizeof(int), (hipStream_t)stream));
      p.tail_quads = l.tail_quads;
    }
    const int nslots = l.n_wgs * plan.waves;
    if (timeline && (rc = timeline_probe(p, nslots, plan.rays_per_tile, stream))) return rc;
    if (render_launch(p, kernel_plan, l, stream)) return HOLO_E_INVALID;
    if (timeline && (rc = timeline_probe(p, nslots, plan.rays_per_tile, stream))) return rc;
  }
  return 0;
}

// points per pass of the feature head: the hidden features of a pass (Hd floats per point) live in the workspace
static const int64_t IMPLICIT_CHUNK = 65536;

size_t holo_implicit_workspace_bytes(const HoloRenderer* r, int64_t n_points, int64_t pts_per_dir, int with_features) {
  if (!r || n_points < 0 || pts_per_dir < 1) return 0;
  const int64_t n_dirs = (n_points + pts_per_dir - 1) / pts_per_dir;
  size_t b = grid_cl_bytes(r) + align256((size_t)n_dirs * 3 * sizeof(float));
  if (with_features && r->cfg.feature_dim > 0) {
    const int64_t chunk = n_points < IMPLICIT_CHUNK ? n_points : IMPLICIT_CHUNK;
    b += (size_t)chunk * r->cfg.dnet_hidden_dim * sizeof(float);
  }
  return b + 256;
}

int holo_implicit_eval_features(HoloRenderer* r, const float* grid, const float* pts, const float* dirs, int64_t n_points,
                                int64_t pts_per_dir, float* densities, float* colours, float* vp_features, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!r || !grid || !pts || !dirs || !densities || !colours || !workspace || n_points < 0 || pts_per_dir < 1) {
    set_error("holo_implicit_eval: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (const int rc = ready("holo_implicit_eval", r, COMMITTED)) return rc;
  if (vp_features && r->cfg.feature_dim <= 0) {
    set_error("holo_implicit_eval_features: the renderer was created with feature_dim = 0");
    return HOLO_E_INVALID;
  }
  const size_t grid_bytes = grid_cl_bytes(r);
  const int64_t n_dirs = (n_points + pts_per_dir - 1) / pts_per_dir;
  if (workspace_bytes < holo_implicit_workspace_bytes(r, n_points, pts_per_dir, vp_features ? 1 : 0) - 256) {
    set_error("holo_implicit_eval: workspace too small (holo_implicit_workspace_bytes)");
    return HOLO_E_WORKSPACE;
  }
  const HoloRenderCfg& c = r->cfg;
  const float* grid_cl = grid_to_channels_last(r, grid, workspace, stream);
  if (!grid_cl) return HOLO_E_INVALID;
  ImplicitEvalParams p;
  mlp_params(r, grid_cl, p);
  p.pts = pts;
  p.dirs = dirs;
  p.rdir = (float*)((char*)workspace + grid_bytes);
  p.n_points = n_points;
  p.pts_per_dir = pts_per_dir;
  p.densities = densities;
  p.colours = colours;
  if (!vp_features) return implicit_eval_launch(p, stream) ? HOLO_E_INVALID : 0;
  // with the feature head: passes of IMPLICIT_CHUNK points (a multiple of pts_per_dir is not needed: the direction of a
  // point is looked up by its GLOBAL index, so a pass may start anywhere): hidden features -> GEMM with the head's
  // weight -> bias + LeakyReLU (the activation the construction quirk attaches to a last layer, custom_modules.py:108-112)
  const int Hd = c.dnet_hidden_dim, Fd = c.feature_dim;
  float* hidden = (float*)((char*)workspace + grid_bytes + align256((size_t)n_dirs * 3 * sizeof(float)));
  const float* w_fnet = r->packed + r->fnet_off;
  const float* b_fnet = w_fnet + (size_t)Fd * Hd;
  if (implicit_dirs_launch(p, stream)) return HOLO_E_INVALID;
  for (int64_t s0 = 0; s0 < n_points; s0 += IMPLICIT_CHUNK) {
    const int64_t m = n_points - s0 < IMPLICIT_CHUNK ? n_points - s0 : IMPLICIT_CHUNK;
    ImplicitEvalParams q = p;
    q.point0 = s0;
    q.n_points = s0 + m;
    q.hidden = hidden;
    if (implicit_points_launch(q, stream)) return HOLO_E_INVALID;
    // vp_features [m][Fd] = hidden [m][Hd] . w_fnet [Fd][Hd]^T
    if (gemm_batch_launch(hidden, Hd, w_fnet, Hd, 0, vp_features + s0 * Fd, Fd, (int)m, Fd, Hd, 1, 0, 0, 0, stream))
      return HOLO_E_INVALID;
    if (bias_leaky_launch(vp_features + s0 * Fd, b_fnet, m, Fd, stream)) return HOLO_E_INVALID;
  }
  return 0;
}

int holo_implicit_eval(HoloRenderer* r, const float* grid, const float* pts, const float* dirs, int64_t n_points,
                       int64_t pts_per_dir, float* densities, float* colours, void* workspace, size_t workspace_bytes,
                       void* stream) {
  return holo_implicit_eval_features(r, grid, pts, dirs, n_points, pts_per_dir, densities, colours, nullptr, workspace,
                                     workspace_bytes, stream);
}

// Training-mode rendering: an explicit list of rays per camera, optional injected random streams.
}  // extern "C"

// the rays of a training-mode call as the ABI hands them over (holo_render_rays, holo_render_rays_backward)
struct RayBatch {
  const HoloCamera* cameras;
  int n_cameras, n_rays;
  const float *xys, *u_coarse, *u_fine, *noise_coarse, *noise_fine;
  float density_noise_std;
};
// ... and what is rendered for them; z_merged / new_flags: optional outputs for the backward pass
struct RayOutputs {
  float *images, *depths, *masks, *images_coarse, *depths_coarse, *masks_coarse, *z_merged;
  unsigned char* new_flags;
};

// grid_cl: the channels-last grid, already converted
static int render_rays_impl(HoloRenderer* r, const float* grid_cl, const RayBatch& in, const RayOutputs& out, void* stream) {
  const HoloRenderCfg& c = r->cfg;
  const int n_rays = in.n_rays;
  const RenderPlan plan = rays_plan(r);
  const int64_t nm = (int64_t)c.n_pts_coarse + c.n_pts_fine;
  const bool noisy = in.density_noise_std > 0.f;
  for (const RenderLaunch& l : render_launches(plan, in.n_cameras, n_rays)) {
    RenderKernelParams p;
    frame_params(r, grid_cl, in.cameras + l.cam0, l.n_cams, p);
    const int64_t o = (int64_t)l.cam0 * n_rays;
    p.train.n_rays = n_rays;
    p.train.xys = in.xys + o * 2;
    p.train.u_coarse = in.u_coarse ? in.u_coarse + o * c.n_pts_coarse : nullptr;
    p.train.u_fine = in.u_fine ? in.u_fine + o * c.n_pts_fine : nullptr;
    p.train.noise_coarse = (in.noise_coarse && noisy) ? in.noise_coarse + o * c.n_pts_coarse : nullptr;
    p.train.noise_fine = (in.noise_fine && noisy) ? in.noise_fine + o * nm : nullptr;
    p.train.noise_std = in.density_noise_std;
    p.train.z_merged = out.z_merged ? out.z_merged + o * nm : nullptr;
    p.train.new_flags = out.new_flags ? out.new_flags + o * nm : nullptr;
    p.rgb = out.images + o * 3;
    p.depth = out.depths + o;
    p.mask = out.masks + o;
    if (out.images_coarse && out.depths_coarse && out.masks_coarse) {
      p.rgb_c = out.images_coarse + o * 3;
      p.depth_c = out.depths_coarse + o;
      p.mask_c = out.masks_coarse + o;
    }
    p.n_tiles = l.n_tiles;
    p.xcd = l.xcd;
    if (render_launch(p, plan, l, stream)) return HOLO_E_INVALID;
  }
  return 0;
}

extern "C" {

int holo_render_rays(HoloRenderer* r, const float* grid, const HoloCamera* cameras, int n_cameras, int n_rays,
                     const float* xys, const float* u_coarse, const float* u_fine, const float* noise_coarse,
                     const float* noise_fine, float density_noise_std, float* images, float* depths, float* masks,
                     float* images_coarse, float* depths_coarse, float* masks_coarse, void* workspace, size_t workspace_bytes,
                     void* stream) {
  if (!r || !grid || !cameras || n_cameras < 1 || n_rays < 1 || !xys || !images || !depths || !masks || !workspace) {
    set_error("holo_render_rays: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (const int rc = ready("holo_render_rays", r, COLOURS_UP_TO_64)) return rc;
  if (workspace_bytes < rays_plan(r).layout.total) {
    set_error("holo_render_rays: workspace too small (holo_render_workspace_bytes)");
    return HOLO_E_WORKSPACE;
  }
  const float* grid_cl = grid_to_channels_last(r, grid, workspace, stream);
  if (!grid_cl) return HOLO_E_INVALID;
  const RayBatch in = {cameras, n_cameras, n_rays, xys, u_coarse, u_fine, noise_coarse, noise_fine, density_noise_std};
  return render_rays_impl(r, grid_cl, in, {images, depths, masks, images_coarse, depths_coarse, masks_coarse, nullptr, nullptr},
                          stream);
}

int holo_implicit_normals(HoloRenderer* r, const float* grid, const float* pts, int64_t n_points, float* normals,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!r || !grid || !pts || !normals || !workspace || n_points < 0) {
    set_error("holo_implicit_normals: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (const int rc = ready("holo_implicit_normals", r, COMMITTED)) return rc;
  if (workspace_bytes < grid_cl_bytes(r)) {
    set_error("holo_implicit_normals: workspace too small (need holo_render_workspace_bytes)");
    return HOLO_E_WORKSPACE;
  }
  const float* grid_cl = grid_to_channels_last(r, grid, workspace, stream);
  if (!grid_cl) return HOLO_E_INVALID;
  ImplicitEvalParams p;
  mlp_params(r, grid_cl, p);
  p.pts = pts;
  p.n_points = n_points;
  return implicit_normals_launch(p, normals, stream) ? HOLO_E_INVALID : 0;
}

// workspace of holo_density_lattice: the channels-last grid | S[v] = w_dens . F[v]
size_t holo_density_lattice_workspace_bytes(const HoloRenderer* r) {
  return r ? grid_cl_bytes(r) + align256((size_t)grid_voxels(r) * sizeof(float)) : 0;
}

int holo_density_lattice(HoloRenderer* r, const float* grid, int m, float* field, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (!r || !grid || !field || !workspace) {
    set_error("holo_density_lattice: null argument");
    return HOLO_E_INVALID;
  }
  if (m < 2 || m > 1024) {
    set_error("holo_density_lattice: the lattice has 2 <= m <= 1024 points per axis (got %d)", m);
    return HOLO_E_INVALID;
  }
  if (const int rc = ready("holo_density_lattice", r, COMMITTED)) return rc;
  if (workspace_bytes < holo_density_lattice_workspace_bytes(r)) {
    set_error("holo_density_lattice: workspace too small (holo_density_lattice_workspace_bytes)");
    return HOLO_E_WORKSPACE;
  }
  const float* grid_cl = grid_to_channels_last(r, grid, workspace, stream);
  if (!grid_cl) return HOLO_E_INVALID;
  MlpParams mp;
  fill_mlp(r, mp);
  float* S = (float*)((char*)workspace + grid_cl_bytes(r));
  if (density_field_launch(grid_cl, mp.w_dens, r->cfg.feature_size, grid_voxels(r), S, stream)) return HOLO_E_INVALID;
  return density_lattice_launch(S, r->cfg.resol, grid_half_extent(r->cfg.resol, r->cfg.volume_extent), mp.b_dens, m, field,
                                stream);
}

}  // extern "C"

// ---- backward of the training-mode renderer (kernels_render_bwd.hip) ------------------------------------
namespace {
struct RbwdLayout {
  int64_t NR, nm, cap, rays_per_chunk;
  int Hd, Hp, C, S;
  size_t o_ggrid, o_fwd, o_zm, o_flags, o_rays, o_grray, o_F, o_YT, o_AT, o_GFT, o_val, o_drad, o_gval, o_GR, o_tmp, o_part,
      o_dWe, o_dbe, o_partr, o_dWrh, o_dir, o_gmax, o_gfix, total;
  bool fixed;  // the deterministic mode of the grid scatter (holo_ctx_set_deterministic)
  // what the stages before and after the chunk kernels write: the replayed forward (outputs, merged depths, flags), the
  // ray records, split-K partials, folded gradients
  struct Scratch {
    float *fwd, *z_merged, *rays, *part, *dWe, *dbe, *partr, *dWrh, *ddir;
    unsigned char* flags;
  };
  // typed pointers into the workspace; the chunk kernels' buffers go straight into their (zeroed) launch parameters
  Scratch bind(void* workspace, RenderBwdChunk& p) const {
    char* ws = (char*)workspace;
    auto at = [&](size_t off) { return (float*)(ws + off); };
    const Scratch s = {at(o_fwd),   at(o_zm),   at(o_rays), at(o_part), at(o_dWe), at(o_dbe),
                       at(o_partr), at(o_dWrh), at(o_dir),  (unsigned char*)(ws + o_flags)};
    p.rays = s.rays, p.z_merged = s.z_merged, p.new_flags = s.flags;
    p.ggrid_cl = at(o_ggrid), p.gr_ray = at(o_grray), p.F = at(o_F), p.YT = at(o_YT), p.AT = at(o_AT), p.GFT = at(o_GFT);
    p.val = (float4*)(ws + o_val), p.drad = (float4*)(ws + o_drad), p.gval = (float4*)(ws + o_gval), p.GR = (float4*)(ws + o_GR);
    p.tmp = (double*)(ws + o_tmp);
    p.gfix = fixed ? (long long*)(ws + o_gfix) : nullptr;
    p.gfix_max = (uint32_t*)(ws + o_gmax);
    return s;
  }
};
RbwdLayout rbwd_layout(const HoloRenderer* r, int n_cameras, int n_rays) {
  RbwdLayout L;
  const HoloRenderCfg& c = r->cfg;
  L.NR = (int64_t)n_cameras * n_rays;
  L.nm = (int64_t)c.n_pts_coarse + c.n_pts_fine;
  L.Hd = c.dnet_hidden_dim;
  L.Hp = (L.Hd + 1 + 3) & ~3;
  L.C = c.feature_size;
  L.S = 16;  // splits of the products over the points
  L.rays_per_chunk = 65536 / L.nm;
  if (L.rays_per_chunk < 1) L.rays_per_chunk = 1;
  if (L.rays_per_chunk > L.NR) L.rays_per_chunk = L.NR;
  L.cap = (L.rays_per_chunk * L.nm + 63) & ~(int64_t)63;  // a multiple of 4 * S
  size_t o = grid_cl_bytes(r);
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  L.o_ggrid = take(grid_cl_bytes(r));
  L.o_fwd = take((size_t)L.NR * 10 * sizeof(float));
  L.o_zm = take((size_t)L.NR * L.nm * sizeof(float));
  L.o_flags = take((size_t)L.NR * L.nm);
  L.o_rays = take((size_t)L.NR * RBWD_REC * sizeof(float));
  L.o_grray = take((size_t)L.NR * 4 * sizeof(float));
  L.o_F = take((size_t)L.cap * L.C * sizeof(float));
  L.o_YT = take((size_t)L.Hp * L.cap * sizeof(float));
  L.o_AT = take((size_t)L.Hp * L.cap * sizeof(float));
  L.o_GFT = take((size_t)L.C * L.cap * sizeof(float));
  L.o_val = take((size_t)L.cap * 16);
  L.o_drad = take((size_t)L.cap * 16);
  L.o_gval = take((size_t)L.cap * 16);
  L.o_GR = take((size_t)L.cap * 16);
  L.o_tmp = take((size_t)L.cap * 32);
  L.o_part = take((size_t)L.S * L.Hp * L.C * sizeof(float));
  L.o_dWe = take((size_t)L.Hp * L.C * sizeof(float));
  L.o_dbe = take((size_t)L.Hp * sizeof(float));
  L.o_partr = take((size_t)L.S * L.Hd * 4 * sizeof(float));
  L.o_dWrh = take((size_t)L.Hd * 4 * sizeof(float));
  L.o_dir = take(128 * sizeof(float));
  L.o_gmax = take(256);
  L.fixed = r->ctx && r->ctx->deterministic;
  L.o_gfix = L.fixed ? take(2 * grid_cl_bytes(r)) : o;  // 64-bit fixed-point image of the grid gradient
  L.total = o + 256;
  return L;
}

// The stages of holo_render_rays_backward, in the order they run.
// 1. the folded weights in the GEMM layouts (once per commit)
int rbwd_pack_weights(HoloRenderer* r, const RbwdLayout& L, void* stream) {
  if (r->bwd_pack_valid) return 0;
  const FVec pk = pack_density_gemm_operands(r->fold, L.C, L.Hd, L.Hp);
  if (!r->bwd_pack) HIP_TRY(hipMalloc((void**)&r->bwd_pack, pk.size() * sizeof(float)));
  if (upload_via_stage(&r->stage, &r->stage_floats, r->bwd_pack, pk.data(), pk.size(), stream)) {
    set_error("holo_render_rays_backward: upload of the folded weights failed");
    return HOLO_E_HIP;
  }
  r->bwd_pack_valid = true;
  return 0;
}
// 2. the forward pass once more: the merged depth list of every ray
int rbwd_replay(HoloRenderer* r, const RbwdLayout& L, const RbwdLayout::Scratch& s, const float* grid_cl, const RayBatch& in,
                float* merged_depths, unsigned char* merged_is_new, void* stream) {
  float* fwd = s.fwd;
  const int rc = render_rays_impl(r, grid_cl, in, {fwd, fwd + L.NR * 3, fwd + L.NR * 4, fwd + L.NR * 5, fwd + L.NR * 8,
                                                   fwd + L.NR * 9, s.z_merged, s.flags}, stream);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (merged_depths)
    HIP_TRY(hipMemcpyAsync(merged_depths, s.z_merged, (size_t)L.NR * L.nm * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (merged_is_new) HIP_TRY(hipMemcpyAsync(merged_is_new, s.flags, (size_t)L.NR * L.nm, hipMemcpyDeviceToDevice, st));
  return 0;
}
// 3. per-ray records
int rbwd_ray_records(const HoloRenderer* r, const RayBatch& in, const float* w_dir, float* rays, void* stream) {
  for (int c0 = 0; c0 < in.n_cameras; c0 += RenderKernelParams::MAX_CAMS) {
    const int ng = in.n_cameras - c0 < RenderKernelParams::MAX_CAMS ? in.n_cameras - c0 : RenderKernelParams::MAX_CAMS;
    RenderBwdRays q;
    memset(&q, 0, sizeof q);
    for (int g = 0; g < ng; ++g) fill_cam(r->cfg, in.cameras[c0 + g], q.cams[g]);
    q.n_cams = ng;
    q.n_rays = in.n_rays;
    q.ray0 = (int64_t)c0 * in.n_rays;
    q.xys = in.xys;
    q.rays = rays;
    q.w_dir = w_dir;
    for (int k = 0; k < 3; ++k) q.b_rad[k] = r->b_rad[k];
    if (rbwd_rays_launch(q, stream)) return HOLO_E_INVALID;
  }
  return 0;
}
// 4. chunks of whole rays: the grid gradient is scattered, the folded parameter gradients add up in chunk order
int rbwd_chunks(const HoloRenderer* r, const RbwdLayout& L, const RbwdLayout::Scratch& s, RenderBwdChunk& p, void* stream) {
  const int C = L.C, Hd = L.Hd, Hp = L.Hp, S = L.S, cap = (int)L.cap, Ks = cap / S;
  const float* WeP = r->bwd_pack;
  const float* WeT = WeP + (size_t)Hp * C;
  int first = 1;
  for (int64_t r0 = 0; r0 < L.NR; r0 += L.rays_per_chunk) {
    const int64_t nr = L.NR - r0 < L.rays_per_chunk ? L.NR - r0 : L.rays_per_chunk;
    p.ray0 = r0;
    p.n_rays_chunk = (int)nr;
    p.n = nr * L.nm;
    if (rbwd_gather_launch(p, stream)) return HOLO_E_INVALID;
    // YT [Hp][cap] = WeP [Hp][C] . F[cap][C]^T
    if (gemm_batch_launch(WeP, C, p.F, C, 0, p.YT, cap, Hp, cap, C, 1, 0, 0, 0, stream)) return HOLO_E_INVALID;
    if (rbwd_point_fwd_launch(p, stream)) return HOLO_E_INVALID;
    if (rbwd_composite_launch(p, stream)) return HOLO_E_INVALID;
    if (rbwd_point_bwd_launch(p, stream)) return HOLO_E_INVALID;
    // GFT [C][cap] = WeT [C][Hp] . YT [Hp][cap]
    if (gemm_batch_launch(WeT, Hp, p.YT, cap, 1, p.GFT, cap, C, cap, Hp, 1, 0, 0, 0, stream)) return HOLO_E_INVALID;
    // dWe partials [S][Hp][C] = YT[:, split] . F[split, :]
    if (gemm_batch_launch(p.YT, cap, p.F, C, 1, s.part, C, Hp, C, Ks, S, Ks, (int64_t)Ks * C, (int64_t)Hp * C, stream))
      return HOLO_E_INVALID;
    if (partial_reduce_launch(s.part, s.dWe, (int64_t)Hp * C, L.S, first ? 0 : 1, stream)) return HOLO_E_INVALID;
    if (rbwd_rowsum_launch(p.YT, L.cap, L.cap, Hp, s.dbe, first ? 0 : 1, stream)) return HOLO_E_INVALID;
    // dWr_h partials [S][Hd][4] = AT[:, split] . GR[split, :]
    if (gemm_batch_launch(p.AT, cap, (const float*)p.GR, 4, 1, s.partr, 4, Hd, 4, Ks, S, Ks, (int64_t)Ks * 4, (int64_t)Hd * 4, stream))
      return HOLO_E_INVALID;
    if (partial_reduce_launch(s.partr, s.dWrh, (int64_t)Hd * 4, L.S, first ? 0 : 1, stream)) return HOLO_E_INVALID;
    if (L.fixed) {  // max |GFT| of the chunk -> fixed-point sums -> added to the gradient in chunk order
      HIP_TRY(hipMemsetAsync(p.gfix_max, 0, sizeof(uint32_t), (hipStream_t)stream));
      if (rbwd_absmax_launch(p, stream)) return HOLO_E_INVALID;
    }
    if (rbwd_scatter_launch(p, stream)) return HOLO_E_INVALID;
    if (L.fixed && rbwd_fix_flush_launch(p, stream)) return HOLO_E_INVALID;
    first = 0;
  }
  return 0;
}
// 5. the folded gradients come to the host, are un-folded to the Linear layers (mlp_folds.h) and published
int rbwd_unfold_publish(HoloRenderer* r, const RbwdLayout& L, const RbwdLayout::Scratch& s, void* stream) {
  const int C = L.C, Hd = L.Hd, De = dir_emb(r->cfg);
  hipStream_t st = (hipStream_t)stream;
  FVec hWe((size_t)L.Hp * C), hbe(L.Hp), hWrh((size_t)Hd * 4), hdir((size_t)3 * (De + 1));
  HIP_TRY(hipMemcpyAsync(hWe.data(), s.dWe, hWe.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hbe.data(), s.dbe, hbe.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hWrh.data(), s.dWrh, hWrh.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hdir.data(), s.ddir, hdir.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const HostParams& P = r->params;
  DensityGrads d = unfold_density_grads(r->fold, P["_density_net.mlp.0.0.weight"], P["_density_net.mlp.0.0.bias"],
                                        P["_density_net.mlp.1.0.weight"], P["_density_net.mlp.2.0.weight"],
                                        P["_density_net.mlp.3.0.weight"], hWe, hbe, C, Hd);
  RadianceGrads rad = unfold_radiance_grads(hWrh, hdir, Hd, De);
  HostGrads& G = r->grads;
  G.put("_density_net.mlp.0.0.weight", std::move(d.dW0)), G.put("_density_net.mlp.0.0.bias", std::move(d.db0));
  G.put("_density_net.mlp.1.0.weight", std::move(d.dW1)), G.put("_density_net.mlp.1.0.bias", std::move(d.db1));
  G.put("_density_net.mlp.2.0.weight", std::move(d.dW2)), G.put("_density_net.mlp.2.0.bias", std::move(d.db2));
  G.put("_density_net.mlp.3.0.weight", std::move(d.dW3)), G.put("_density_net.mlp.3.0.bias", std::move(d.db3));
  G.put("_radiance_net.mlp.0.0.weight", std::move(rad.dWr)), G.put("_radiance_net.mlp.0.0.bias", std::move(rad.dbr));
  return G.publish(stream);
}
}  // namespace

extern "C" {

size_t holo_render_rays_backward_workspace_bytes(const HoloRenderer* r, int n_cameras, int n_rays) {
  if (!r || n_cameras < 1 || n_rays < 1) return 0;
  return rbwd_layout(r, n_cameras, n_rays).total;
}

int holo_render_rays_backward(HoloRenderer* r, const float* grid, const HoloCamera* cameras, int n_cameras, int n_rays,
                              const float* xys, const float* u_coarse, const float* u_fine, const float* noise_coarse,
                              const float* noise_fine, float density_noise_std, const float* grad_images,
                              const float* grad_depths, const float* grad_masks, const float* grad_images_coarse,
                              const float* grad_depths_coarse, const float* grad_masks_coarse, float* grad_grid,
                              float* merged_depths, unsigned char* merged_is_new, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (!r || !grid || !cameras || n_cameras < 1 || n_rays < 1 || !xys || !grad_grid || !workspace) {
    set_error("holo_render_rays_backward: null/invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ready("holo_render_rays_backward", r, COLOURS_UP_TO_64);
  if (rc) return rc;
  const RbwdLayout L = rbwd_layout(r, n_cameras, n_rays);
  if (workspace_bytes < L.total) {
    set_error("holo_render_rays_backward: workspace too small (holo_render_rays_backward_workspace_bytes)");
    return HOLO_E_WORKSPACE;
  }
  const HoloRenderCfg& c = r->cfg;
  const RayBatch in = {cameras, n_cameras, n_rays, xys, u_coarse, u_fine, noise_coarse, noise_fine, density_noise_std};
  hipStream_t st = (hipStream_t)stream;
  if ((rc = rbwd_pack_weights(r, L, stream))) return rc;
  MlpParams mlp;
  fill_mlp(r, mlp);
  const float* grid_cl = grid_to_channels_last(r, grid, workspace, stream);
  if (!grid_cl) return HOLO_E_INVALID;
  RenderBwdChunk p;
  base_params(r, grid_cl, p);
  const RbwdLayout::Scratch s = L.bind(workspace, p);
  HIP_TRY(hipMemsetAsync(p.ggrid_cl, 0, grid_cl_bytes(r), st));
  if (L.fixed) HIP_TRY(hipMemsetAsync(p.gfix, 0, 2 * grid_cl_bytes(r), st));
  HIP_TRY(hipMemsetAsync(p.AT, 0, (size_t)L.Hp * L.cap * sizeof(float), st));
  if ((rc = rbwd_replay(r, L, s, grid_cl, in, merged_depths, merged_is_new, stream))) return rc;
  if ((rc = rbwd_ray_records(r, in, mlp.w_dir, s.rays, stream))) return rc;
  p.Hd = L.Hd;
  p.Hp = L.Hp;
  p.nm = (int)L.nm;
  p.n_coarse = c.n_pts_coarse;
  p.rays_per_cam = n_rays;
  p.ld = L.cap;
  p.n_pad = L.cap;
  p.be = r->bwd_pack + (size_t)2 * L.Hp * L.C;
  p.w_rad = mlp.w_rad;
  const bool noisy = density_noise_std > 0.f;
  p.noise_fine = noisy ? noise_fine : nullptr;
  p.noise_coarse = noisy ? noise_coarse : nullptr;
  p.noise_std = density_noise_std;
  p.g_rgb = grad_images, p.g_depth = grad_depths, p.g_mask = grad_masks;
  p.g_rgb_c = grad_images_coarse, p.g_depth_c = grad_depths_coarse, p.g_mask_c = grad_masks_coarse;
  for (int k = 0; k < 3; ++k) p.bg[k] = c.bg_color[k];
  p.background_opacity = c.background_opacity;
  if ((rc = rbwd_chunks(r, L, s, p, stream))) return rc;
  if (rbwd_dir_grad_launch(p.gr_ray, s.rays, L.NR, s.ddir, stream)) return HOLO_E_INVALID;
  if (ndhwc_to_ncdhw_launch(p.ggrid_cl, grad_grid, 1, L.C, grid_voxels(r), stream)) return HOLO_E_INVALID;
  return rbwd_unfold_publish(r, L, s, stream);
}

int holo_renderer_get_grad(HoloRenderer* r, const char* name, float* out_dev, int64_t numel, void* stream) {
  if (!r || !name || !out_dev) {
    set_error("holo_renderer_get_grad: null argument");
    return HOLO_E_INVALID;
  }
  return r->grads.fetch("holo_renderer_get_grad", name, out_dev, numel, stream);
}

}  // extern "C"
