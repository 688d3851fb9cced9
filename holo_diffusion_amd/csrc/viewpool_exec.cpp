// viewpool_exec.cpp — host side of the view-pooling entry (holo_view_pool): argument checks, layout conversion of the
// caller's NCHW feature maps into the workspace, camera centres, launch.
//
// Reference interface replaced (relative to /root/reference/holo_diffusion):
//   HoloDiffusionModel.forward, image_rgb branch      holo_diffusion_model.py:327-374
//   (ViewPooler = ViewSampler + AngleWeightedReductionFeatureAggregator of PyTorch3D 0.7.4, configs/apple.yaml:183-196;
//    _get_point_to_source_camera_ray_dirs custom_modules.py:279-334; pooled_feature_mapper :113,368; tanh :373)
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/holo_abi.h"
#include "holo_common.h"
#include "holo_kernels.h"
#include "host_params.h"
#include "mlp_folds.h"
#include "viewpool_layout.h"

using namespace holo;

// channels-last images of all source-view feature maps (channels padded to fours), each on a 256-byte boundary
static size_t maps_bytes(const HoloViewFeature* feats, int n_feats, int n_views, size_t elem_bytes) {
  size_t b = 0;
  for (int k = 0; k < n_feats; ++k)
    b += align256((size_t)n_views * feats[k].height * feats[k].width * ((feats[k].channels + 3) / 4 * 4) * elem_bytes);
  return b;
}
// the channels-last copy of one map at ws (advanced behind it)
static int stage_map(const HoloViewFeature& f, int n_views, ViewPoolParams::Feat& o, char*& ws, void* stream) {
  o.C = f.channels;
  o.Cp = (f.channels + 3) / 4 * 4;
  o.H = f.height;
  o.W = f.width;
  o.data = (const float*)ws;
  if (nchw_to_nhwc_pad_launch(f.feats, (float*)ws, n_views, o.C, o.Cp, (int64_t)o.H * o.W, stream)) return HOLO_E_INVALID;
  ws += align256((size_t)n_views * o.H * o.W * o.Cp * sizeof(float));
  return 0;
}
// one source view and its camera centre C = -T R^T (custom_modules.py:288-296, 304-312)
static void fill_pool_cam(const HoloCamera& c, ViewPoolParams::Cam& o) {
  for (int k = 0; k < 9; ++k) o.Rm[k] = c.R[k];
  for (int k = 0; k < 3; ++k) o.T[k] = c.T[k];
  for (int k = 0; k < 2; ++k) {
    o.focal[k] = c.focal[k];
    o.pp[k] = c.principal_point[k];
  }
  for (int j = 0; j < 3; ++j) o.centre[j] = -(c.T[0] * c.R[j * 3 + 0] + c.T[1] * c.R[j * 3 + 1] + c.T[2] * c.R[j * 3 + 2]);
}

static_assert(VIEW_POOL_MAX_FEATS == ViewPoolParams::MAX_FEATS, "viewpool_layout.h lays out the maps of ViewPoolParams");

extern "C" {

size_t holo_view_pool_workspace_bytes(const HoloViewPoolCfg* cfg, const HoloViewFeature* feats, int n_feats, int n_views) {
  if (!cfg || !feats || n_feats < 1 || n_views < 1) return 0;
  return view_pool_layout(*cfg, feats, n_feats, n_views, false, 0, false).total;
}

}  // extern "C"

// everything of holo_view_pool up to the launch: argument checks, the layout L of the workspace (forward or backward),
// channels-last copies of the feature maps and the transposed mapper weight at its head, cameras
static int setup_view_pool(HoloCtx* ctx, const HoloViewPoolCfg* cfg, const HoloViewFeature* feats, int n_feats,
                           const HoloCamera* cameras, int n_views, const float* mapper_weight, const float* mapper_bias,
                           void* workspace, size_t workspace_bytes, bool backward, void* stream, ViewPoolParams& p,
                           ViewPoolLayout& L) {
  if (!ctx || !cfg || !feats || !cameras || !mapper_weight || !workspace) {
    set_error("holo_view_pool: null argument");
    return HOLO_E_INVALID;
  }
  if (n_views < 1 || n_views > ViewPoolParams::MAX_VIEWS || n_feats < 1 || n_feats > ViewPoolParams::MAX_FEATS ||
      cfg->resol < 2 || cfg->feature_size < 1) {
    set_error("holo_view_pool: 1..%d source views, 1..%d feature maps, resol >= 2, feature_size >= 1", ViewPoolParams::MAX_VIEWS,
              ViewPoolParams::MAX_FEATS);
    return HOLO_E_UNSUPPORTED;
  }
  L = view_pool_layout(*cfg, feats, n_feats, n_views, backward, ctx->num_cus, ctx->deterministic);
  if (workspace_bytes < L.total) {
    set_error("holo_view_pool: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  memset(&p, 0, sizeof p);
  char* const base = (char*)workspace;
  int quad = 0, outc = 0;
  for (int k = 0; k < n_feats; ++k) {
    const HoloViewFeature& f = feats[k];
    if (!f.feats || f.channels < 1 || f.height < 1 || f.width < 1) {
      set_error("holo_view_pool: feature map %d is empty", k);
      return HOLO_E_INVALID;
    }
    ViewPoolParams::Feat& o = p.feat[k];
    o.quad0 = quad;
    o.out0 = outc;
    char* at = base + L.map[k];
    if (stage_map(f, n_views, o, at, stream)) return HOLO_E_INVALID;
    quad += o.Cp / 4;
    outc += 2 * o.C;
  }
  if (outc > ViewPoolParams::MAX_AGG) {
    set_error("holo_view_pool: %d aggregated features (at most %d)", outc, ViewPoolParams::MAX_AGG);
    return HOLO_E_UNSUPPORTED;
  }
  p.n_feats = n_feats;
  p.n_quads = quad;
  p.A = outc;
  p.F = cfg->feature_size;
  float* wt = (float*)(base + L.wt);
  if (transpose_small_launch(mapper_weight, wt, p.F, p.A, stream)) return HOLO_E_INVALID;  // (F, A) -> (A, F)
  p.wt = wt;
  p.bias = mapper_bias;
  p.n_views = n_views;
  for (int v = 0; v < n_views; ++v) fill_pool_cam(cameras[v], p.cams[v]);
  p.R = cfg->resol;
  p.half_extent = grid_half_extent(cfg->resol, cfg->volume_extent);
  p.gamma = cfg->weight_by_ray_angle_gamma;
  p.min_weight = cfg->min_ray_angle_weight;
  p.proj_eps = cfg->projection_eps;
  return 0;
}

extern "C" {

int holo_view_pool(HoloCtx* ctx, const HoloViewPoolCfg* cfg, const HoloViewFeature* feats, int n_feats,
                   const HoloCamera* cameras, int n_views, const float* mapper_weight, const float* mapper_bias,
                   float* voxel_features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!voxel_features) {
    set_error("holo_view_pool: null argument");
    return HOLO_E_INVALID;
  }
  ViewPoolParams p;
  ViewPoolLayout L;
  const int rc = setup_view_pool(ctx, cfg, feats, n_feats, cameras, n_views, mapper_weight, mapper_bias, workspace,
                                 workspace_bytes, false, stream, p, L);
  if (rc) return rc;
  p.out = voxel_features;
  return view_pool_launch(p, stream) ? HOLO_E_INVALID : 0;
}

// how many source views see each voxel centre of holo_view_pool's grid (the frustum test only)
int holo_view_coverage(HoloCtx* ctx, const HoloViewPoolCfg* cfg, const HoloCamera* cameras, int n_views,
                       const int32_t* heights, const int32_t* widths, float* coverage, void* stream) {
  if (!ctx || !cfg || !cameras || !heights || !widths || !coverage) {
    set_error("holo_view_coverage: null argument");
    return HOLO_E_INVALID;
  }
  if (n_views < 1 || n_views > ViewPoolParams::MAX_VIEWS || cfg->resol < 2) {
    set_error("holo_view_coverage: 1..%d source views, resol >= 2", ViewPoolParams::MAX_VIEWS);
    return HOLO_E_UNSUPPORTED;
  }
  ViewCoverageParams p;
  memset(&p, 0, sizeof p);
  for (int v = 0; v < n_views; ++v) {
    if (heights[v] < 1 || widths[v] < 1) {
      set_error("holo_view_coverage: view %d has an empty map", v);
      return HOLO_E_INVALID;
    }
    fill_pool_cam(cameras[v], p.cams[v]);
    p.H[v] = heights[v];
    p.W[v] = widths[v];
  }
  p.n_views = n_views;
  p.R = cfg->resol;
  p.half_extent = grid_half_extent(cfg->resol, cfg->volume_extent);
  p.proj_eps = cfg->projection_eps;
  p.out = coverage;
  return view_coverage_launch(p, stream) ? HOLO_E_INVALID : 0;
}

// ---- backward (kernels_viewpool_bwd.hip).  Workspace (viewpool_layout.h): the forward's part, then the zeroed
//      channels-last gradient maps, then the per-workgroup partials of d weight / d bias.
size_t holo_view_pool_backward_workspace_bytes(HoloCtx* ctx, const HoloViewPoolCfg* cfg, const HoloViewFeature* feats,
                                               int n_feats, int n_views) {
  if (!ctx || !cfg || !feats || n_feats < 1 || n_views < 1) return 0;
  return view_pool_layout(*cfg, feats, n_feats, n_views, true, ctx->num_cus, ctx->deterministic).total;
}

int holo_view_pool_backward(HoloCtx* ctx, const HoloViewPoolCfg* cfg, const HoloViewFeature* feats, int n_feats,
                            const HoloCamera* cameras, int n_views, const float* mapper_weight, const float* mapper_bias,
                            const float* grad_voxel_features, float* const* grad_feats, float* grad_mapper_weight,
                            float* grad_mapper_bias, void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad_voxel_features) {
    set_error("holo_view_pool_backward: null argument");
    return HOLO_E_INVALID;
  }
  const Knobs knobs = Knobs::from_env();  // per call: this entry has no handle (holo_knobs.h, CALL)
  ViewPoolBwdParams b;
  memset(&b, 0, sizeof b);
  ViewPoolLayout L;
  int rc = setup_view_pool(ctx, cfg, feats, n_feats, cameras, n_views, mapper_weight, mapper_bias, workspace, workspace_bytes,
                           true, stream, b.fwd, L);
  if (rc) return rc;
  char* const base = (char*)workspace;
  b.gout = grad_voxel_features;
  for (int k = 0; k < n_feats; ++k)
    if (grad_feats && grad_feats[k]) {
      b.gfeat[k] = (float*)(base + L.gmap[k]);
      b.want_feats = 1;
      if (hipMemsetAsync(b.gfeat[k], 0, L.map_bytes[k], (hipStream_t)stream) != hipSuccess) {
        set_error("holo_view_pool_backward: hipMemsetAsync failed");
        return HOLO_E_HIP;
      }
    }
  const int n_wgs = L.n_wgs;
  b.partial = (float*)(base + L.partial);
  b.dW = grad_mapper_weight;
  b.dbias = grad_mapper_bias;
  if (L.fixed && b.want_feats) {
    for (int k = 0; k < n_feats; ++k)
      if (b.gfeat[k]) b.gfix[k] = (long long*)(base + L.gfix[k]);
    b.fix_max = (uint32_t*)(base + L.fix_max);
    if (hipMemsetAsync(base + L.gfix[0], 0, L.fix_end - L.gfix[0], (hipStream_t)stream) != hipSuccess) {
      set_error("holo_view_pool_backward: hipMemsetAsync failed");
      return HOLO_E_HIP;
    }
  }
  if (view_pool_bwd_launch(b, n_wgs, knobs, stream)) return HOLO_E_UNSUPPORTED;
  for (int k = 0; k < n_feats; ++k)
    if (b.gfeat[k]) {
      const ViewPoolParams::Feat& f = b.fwd.feat[k];
      if (b.gfix[k] && fix_flush_launch(b.gfix[k], b.fix_max + k, b.gfeat[k], (int64_t)n_views * f.H * f.W * f.Cp, stream))
        return HOLO_E_INVALID;
      if (nhwc_pad_to_nchw_launch(b.gfeat[k], grad_feats[k], n_views, f.C, f.Cp, (int64_t)f.H * f.W, stream)) return HOLO_E_INVALID;
    }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// MLPMeanFeatureAggregator path (custom_modules.py:162-334; configs/hydrant.yaml:184): parameter binding, the float64
// fold of the affine stretches (see kernels_viewpool.hip) and the launch.
// ---------------------------------------------------------------------------------------------------------------------
struct HoloMlpMeanPooler {
  HoloCtx* ctx;
  HoloMlpMeanCfg cfg;
  Knobs knobs;  // snapshot of holo_mlp_mean_create (holo_knobs.h): the backward's chunk layout, for its size query and its run
  HostParams params;  // raw parameters (host copies)
  MlpMeanShape shape;  // of the fold (mlp_folds.h)
  int D = 0, E = 0, dp = 0, emb0 = 0;
  int quad0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float* dev = nullptr;  // a | am | cb | g | g0 | l
  float* stage = nullptr;  // staging buffer of upload_via_stage
  size_t stage_floats = 0;
  float l0 = 0.f;
  bool committed = false;
  HostGrads grads{"holo_mlp_mean_backward"};  // by reference parameter name
};

static int mlp_mean_fill(HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, const HoloCamera* cameras, int n_views,
                         void* stream, MlpMeanParams& p, char*& ws);

int holo_mlp_mean_create(HoloCtx* ctx, const HoloMlpMeanCfg* cfg, HoloMlpMeanPooler** out) {
  if (!ctx || !cfg || !out) {
    set_error("holo_mlp_mean_create: null argument");
    return HOLO_E_INVALID;
  }
  if (cfg->n_hidden != 128 || cfg->n_layers != 1 || cfg->feature_size < 1 || cfg->feature_size > 32 || cfg->dim_out < 1 ||
      cfg->n_harmonic_functions_ray < 0 || cfg->n_harmonic_functions_ray > 8 || cfg->n_feats < 1 ||
      cfg->n_feats > ViewPoolParams::MAX_FEATS || cfg->resol < 2) {
    set_error("holo_mlp_mean_create: unsupported configuration (n_hidden 128, n_layers 1, feature_size <= 32, "
              "1..%d feature maps, <= 8 harmonic functions)", ViewPoolParams::MAX_FEATS);
    return HOLO_E_UNSUPPORTED;
  }
  HoloMlpMeanPooler* h = new HoloMlpMeanPooler;
  h->ctx = ctx;
  h->cfg = *cfg;
  h->knobs = Knobs::from_env();
  int quad = 0;
  for (int k = 0; k < cfg->n_feats; ++k) {
    if (cfg->channels[k] < 1) {
      delete h;
      set_error("holo_mlp_mean_create: feature map %d has no channels", k);
      return HOLO_E_INVALID;
    }
    h->quad0[k] = quad;
    quad += (cfg->channels[k] + 3) / 4;
    h->D += cfg->channels[k];
  }
  h->E = 3 * (2 * cfg->n_harmonic_functions_ray + 1);
  h->D += h->E;
  h->emb0 = quad * 4;
  const int dq = h->emb0 + (h->E + 3) / 4 * 4;
  static const int widths[5] = {32, 48, 64, 96, 128};
  for (int w : widths)
    if (!h->dp && dq <= w) h->dp = w;
  if (!h->dp) {
    delete h;
    set_error("holo_mlp_mean_create: %d input channels (padded %d) exceed the kernel's 128", h->D, dq);
    return HOLO_E_UNSUPPORTED;
  }
  const int64_t nh = cfg->n_hidden, D = h->D, dout = cfg->dim_out, F = cfg->feature_size;
  h->params.declare("_first_sampled.weight", {nh, D});
  h->params.declare("_first_sampled.bias", {nh});
  h->params.declare("_first_mean.weight", {nh, D});
  h->params.declare("_first_mean.bias", {nh});
  h->params.declare("_mlp.mlp.0.0.weight", {nh, nh});
  h->params.declare("_mlp.mlp.0.0.bias", {nh});
  h->params.declare("_last.weight", {dout, nh});
  h->params.declare("_last.bias", {dout});
  h->params.declare("pooled_feature_mapper.weight", {F, dout});
  h->params.declare("pooled_feature_mapper.bias", {F});
  h->shape = {(int)nh, h->D, h->dp, (int)F, (int)dout, {}};
  for (int k = 0; k < cfg->n_feats; ++k)
    for (int j = 0; j < cfg->channels[k]; ++j) h->shape.col.push_back(h->quad0[k] * 4 + j);
  for (int j = 0; j < h->E; ++j) h->shape.col.push_back(h->emb0 + j);
  if (hipMalloc((void**)&h->dev, (h->shape.image_floats() + 64) * sizeof(float)) != hipSuccess) {
    delete h;
    set_error("holo_mlp_mean_create: hipMalloc failed");
    return HOLO_E_HIP;
  }
  *out = h;
  return 0;
}

int holo_mlp_mean_destroy(HoloMlpMeanPooler* h) {
  if (!h) return 0;
  if (h->dev) (void)hipFree(h->dev);
  if (h->stage) (void)hipFree(h->stage);
  h->grads.release();
  delete h;
  return 0;
}

int holo_mlp_mean_set_param(HoloMlpMeanPooler* h, const char* name, const void* dev_ptr, int ndim, const int64_t* shape,
                            void* stream) {
  if (!h || !name || !dev_ptr || !shape) {
    set_error("holo_mlp_mean_set_param: null argument");
    return HOLO_E_INVALID;
  }
  const int rc = h->params.set("holo_mlp_mean_set_param", name, dev_ptr, ndim, shape, stream);
  if (!rc) h->committed = false;
  return rc;
}

// Folds the affine stretches on both sides of the LeakyReLU (mlp_folds.h) and uploads the kernels' image of them.
int holo_mlp_mean_commit(HoloMlpMeanPooler* h, void* stream) {
  if (!h) {
    set_error("holo_mlp_mean_commit: null");
    return HOLO_E_INVALID;
  }
  if (const char* missing = h->params.first_missing()) {
    set_error("holo_mlp_mean_commit: parameter '%s' has not been set", missing);
    return HOLO_E_STATE;
  }
  const HostParams& P = h->params;
  const MlpMeanFold fold =
      fold_mlp_mean(h->shape, P["_first_sampled.weight"], P["_first_sampled.bias"], P["_first_mean.weight"], P["_first_mean.bias"],
                    P["_mlp.mlp.0.0.weight"], P["_mlp.mlp.0.0.bias"], P["_last.weight"], P["_last.bias"],
                    P["pooled_feature_mapper.weight"], P["pooled_feature_mapper.bias"]);
  h->l0 = fold.l0;
  if (upload_via_stage(&h->stage, &h->stage_floats, h->dev, fold.image.data(), fold.image.size(), stream)) {
    set_error("holo_mlp_mean_commit: upload of the folded weights failed");
    return HOLO_E_HIP;
  }
  h->committed = true;
  return 0;
}

size_t holo_mlp_mean_workspace_bytes(const HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, int n_views) {
  if (!h || !feats || n_feats < 1 || n_views < 1) return 0;
  return maps_bytes(feats, n_feats, n_views, sizeof(float)) + 256;
}

int holo_mlp_mean_pool(HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, const HoloCamera* cameras,
                       int n_views, float* voxel_features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !feats || !cameras || !voxel_features || !workspace) {
    set_error("holo_mlp_mean_pool: null argument");
    return HOLO_E_INVALID;
  }
  if (!h->committed) {
    set_error("holo_mlp_mean_pool: call holo_mlp_mean_commit after setting the parameters");
    return HOLO_E_STATE;
  }
  if (n_feats != h->cfg.n_feats || n_views < 1 || n_views > ViewPoolParams::MAX_VIEWS) {
    set_error("holo_mlp_mean_pool: %d feature maps (created for %d), 1..%d source views", n_feats, h->cfg.n_feats,
              ViewPoolParams::MAX_VIEWS);
    return HOLO_E_INVALID;
  }
  if (workspace_bytes < holo_mlp_mean_workspace_bytes(h, feats, n_feats, n_views)) {
    set_error("holo_mlp_mean_pool: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  MlpMeanParams p;
  char* ws = (char*)workspace;
  const int rc = mlp_mean_fill(h, feats, n_feats, cameras, n_views, stream, p, ws);
  if (rc) return rc;
  p.vp.out = voxel_features;
  return mlp_mean_pool_launch(p, h->ctx->num_cus, stream) ? HOLO_E_INVALID : 0;
}

}  // extern "C"

// the forward's launch parameters: channels-last copies of the maps at ws (advanced), cameras, folded weights
static int mlp_mean_fill(HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, const HoloCamera* cameras, int n_views,
                         void* stream, MlpMeanParams& p, char*& ws) {
  memset(&p, 0, sizeof p);
  for (int k = 0; k < n_feats; ++k) {
    const HoloViewFeature& f = feats[k];
    if (!f.feats || f.channels != h->cfg.channels[k] || f.height < 1 || f.width < 1) {
      set_error("holo_mlp_mean_pool: feature map %d must have %d channels", k, h->cfg.channels[k]);
      return HOLO_E_INVALID;
    }
    p.vp.feat[k].quad0 = h->quad0[k];
    if (stage_map(f, n_views, p.vp.feat[k], ws, stream)) return HOLO_E_INVALID;
  }
  p.vp.n_feats = n_feats;
  p.vp.n_views = n_views;
  for (int v = 0; v < n_views; ++v) fill_pool_cam(cameras[v], p.vp.cams[v]);
  p.vp.R = h->cfg.resol;
  p.vp.half_extent = grid_half_extent(h->cfg.resol, h->cfg.volume_extent);
  p.vp.proj_eps = h->cfg.projection_eps;
  p.vp.F = h->cfg.feature_size;
  const int nh = h->cfg.n_hidden, F = h->cfg.feature_size;
  p.a = h->dev;
  p.am = p.a + (size_t)nh * h->dp;
  p.cb = p.am + (size_t)nh * h->dp;
  p.g = p.cb + nh;
  p.g0 = p.g + (size_t)F * nh;
  p.l = p.g0 + F;
  p.l0 = h->l0;
  p.dp = h->dp;
  p.emb0 = h->emb0;
  p.n_harmonic = h->cfg.n_harmonic_functions_ray;
  return 0;
}

// ---- backward (kernels_viewpool_bwd.hip: the MLPMean section).  Workspace layout, shared by the size query and the run.
struct MmBwdLayout {
  int64_t P, NR, NRp, Pp;  // per CHUNK of voxels
  int64_t Pall;
  int nchunks;
  int S, S2, FW, dp;
  size_t maps, gmaps, X, MEAN, CM, PRE, H, U, DUL, DULT, DPRET, DC, DCT, DX, DCA, part, fold, gfix, fixmax, total;
  bool fixed;  // deterministic mode (holo_ctx_set_deterministic): fixed-point images of the gradient maps
  // typed pointers into the workspace, straight into the kernels' parameters (b.fwd is filled): the row buffers, and for
  // every map whose gradient is wanted its channels-last image and, in the deterministic mode, the fixed-point one
  void bind(char* base, float* const* grad_feats, MlpMeanBwdParams& b) const {
    auto fp = [&](size_t off) { return (float*)(base + off); };
    b.X = fp(X), b.MEAN = fp(MEAN), b.CM = fp(CM), b.PRE = fp(PRE), b.H = fp(H), b.U = fp(U), b.DUL = fp(DUL);
    b.DULT = fp(DULT), b.DPRET = fp(DPRET), b.DC = fp(DC), b.DCT = fp(DCT), b.DX = fp(DX), b.DCA = fp(DCA);
    char *g = base + gmaps, *gx = base + gfix;
    for (int k = 0; k < b.fwd.vp.n_feats; ++k) {
      const ViewPoolParams::Feat& f = b.fwd.vp.feat[k];
      const size_t bytes = align256((size_t)b.fwd.vp.n_views * f.H * f.W * f.Cp * sizeof(float));
      if (grad_feats && grad_feats[k]) b.gfeat[k] = (float*)g;
      if (fixed && b.gfeat[k]) b.gfix[k] = (long long*)gx;
      g += bytes, gx += 2 * bytes;
    }
    if (fixed) b.fix_max = (uint32_t*)(base + fixmax);
  }
};
static MmBwdLayout mm_bwd_layout(const HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, int n_views) {
  MmBwdLayout L;
  memset(&L, 0, sizeof L);
  const int R = h->cfg.resol, F = h->cfg.feature_size;
  // the row buffers hold one CHUNK of voxels (all chunks the same size: the padding of the split-K operands stays valid):
  // the largest power-of-two fraction of the grid whose rows fit a 4 GiB budget (~2.5 KB per (voxel, view): 64^3 x 4 views
  // runs in one pass - 3.5 GB, 14.0 ms; chunked it measured 16.8 ms in 4 passes, 17.2 ms in 8 -, 64^3 x 16 views in four
  // passes of 65 536 voxels instead of 14 GB).  HOLO_MLP_MEAN_BWD_CHUNK=<voxels>: development / test knob
  L.Pall = (int64_t)R * R * R;
  L.nchunks = 1;
  {
    const int64_t row_bytes = (int64_t)(2 * h->dp + 3 * 128 + 3 * ((F + 1 + 3) / 4 * 4)) * 4 * n_views;
    int64_t target = ((int64_t)4 << 30) / (row_bytes > 0 ? row_bytes : 1);
    if (EMU_BUILD) target = 2048;  // (the emulation's small grids: two chunks at 16^3; the knob is not honoured there)
    else if (h->knobs.mlp_mean_bwd_chunk > 0) target = h->knobs.mlp_mean_bwd_chunk;
    while (L.Pall / L.nchunks > target && (L.Pall % (2 * L.nchunks)) == 0) L.nchunks *= 2;
  }
  L.P = L.Pall / L.nchunks;
  L.NR = L.P * n_views;
  L.dp = h->dp;
  L.FW = (F + 1 + 3) / 4 * 4;
  auto splits = [](int64_t rows, int64_t& padded) {
    int64_t S = rows / 1024;
    S = S < 1 ? 1 : (S > 128 ? 128 : S);
    const int64_t kc = ((rows + S - 1) / S + 31) / 32 * 32;
    padded = S * kc;
    return (int)S;
  };
  L.S = splits(L.NR, L.NRp);
  L.S2 = splits(L.P, L.Pp);
  size_t off = 0;
  auto take = [&](size_t floats) {
    const size_t o = off;
    off += align256(floats * sizeof(float));
    return o;
  };
  const size_t mapf = maps_bytes(feats, n_feats, n_views, sizeof(float)) / sizeof(float);
  L.maps = take(mapf);
  L.gmaps = take(mapf);
  L.X = take((size_t)L.NRp * L.dp);
  L.MEAN = take((size_t)L.Pp * L.dp);
  L.CM = take((size_t)L.P * 128);
  L.PRE = take((size_t)L.NR * 128);
  L.H = take((size_t)L.NRp * 128);
  L.U = take((size_t)L.NR * L.FW);
  L.DUL = take((size_t)L.NR * L.FW);
  L.DULT = take((size_t)L.FW * L.NRp);
  L.DPRET = take((size_t)128 * L.NRp);
  L.DC = take((size_t)L.P * 128);
  L.DCT = take((size_t)128 * L.Pp);
  L.DX = take((size_t)L.NR * L.dp);
  L.DCA = take((size_t)L.P * L.dp);
  const size_t pa = (size_t)L.S * 128 * L.dp, pam = (size_t)L.S2 * 128 * L.dp, pg = (size_t)L.S * L.FW * 128;
  const size_t pcol = (size_t)256 * 256;
  L.part = take(pa > pam ? (pa > pg ? (pa > pcol ? pa : pcol) : (pg > pcol ? pg : pcol)) : (pam > pg ? (pam > pcol ? pam : pcol) : (pg > pcol ? pg : pcol)));
  L.fold = take((size_t)2 * 128 * L.dp + 128 + (size_t)L.FW * 128 + L.FW);  // dA | dAm | dcb | dGext | dg0 dl0
  L.fixed = h->ctx && h->ctx->deterministic;
  L.gfix = L.fixed ? take(2 * mapf) : off;
  L.fixmax = L.fixed ? take(64) : off;
  L.total = off + 256;
  return L;
}

extern "C" {

size_t holo_mlp_mean_backward_workspace_bytes(const HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, int n_views) {
  if (!h || !feats || n_feats < 1 || n_views < 1) return 0;
  return mm_bwd_layout(h, feats, n_feats, n_views).total;
}

int holo_mlp_mean_backward(HoloMlpMeanPooler* h, const HoloViewFeature* feats, int n_feats, const HoloCamera* cameras, int n_views,
                           const float* grad_voxel_features, float* const* grad_feats, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (!h || !feats || !cameras || !grad_voxel_features || !workspace) {
    set_error("holo_mlp_mean_backward: null argument");
    return HOLO_E_INVALID;
  }
  if (!h->committed) {
    set_error("holo_mlp_mean_backward: call holo_mlp_mean_commit after setting the parameters");
    return HOLO_E_STATE;
  }
  if (n_feats != h->cfg.n_feats || n_views < 1 || n_views > ViewPoolParams::MAX_VIEWS || (h->cfg.feature_size & 3)) {
    set_error("holo_mlp_mean_backward: %d feature maps (created for %d), 1..%d source views, feature_size a multiple of 4", n_feats,
              h->cfg.n_feats, ViewPoolParams::MAX_VIEWS);
    return HOLO_E_INVALID;
  }
  const MmBwdLayout L = mm_bwd_layout(h, feats, n_feats, n_views);
  if (workspace_bytes < L.total) {
    set_error("holo_mlp_mean_backward: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  // zero everything behind the forward's maps: the gradient maps, the padding rows of the split-K operands
  HIP_TRY(hipMemsetAsync(base + L.gmaps, 0, L.total - 256 - L.gmaps, st));
  MlpMeanBwdParams b;
  memset(&b, 0, sizeof b);
  char* ws = base + L.maps;
  int rc = mlp_mean_fill(h, feats, n_feats, cameras, n_views, stream, b.fwd, ws);
  if (rc) return rc;
  const int F = h->cfg.feature_size, dp = L.dp, FW = L.FW;
  b.gout = grad_voxel_features;
  b.FW = FW;
  b.NRp = L.NRp;
  b.Pp = L.Pp;
  L.bind(base, grad_feats, b);
  float* part = (float*)(base + L.part);
  float* fold = (float*)(base + L.fold);
  float *dA = fold, *dAm = dA + (size_t)128 * dp, *dcb = dAm + (size_t)128 * dp, *dG = dcb + 128, *dgl = dG + (size_t)FW * 128;
  const int NR = (int)L.NR, P = (int)L.P;
  const int Kc = (int)(L.NRp / L.S), Kc2 = (int)(L.Pp / L.S2);
#define MM_TRY(x)                      \
  do {                                 \
    if (x) return HOLO_E_INVALID;      \
  } while (0)
  bool want = false;
  for (int k = 0; k < n_feats; ++k) want |= b.gfeat[k] != nullptr;
  b.Pc = L.P;
  b.Pall = L.Pall;
  for (int ck = 0; ck < L.nchunks; ++ck) {
    b.p0 = (int64_t)ck * L.P;
    const int acc = ck > 0 ? 1 : 0;  // the parameter gradients of the chunks add up in chunk order
    // forward recomputation
    MM_TRY(mm_bwd_step_launch(b, 0, stream));                                                                    // X, MEAN
    MM_TRY(gemm_batch_launch(b.MEAN, dp, b.fwd.am, dp, 0, b.CM, 128, P, 128, dp, 1, 0, 0, 0, stream));                     // CM = MEAN Am^T
    MM_TRY(gemm_batch_launch(b.X, dp, b.fwd.a, dp, 0, b.PRE, 128, NR, 128, dp, 1, 0, 0, 0, stream));                       // PRE = X A^T
    MM_TRY(mm_bwd_step_launch(b, 1, stream));                                                                    // + CM + b', H
    MM_TRY(gemm_batch_launch(b.H, 128, b.fwd.g, 128, 0, b.U, FW, NR, F, 128, 1, 0, 0, 0, stream));                         // U = H G^T
    MM_TRY(mm_bwd_step_launch(b, 2, stream));                                                                    // DUL, DULT
    // dG (rows 0..F-1) and dl (row F) = DULT H, split over the rows
    MM_TRY(gemm_batch_launch(b.DULT, (int)L.NRp, b.H, 128, 1, part, 128, FW, 128, Kc, L.S, Kc, (int64_t)Kc * 128, (int64_t)FW * 128, stream));
    MM_TRY(mm_sum_partials_launch(part, L.S, (int64_t)FW * 128, dG, stream, acc));
    MM_TRY(mm_colsum_launch(b.DUL, L.NR, FW, FW, part, 1024, dgl, stream, acc));                                 // dg0 | dl0
    MM_TRY(gemm_batch_launch(b.DUL, FW, b.fwd.g, 128, 1, b.H, 128, NR, 128, F, 1, 0, 0, 0, stream));                       // DH = DU G  (into H)
    MM_TRY(mm_bwd_step_launch(b, 3, stream));                                                                    // DPRE (in PRE), DPRET, DC, DCT
    MM_TRY(gemm_batch_launch(b.DPRET, (int)L.NRp, b.X, dp, 1, part, dp, 128, dp, Kc, L.S, Kc, (int64_t)Kc * dp, (int64_t)128 * dp, stream));
    MM_TRY(mm_sum_partials_launch(part, L.S, (int64_t)128 * dp, dA, stream, acc));
    MM_TRY(gemm_batch_launch(b.DCT, (int)L.Pp, b.MEAN, dp, 1, part, dp, 128, dp, Kc2, L.S2, Kc2, (int64_t)Kc2 * dp, (int64_t)128 * dp, stream));
    MM_TRY(mm_sum_partials_launch(part, L.S2, (int64_t)128 * dp, dAm, stream, acc));
    MM_TRY(mm_colsum_launch(b.DC, L.P, 128, 128, part, 256, dcb, stream, acc));
    if (want) {
      MM_TRY(gemm_batch_launch(b.PRE, 128, b.fwd.a, dp, 1, b.DX, dp, NR, dp, 128, 1, 0, 0, 0, stream));                    // DX = DPRE A
      MM_TRY(gemm_batch_launch(b.DC, 128, b.fwd.am, dp, 1, b.DCA, dp, P, dp, 128, 1, 0, 0, 0, stream));                    // DCA = DC Am
      if (L.fixed && ck > 0) HIP_TRY(hipMemsetAsync(b.fix_max, 0, 64, st));  // every chunk has its own binary point
      MM_TRY(mm_bwd_step_launch(b, 4, stream));
      if (L.fixed)  // the chunk's sums are added to the gradient maps in chunk order
        for (int k = 0; k < n_feats; ++k)
          if (b.gfix[k]) {
            const ViewPoolParams::Feat& f = b.fwd.vp.feat[k];
            MM_TRY(fix_flush_launch(b.gfix[k], b.fix_max + k, b.gfeat[k], (int64_t)n_views * f.H * f.W * f.Cp, stream));
          }
    }
  }
  if (want) {
    for (int k = 0; k < n_feats; ++k)
      if (b.gfeat[k]) {
        const ViewPoolParams::Feat& f = b.fwd.vp.feat[k];
        MM_TRY(nhwc_pad_to_nchw_launch(b.gfeat[k], grad_feats[k], n_views, f.C, f.Cp, (int64_t)f.H * f.W, stream));
      }
  }
#undef MM_TRY
  // ---- the folded gradients come to the host and are un-folded in float64 (the chain rule of holo_mlp_mean_commit's fold)
  FVec hf((size_t)2 * 128 * dp + 128 + (size_t)FW * 128 + FW);
  HIP_TRY(hipMemcpyAsync(hf.data(), fold, hf.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const HostParams& W = h->params;
  MlpMeanGrads d = unfold_mlp_mean_grads(h->shape, FW, W["_first_sampled.weight"], W["_first_sampled.bias"], W["_first_mean.weight"],
                                         W["_first_mean.bias"], W["_mlp.mlp.0.0.weight"], W["_last.weight"], W["_last.bias"],
                                         W["pooled_feature_mapper.weight"], hf);
  HostGrads& G = h->grads;
  G.put("_first_sampled.weight", std::move(d.dWs)), G.put("_first_mean.weight", std::move(d.dWm));
  G.put("_first_sampled.bias", d.dbsm), G.put("_first_mean.bias", std::move(d.dbsm));  // the fold sees only bs + bm
  G.put("_mlp.mlp.0.0.weight", std::move(d.dW1)), G.put("_mlp.mlp.0.0.bias", std::move(d.db1));
  G.put("_last.weight", std::move(d.dWl)), G.put("_last.bias", std::move(d.dbl));
  G.put("pooled_feature_mapper.weight", std::move(d.dM)), G.put("pooled_feature_mapper.bias", std::move(d.dmb));
  return G.publish(stream);
}

int holo_mlp_mean_get_grad(HoloMlpMeanPooler* h, const char* name, float* out_dev, int64_t numel, void* stream) {
  if (!h || !name || !out_dev) {
    set_error("holo_mlp_mean_get_grad: null argument");
    return HOLO_E_INVALID;
  }
  return h->grads.fetch("holo_mlp_mean_get_grad", name, out_dev, numel, stream);
}

}  // extern "C"
