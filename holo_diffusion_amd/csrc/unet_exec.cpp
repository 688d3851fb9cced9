// unet_exec.cpp — native runtime of the denoiser: replays the static launch plan of UNetModel.forward (built by Planner,
// unet_plan.h) and the training plan (built by TrainPlanner, unet_train_plan.h) on streams, and holds the C ABI of the
// denoiser, the sampler steps, Adam and the timers.
//
// The plan is a flat vector of ops; forward() only patches the three caller pointers (x, timesteps, y) and launches.  No
// allocation, no host synchronisation inside forward().
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <optional>
#include <string>
#include <vector>

#include "../../include/holo_abi.h"
#include "conv_weights.h"
#include "holo_common.h"
#include "holo_kernels.h"
#include "unet_plan.h"
#include "unet_train_plan.h"

namespace holo {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

}  // namespace holo

using namespace holo;
using namespace holo::unetplan;

int holo::pack_conv_weights(const float* src, const ConvWeights& dst, void* stream) {
  const ConvWeightLayout& l = dst.layout;
  int rc = repack_conv_weight_launch(src, dst.f32, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  if (!rc && dst.bf) rc = repack_conv_weight_bf16_launch(src, dst.bf, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  if (!rc && dst.wino2) rc = repack_conv_weight_wino2_launch(src, dst.wino2, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  if (!rc && dst.wino3) rc = repack_conv_weight_wino3_launch(src, dst.wino3, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  return rc;
}

// struct HoloCtx { device, num_cus }: holo_kernels.h (shared with render_exec.cpp)

struct HoloUnet {
  HoloCtx* ctx;
  UnetDesc d;  // everything a plan is built from (unet_plan.h)
  float* pstore = nullptr;       // one allocation for all private parameter copies
  uint16_t* pstore_bf = nullptr;  // bf16 copies of the conv weights
  float* pstore_wino = nullptr;  // Winograd copies of the conv weights
  Plan plan;                                        // inference (holo_unet_forward, _forward_cl, _fetch_block, _time_*)
  std::map<std::pair<int, bool>, size_t> ws_cache;  // (batch, batch_invariant) -> workspace bytes
  // ---- training (holo_unet_backward): weights of the transposed convolutions, packed like the forward ones
  // ([Cin][Cout] flipped taps for the stride-1 convs; [tap][Cout][Cin] for the stride-2 Downsample convs, whose stride-1
  // form lives under "<name>#s1"), supplied by holo_unet_set_dgrad_weight; this table owns every buffer it points to
  DgradTable dgrad;
  std::vector<float*> adam_copies;  // holo_unet_adam_step: per parameter, its plain private copy (null for a conv weight)
  float* dgrad_tmp = nullptr;  // the flipped / transposed OIDHW weight on its way into the packs: the largest conv weight's numel
  TrainPlan tplan;
  const int64_t* t_dev = nullptr;  // timesteps of the running call (time_embed backward)
  bool tape_valid = false;         // holo_unet_forward_train ran and nothing has consumed its tape
  std::map<int, size_t> tws_cache;
  // ---- the side lane of an inference plan (Planner::plan_side_lane, run_lanes): one non-blocking stream, the fork event, one
  // join event per consumer and the event of the error path; created by the first forward whose plan has a side lane
  void* side_stream = nullptr;
  void *fork_event = nullptr, *tail_event = nullptr;
  std::vector<void*> join_events;
};

namespace {

bool params_set(const HoloUnet* u, const char* entry) {
  for (auto& s : u->d.params)
    if (!s.set) {
      set_error("%s: parameter '%s' has not been set", entry, s.name.c_str());
      return false;
    }
  return true;
}

// the training plan of (batch, ws), rebuilt when either changed; `entry` names the caller in the workspace message
int ensure_train_plan(HoloUnet* u, const char* entry, int batch, void* ws, size_t ws_bytes) {
  if (!u->tplan.built_for(batch, ws)) {
    if (u->d.compute_mode != 0) {
      set_error("holo_unet_backward: the backward pass runs in the fp32 mode only");
      return HOLO_E_UNSUPPORTED;
    }
    if (!params_set(u, "holo_unet_backward")) return HOLO_E_STATE;
    TrainPlanner tp(&u->d, u->dgrad, batch, ws, u->tplan);
    tp.build();
    int rc = 0;
    if (!tp.err.empty()) {
      set_error("%s", tp.err.c_str());
      rc = HOLO_E_STATE;
    } else if (!tp.pl.regions_ok()) {
      set_error("internal: small-buffer regions overflow");
      rc = HOLO_E_INVALID;
    }
    if (rc) {
      u->tplan.invalidate();
      return rc;
    }
  }
  if (ws_bytes < u->tplan.bytes) {
    set_error("%s: workspace too small (%zu < %zu)", entry, ws_bytes, u->tplan.bytes);
    u->tplan.invalidate();
    return HOLO_E_WORKSPACE;
  }
  return 0;
}

int ensure_plan(HoloUnet* u, int batch, void* ws) {
  if (u->plan.built_for(batch, ws)) return 0;
  if (!params_set(u, "holo_unet_forward")) return HOLO_E_STATE;
  if (u->d.batch_invariant && u->d.compute_mode != 0) {  // (both setters refuse this; a guard for the plan itself)
    set_error("holo_unet_forward: the batch-invariant plan is exact-fp32 only");
    return HOLO_E_UNSUPPORTED;
  }
  Planner pl(&u->d, batch, ws, u->plan);
  pl.build();
  if (pl.err.empty()) preactivate_rowtile(u->plan, pl.knobs);
  int rc = 0;
  if (!pl.err.empty()) {
    set_error("holo_unet_forward: %s", pl.err.c_str());
    rc = HOLO_E_UNSUPPORTED;
  } else if (!pl.regions_ok()) {
    set_error("internal: small-buffer regions overflow");
    rc = HOLO_E_INVALID;
  }
  if (rc) u->plan.invalidate();
  return rc;
}

int run_op(const HoloUnet* u, const Op& op, int N, const float* x, const int64_t* t, float* y, void* stream) {
  switch (op.kind) {
    case OP_IN:
      return ncdhw_to_ndhwc_launch(x, op.in.dst, N, op.in.C, op.in.V, 0, stream, op.in.dst_bf16);
    case OP_TEMB:
      return time_embed_launch(t, N, u->d.cfg.model_channels, u->d.ted, op.temb.w1, op.temb.b1, op.temb.w2, op.temb.b2,
                               op.temb.emb, op.temb.emb_silu, op.temb.load_kind, stream);
    case OP_EMBLIN:
      return rows_linear_launch(op.emblin.emb_silu, op.emblin.w, op.emblin.b, op.emblin.out, N, u->d.emb_rows, u->d.ted, stream);
    case OP_STATS:
      return gn_stats_launch(op.stats.x, op.stats.part, N, op.stats.C, op.stats.V, stream, op.stats.x_bf16);
    case OP_FINAL: {
      const GnFinalize& f = op.fin;
      return gn_finalize_launch(f.part0, f.C0, f.B0, f.part1, f.C1, f.B1, N, f.V, f.groups, 1e-5f, f.gamma, f.beta, f.film,
                                f.film_stride, f.film_cout, f.coef, stream, f.moments, f.x0, f.x1, f.act, f.act_silu);
    }
    case OP_CONV:
      return conv_launch(op.conv, stream);
    case OP_GEMM:
      return gemm_launch(op.gemm, stream);
    case OP_SOFTMAX:
      return softmax_rows_launch(op.softmax.S, op.softmax.rows, op.softmax.cols, stream);
    case OP_FLASH: {
      const Flash& f = op.flash;
      if (f.form == 2) return flash_attn_bf16v2_launch(f.attn, f.packed, f.out_bf16, f.ksplit, f.lazy, stream, f.operands_packed);
      return flash_attn_launch(f.attn, stream);
    }
    case OP_OUT:
      return ndhwc_to_ncdhw_launch(op.out.src, y, N, op.out.C, op.out.V, stream);
  }
  return 0;
}

// The side lane's stream and events (the handle owns them; holo_unet_destroy).  The emulation build has one stream: its
// side lane is the caller's stream, fork and join are nothing (run_lanes).
int ensure_lanes(HoloUnet* u, int n_joins) {
#ifndef HOLO_EMU
  if (!u->side_stream) HIP_TRY(hipStreamCreateWithFlags((hipStream_t*)&u->side_stream, hipStreamNonBlocking));
  for (void** e : {&u->fork_event, &u->tail_event})
    if (!*e) HIP_TRY(hipEventCreateWithFlags((hipEvent_t*)e, hipEventDisableTiming));
  while ((int)u->join_events.size() < n_joins) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    u->join_events.push_back(e);
  }
#endif
  (void)u, (void)n_joins;
  return 0;
}

// Issues the ops of a plan in plan order from the host, each on its lane: `run(i, op, stream)` launches op i (or skips it)
// and returns its code.  Plan order is a valid serial order, and a side op stands in front of its consumer in it, so every
// event is recorded before anything waits for it - host order alone guarantees that.  The side stream starts behind everything
// the caller's stream holds at the fork, so the side ops of one call cannot overtake the previous call either.  Whatever
// happens after the fork, the caller's stream is left waiting for the side stream: on success through the consumers' joins
// (the last of them stands behind every side op, the side stream runs in order), on an error through the tail event.
template <class Run>
int run_lanes(HoloUnet* u, const Plan& plan, void* stream, Run run) {
  int rc = 0;
#ifdef HOLO_EMU
  for (size_t i = 0; i < plan.ops.size() && !rc; ++i) rc = run((int)i, plan.ops[i], stream);
#else
  if (!plan.n_joins) {
    for (size_t i = 0; i < plan.ops.size() && !rc; ++i) rc = run((int)i, plan.ops[i], stream);
    return rc ? (rc < 0 ? rc : HOLO_E_INVALID) : 0;
  }
  if ((rc = ensure_lanes(u, plan.n_joins))) return rc;
  const hipStream_t main = (hipStream_t)stream, side = (hipStream_t)u->side_stream;
  bool forked = false;
  hipError_t he = hipSuccess;
  for (size_t i = 0; i < plan.ops.size() && !rc && he == hipSuccess; ++i) {
    const Op& op = plan.ops[i];
    if (op.fork) {
      if ((he = hipEventRecord((hipEvent_t)u->fork_event, main)) != hipSuccess) break;
      if ((he = hipStreamWaitEvent(side, (hipEvent_t)u->fork_event, 0)) != hipSuccess) break;
      forked = true;
    }
    if (op.side) {
      rc = run((int)i, op, side);
      if (!rc && op.join >= 0) he = hipEventRecord((hipEvent_t)u->join_events[op.join], side);
    } else {
      if (op.join >= 0 && (he = hipStreamWaitEvent(main, (hipEvent_t)u->join_events[op.join], 0)) != hipSuccess) break;
      rc = run((int)i, op, main);
    }
  }
  if (he != hipSuccess) {
    set_error("the side lane of the forward failed: %s", hipGetErrorString(he));
    rc = HOLO_E_HIP;
  }
  if (rc && forked) {  // (best effort: the caller's stream still ends behind the side stream)
    if (hipEventRecord((hipEvent_t)u->tail_event, side) == hipSuccess) (void)hipStreamWaitEvent(main, (hipEvent_t)u->tail_event, 0);
  }
#endif
  return rc ? (rc < 0 ? rc : HOLO_E_INVALID) : 0;
}

// the forward of a plan (inference or training) on the caller's tensors; y may be null where the caller does not want it
int run_plan(HoloUnet* u, const Plan& plan, const float* x, const int64_t* t, float* y, void* stream) {
  return run_lanes(u, plan, stream, [&](int, const Op& op, void* st) {
    return op.kind == OP_OUT && !y ? 0 : run_op(u, op, plan.batch, x, t, y, st);
  });
}
int run_bwd_op(const BwdOp& op, const int64_t* t, void* stream) {
  switch (op.kind) {
    case BOP_CONV:
      return conv_launch(op.conv, stream);
    case BOP_WGRAD:
      return conv_wgrad_launch(op.wgrad.p, op.wgrad.plan, op.wgrad.dw, 0, stream);
    case BOP_COLSUM:
      return colsum_launch(op.colsum.g, op.colsum.M, op.colsum.C, op.colsum.scratch, op.colsum.out, 0, stream);
    case BOP_GN_BWD:
      return gn_bwd_launch(op.gn, stream);
    case BOP_ADD:
      return add_launch(op.add.dst, op.add.src, op.add.n, op.add.acc, stream);
    case BOP_SPLIT_CAT:
      return split_cat_launch(op.split.g, op.split.g0, op.split.g1, op.split.M, op.split.C0, op.split.C1, op.split.acc0, op.split.acc1, stream);
    case BOP_SUMPOOL2:
      return sumpool2_launch(op.pool.gup, op.pool.gin, op.pool.N, op.pool.R, op.pool.C, op.pool.acc, stream);
    case BOP_ZERO_INSERT2:
      return zero_insert2_launch(op.zins.gy, op.zins.out, op.zins.N, op.zins.Rs, op.zins.C, stream);
    case BOP_DGRAD_S2:
      return conv_dgrad_s2_launch(op.s2.gy, op.s2.wt, op.s2.gx, op.s2.N, op.s2.RI, op.s2.RO, op.s2.Ci, op.s2.Co, op.s2.acc, stream);
    case BOP_GEMM:
      return gemm_launch(op.gemm, stream);
    case BOP_SOFTMAX:
      return softmax_rows_launch(op.softmax.S, op.softmax.rows, op.softmax.cols, stream);
    case BOP_ATTN_DS:
      return attn_ds_launch(op.ds.P, op.ds.dP, op.ds.rows, op.ds.cols, stream);
    case BOP_TRANSPOSE:
      return transpose_launch(op.tr.in, op.tr.out, op.tr.batch, op.tr.T, stream);
    case BOP_FILM_BWD: {
      const FilmBwd& f = op.film;
      return film_bwd_launch(f.dfilm, f.embs, f.w, f.dw, f.db, f.gembs, f.N, f.rows, f.K, stream);
    }
    case BOP_TEMB_BWD: {
      const TimeEmbedBwd& e = op.temb;
      return time_embed_bwd_launch(t, e.N, e.mc, e.ted, e.w1, e.b1, e.w2, e.b2, e.gembs, e.dw1, e.db1, e.dw2, e.db2, stream);
    }
  }
  return 0;
}
// the backward launches of a training plan whose taped forward has run on `workspace` (u->t_dev: that forward's timesteps)
int run_backward(const HoloUnet* u, const TrainPlan& tp, const float* grad_out, float* grad_x, void* workspace, void* stream) {
  const HoloUnetCfg& c = u->d.cfg;
  const int batch = tp.fwd.batch;
  const int64_t V = (int64_t)c.image_size * c.image_size * c.image_size;
  if (ncdhw_to_ndhwc_launch(grad_out, (float*)((char*)workspace + tp.gy_off), batch, c.out_channels, V, 0, stream))
    return HOLO_E_INVALID;
  for (const BwdOp& op : tp.bops) {
    const int rc = run_bwd_op(op, u->t_dev, stream);
    if (rc) return rc < 0 ? rc : HOLO_E_INVALID;
  }
  if (grad_x && ndhwc_to_ncdhw_launch((const float*)((char*)workspace + tp.gx_off), grad_x, batch, c.in_channels, V, stream))
    return HOLO_E_INVALID;
  return 0;
}

// The sampler step entries (holo_*_step*, include/holo_abi.h): each names the pointers it needs, then its launcher checks the shapes
template <class Launch>
int step_entry(const char* entry, bool args_ok, Launch launch) {
  if (!args_ok) {
    set_error("%s: null/invalid argument", entry);
    return HOLO_E_INVALID;
  }
  return launch() ? HOLO_E_INVALID : 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int holo_abi_version(void) { return HOLO_ABI_VERSION; }
const char* holo_last_error(void) { return get_error(); }

int holo_ctx_create(int device_id, HoloCtx** out) {
  if (!out) {
    set_error("holo_ctx_create: null out");
    return HOLO_E_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  HoloCtx* c = new HoloCtx;
  c->device = device_id;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // (HOLO_NUM_CUS, test knob: planners size grids / split-K for this many CUs - the one knob read here, holo_knobs.h)
  if (const int64_t v = Knobs::from_env().num_cus) c->num_cus = (int)v;
  *out = c;
  return 0;
}
int holo_ctx_destroy(HoloCtx* ctx) {
  delete ctx;
  return 0;
}
int holo_ctx_set_deterministic(HoloCtx* ctx, int on) {
  if (!ctx) {
    set_error("holo_ctx_set_deterministic: null context");
    return HOLO_E_INVALID;
  }
  ctx->deterministic = on ? 1 : 0;
  return 0;
}
int holo_ctx_get_deterministic(const HoloCtx* ctx) { return ctx ? ctx->deterministic : 0; }

int holo_unet_create(HoloCtx* ctx, const HoloUnetCfg* cfg, HoloUnet** out) {
  if (!ctx || !cfg || !out) {
    set_error("holo_unet_create: null argument");
    return HOLO_E_INVALID;
  }
  if (!cfg->homogeneous_resample) {
    set_error("holo_unet_create: only homogeneous_resample=True is supported");
    return HOLO_E_UNSUPPORTED;
  }
  if (cfg->n_channel_mult < 1 || cfg->n_channel_mult > 8 || cfg->n_attention_resolutions > 8 ||
      cfg->model_channels % 32 || cfg->in_channels % 4 || cfg->out_channels % 4 || cfg->model_channels > 256 ||
      cfg->image_size % (1 << (cfg->n_channel_mult - 1))) {
    set_error("holo_unet_create: unsupported configuration");
    return HOLO_E_UNSUPPORTED;
  }
  HoloUnet* u = new HoloUnet;
  u->ctx = ctx;
  u->d.cfg = *cfg;
  u->d.num_cus = ctx->num_cus;
  build_structure(&u->d);
  enumerate_params(&u->d);
  u->d.knobs = Knobs::from_env();
  // private parameter storage
  const StoreSizes n = carve_params(&u->d, nullptr, nullptr, nullptr);
  if (hipMalloc((void**)&u->pstore, (size_t)n.f32 * sizeof(float)) != hipSuccess ||
      (n.bf && hipMalloc((void**)&u->pstore_bf, (size_t)n.bf * sizeof(uint16_t)) != hipSuccess) ||
      (n.wino && hipMalloc((void**)&u->pstore_wino, (size_t)n.wino * sizeof(float)) != hipSuccess)) {
    set_error("holo_unet_create: hipMalloc of the parameter stores (%lld floats, %lld bf16 weights, %lld Winograd floats) failed",
              (long long)n.f32, (long long)n.bf, (long long)n.wino);
    holo_unet_destroy(u);
    return HOLO_E_HIP;
  }
  carve_params(&u->d, u->pstore, u->pstore_bf, u->pstore_wino);
  *out = u;
  return 0;
}

int holo_unet_destroy(HoloUnet* net) {
  if (!net) return 0;
  if (net->pstore) (void)hipFree(net->pstore);
  if (net->pstore_bf) (void)hipFree(net->pstore_bf);
  if (net->pstore_wino) (void)hipFree(net->pstore_wino);
  for (auto& kv : net->dgrad)
    for (float* buf : {kv.second.f32, kv.second.wino2, kv.second.wino3})
      if (buf) (void)hipFree(buf);
  if (net->dgrad_tmp) (void)hipFree(net->dgrad_tmp);
#ifndef HOLO_EMU
  if (net->side_stream) {  // (every forward left the caller's stream waiting for it; drain it before its events go)
    (void)hipStreamSynchronize((hipStream_t)net->side_stream);
    (void)hipStreamDestroy((hipStream_t)net->side_stream);
  }
  for (void* e : {net->fork_event, net->tail_event})
    if (e) (void)hipEventDestroy((hipEvent_t)e);
  for (void* e : net->join_events) (void)hipEventDestroy((hipEvent_t)e);
#endif
  delete net;
  return 0;
}

int holo_unet_num_params(const HoloUnet* net) { return net ? (int)net->d.params.size() : 0; }

int holo_unet_param_info(const HoloUnet* net, int index, char* name, int name_cap, int64_t shape[8], int* ndim) {
  if (!net || index < 0 || index >= (int)net->d.params.size()) {
    set_error("holo_unet_param_info: bad index");
    return HOLO_E_INVALID;
  }
  const ParamSlot& s = net->d.params[index];
  if (name && name_cap > 0) {
    strncpy(name, s.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ndim) *ndim = (int)s.shape.size();
  if (shape)
    for (size_t i = 0; i < s.shape.size() && i < 8; ++i) shape[i] = s.shape[i];
  return 0;
}

int holo_unet_set_param(HoloUnet* net, const char* name, const void* dev_ptr, int dtype, int ndim,
                        const int64_t* shape, void* stream) {
  if (!net || !name || !dev_ptr) {
    set_error("holo_unet_set_param: null argument");
    return HOLO_E_INVALID;
  }
  if (dtype != HOLO_DTYPE_F32) {
    set_error("holo_unet_set_param: only fp32 parameters are supported");
    return HOLO_E_UNSUPPORTED;
  }
  auto it = net->d.pindex.find(name);
  if (it == net->d.pindex.end()) {
    set_error("holo_unet_set_param: unknown parameter '%s'", name);
    return HOLO_E_INVALID;
  }
  ParamSlot& s = net->d.params[it->second];
  bool ok = ndim == (int)s.shape.size();
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == s.shape[i];
  if (!ok) {
    set_error("holo_unet_set_param: shape mismatch for '%s'", name);
    return HOLO_E_INVALID;
  }
  if (s.is_conv()) {
    if (const int rc = pack_conv_weights((const float*)dev_ptr, s.w, stream)) return rc;
  } else {  // biases, GroupNorm parameters, Linear layers: a copy kernel with system-scope loads (holo_ld_sys) - like the
            // weight repack kernels, every ingestion of a caller-provided tensor reads it past the L2
    if (copy_sys_launch((const float*)dev_ptr, s.w.f32, s.numel, stream)) return HOLO_E_INVALID;
  }
  s.set = true;
  return 0;
}

int holo_unet_set_compute_dtype(HoloUnet* net, int dtype) {
  if (!net || (dtype != HOLO_DTYPE_F32 && dtype != HOLO_DTYPE_BF16 && dtype != HOLO_DTYPE_F32_BF16X3)) {
    set_error("holo_unet_set_compute_dtype: HOLO_DTYPE_F32, HOLO_DTYPE_BF16 or HOLO_DTYPE_F32_BF16X3");
    return HOLO_E_INVALID;
  }
  const int mode = dtype == HOLO_DTYPE_BF16 ? 1 : dtype == HOLO_DTYPE_F32_BF16X3 ? 2 : 0;
  if (mode != 0 && net->d.batch_invariant) {
    set_error("holo_unet_set_compute_dtype: the batch-invariant plan is exact-fp32 only; turn it off first "
              "(holo_unet_set_batch_invariant(net, 0))");
    return HOLO_E_UNSUPPORTED;
  }
  if (mode != net->d.compute_mode) {
    net->d.compute_mode = mode;
    net->plan.invalidate();  // re-plan: the conv ops carry the choice
    net->ws_cache.clear();   // ... and the plan's workspace differs between modes (fused skips, statistics slabs)
  }
  return 0;
}

int holo_unet_set_batch_invariant(HoloUnet* net, int on) {
  if (!net) {
    set_error("holo_unet_set_batch_invariant: null net");
    return HOLO_E_INVALID;
  }
  // Exact fp32 only.  The bf16 modes are refused rather than half supported: their plans pick kernels (the persistent
  // bf16 convolution, the streaming bf16 1x1x1 GEMMs, the packed bf16 attention) whose geometry helpers size their
  // work per launch, and no test pins the rows of those modes.
  if (on && net->d.compute_mode != 0) {
    set_error("holo_unet_set_batch_invariant: batch-invariant plans are exact-fp32 only (compute dtype HOLO_DTYPE_F32); "
              "the bf16 and bf16x3 modes are not supported");
    return HOLO_E_UNSUPPORTED;
  }
  if ((on != 0) != net->d.batch_invariant) {
    net->d.batch_invariant = on != 0;
    net->plan.invalidate();  // re-plan: the conv ops carry the choices (ws_cache is keyed on the flag)
  }
  return 0;
}

size_t holo_unet_workspace_bytes(HoloUnet* net, int batch) {
  if (!net || batch < 1) return 0;
  const std::pair<int, bool> key(batch, net->d.batch_invariant);
  auto it = net->ws_cache.find(key);
  if (it != net->ws_cache.end()) return it->second;
  Plan sizing;  // built on no workspace and dropped
  Planner pl(&net->d, batch, nullptr, sizing);
  pl.build();
  preactivate_rowtile(sizing, pl.knobs);
  net->ws_cache[key] = sizing.bytes;
  return sizing.bytes;
}

int holo_unet_forward(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, float* y, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!net || !x || !timesteps || !y || !workspace || batch < 1) {
    set_error("holo_unet_forward: null/invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  if (workspace_bytes < net->plan.bytes) {
    set_error("holo_unet_forward: workspace too small (%zu < %zu)", workspace_bytes, net->plan.bytes);
    return HOLO_E_WORKSPACE;
  }
  return run_plan(net, net->plan, x, timesteps, y, stream);
}

int holo_unet_forward_cl(HoloUnet* net, int batch, const float* x_cl, const int64_t* timesteps, float* y_cl, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!net || !x_cl || !timesteps || !y_cl || !workspace || batch < 1) {
    set_error("holo_unet_forward_cl: null/invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  const Plan& plan = net->plan;
  if (workspace_bytes < plan.bytes) {
    set_error("holo_unet_forward_cl: workspace too small (%zu < %zu)", workspace_bytes, plan.bytes);
    return HOLO_E_WORKSPACE;
  }
  if (plan.cl_refusal) {
    set_error("%s", plan.cl_refusal);
    return HOLO_E_UNSUPPORTED;
  }
  // the first / last convolution (Planner::find_cl_ends) run on the caller's channels-last tensors instead of the plan's
  // own input / output buffers, and the two layout passes are skipped
  const bool bf16_storage = net->d.compute_mode == 1;  // the plan's input buffer is bf16: a cast replaces the layout pass
  return run_lanes(net, plan, stream, [&](int i, const Op& op, void* st) {
    if (op.kind == OP_IN && bf16_storage)  // fp32 channels-last -> the plan's bf16 channels-last input buffer
      return f32_to_bf16_launch(x_cl, op.in.dst, (int64_t)batch * op.in.C * op.in.V, st) ? (int)HOLO_E_INVALID : 0;
    if (op.kind == OP_IN || op.kind == OP_OUT) return 0;
    if (i == plan.first_conv || i == plan.last_conv) {
      Op o2 = op;
      if (i == plan.first_conv && !bf16_storage) o2.conv.src0 = x_cl;
      if (i == plan.last_conv) o2.conv.out = y_cl;
      return run_op(net, o2, batch, x_cl, timesteps, y_cl, st);
    }
    return run_op(net, op, batch, x_cl, timesteps, y_cl, st);
  });
}

int holo_unet_fetch_block(HoloUnet* net, const char* tag, float* dst, int64_t dst_capacity, int64_t* numel,
                          void* workspace, void* stream) {
  if (!net || !tag || !dst || !workspace) {
    set_error("holo_unet_fetch_block: null argument");
    return HOLO_E_INVALID;
  }
  if (!net->d.knobs.keep_intermediates) {
    set_error("holo_unet_fetch_block: create the net with HOLO_KEEP_INTERMEDIATES=1");
    return HOLO_E_STATE;
  }
  const Plan& plan = net->plan;
  if (plan.ws != workspace || plan.ops.empty()) {
    set_error("holo_unet_fetch_block: no forward has run on this workspace");
    return HOLO_E_STATE;
  }
  auto it = plan.block_outputs.find(tag);
  if (it == plan.block_outputs.end()) {
    set_error("holo_unet_fetch_block: unknown tag '%s'", tag);
    return HOLO_E_INVALID;
  }
  const Act& a = it->second;
  const int64_t V = (int64_t)a.R * a.R * a.R;
  const int64_t n = (int64_t)plan.batch * V * a.C;
  if (numel) *numel = n;
  if (dst_capacity < n) {
    set_error("holo_unet_fetch_block: destination too small");
    return HOLO_E_INVALID;
  }
  return ndhwc_to_ncdhw_launch((const float*)((char*)workspace + a.off), dst, plan.batch, a.C, V, stream,
                               net->d.compute_mode == 1 ? 1 : 0);
}

int holo_unet_time_convs(HoloUnet* net, int batch, void* workspace, size_t workspace_bytes, int iters, void* stream,
                         float* total_ms, double* total_flops, int* n_launches) {
  if (!net || !workspace || iters < 1) {
    set_error("holo_unet_time_convs: invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  if (workspace_bytes < net->plan.bytes) {
    set_error("holo_unet_time_convs: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  double flops = 0.0;
  int launches = 0;
  for (const Op& op : net->plan.ops)
    if (op.kind == OP_CONV && op.conv.ksz == 3) {
      flops += conv_flops(op.conv);
      ++launches;
    }
  HIP_TRY(hipEventRecord(e0, (hipStream_t)stream));
  for (int it = 0; it < iters; ++it)
    for (const Op& op : net->plan.ops)
      if (op.kind == OP_CONV && op.conv.ksz == 3) {
        rc = conv_launch(op.conv, stream);
        if (rc) return HOLO_E_INVALID;
      }
  HIP_TRY(hipEventRecord(e1, (hipStream_t)stream));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (total_ms) *total_ms = ms / iters;
  if (total_flops) *total_flops = flops;
  if (n_launches) *n_launches = launches;
  return 0;
}

int holo_unet_time_ops(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, float* y, void* workspace,
                       size_t workspace_bytes, int iters, void* stream, HoloOpTiming* out, int cap, int* n_ops) {
  if (!net || !workspace || !x || !timesteps || !y || iters < 1 || !n_ops || (cap > 0 && !out)) {
    set_error("holo_unet_time_ops: invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  if (workspace_bytes < net->plan.bytes) {
    set_error("holo_unet_time_ops: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  int n = 0;
  for (const Op& op : net->plan.ops) {
    rc = run_op(net, op, batch, x, timesteps, y, stream);  // untimed first touch (also keeps the data flow valid)
    if (rc) return HOLO_E_INVALID;
    if (n < cap) {
      HIP_TRY(hipEventRecord(e0, (hipStream_t)stream));
      for (int it = 0; it < iters; ++it) run_op(net, op, batch, x, timesteps, y, stream);
      HIP_TRY(hipEventRecord(e1, (hipStream_t)stream));
      HIP_TRY(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
      HoloOpTiming& t = out[n];
      memset(&t, 0, sizeof(t));
      t.op = (int)op.kind;
      t.ms = ms / iters;
      if (op.kind == OP_CONV) {
        const ConvParams& c = op.conv;
        t.kernel = (int)c.kernel;
        t.tile_depth = c.tz;  // (0 off the halo forms)
        t.fused_skip = c.skip_w ? 1 : 0;
        t.nsplit = c.nsplit;
        t.cin = c.C0 + c.C1;
        t.cout = c.Cout;
        t.out_dim = c.OD;
        t.stride = c.stride;
        t.upsample = c.ups;
        t.ksz = c.ksz;
        t.flops = conv_flops(c);
        t.flops_executed = conv_exec_flops(c);
      } else if (op.kind == OP_FLASH) {
        const AttnParams& at = op.flash.attn;
        t.cin = t.cout = at.C;
        t.out_dim = at.T;
        t.flops = 4.0 * at.N * (double)at.T * at.T * at.C;
      } else if (op.kind == OP_GEMM) {
        t.cin = op.gemm.K;
        t.cout = op.gemm.Nn;
        t.out_dim = op.gemm.M;
        t.flops = 2.0 * op.gemm.nb0 * op.gemm.nb1 * (double)op.gemm.M * op.gemm.Nn * op.gemm.K;
      }
    }
    ++n;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *n_ops = n;
  return 0;
}

// ---- training: backward of the denoiser -----------------------------------------------------------------------------
// The transposed-convolution copies of convolution weight `s` from the caller's OIDHW tensor: holo_unet_set_dgrad_weight, and
// the refresh of holo_unet_adam_step (which meets every buffer already allocated).
static int prepare_dgrad_weight(HoloUnet* net, const ParamSlot& s, const void* dev_ptr, void* stream) {
  const int Co = (int)s.shape[0], Ci = (int)s.shape[1], T = s.kind == P_CONV3 ? 27 : 1;
  const std::string& nm = s.name;
  const bool down = is_downsample_weight(nm);
  if (down) {  // [tap][co][ci] for conv_dgrad_s2_kernel (the fallback), then the stride-1 form below under "<name>#s1":
               // the transposed stride-2 convolution runs as zero insertion + the stride-1 transposed convolution
    float*& d2 = net->dgrad[nm].f32;
    if (!d2) HIP_TRY(hipMalloc((void**)&d2, (size_t)T * Co * Ci * sizeof(float)));
    if (weight_tco_ci_launch((const float*)dev_ptr, d2, Co, Ci, T, stream)) return HOLO_E_INVALID;
    if ((Co & 3) || (Ci & 3)) return 0;
  }
  // The transposed convolution (Cout' = Ci, Cin' = Co), packed like a forward weight.  Its buffers are created at the first
  // call for this weight (an inference-only user pays nothing): the fp32 pack, and the Winograd packs of dgrad_copies - the
  // dgrad of a wide-level 3x3x3 conv runs on conv_wino2_kernel / conv_wino3_kernel like the forward conv.
  ConvWeights& dw = net->dgrad[down ? nm + "#s1" : nm];
  const ConvWeightLayout l = dw.layout = s.layout(true);
  const ConvCopies c = dgrad_copies(l, net->d.compute_mode, net->d.knobs);
  if (!dw.f32) HIP_TRY(hipMalloc((void**)&dw.f32, (size_t)l.f32_floats() * sizeof(float)));
  if ((c.wino2 && !dw.wino2) || (c.wino3 && !dw.wino3)) {  // a plan sized before these copies existed chose other kernels
    net->tws_cache.clear();                                 // (and scratch sizes)
    net->tplan.invalidate();
    if (!dw.wino2) HIP_TRY(hipMalloc((void**)&dw.wino2, (size_t)l.wino2_floats() * sizeof(float)));
    if (c.wino3 && !dw.wino3) HIP_TRY(hipMalloc((void**)&dw.wino3, (size_t)l.wino3_floats() * sizeof(float)));
  }
  if (!net->dgrad_tmp) {
    int64_t largest = 0;
    for (const ParamSlot& q : net->d.params)
      if (q.is_conv() && q.numel > largest) largest = q.numel;
    HIP_TRY(hipMalloc((void**)&net->dgrad_tmp, (size_t)largest * sizeof(float)));
  }
  if (flip_transpose_weight_launch((const float*)dev_ptr, net->dgrad_tmp, Co, Ci, T, stream)) return HOLO_E_INVALID;
  if (pack_conv_weights(net->dgrad_tmp, dw, stream)) return HOLO_E_INVALID;
  return 0;
}

int holo_unet_set_dgrad_weight(HoloUnet* net, const char* name, const void* dev_ptr, void* stream) {
  if (!net || !name || !dev_ptr) {
    set_error("holo_unet_set_dgrad_weight: null argument");
    return HOLO_E_INVALID;
  }
  auto it = net->d.pindex.find(name);
  if (it == net->d.pindex.end() || !net->d.params[it->second].is_conv()) {
    set_error("holo_unet_set_dgrad_weight: '%s' is not a convolution weight", name);
    return HOLO_E_INVALID;
  }
  return prepare_dgrad_weight(net, net->d.params[it->second], dev_ptr, stream);
}

size_t holo_unet_backward_workspace_bytes(HoloUnet* net, int batch) {
  if (!net || batch < 1) return 0;
  auto it = net->tws_cache.find(batch);
  if (it != net->tws_cache.end()) return it->second;
  TrainPlan sizing;  // built on no workspace (TrainPlanner::find_dgw: no transposed weight is missed there) and dropped
  TrainPlanner tp(&net->d, net->dgrad, batch, nullptr, sizing);
  tp.build();
  if (!tp.err.empty()) {
    set_error("%s", tp.err.c_str());
    return 0;
  }
  net->tws_cache[batch] = sizing.bytes;
  return sizing.bytes;
}

// The two halves of holo_unet_backward as entries of their own (ABI 4): a caller whose cotangent depends on the output - the
// clamp of pred_xstart in HoloDiffusionModel.training_backward - runs the taped forward, forms grad_out from y, then the backward,
// instead of paying a plain forward first.
int holo_unet_forward_train(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, float* y, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!net || !x || !timesteps || !workspace || batch < 1) {
    set_error("holo_unet_forward_train: null/invalid argument");
    return HOLO_E_INVALID;
  }
  net->tape_valid = false;
  int rc = ensure_train_plan(net, "holo_unet_forward_train", batch, workspace, workspace_bytes);
  if (rc) return rc;
  net->t_dev = timesteps;
  rc = run_plan(net, net->tplan.fwd, x, timesteps, y, stream);
  net->tape_valid = rc == 0;
  return rc;
}

int holo_unet_backward_taped(HoloUnet* net, int batch, const float* grad_out, float* grad_x, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (!net || !grad_out || !workspace || batch < 1) {
    set_error("holo_unet_backward_taped: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (!net->tape_valid || !net->tplan.built_for(batch, workspace) || workspace_bytes < net->tplan.bytes) {
    set_error("holo_unet_backward_taped: no taped forward of this batch on this workspace (holo_unet_forward_train first)");
    return HOLO_E_STATE;
  }
  net->tape_valid = false;  // the backward consumes the tape (gradient buffers share its workspace)
  return run_backward(net, net->tplan, grad_out, grad_x, workspace, stream);
}

int holo_unet_backward(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, const float* grad_out, float* y,
                       float* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
  if (!net || !x || !timesteps || !grad_out || !workspace || batch < 1) {
    set_error("holo_unet_backward: null/invalid argument");
    return HOLO_E_INVALID;
  }
  net->tape_valid = false;
  int rc = ensure_train_plan(net, "holo_unet_backward", batch, workspace, workspace_bytes);
  if (rc) return rc;
  net->t_dev = timesteps;
  rc = run_plan(net, net->tplan.fwd, x, timesteps, y, stream);
  return rc ? rc : run_backward(net, net->tplan, grad_out, grad_x, workspace, stream);
}

int holo_unet_get_grad(HoloUnet* net, const char* name, float* dst, int64_t numel, const void* workspace, void* stream) {
  if (!net || !name || !dst || !workspace) {
    set_error("holo_unet_get_grad: null argument");
    return HOLO_E_INVALID;
  }
  auto it = net->d.pindex.find(name);
  if (it == net->d.pindex.end()) {
    set_error("holo_unet_get_grad: unknown parameter '%s'", name);
    return HOLO_E_INVALID;
  }
  if (net->tplan.fwd.ws != workspace || net->tplan.grad_off.size() != net->d.params.size()) {
    set_error("holo_unet_get_grad: no backward pass has run on this workspace");
    return HOLO_E_STATE;
  }
  const ParamSlot& s = net->d.params[it->second];
  if (numel != s.numel) {
    set_error("holo_unet_get_grad: '%s' has %lld elements, not %lld", name, (long long)s.numel, (long long)numel);
    return HOLO_E_INVALID;
  }
  HIP_TRY(hipMemcpyAsync(dst, (const char*)workspace + net->tplan.grad_off[it->second], (size_t)numel * sizeof(float),
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// ---- parameter update (kernels_optim.hip) ----------------------------------------------------------------------------
// A float of the configuration as the double the caller wrote: the shortest decimal that rounds to it (0.9f -> 0.9).  torch
// forms 1 - beta2 and the bias corrections from the DOUBLE hyper-parameters; (double)0.999f would put 1.3e-5 of relative
// error into 1 - beta2.
static double widen_decimal(float f) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof(buf), "%.*g", prec, (double)f);
    if (strtof(buf, nullptr) == f) break;
  }
  return strtod(buf, nullptr);
}

static int adam_scalars(const char* who, const HoloAdamCfg* cfg, AdamScalars* s, double* dbg) {
  if (cfg->step < 1 || !(cfg->lr >= 0.f) || !(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) || !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f) ||
      !(cfg->eps >= 0.f) || !(cfg->weight_decay >= 0.f)) {
    set_error("%s: step >= 1, lr >= 0, betas in [0, 1), eps >= 0 and weight_decay >= 0 are required", who);
    return HOLO_E_INVALID;
  }
  const double lr = widen_decimal(cfg->lr), b1 = widen_decimal(cfg->beta1), b2 = widen_decimal(cfg->beta2);
  const double wd = widen_decimal(cfg->weight_decay);
  const double bc1 = 1.0 - pow(b1, (double)cfg->step), bc2 = 1.0 - pow(b2, (double)cfg->step);
  const double step_size = lr / bc1, bc2_sqrt = sqrt(bc2);
  if (s) {
    s->w1 = (float)(1.0 - b1);
    s->beta2 = (float)b2;
    s->w2 = (float)(1.0 - b2);
    s->eps = cfg->eps;
    s->neg_step_size = (float)-step_size;
    s->bc2_sqrt = (float)bc2_sqrt;
    s->weight_decay = (float)wd;
    s->decay = (float)(1.0 - lr * wd);
    s->adamw = cfg->adamw != 0;
  }
  if (dbg) {
    const double v[6] = {bc1, bc2, step_size, bc2_sqrt, 1.0 - b1, 1.0 - b2};
    memcpy(dbg, v, sizeof(v));
  }
  return 0;
}

int holo_adam_scalars(const HoloAdamCfg* cfg, double* out) {
  if (!cfg || !out) {
    set_error("holo_adam_scalars: null argument");
    return HOLO_E_INVALID;
  }
  return adam_scalars("holo_adam_scalars", cfg, nullptr, out);
}

int holo_adam_step(HoloCtx* ctx, const HoloAdamTensor* tensors, int n, const HoloAdamCfg* cfg, const float* clip_coef_dev,
                   void* stream) {
  if (!tensors || !cfg || n < 0) {
    set_error("holo_adam_step: null/invalid argument");
    return HOLO_E_INVALID;
  }
  (void)ctx;
  AdamScalars s;
  if (const int rc = adam_scalars("holo_adam_step", cfg, &s, nullptr)) return rc;
  return adam_step_launch(tensors, nullptr, n, s, clip_coef_dev, stream) ? HOLO_E_INVALID : 0;
}

size_t holo_grad_norm_workspace_bytes(const HoloAdamTensor* tensors, int n) {
  if (!tensors || n < 0) return 0;
  return (size_t)grad_norm_partials(tensors, n) * sizeof(double);
}

int holo_grad_norm(HoloCtx* ctx, const HoloAdamTensor* tensors, int n, float max_norm, void* workspace, size_t ws_bytes,
                   float* total_norm_dev, float* clip_coef_dev, void* stream) {
  if (!tensors || n < 0 || !total_norm_dev || !clip_coef_dev) {
    set_error("holo_grad_norm: null/invalid argument");
    return HOLO_E_INVALID;
  }
  (void)ctx;
  const size_t need = holo_grad_norm_workspace_bytes(tensors, n);
  if (need && (!workspace || ws_bytes < need || ((uintptr_t)workspace & 7))) {
    set_error("holo_grad_norm: workspace of %zu bytes (8-byte aligned) needed, got %zu", need, ws_bytes);
    return HOLO_E_WORKSPACE;
  }
  return grad_norm_launch(tensors, n, max_norm, (double*)workspace, total_norm_dev, clip_coef_dev, stream) ? HOLO_E_INVALID : 0;
}

int holo_unet_adam_step(HoloUnet* net, const HoloAdamTensor* tensors, int n, const HoloAdamCfg* cfg, const float* clip_coef_dev,
                        void* stream) {
  if (!net || !tensors || !cfg) {
    set_error("holo_unet_adam_step: null argument");
    return HOLO_E_INVALID;
  }
  if (n != (int)net->d.params.size()) {
    set_error("holo_unet_adam_step: %d tensors for %d parameters (holo_unet_param_info order)", n, (int)net->d.params.size());
    return HOLO_E_INVALID;
  }
  AdamScalars sc;
  if (const int rc = adam_scalars("holo_unet_adam_step", cfg, &sc, nullptr)) return rc;
  for (int i = 0; i < n; ++i) {
    const ParamSlot& s = net->d.params[i];
    if (!s.set) {
      set_error("holo_unet_adam_step: parameter '%s' was never bound (holo_unet_set_param)", s.name.c_str());
      return HOLO_E_STATE;
    }
    if (tensors[i].numel != s.numel || !tensors[i].param) {
      set_error("holo_unet_adam_step: tensor %d must be '%s' with %lld elements", i, s.name.c_str(), (long long)s.numel);
      return HOLO_E_INVALID;
    }
  }
  // (a) the update; a parameter the library keeps as a plain copy is written there by the same kernel
  if (net->adam_copies.size() != net->d.params.size()) {
    net->adam_copies.clear();
    for (const ParamSlot& s : net->d.params) net->adam_copies.push_back(s.is_conv() ? nullptr : s.w.f32);
  }
  net->tape_valid = false;  // (d) the taped activations belong to the old weights
  if (adam_step_launch(tensors, net->adam_copies.data(), n, sc, clip_coef_dev, stream)) return HOLO_E_INVALID;
  for (int i = 0; i < n; ++i) {
    const ParamSlot& s = net->d.params[i];
    if (!s.is_conv()) continue;
    // (b) the forward packs, (c) the transposed-convolution packs that exist (a Downsample weight: "<name>" and "<name>#s1")
    if (const int rc = pack_conv_weights(tensors[i].param, s.w, stream)) return rc;
    if (net->dgrad.count(s.name) || net->dgrad.count(s.name + "#s1"))
      if (const int rc = prepare_dgrad_weight(net, s, tensors[i].param, stream)) return rc;
  }
  return 0;
}

int holo_ddpm_step(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, int batch,
                   int64_t elems_per_sample, const float* x_t, const float* model_out, const float* noise,
                   int clip_denoised, float* sample, float* pred_xstart, void* stream) {
  return step_entry("holo_ddpm_step",
                    tables && timesteps && x_t && model_out && noise && sample && pred_xstart && batch >= 1, [&] {
    return ddpm_step_launch(tables, num_timesteps, timesteps, batch, elems_per_sample, x_t, model_out, noise, clip_denoised,
                            sample, pred_xstart, stream);
  });
}

int holo_ddpm_step_philox(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, int batch,
                          int64_t elems_per_sample, const float* x_t, const float* model_out, uint64_t seed,
                          uint64_t stream_offset, int clip_denoised, float* sample, float* pred_xstart, float* noise_out,
                          int ncdhw_channels, void* stream) {
  return step_entry("holo_ddpm_step_philox", tables && timesteps && x_t && model_out && sample && batch >= 1, [&] {
    return ddpm_step_philox_launch(tables, num_timesteps, timesteps, batch, elems_per_sample, x_t, model_out, seed, nullptr,
                                   stream_offset, clip_denoised, sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

int holo_ddpm_step_philox_rows(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, int batch,
                               int64_t elems_per_sample, const float* x_t, const float* model_out, uint64_t seed,
                               const uint32_t* row_streams, uint32_t timestep_index, int clip_denoised, float* sample,
                               float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddpm_step_philox_rows",
                    tables && timesteps && x_t && model_out && row_streams && sample && batch >= 1, [&] {
    return ddpm_step_philox_launch(tables, num_timesteps, timesteps, batch, elems_per_sample, x_t, model_out, seed,
                                   row_streams, timestep_index, clip_denoised, sample, pred_xstart, noise_out,
                                   ncdhw_channels, stream);
  });
}

// gaussian_diffusion.py:645-727 (ddim_sample / ddim_reverse_sample, the elementwise tail)
int holo_ddim_step(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                   const float* model_out, const float* noise, int clip_denoised, float* sample, float* pred_xstart,
                   void* stream) {
  return step_entry("holo_ddim_step", coefs && x_t && model_out && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_launch(coefs, batch, elems_per_sample, x_t, model_out, noise, clip_denoised, sample, pred_xstart, stream);
  });
}

// gaussian_diffusion.py:645-693 with the noise of :685 drawn in the kernel
int holo_ddim_step_philox(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                          const float* model_out, uint64_t seed, uint64_t stream_offset, int clip_denoised, float* sample,
                          float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddim_step_philox", coefs && x_t && model_out && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_philox_launch(coefs, batch, elems_per_sample, x_t, model_out, seed, nullptr, stream_offset, clip_denoised,
                                   sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

int holo_ddim_step_philox_rows(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                               const float* model_out, uint64_t seed, const uint32_t* row_streams, uint32_t timestep_index,
                               int clip_denoised, float* sample, float* pred_xstart, float* noise_out, int ncdhw_channels,
                               void* stream) {
  return step_entry("holo_ddim_step_philox_rows",
                    coefs && x_t && model_out && row_streams && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_philox_launch(coefs, batch, elems_per_sample, x_t, model_out, seed, row_streams, timestep_index,
                                   clip_denoised, sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

// DPM-Solver++ multistep update (the elementwise tail of ImplicitronGaussianDiffusion.dpm_sample_loop*)
int holo_dpm_step(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                  const float* model_out, const float* hist1, const float* hist2, int clip_denoised, float* sample,
                  float* pred_xstart, void* stream) {
  return step_entry("holo_dpm_step", coefs && x_t && model_out && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return dpm_step_launch(coefs, batch, elems_per_sample, x_t, model_out, hist1, hist2, clip_denoised, sample, pred_xstart,
                           stream);
  });
}

// gaussian_diffusion.py:429-433 (condition_mean) inside p_sample :499-506
int holo_ddpm_step_guided(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, const float* variances,
                          int batch, int64_t elems_per_sample, const float* x_t, const float* model_out, const float* grad,
                          const float* noise, int clip_denoised, float* sample, float* pred_xstart, void* stream) {
  return step_entry("holo_ddpm_step_guided",
                    tables && timesteps && variances && x_t && model_out && grad && noise && sample && batch >= 1, [&] {
    return ddpm_step_guided_launch(tables, num_timesteps, timesteps, variances, batch, elems_per_sample, x_t, model_out, grad,
                                   noise, clip_denoised, sample, pred_xstart, stream);
  });
}

// the same with the noise of :498 drawn in the kernel; row_streams null: the offset form, else one stream per row
int holo_ddpm_step_guided_philox(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps,
                                 const float* variances, int batch, int64_t elems_per_sample, const float* x_t,
                                 const float* model_out, const float* grad, uint64_t seed, uint64_t stream_offset,
                                 const uint32_t* row_streams, uint32_t timestep_index, int clip_denoised, float* sample,
                                 float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddpm_step_guided_philox",
                    tables && timesteps && variances && x_t && model_out && grad && sample && batch >= 1, [&] {
    return ddpm_step_guided_philox_launch(tables, num_timesteps, timesteps, variances, batch, elems_per_sample, x_t, model_out,
                                          grad, seed, row_streams, row_streams ? (uint64_t)timestep_index : stream_offset,
                                          clip_denoised, sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

// gaussian_diffusion.py:445-453 (condition_score) followed by ddim_sample :674-693
int holo_ddim_step_guided(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                          const float* model_out, const float* grad, const float* noise, int clip_denoised, float* sample,
                          float* pred_xstart, void* stream) {
  return step_entry("holo_ddim_step_guided",
                    coefs && x_t && model_out && grad && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_guided_launch(coefs, batch, elems_per_sample, x_t, model_out, grad, noise, clip_denoised, sample,
                                   pred_xstart, stream);
  });
}

// the same with the noise of :685 drawn in the kernel; row_streams as holo_ddpm_step_guided_philox
int holo_ddim_step_guided_philox(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                                 const float* model_out, const float* grad, uint64_t seed, uint64_t stream_offset,
                                 const uint32_t* row_streams, uint32_t timestep_index, int clip_denoised, float* sample,
                                 float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddim_step_guided_philox",
                    coefs && x_t && model_out && grad && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_guided_philox_launch(coefs, batch, elems_per_sample, x_t, model_out, grad, seed, row_streams,
                                          row_streams ? (uint64_t)timestep_index : stream_offset, clip_denoised, sample,
                                          pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

// masked (inpainting) DDPM step: the known part noised to level t - 1 blended with the DDPM update by a per-voxel mask
int holo_ddpm_step_inpaint(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps,
                           const float* known_coefs, int batch, int64_t elems_per_sample, int channels, int layout,
                           const float* x_t, const float* model_out, const float* x0_known, const float* mask,
                           const float* noise, const float* noise_known, int clip_denoised, float* sample,
                           float* pred_xstart, void* stream) {
  return step_entry("holo_ddpm_step_inpaint", tables && timesteps && known_coefs && x_t && model_out && x0_known && mask &&
                                                  noise && sample && batch >= 1, [&] {
    return ddpm_step_inpaint_launch(tables, num_timesteps, timesteps, known_coefs, batch, elems_per_sample, channels, layout,
                                    x_t, model_out, x0_known, mask, noise, noise_known, clip_denoised, sample, pred_xstart,
                                    stream);
  });
}

// the same with both noises drawn in the kernel; row_streams as holo_ddpm_step_guided_philox
int holo_ddpm_step_inpaint_philox(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps,
                                  const float* known_coefs, int batch, int64_t elems_per_sample, int channels, int layout,
                                  const float* x_t, const float* model_out, const float* x0_known, const float* mask,
                                  uint64_t seed, uint64_t stream_offset, const uint32_t* row_streams, uint32_t timestep_index,
                                  int clip_denoised, float* sample, float* pred_xstart, float* noise_out,
                                  float* noise_known_out, void* stream) {
  return step_entry("holo_ddpm_step_inpaint_philox",
                    tables && timesteps && known_coefs && x_t && model_out && x0_known && mask && sample && batch >= 1, [&] {
    return ddpm_step_inpaint_philox_launch(tables, num_timesteps, timesteps, known_coefs, batch, elems_per_sample, channels,
                                           layout, x_t, model_out, x0_known, mask, seed, row_streams,
                                           row_streams ? (uint64_t)timestep_index : stream_offset, clip_denoised, sample,
                                           pred_xstart, noise_out, noise_known_out, stream);
  });
}

// q_sample (gaussian_diffusion.py:189-204) on a row (a, b) per sample, and its form with the noise drawn in the kernel
int holo_q_sample(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x, const float* noise,
                  float* out, void* stream) {
  return step_entry("holo_q_sample", coefs && x && noise && out && batch >= 1 && elems_per_sample >= 4, [&] {
    return q_sample_launch(coefs, batch, elems_per_sample, x, noise, out, stream);
  });
}

int holo_q_sample_philox(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x, uint64_t seed,
                         uint64_t stream_offset, const uint32_t* row_streams, uint32_t timestep_index, float* out,
                         float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_q_sample_philox", coefs && x && out && batch >= 1 && elems_per_sample >= 4, [&] {
    return q_sample_philox_launch(coefs, batch, elems_per_sample, x, seed, row_streams,
                                  row_streams ? (uint64_t)timestep_index : stream_offset, out, noise_out, ncdhw_channels,
                                  stream);
  });
}

// The losses of training_losses (gaussian_diffusion.py:941-959) and the terms of _vb_terms_bpd / calc_bpd_loop (:817-850,
// :1027-1029): one streaming launch and a one-workgroup finalize each, partial sums in the caller's workspace
static bool loss_shape_ok(int batch, int64_t per) { return batch >= 1 && batch <= 65535 && per >= 4 && (per & 3) == 0; }

size_t holo_diffusion_loss_workspace_bytes(int batch, int64_t elems_per_sample) {
  if (!loss_shape_ok(batch, elems_per_sample)) {
    set_error("holo_diffusion_loss_workspace_bytes: batch in 1 .. 65535 and elems_per_sample a positive multiple of 4");
    return 0;
  }
  return (size_t)loss_partials(batch, elems_per_sample) * sizeof(double);
}

static int loss_workspace_ok(const char* entry, int batch, int64_t per, const void* workspace, size_t ws_bytes) {
  if (!loss_shape_ok(batch, per)) {
    set_error("%s: batch must be in 1 .. 65535 and elems_per_sample a positive multiple of 4", entry);
    return HOLO_E_INVALID;
  }
  const size_t need = (size_t)loss_partials(batch, per) * sizeof(double);
  if (!workspace || ws_bytes < need || ((uintptr_t)workspace & 7)) {
    set_error("%s: workspace of %zu bytes (8-byte aligned) needed, got %zu", entry, need, workspace ? ws_bytes : (size_t)0);
    return HOLO_E_WORKSPACE;
  }
  return 0;
}

int holo_diffusion_loss(HoloCtx*, int batch, int64_t elems_per_sample, const float* target, const float* model_out,
                        const float* row_scale, double* terms, float* grad_out, void* workspace, size_t ws_bytes,
                        void* stream) {
  if (!target || !model_out) {
    set_error("holo_diffusion_loss: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (!terms && !grad_out) {
    set_error("holo_diffusion_loss: at least one of terms and grad_out must be given");
    return HOLO_E_INVALID;
  }
  if (const int rc = loss_workspace_ok("holo_diffusion_loss", batch, elems_per_sample, workspace, ws_bytes)) return rc;
  return diffusion_loss_launch(batch, elems_per_sample, target, model_out, row_scale, terms, grad_out, (double*)workspace, stream)
             ? HOLO_E_INVALID
             : 0;
}

int holo_vb_terms(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_start, const float* x_t,
                  const float* noise, const float* model_out, int clip_denoised, double* terms, void* workspace,
                  size_t ws_bytes, void* stream) {
  if (!coefs || !x_start || !x_t || !model_out || !terms) {
    set_error("holo_vb_terms: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (const int rc = loss_workspace_ok("holo_vb_terms", batch, elems_per_sample, workspace, ws_bytes)) return rc;
  return vb_terms_launch(coefs, batch, elems_per_sample, x_start, x_t, noise, model_out, clip_denoised, terms,
                         (double*)workspace, stream)
             ? HOLO_E_INVALID
             : 0;
}

int holo_tanh(HoloCtx* ctx, const float* x, float* y, int64_t n, void* stream) {
  (void)ctx;
  return tanh_launch(x, y, n, stream);
}
int holo_clip(HoloCtx* ctx, const float* x, float* y, float lo, float hi, int64_t n, void* stream) {
  (void)ctx;
  return clip_launch(x, y, lo, hi, n, stream);
}

int holo_event_timer_create(void** timer) {
  hipEvent_t* ev = new hipEvent_t[2];
  if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
    set_error("hipEventCreate failed");
    return HOLO_E_HIP;
  }
  *timer = ev;
  return 0;
}
int holo_event_timer_start(void* timer, void* stream) {
  HIP_TRY(hipEventRecord(((hipEvent_t*)timer)[0], (hipStream_t)stream));
  return 0;
}
int holo_event_timer_stop(void* timer, void* stream, float* elapsed_ms) {
  hipEvent_t* ev = (hipEvent_t*)timer;
  HIP_TRY(hipEventRecord(ev[1], (hipStream_t)stream));
  HIP_TRY(hipEventSynchronize(ev[1]));
  HIP_TRY(hipEventElapsedTime(elapsed_ms, ev[0], ev[1]));
  return 0;
}
int holo_event_timer_destroy(void* timer) {
  hipEvent_t* ev = (hipEvent_t*)timer;
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  delete[] ev;
  return 0;
}

}  // extern "C"
