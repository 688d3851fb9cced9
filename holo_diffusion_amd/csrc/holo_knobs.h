// holo_knobs.h — every HOLO_* environment variable the library reads: ONE table, and the only getenv of csrc/.
//
// WHEN a knob is read (the `when` column).  A snapshot is a plain `Knobs` value taken by Knobs::from_env():
//   CTX     holo_ctx_create.  HOLO_NUM_CUS only: the Python layer caches one context per device for the life of the
//           process, so nothing else may be frozen there.
//   HANDLE  handle creation (holo_unet_create, holo_renderer_create, holo_mlp_mean_create): the knobs that decide what the
//           handle allocates or how its workspace is laid out.  The snapshot lives in the handle; its size queries, its
//           calls and (for the denoiser) holo_unet_set_dgrad_weight use that copy and never read again.
//   PLAN    plan construction (Planner / TrainPlanner, hence the *_workspace_bytes sizing entries and time_ops): every knob
//           that shapes a plan.  conv_plan, flash_attn_splits, flash_attn_bf16v2_ksplit and wgrad_plan take the planner's
//           snapshot; what a launcher needs of it is stored IN THE OP (key splits and the lazy / exact choice of the bf16
//           attention, the weight-gradient geometry, the timestep-load flag), so Plan + handle determine what runs.
//   CALL    an entry without a handle or a plan (holo_view_pool_backward): once at the ABI entry, passed down.
// Launch functions (*_launch and everything reached from holo_unet_forward* / holo_unet_backward / holo_render* after
// planning) never read the environment.
// (HOLO_CONV_WINO3 is read twice: HANDLE decides whether the F(2x2x2) weights exist, PLAN whether conv_plan may pick them.)
//
// HOW a knob is parsed (the `kind` column; the rules the scattered reads had):
//   INT   integer (strtoll), the default when unset or empty
//   RAW   integer (atoll) of whatever is set - the empty string is 0 -, the default when unset
//   SET   true when the variable is set at all, whatever its text
//   CH    true when the first character is the one in the default column
//   POS   a positive integer; anything else (unset, 0, negative, text) is 0 = ignored
// KNOB_UNSET as a default keeps "unset" distinguishable where the default depends on the device or the build (named in the
// row's text).  Range clamps (HOLO_FLASH_SPLIT, HOLO_FLASH_V2_KSPLIT) stay where the shape is known.
#pragma once

#include <stdint.h>
#include <stdlib.h>

namespace holo {

#ifdef HOLO_EMU  // the TEST-ONLY host emulation (holo_common.h): a few defaults are sized for its tiny cases
constexpr bool EMU_BUILD = true;
#else
constexpr bool EMU_BUILD = false;
#endif

constexpr int64_t KNOB_UNSET = INT64_MIN;

// X(field, environment name, kind, default, when, what it does)
#define HOLO_KNOBS(X)                                                                                                      \
  X(num_cus, "HOLO_NUM_CUS", POS, 0, CTX, "planners size grids and split-K for this many CUs (default: the device's)")     \
  X(conv_wino, "HOLO_CONV_WINO", INT, 1, HANDLE, "0: no Winograd copies of the conv weights (forward and dgrad)")          \
  X(conv_wino3, "HOLO_CONV_WINO3", INT, 1, HANDLE_PLAN, "0: no F(2x2x2, 3x3x3) copies / conv_wino3_kernel never chosen")   \
  X(keep_intermediates, "HOLO_KEEP_INTERMEDIATES", CH, '1', HANDLE,                                                        \
    "1: the plan releases no activation, holo_unet_fetch_block works")                                                     \
  X(render_v1, "HOLO_RENDER_V1", SET, 0, HANDLE, "the ray-per-column render kernel for everything")                        \
  X(render2_nw, "HOLO_RENDER2_NW", INT, 0, HANDLE, "8: the 8-wave form of render2_kernel's 12-wave configurations")        \
  X(render2_nrm_nw, "HOLO_RENDER2_NRM_NW", INT, 0, HANDLE,                                                                 \
    "8: rendered normals two waves per SIMD instead of 10 waves (the emulation build always runs 8)")                      \
  X(render_wgs, "HOLO_RENDER_WGS", POS, 0, HANDLE, "persistent render workgroups (default: one per CU)")                   \
  X(render_xcd, "HOLO_RENDER_XCD", RAW, KNOB_UNSET, HANDLE,                                                                \
    "XCD ranges of the render tile order (default 8; 2 in the emulation build; <= 1: plain order)")                        \
  X(render_tail, "HOLO_RENDER_TAIL", RAW, KNOB_UNSET, HANDLE,                                                              \
    "4-ray tiles at the end of every XCD range handed out as single rays (default: about two rounds; 3 in the "            \
    "emulation build; 0: off)")                                                                                            \
  X(render_static_tiles, "HOLO_RENDER_STATIC_TILES", SET, 0, HANDLE, "static tile stride instead of the dynamic hand-out") \
  X(render_timeline, "HOLO_RENDER_TIMELINE", SET, 0, HANDLE, "per-phase clocks of every render launch (synchronises!)")    \
  X(mlp_mean_bwd_chunk, "HOLO_MLP_MEAN_BWD_CHUNK", POS, 0, HANDLE,                                                         \
    "voxels per chunk of holo_mlp_mean_backward (default: what fits 4 GiB of rows; the emulation build: always 2048)")     \
  X(conv_wino_small, "HOLO_CONV_WINO_SMALL", INT, 1, PLAN, "0: under-filled levels take 64-voxel tiles, not Winograd")     \
  X(conv_force_tz2, "HOLO_CONV_FORCE_TZ2", INT, 0, PLAN, "1: 128-voxel tiles (hence the Winograd kernels) on small grids") \
  X(conv_qkv_fused, "HOLO_CONV_QKV_FUSED", INT, 1, PLAN, "0: row-tile qkv convolution + attn_pack_kernel")                 \
  X(conv1x1_bf16_stream, "HOLO_CONV1X1_BF16_STREAM", INT, 1, PLAN, "0: the row-tile kernel for bf16 1x1x1 convolutions")   \
  X(conv1x1_stream_min_m, "HOLO_CONV1X1_STREAM_MIN_M", INT, 131072, PLAN,                                                  \
    "rows from which a raw-input fp32 1x1x1 convolution streams (0: never)")                                               \
  X(conv1x1_small, "HOLO_CONV1X1_SMALL", INT, 1, PLAN, "0: the row-tile kernel for the fp32 attention's 1x1x1 convs")      \
  X(conv_s2t, "HOLO_CONV_S2T", INT, -1, PLAN, "stride-2 bf16 halo kernel: 0 never, 1 wherever defined (default: by fill)") \
  X(conv_bf16t, "HOLO_CONV_BF16T", INT, -1, PLAN, "bf16 wide-tile kernel: 0 never, 1 everywhere (default: by fill / K)")   \
  X(conv_bf16p, "HOLO_CONV_BF16P", INT, -1, PLAN,                                                                          \
    "its persistent form: 0 never, 1 every wide-tile launch, 2 activated input too (default: raw input)")                  \
  X(conv_bf16p_wgs, "HOLO_CONV_BF16P_WGS", INT, 0, PLAN, "at most this many persistent workgroups (0: no cap)")            \
  X(conv_wino3_min_items, "HOLO_CONV_WINO3_MIN_ITEMS", INT, KNOB_UNSET, PLAN,                                              \
    "work items from which conv_wino3_kernel runs (default: num_cus / 2)")                                                 \
  X(conv_wino3_up, "HOLO_CONV_WINO3_UP", INT, 1, PLAN,                                                                     \
    "0: upsampling convolutions on conv_wino3_kernel's generic form (64 pseudo-taps), not its 27-tap form")               \
  X(no_skip_fusion, "HOLO_NO_SKIP_FUSION", SET, 0, PLAN, "a ResBlock's 1x1x1 skip always as its own launch")               \
  X(skip_fusion_below_r, "HOLO_SKIP_FUSION_BELOW_R", RAW, 64, PLAN,                                                        \
    "exact fp32: the skip is fused into the second convolution below this grid edge")                                      \
  X(side_lane_cus, "HOLO_SIDE_LANE_CUS", INT, 128, PLAN,                                                                   \
    "exact fp32 inference: CUs the skip half of a split up-path concat convolution is planned for (0: nothing is split)")  \
  X(side_lane_min_r, "HOLO_SIDE_LANE_MIN_R", INT, 32, PLAN, "smallest grid edge whose concat convolutions are split")      \
  X(side_lane_fork_r, "HOLO_SIDE_LANE_FORK_R", INT, 8, PLAN,                                                               \
    "the side lane starts in front of the first descent level whose grid edge is at most this")                            \
  X(rowtile_preact, "HOLO_ROWTILE_PREACT", INT, 1, PLAN,                                                                   \
    "0: row-tile convolutions of the deepest level apply GroupNorm + SiLU themselves, per tap and Cout tile")              \
  X(no_flash_attn, "HOLO_NO_FLASH_ATTN", SET, 0, PLAN, "attention as GEMM + softmax + GEMM")                               \
  X(bf16_flash_min_t, "HOLO_BF16_FLASH_MIN_T", RAW, 1024, PLAN, "tokens from which the bf16 mode takes its bf16 attention") \
  X(flash_split, "HOLO_FLASH_SPLIT", INT, 0, PLAN, "key splits of the fp32 attention, clamped to [1, T/128] (0: by fill)") \
  X(flash_v2_ksplit, "HOLO_FLASH_V2_KSPLIT", INT, 0, PLAN,                                                                 \
    "key splits of the bf16 attention: 1..8 dividing T into multiples of 128, else ignored")                               \
  X(attn_exact, "HOLO_ATTN_EXACT", SET, 0, PLAN, "bf16 attention: the exact loop alone, no LAZY pass")                     \
  X(debug_timestep_load, "HOLO_DEBUG_TIMESTEP_LOAD", INT, 0, PLAN, "how time_embed_kernel loads the timesteps (see it)")   \
  X(dgrad_s2_direct, "HOLO_DGRAD_S2_DIRECT", CH, '1', PLAN, "1: conv_dgrad_s2_kernel for every Downsample dgrad")          \
  X(wgrad_tiles, "HOLO_WGRAD_TILES", POS, 0, PLAN, "> 0: the tile weight-gradient kernel instead of the row-staged one")   \
  X(wgrad_reduce_tile_min, "HOLO_WGRAD_REDUCE_TILE_MIN", RAW, 1024, PLAN,                                                  \
    "64-element tiles from which the weight-gradient reduce runs its tile form")                                           \
  X(debug_plan, "HOLO_DEBUG_PLAN", SET, 0, PLAN, "[plan] lines on stderr: what every convolution / attention launches")    \
  X(viewpool_bwd_v1, "HOLO_VIEWPOOL_BWD_V1", CH, '1', CALL, "1: the register-accumulating view-pool backward kernel")      \
  HOLO_KNOBS_DEV(X)  /* (below) */

#ifdef HOLO_DEV_PROBES  // timing probes of a development build only (-DHOLO_DEV_PROBES): they DROP gradients
#define HOLO_KNOBS_DEV(X)                                                                                                  \
  X(viewpool_bwd_probe, "HOLO_VIEWPOOL_BWD_PROBE", RAW, KNOB_UNSET, CALL,                                                  \
    "view-pool backward: 0 no pass 2, 2 pass 2 without its atomics, 10 + k the atomics of map k alone")                    \
  X(viewpool_bwd_occ, "HOLO_VIEWPOOL_BWD_OCC", CH, '3', CALL, "view-pool backward: 3 = the 166-register build")
#else
#define HOLO_KNOBS_DEV(X)
#endif

typedef int64_t knob_INT_t, knob_RAW_t, knob_POS_t;
typedef bool knob_SET_t, knob_CH_t;
static inline int64_t knob_INT(const char* e, int64_t dflt) { return e && e[0] ? strtoll(e, nullptr, 10) : dflt; }
static inline int64_t knob_RAW(const char* e, int64_t dflt) { return e ? atoll(e) : dflt; }
static inline bool knob_SET(const char* e, int) { return e != nullptr; }
static inline bool knob_CH(const char* e, char c) { return e && e[0] == c; }
static inline int64_t knob_POS(const char* e, int) { return e && atoll(e) > 0 ? atoll(e) : 0; }

struct Knobs {
#define HOLO_KNOB_FIELD(field, env, kind, dflt, when, doc) knob_##kind##_t field;
  HOLO_KNOBS(HOLO_KNOB_FIELD)
#undef HOLO_KNOB_FIELD
  static Knobs from_env() {
    Knobs k;
#define HOLO_KNOB_READ(field, env, kind, dflt, when, doc) k.field = knob_##kind(getenv(env), dflt);
    HOLO_KNOBS(HOLO_KNOB_READ)
#undef HOLO_KNOB_READ
    return k;
  }
};

}  // namespace holo
