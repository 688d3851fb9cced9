// render_plan.h — where a launch of the fused renderer is decided: the kernel family and instantiation, waves per workgroup,
// the workgroup cap, the tile hand-out, the workspace layout of holo_render and the list of launches of a call.  Host-only
// arithmetic on plain values: no HIP header, so the planner is swept on the CPU (tests/cpu/render_plan_check.cpp).
// render_exec.cpp plans, sizes and binds from a RenderPlan; render_launch (kernels_render.hip) switches on its fields and
// trusts render_can_launch for everything an instantiation needs.  The two constexpr wave rules below are the ones the
// kernels' __launch_bounds__ and slot index (blockIdx.x * NW + wave) are compiled with.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "holo_knobs.h"

namespace holo {

constexpr int RENDER_HD = 256;       // RenderMLP.dnet_hidden_dim the kernels are built for
constexpr int RENDER_MAXC = 64;      // most coarse samples per ray (cdf rows in LDS, rows of a scratch slot)
constexpr int RENDER_MAX_CAMS = 32;  // cameras the launch parameters hold (RenderKernelParams::MAX_CAMS)
// scratch slot of one resident wave of the ray-per-column kernel: (sigma, r, g, b) of 64 coarse samples x 32 rays
constexpr size_t RENDER_SLOT_BYTES = (size_t)RENDER_MAXC * 32 * 4 * sizeof(float);

// ---- waves per workgroup (= per CU).  CH = feature_size / 2 ------------------------------------------------------------
// render_kernel (ray per column): 12 (3 per SIMD, 168 VGPRs) for the released configurations; the normals variant and
// 64-feature grids need more registers per wave (2 per SIMD, 256 VGPRs); 128 new samples per ray need twice the LDS rows
constexpr int render_waves(int ch, int zcap, bool nrm) {
  return (ch <= 16 && !nrm) ? (zcap <= 64 ? 12 : 6) : (zcap <= 64 ? 8 : 4);
}
// render2_kernel ((ray, depth)-tiled): the per-wave rows are 9.4 KB (64 new samples per ray) / 14.6 KB (128), + 2 KB with
// normals; with the 40 KB RenderMLP image of 32 grid features 12 / 8 waves fit (64 grid features: 73 KB image, 8 / 4 waves)
// NRM: built for <= 32 grid features and <= 64 new samples per ray (the BASELINE / released configurations; anything else
// renders its normals on the ray-per-column kernel, render_instance_exists).  10 waves per CU (what the LDS holds): with the
// per-corner scalars read from the density scalar field the evaluation fits the 168 registers of three waves per SIMD
// (84 bytes of scratch outside the MFMA loops; with the scalars formed per sample it was 580 bytes and 25 M rays/s).
// Measured at 400^2, 8 frames: 40.2 M rays/s on 10 waves, 39.0 M on 8 (HOLO_RENDER2_NRM_NW=8, the emulation's choice)
constexpr int render2_waves(int ch, int zf, bool nrm = false) {
  return nrm ? 10 : (zf <= 64 ? (ch <= 16 ? 12 : 8) : (ch <= 16 ? 8 : 4));
}

enum class RenderFamily : int32_t {
  RayPerColumn = 0,  // render_kernel<CH, SP, NRM, ZCAP>: 32 rays per wave tile, one scratch slot per resident wave
  Tiled = 1,         // render2_kernel<CH, ZF, TRAIN, NW, NRM>: 4 rays per wave tile, everything per ray in LDS
};

// the shape of a call, as the entries see it
struct RenderShape {
  int feature_size, n_coarse, n_fine;
  bool normals;  // rendered normals wanted
  bool split3;   // the bf16x3 split arithmetic is ACTIVE (asked for, and 32 features)
  bool train;    // training mode (holo_render_rays): a list of rays per camera
  int resol;
  int hidden;    // dnet_hidden_dim
};

struct RenderRegion {
  size_t off, bytes;
  size_t end() const { return off + bytes; }
};
// the workspace of holo_render, in this order; `pad` closes it and total = pad.end()
struct RenderLayout {
  RenderRegion grid_cl;     // the caller's grid as channels-last voxels
  RenderRegion tile_ctr;    // tiled kernel, evaluation mode: the eight counters of the dynamic hand-out
  RenderRegion val_ws;      // ray-per-column kernel: one slot per resident wave
  RenderRegion nrm_ws;      // ... and the same again for the normals (see render_plan for the tiled kernel's 256 bytes)
  RenderRegion dens_field;  // S[v] = w_dens . F[v] of the tiled kernel's normals
  RenderRegion pad;
  size_t total;
};

struct RenderPlan {
  RenderFamily family;
  int ch;          // CH
  int z;           // ZCAP (ray per column) / ZF (tiled): 64 or 128 rows
  bool sp, nrm, train;
  int waves;       // per workgroup: the NW the instantiation is compiled with
  int rays_per_tile;
  int wg_cap;      // most workgroups of a launch: HOLO_RENDER_WGS, or one per CU
  int64_t slots;   // resident waves at the cap = scratch slots
  bool dynamic;    // tiles handed out through the counters (else: a static stride)
  int xcd;         // XCD ranges a full launch is split into (<= 1: plain order)
  int64_t tail;    // HOLO_RENDER_TAIL, or KNOB_UNSET: about two rounds of single-ray items per range (3 with emu)
  bool emu;
  int feature_size, n_coarse, n_fine, hidden;  // what render_can_launch checks the ranges of
  RenderLayout layout;
};

inline size_t render_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Which instantiations are compiled into the library (render_launch's switch, kernels_render.hip).
constexpr bool render_instance_exists(RenderFamily family, int ch, int z, bool sp, bool nrm, bool train) {
  if (!(ch == 8 || ch == 16 || ch == 32) || !(z == 64 || z == 128)) return false;
  if (family == RenderFamily::RayPerColumn) return !train && (!sp || ch == 16);
  // tiled: exact fp32 only; training mode returns no normals; normals for <= 32 features and <= 64 new samples
  return !sp && !(train && nrm) && (!nrm || (ch <= 16 && z == 64));
}

// Why render_launch would refuse this plan, or null: the ranges every kernel is written for, the instantiation, and the
// wave count it is compiled with.  No policy, no knob, no CU count.
inline const char* render_refusal(const RenderPlan& p) {
  if (p.hidden != RENDER_HD) return "render: dnet_hidden_dim must be 256";
  if (p.n_coarse < 3 || p.n_coarse > RENDER_MAXC || p.n_fine < 2 || p.n_fine > 128)
    return "render: n_pts_coarse must be in [3,64] and n_pts_fine in [2,128]";
  if (!(p.feature_size == 16 || p.feature_size == 32 || p.feature_size == 64) || p.ch * 2 != p.feature_size)
    return "render: the fused renderer is built for feature_size 16, 32 or 64 (128 input features are supported by the "
           "stand-alone implicit function only)";
  if (p.train && p.nrm) return "render: training-mode rendering returns no normals";
  if (p.z != (p.n_fine <= 64 ? 64 : 128)) return "render: the plan's row count does not hold n_pts_fine";
  if (!render_instance_exists(p.family, p.ch, p.z, p.sp, p.nrm, p.train))
    return p.nrm && p.family == RenderFamily::Tiled
               ? "render: rendered normals of more than 32 grid features or 64 new samples run on the ray-per-column kernel"
               : "render: no such instantiation";
  bool waves_ok;
  if (p.family == RenderFamily::RayPerColumn) waves_ok = p.waves == render_waves(p.ch, p.z, p.nrm);
  else if (p.nrm) waves_ok = p.waves == render2_waves(p.ch, p.z, true) || p.waves == 8;
  else waves_ok = p.waves == render2_waves(p.ch, p.z) || (p.waves == 8 && render2_waves(p.ch, p.z) == 12);
  if (!waves_ok || 64 * p.waves > 1024) return "render: the plan's waves per workgroup fit no instantiation";
  if (p.rays_per_tile != (p.family == RenderFamily::Tiled ? 4 : 32) || p.wg_cap < 1 || p.slots != (int64_t)p.wg_cap * p.waves)
    return "render: the plan's tile size or slot count does not fit its kernel";
  if (p.dynamic && (p.family != RenderFamily::Tiled || p.layout.tile_ctr.bytes < 8 * sizeof(int)))
    return "render: dynamic tile hand-out needs the tiled kernel and its counters";
  if (p.family == RenderFamily::RayPerColumn &&
      (p.layout.val_ws.bytes < (size_t)p.slots * RENDER_SLOT_BYTES || (p.nrm && p.layout.nrm_ws.bytes < (size_t)p.slots * RENDER_SLOT_BYTES)))
    return "render: the plan's scratch is smaller than its resident waves";
  return nullptr;
}
inline bool render_can_launch(const RenderPlan& p) { return render_refusal(p) == nullptr; }

// The plan of a renderer handle for one kind of call.  `k`: the handle's snapshot of the knobs; `emu`: the sizes of the
// TEST-ONLY emulation build (the library passes EMU_BUILD).
inline RenderPlan render_plan(const RenderShape& s, int num_cus, const Knobs& k, bool emu) {
  RenderPlan p = {};
  p.feature_size = s.feature_size, p.n_coarse = s.n_coarse, p.n_fine = s.n_fine, p.hidden = s.hidden;
  p.ch = s.feature_size / 2;
  p.z = s.n_fine <= 64 ? 64 : 128;
  p.nrm = s.normals, p.train = s.train, p.emu = emu;
  // the (ray, depth)-tiled kernel wherever it is built; the ray-per-column kernel for the bf16x3 split arithmetic, for the
  // normals the tiled kernel has no instantiation of (more than 32 features or 64 new samples) and - development knob
  // HOLO_RENDER_V1=1 - for everything in evaluation mode
  const bool tiled = s.train || (!s.split3 && !k.render_v1 &&
                                 (!s.normals || render_instance_exists(RenderFamily::Tiled, p.ch, p.z, false, true, false)));
  p.family = tiled ? RenderFamily::Tiled : RenderFamily::RayPerColumn;
  p.sp = !tiled && s.split3;
  p.rays_per_tile = tiled ? 4 : 32;
  if (!tiled) {
    p.waves = render_waves(p.ch, p.z, s.normals);
  } else if (s.normals) {
    // HOLO_RENDER2_NRM_NW=8: the two-waves-per-SIMD form (development knob; what the emulation build always runs)
    p.waves = (k.render2_nrm_nw == 8 || emu) ? 8 : render2_waves(p.ch, p.z, true);
  } else {
    // HOLO_RENDER2_NW=8: development knob, the 8-wave form of the 12-wave configurations
    p.waves = render2_waves(p.ch, p.z);
    if (k.render2_nw == 8 && p.waves == 12) p.waves = 8;
  }
  // The persistent kernels run ONE workgroup per CU; every wave of it is a worker.  The scratch therefore depends on the
  // chip and the configuration only - not on the number of cameras or the image size.
  p.wg_cap = k.render_wgs > 0 ? (int)k.render_wgs : num_cus > 0 ? num_cus : 256;
  p.slots = (int64_t)p.wg_cap * p.waves;
  p.dynamic = tiled && !s.train && !k.render_static_tiles;
  p.xcd = s.train ? 1 : k.render_xcd != KNOB_UNSET ? (int)k.render_xcd : emu ? 2 : 8;
  p.tail = k.render_tail;

  const size_t vox = (size_t)s.resol * s.resol * s.resol;
  const size_t slot_bytes = (size_t)p.slots * RENDER_SLOT_BYTES;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const RenderRegion r = {o, bytes};
    o += bytes;
    return r;
  };
  RenderLayout& L = p.layout;
  L.grid_cl = take(render_align256(vox * (size_t)s.feature_size * sizeof(float)));
  L.tile_ctr = take(tiled && !s.train ? 256 : 0);
  L.val_ws = take(tiled ? 0 : slot_bytes);
  // (with normals the tiled kernel's workspace has always carried a second 256 bytes that nothing reads: kept, the size
  // query answers what it answered)
  L.nrm_ws = take(!s.normals ? 0 : tiled ? 256 : slot_bytes);
  // (reserved whenever normals are wanted; read by the tiled kernel only)
  L.dens_field = take(s.normals ? render_align256(vox * sizeof(float)) : 0);
  L.pad = take(256);
  L.total = o;
  return p;
}

// One launch of a call: cameras [cam0, cam0 + n_cams), n_tiles wave tiles on n_wgs workgroups.
struct RenderLaunch {
  int cam0, n_cams;
  int64_t n_tiles;
  int n_wgs;
  int xcd;         // > 1: XCD-aware tile order
  bool dynamic;    // the counters are zeroed and handed to the kernel
  int tail_quads;  // dynamic only: the last 4-ray tiles of every XCD range that go out as single-ray items
};

// The launches of a call over n_cameras cameras of rays_per_cam rays each (pixels of a frame; the ray list's length in
// training mode).  The launch parameters hold RENDER_MAX_CAMS cameras.  Evaluation mode splits more cameras EVENLY over the
// launches (40 frames = 20 + 20, not 32 + 8: every launch then ends on an almost full round of wave tiles); training mode
// fills every launch but the last.
inline std::vector<RenderLaunch> render_launches(const RenderPlan& p, int n_cameras, int64_t rays_per_cam) {
  std::vector<RenderLaunch> out;
  const int n_launches = (n_cameras + RENDER_MAX_CAMS - 1) / RENDER_MAX_CAMS;
  const int G = p.train ? RENDER_MAX_CAMS : (n_cameras + n_launches - 1) / (n_launches > 0 ? n_launches : 1);
  for (int c0 = 0; c0 < n_cameras; c0 += G) {
    RenderLaunch l = {};
    l.cam0 = c0;
    l.n_cams = n_cameras - c0 < G ? n_cameras - c0 : G;
    l.n_tiles = (int64_t)l.n_cams * ((rays_per_cam + p.rays_per_tile - 1) / p.rays_per_tile);
    // no more workgroups than there is work for (a tiny launch must not stage the MLP on idle CUs)
    const int64_t want = (l.n_tiles + p.waves - 1) / p.waves;
    l.n_wgs = want > p.wg_cap ? p.wg_cap : (int)want;
    l.xcd = (p.xcd > 1 && l.n_wgs == p.wg_cap && l.n_wgs % p.xcd == 0) ? p.xcd : 1;
    l.dynamic = p.dynamic;
    if (l.dynamic) {
      // the end of every XCD range in single-ray items: about two rounds of them on the range's resident waves
      // (HOLO_RENDER_TAIL=<quads per range>: development knob, 0 = off; the emulation's tiny frames: a few tail tiles in
      // every test)
      l.tail_quads = p.tail != KNOB_UNSET ? (int)p.tail : p.emu ? 3 : (l.n_wgs * p.waves / l.xcd) / 2;
    }
    out.push_back(l);
  }
  return out;
}

}  // namespace holo
