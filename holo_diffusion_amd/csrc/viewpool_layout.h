// viewpool_layout.h — the workspaces of holo_view_pool and holo_view_pool_backward as values: one function from the call's
// shape to byte offsets and a total, shared by the size query and the run (viewpool_exec.cpp).  Host-only arithmetic, no HIP
// header: checked on the CPU together with the renderer's plan (tests/cpu/render_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/holo_abi.h"

namespace holo {

constexpr int VIEW_POOL_MAX_FEATS = 8;  // ViewPoolParams::MAX_FEATS

// Every region starts on a 256-byte boundary.  Order: the channels-last images of the source-view feature maps (channels
// padded to fours) | the transposed mapper weight (A, F) | and for the backward: the zeroed channels-last gradient maps |
// the per-workgroup partials of d weight / d bias | in the deterministic mode the 64-bit fixed-point images of the gradient
// maps and one word per map | pad.
struct ViewPoolLayout {
  size_t map[VIEW_POOL_MAX_FEATS], map_bytes[VIEW_POOL_MAX_FEATS];  // (bytes: unpadded, n_views x H x W x Cp floats)
  size_t wt;
  size_t gmap[VIEW_POOL_MAX_FEATS];
  size_t partial;
  int n_wgs;     // workgroups of the backward launch = rows of `partial`
  bool fixed;    // holo_ctx_set_deterministic
  size_t gfix[VIEW_POOL_MAX_FEATS], fix_max, fix_end;  // [gfix[0], fix_end) is zeroed before the launch
  size_t pad, total;
};

// backward = false: holo_view_pool (num_cus and deterministic are not used)
inline ViewPoolLayout view_pool_layout(const HoloViewPoolCfg& cfg, const HoloViewFeature* feats, int n_feats, int n_views,
                                       bool backward, int num_cus, bool deterministic) {
  ViewPoolLayout L = {};
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) & ~(size_t)255;
    return at;
  };
  // (the size queries answer for any number of maps; the run refuses more than VIEW_POOL_MAX_FEATS)
  auto maps = [&](size_t* off, size_t* bytes, size_t elem_bytes) {
    for (int k = 0; k < n_feats; ++k) {
      const size_t b = (size_t)n_views * feats[k].height * feats[k].width * ((feats[k].channels + 3) / 4 * 4) * elem_bytes;
      const size_t at = take(b);
      if (k < VIEW_POOL_MAX_FEATS) {
        off[k] = at;
        if (bytes) bytes[k] = b;
      }
    }
  };
  int sumC = 0;
  for (int k = 0; k < n_feats; ++k) sumC += feats[k].channels;
  const size_t F = (size_t)cfg.feature_size;
  maps(L.map, L.map_bytes, sizeof(float));
  L.wt = take((size_t)2 * sumC * F * sizeof(float));
  L.pad = 256;
  if (backward) {
    maps(L.gmap, nullptr, sizeof(float));
    const int64_t groups = ((int64_t)cfg.resol * cfg.resol * cfg.resol + 15) / 16;
    const int64_t n = 4 * (int64_t)num_cus;  // (view_pool_bwd2_kernel: four resident workgroups per CU)
    L.n_wgs = (int)(groups < n ? groups : n);
    L.partial = take((size_t)L.n_wgs * ((size_t)2 * sumC * F + F) * sizeof(float));
    L.fixed = deterministic;
    L.gfix[0] = L.fix_max = L.fix_end = o;
    if (deterministic) {
      maps(L.gfix, nullptr, sizeof(long long));
      L.fix_max = take(256);
      L.fix_end = o;
    }
    L.pad = 512;  // (the forward's pad and the backward's own: what the size query has always answered)
  }
  L.total = o + L.pad;
  return L;
}

}  // namespace holo
