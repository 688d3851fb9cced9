// bwd_plan.h — the launch descriptions of the denoiser's backward kernels (WgradParams, GnBwdParams) and the sizing rules their
// launchers (kernels_bwd.hip) share with the training planner (unet_train_plan.cpp): which weight-gradient kernel a shape
// takes, into how many slabs its rows are split, how large every scratch is.  Host-only arithmetic, no HIP header: ONE
// definition of each rule, reachable from a plain C++ program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "holo_knobs.h"

namespace holo {

struct WgradParams {   // dW[co][ci][tap] = sum_m gy[m][co] act(coef . x)[m + tap][ci]; geometry as ConvParams
  const float* gy;     // [M_out][Cout]
  const float* src0;
  const float* src1;   // virtual concat (may be null); C0 % 32 == 0 then
  int C0, C1;
  int N, ID, IH, IW, ups, OD, OH, OW, stride, pad, ksz, ntaps;
  int Cout;
  const float* coef;   // [N][Cin][2] or null
  int act;
  float* partial;      // [splits][Cout][Cin][ntaps] scratch (wgrad_partial_bytes)
};
struct WgradPlan {  // what wgrad_plan chose for a WgradParams: the scratch is sized and the launch shaped from the same value
  int rows;         // 1: the row-staged kernel (conv_wgrad_rows_kernel), 0: the tile kernel
  int splits;       // slabs of rows, one partial each
  int reduce_tile;  // row-staged kernel: the tile form of the reduce
};
constexpr int WR_MAXW = 64;  // the longest row the row-staged kernel stages (its LDS: kernels_bwd.hip)
// the row-staged kernel serves the stride-1 3x3x3 convolutions of rows up to 64 voxels (HOLO_WGRAD_TILES=1: tile kernel)
inline bool wgrad_rows_ok(const WgradParams& p, const Knobs& k) {
  if (k.wgrad_tiles > 0) return false;
  const int Cin = p.C0 + p.C1;
  return p.ksz == 3 && p.stride == 1 && p.pad == 1 && p.OW <= WR_MAXW && (p.OW & 1) == 0 && p.ID == p.OD && p.IH == p.OH &&
         p.IW == p.OW && (Cin & 3) == 0 && (p.Cout & 3) == 0 && (p.C0 & 3) == 0 && (p.C1 & 3) == 0 && (!p.src1 || (p.C0 & 31) == 0);
}
inline WgradPlan wgrad_plan(const WgradParams& p, int num_cus, const Knobs& k) {
  const int Cin = p.C0 + p.C1;
  const int64_t nrows = (int64_t)p.N * p.OD * p.OH;
  const int ncu = num_cus > 0 ? num_cus : 256;
  WgradPlan g;
  g.rows = wgrad_rows_ok(p, k) ? 1 : 0;
  // row-staged kernel: the tile form of the reduce from HOLO_WGRAD_REDUCE_TILE_MIN 64-element tiles on (development / test knob)
  g.reduce_tile = g.rows && ((int64_t)p.Cout * Cin + 63) / 64 >= k.wgrad_reduce_tile_min && p.ntaps <= 28;
  int64_t s;
  if (g.rows) {  // workgroups per CU by LDS / registers (1 or 2); slabs of at least 8 rows keep the row ring useful
    const int64_t pairs = (int64_t)((p.Cout + 31) / 32) * ((Cin + 31) / 32);
    s = ((p.OW > 32 ? 1 : 2) * (int64_t)ncu + pairs - 1) / pairs;
    if (s > nrows / 8) s = nrows / 8;
  } else {
    const int64_t tiles = (int64_t)((p.Cout + 31) / 32) * ((Cin + 31) / 32) * p.ntaps;
    s = (8LL * ncu + tiles - 1) / tiles;  // ~8 workgroups per CU in flight over the launch
    if (s > nrows / 4) s = nrows / 4;
  }
  if (s < 1) s = 1;
  if (s > 64) s = 64;
  g.splits = (int)s;
  return g;
}
inline size_t wgrad_partial_bytes(const WgradParams& p, const WgradPlan& g) {
  return (size_t)g.splits * p.Cout * (p.C0 + p.C1) * p.ntaps * sizeof(float);
}

inline size_t colsum_scratch_bytes(int C) { return (size_t)256 * C * sizeof(double); }

struct GnBwdParams {   // GroupNorm32 (+ FiLM) (+ SiLU) backward over the virtual concat [x0 | x1]
  const float* x0;
  const float* x1;
  int C0, C1, N;
  int64_t V;
  const float* ga;     // [N][V][C0 + C1] gradient w.r.t. the activated tensor
  const float* coef;   // forward (a, b)
  const float* mom;    // forward (mean, rstd) per channel
  const float* gamma;
  const float* beta;
  const float* film;   // [N][film_stride]: scale at +c, shift at +film_cout + c (null: no FiLM)
  int film_stride, film_cout;
  int act;
  double* part;        // scratch (gn_bwd_scratch_bytes)
  float* grp;          // scratch [N][Cin][2]
  float* dgamma;
  float* dbeta;
  float* dfilm;        // [N][film_stride] gradient of the FiLM rows (null without FiLM)
  int acc_params;
  float* gx0;          // gradient w.r.t. x0 / x1 (raw tensors)
  float* gx1;
  int acc0, acc1;      // accumulate into gx0 / gx1 instead of overwriting
};
inline int gn_bwd_blocks(int64_t V) {
  int64_t b = V / 64;
  if (b > 512) b = 512;
  if (b < 1) b = 1;
  return (int)b;
}
inline size_t gn_bwd_scratch_bytes(const GnBwdParams& p) {
  return (size_t)gn_bwd_blocks(p.V) * p.N * (p.C0 + p.C1) * 2 * sizeof(double);
}

}  // namespace holo
