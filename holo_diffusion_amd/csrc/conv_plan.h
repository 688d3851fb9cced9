// conv_plan.h — the forward convolution's launch description (ConvParams), the kernels it can run on (ConvKernel) and the
// planner that picks one: which kernel, its tile depth, split-K and grid (definitions in conv_plan.cpp).  Host-only
// arithmetic: no HIP header, so the planner is swept on the CPU (tests/cpu/conv_plan_check.cpp).  conv_launch
// (kernels_conv.hip) runs what conv_plan chose and trusts conv_can_launch for everything a kernel needs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "holo_knobs.h"

namespace holo {

// the tile extents the planner shares with the kernels (kernels_conv.hip, kernels_conv1x1_bf16.hip)
namespace conv_tile {
constexpr int BM = 128;      // output voxels per workgroup of the gather and halo kernels
constexpr int BK = 32;       // input channels per K chunk
constexpr int SM_ROWS = 64;  // output voxels per workgroup of the row-tile kernel
constexpr int SG = 8;        // ... and the K chunks of one of its staging groups
constexpr int Q1_MAXK = 16;  // bf16 1x1x1 streaming kernels: k-steps of 16 input channels (Cin <= 256)
constexpr int Q1_MAXSB = 12;  // ... and 32-channel slices per workgroup (48 KB of weights at 64 input channels)
}  // namespace conv_tile

// ---------------------------------------------------------------------------------------------
// conv3d as implicit GEMM on fp32 MFMA (kernels_conv.hip).
//   out[m][co] = bias[co] + residual[m][co] + sum_{tap,ci} W[tap][co][ci] * in'(m, tap, ci)
// with m = ((n*OD+od)*OH+oh)*OW+ow over channels-last (NDHWC) activations.
// in' = optional per-(n,channel) affine (GroupNorm folded with FiLM) + optional SiLU, applied while
// the tile is staged, zero padding applied AFTER the activation; optional nearest x2 upsample on load;
// optional virtual channel concat of two sources (UNet skip connection, unet.py:829).
// ---------------------------------------------------------------------------------------------
// The kernel conv_plan chose for a launch.  The values are the HoloOpTiming.kernel ids of holo_unet_time_ops
// (include/holo_abi.h); id 3, the retired depth-only Winograd form, is not used.
enum class ConvKernel : int32_t {
  Gather = 0,          // per-tap gather kernel (conv_igemm_kernel)
  Halo = 1,            // LDS voxel-halo kernel (conv_halo_kernel; conv_halo_split_kernel in the bf16x3 mode)
  RowTile = 2,         // row-tile kernel (conv_small_kernel): 1x1x1, strided and deepest-level convolutions
  Wino2 = 4,           // (z,y) Winograd form of the 128-voxel halo kernel (conv_wino2_kernel)
  Bf16Wide = 5,        // bf16 wide-tile kernel (conv_bf16t_kernel)
  Wino3 = 6,           // F(2x2x2, 3x3x3) Winograd form (conv_wino3_kernel, kernels_conv3.hip)
  Stream1x1 = 7,       // streaming 1x1x1 kernel (conv1x1_stream_kernel): large grids, raw input
  Bf16Persistent = 8,  // the wide-tile kernel's persistent wave-specialised form (conv_bf16p_kernel, kernels_conv_bf16p.hip)
  S2Bf16 = 9,          // stride-2 bf16 halo kernel (conv_s2_bf16_kernel, kernels_conv_s2.hip)
  Qkv = 10,            // qkv convolution fused with the attention's operand packing (conv1x1_qkv_bf16_kernel)
  Bf16Stream1x1 = 11,  // streaming 1x1x1 convolution on bf16 storage (conv1x1_bf16_stream_kernel)
  Small1x1 = 12,       // exact-fp32 1x1x1 convolution of a small grid, K split over the waves (conv1x1_small_kernel)
};

struct ConvParams {
  const float* src0;
  const float* src1;  // may be null
  int C0, C1;         // channels of src0 / src1; C0 % 32 == 0 when src1 != null; (C0+C1) % 4 == 0
  int N, ID, IH, IW;  // logical input dims (AFTER upsampling when ups=1)
  int ups;            // 1: sources have dims ID/2 x IH/2 x IW/2 and are read at (z>>1,y>>1,x>>1)
  int OD, OH, OW;
  int stride, pad, ksz;  // ksz = 3 (27 taps) or 1
  int Cout;
  const float* w;         // packed [ksz^3][CinP/32][CoutP/16][2][4][16][4] (repack_conv_weight_launch), zero padded to the
                          // CoutP / CinP of conv_weight_layout (conv_weights.h: the one place that rounds them)
  int CoutP, CinP;
  const float* coef;      // [N][Cin][2] = (a,b): x' = a*x+b ; null = identity
  int act;                // 1: SiLU after the affine (only with coef)
  const float* bias;      // [Cout] or null
  const float* residual;  // [M][Cout] or null
  float* out;             // [M][Cout]
  // optional fused 1x1x1 skip connection (halo kernel only): out += skip_w . [skip_src0 | skip_src1] + skip_bias
  const float* skip_src0;
  const float* skip_src1;
  int skip_C0, skip_C1;
  const float* skip_w;    // packed like w with one tap
  // bf16-multiply variant of the halo kernel (opt-in, holo_unet_set_compute_dtype): the same weights rounded to
  // bf16 (RNE), packed [ksz^3][CinP/32][CoutP/16][lane 64][8 bf16] = one 1 KB block of B operands of
  // v_mfma_f32_16x16x32_bf16 per (tap, chunk, 16-Cout slice).  Used when bf16 != 0 and the launch is on the halo path.
  // The buffer holds THREE such planes (hi, mid, lo: w = hi + mid + lo exactly); bf16 == 1 uses plane 0 only,
  // bf16 == 2 the fp32-accurate bf16x3 kernel (conv_halo_split_kernel) all three.
  const uint16_t* w_bf;
  const uint16_t* skip_w_bf;
  int bf16;
  int skip_CinP;
  const float* skip_bias;
  double* stats;          // optional: GroupNorm partial sums of `out`, [N][conv_stats_slabs(p)][Cout][2]
  float* partial;         // [nsplit][M][Cout] scratch when nsplit > 1
  int nsplit;             // split-K factor over (tap, cin-chunk) chunks
  int chunks_per_split;
  int skip_chunks_per_split;  // halo kernel with a fused skip: skip chunks are dealt evenly to the same splits
  int tz;                 // halo forms: tile depth (set by conv_plan; left 0 for the other kernels)
  int grid_x;             // halo kernel: persistent workgroups along x (set by conv_plan)
  int stagger_ticks;      // halo kernel: phase offset (100 MHz ticks) of the workgroup in the odd slot of a CU
  unsigned long long* dbg;  // optional timeline probe (scripts/conv_timeline.cpp): [tile][8] {t_start, t_first_halo,
                            // t_loops_done, t_end (100 MHz wall clock), HW_ID, XCC_ID, 0, 0}; null in production
  ConvKernel kernel;      // set by conv_plan
  // (z,y) Winograd form (conv_wino2_kernel): U = sum_kz,ky G[xi_z][kz] G[xi_y][ky] w[kz][ky][kx], 48 pseudo-taps
  // (xi_z*4 + xi_y)*3 + kx; the fused skip as 4 pseudo-taps (xi_z,xi_y in {1,2}^2: +-w/4).  Null = not prepared for this
  // conv (the direct kernel runs).
  const float* w_wino2;
  const float* skip_w_wino2;
  // F(2x2x2, 3x3x3) form (conv_wino3_kernel, kernels_conv3.hip): the 64 pseudo-taps in the wave's consumption order
  // (repack_conv_weight_wino3_launch); the fused skip as 8 signed copies of the 1x1x1 weight
  const float* w_wino3;
  const float* skip_w_wino3;
  // set by conv_plan: the launch runs that kernel's upsampling form (conv_wino3_up_kernel: ups, raw input, no fused skip -
  // the 27 pseudo-taps whose A operands are not identically zero; same results, 27/64 of the MFMAs)
  int wino3_up;
  // bf16 wide-tile kernel (conv_bf16t_kernel, 8x8x8 output tiles, v_mfma_f32_32x32x16_bf16): plane 3 of the bf16
  // weight buffer, packed [ksz^3][CinP/16][CoutP/32][lane 64][8 bf16] = one 1 KB block of B operands per
  // (tap, 16-channel chunk, 32-Cout slice); lane's 8 values are channels 8*(lane>>5) .. +7 of output channel lane&31
  const uint16_t* w_bft;
  const uint16_t* skip_w_bft;
  // bf16 STORAGE (compute mode bf16): the buffers behind these float* are bf16 (uint16_t) channels-last tensors;
  // coefficients, bias, statistics and split-K scratch stay fp32 / double
  int in_bf16;            // src0 / src1 / skip_src0 / skip_src1
  int res_bf16;           // residual
  int out_bf16;           // out
  // the qkv convolution of an AttentionBlock fused with the operand packing of the bf16 attention (kernels_conv1x1_bf16.hip;
  // set by the planner when the launch may take that form, conv_plan decides: ConvKernel::Qkv): `out` is then NOT written
  uint16_t* qkv_q;        // bf16 [sample, head][T][CH], scaled by qkv_scale
  uint16_t* qkv_k;        // bf16 [sample, head][T][CH]
  uint16_t* qkv_vt;       // bf16 [sample, head][CH][T]
  float qkv_scale;        // CH^-1/2 * log2 e
  int qkv_T, qkv_CH, qkv_H;
  int qkv_sb, qkv_rows;   // set by conv_plan: 32-channel slices / rows per workgroup
};

// which form of the halo kernel a launch on ConvKernel::Halo takes (the planner's slab rule and conv_launch's instantiation):
// the fp32-accurate bf16x3 kernel (conv_halo_split_kernel), else the bf16-product or the fp32 form of conv_halo_kernel
inline bool conv_halo_bf16x3(const ConvParams& p) { return p.bf16 == 2 && p.w_bf && p.Cout >= 64 && !p.skip_w; }
inline bool conv_halo_bf16(const ConvParams& p) { return p.bf16 == 1 && p.w_bf && (!p.skip_w || p.skip_w_bf); }

// Picks split-K so that the grid fills the chip; returns bytes of `partial` scratch needed (0 if none).
// plan_n > 0: every choice (kernel, tile depth, split-K) is made as for a launch of plan_n samples, and only the grid and the
// scratch are sized for p.N - with plan_n = 1 each sample of a batch is computed as at batch 1 (the batch-invariant plan of
// holo_unet_set_batch_invariant).  0: choices for p.N.  `k`: the caller's snapshot of the knobs (holo_knobs.h).
size_t conv_plan(ConvParams& p, int num_cus, const Knobs& k, int plan_n = 0);
// Capability: `kernel` (and the instantiation its launcher would pick) computes the launch `p` correctly - operand kinds,
// divisibility, the template instantiations that exist, every addressing limit.  No policy, no knob, no CU count.
bool conv_can_run(ConvKernel kernel, const ConvParams& p);
// ... and what conv_plan set fits p.kernel (split-K, tile depth, grid).  conv_launch refuses exactly what this refuses; conv_plan
// never produces it.
bool conv_can_launch(const ConvParams& p);
const char* conv_kernel_name(ConvKernel k);
int conv_stats_slabs(const ConvParams& p);
double conv_flops(const ConvParams& p);       // algorithmic (the reference's multiply-adds x 2)
double conv_exec_flops(const ConvParams& p);  // issued to the matrix pipe (differs for the Winograd kernels)

// GroupNorm statistics (gn_stats_kernel, splitk_reduce_kernel): the slab count B(C, V) the buffers must be sized for
void gn_stats_geometry(int C, int64_t V, int* n_blocks, int* vox_per_block);

}  // namespace holo
