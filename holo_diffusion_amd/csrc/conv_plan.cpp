// conv_plan.cpp — which of the twelve convolution kernels a launch runs on, and its geometry.
//
// Two kinds of condition, kept apart:
//   CAPABILITY  conv_<kernel>_can_run(p, d): everything the kernel and the instantiations its launcher has need to compute
//               the launch correctly.  Stated here ONCE: conv_plan asks it before it picks the kernel, conv_launch (through
//               conv_can_launch) before it launches, so the planner cannot pick what the launcher refuses.
//   POLICY      the chooser of conv_plan: where a kernel that can run is also WANTED (filling the chip, the knobs, num_cus).
// Plain C++: nothing of HIP, swept on the CPU by tests/cpu/conv_plan_check.cpp.
#include "conv_plan.h"

#include <stdio.h>

namespace holo {

using namespace conv_tile;

namespace {

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int64_t LIM24 = (int64_t)1 << 24, LIM31 = (int64_t)1 << 31, LIM32 = (int64_t)1 << 32;

// workgroups per CU the row-tile kernel's split-K aims at
constexpr int SM_SPLIT_WGS_PER_CU = 2;
// the bf16 wide-tile kernel also runs on under-filled levels (split over 16-channel chunks) once the K extent is long
// enough to pay for the partials - measured at 128^3: from 192 input channels (main + fused skip) it beats the 64/128-voxel
// halo kernel (32^3 .. 8^3 levels together 1.96 -> 1.7 ms), below that it loses
constexpr int BF16T_LONG_K = 192;
// workgroups per CU its split-K aims at: two on the 32^3 level and above, ONE below it and for raw-input launches
// (measured at 128^3, profiles/r06_bf16t_split_target.txt: the 16^3 / 8^3 launches 43.6 -> 39.0, 41.5 -> 36.4,
// 41.2 -> 35.9 us with half the partial sums to write and reduce; the 32^3 launches the other way round, 59.8 vs 66.4;
// the raw-input Upsample convolution at 32^3 un-split lands on the persistent form: 126.7 -> 91.5 us)
constexpr int BF16T_SPLIT_WGS_PER_CU_TOP = 2;
constexpr int BF16T_SPLIT_WGS_PER_CU = 1;

// what a launch's extents come to, computed once per ConvParams
struct ConvDims {
  int Cin, SCin;          // input channels of the convolution / of its fused skip (0 without one)
  int ncc, nsk;           // ... in 32-channel chunks
  int ncc16, nsk16;       // ... in the wide-tile kernels' 16-channel chunks
  int nchunks;            // (tap, 32-channel chunk) pairs
  int bn;                 // the Cout tile: 64 | 32 (conv_cout_tile)
  int64_t V, M, src_vox;  // output voxels per sample / of all samples, voxels of a source sample
  int cmax;               // the widest single source, the skip's included
  bool same_grid;         // stride 1: the input grid is the output grid
  bool halo;              // the launch has the 3x3x3 shape and the tiles of the halo forms
  explicit ConvDims(const ConvParams& p) {
    Cin = p.C0 + p.C1;
    SCin = p.skip_w ? p.skip_C0 + p.skip_C1 : 0;
    ncc = (int)cdiv(Cin, BK), nsk = (int)cdiv(SCin, BK);
    ncc16 = (int)cdiv(Cin, 16), nsk16 = (int)cdiv(SCin, 16);
    nchunks = p.ksz * p.ksz * p.ksz * ncc;
    bn = p.Cout >= 64 ? 64 : 32;
    V = (int64_t)p.OD * p.OH * p.OW, M = p.N * V, src_vox = (int64_t)p.ID * p.IH * p.IW;
    const int c = p.C0 > p.C1 ? p.C0 : p.C1, s = p.skip_C0 > p.skip_C1 ? p.skip_C0 : p.skip_C1;
    cmax = c > s ? c : s;
    same_grid = p.ID == p.OD && p.IH == p.OH && p.IW == p.OW;
    // the halo kernels address a source sample, and the wide-tile epilogue an output sample, with 32-bit byte offsets
    const bool fits32 = src_vox * cmax * 4 < LIM32 && V * p.Cout * 4 < LIM32;
    halo = p.ksz == 3 && p.stride == 1 && p.pad == 1 && (p.OD % 2) == 0 && (p.OH % 8) == 0 && (p.OW % 8) == 0 &&  // (TZ=1 tiles need no z divisibility)
           same_grid && (Cin % 16) == 0 && fits32;
  }
};

// ---- capability: one predicate per kernel (in the order of the chooser)

// every kernel: float4 channel quads, and a concat seam on a K chunk boundary
bool conv_channels_ok(const ConvParams& p, const ConvDims& d) {
  return (d.Cin & 3) == 0 && (p.C0 & 3) == 0 && (p.Cout & 3) == 0 && (!p.src1 || (p.C0 % BK) == 0);
}

// the bf16 1x1x1 streaming kernels (kernels_conv1x1_bf16.hip): NK = Cin / 16 in {4, 8, 12, 16} are instantiated; GroupNorm's
// affine is applied on load, an activation is not
bool q1_operands_ok(const ConvParams& p, const ConvDims& d) {
  return p.ksz == 1 && p.stride == 1 && !p.ups && p.bf16 == 1 && p.in_bf16 && p.w_bft && !p.skip_w && !p.act && p.C1 == 0 &&
         (d.Cin % 64) == 0 && d.Cin >= 64 && d.Cin <= 16 * Q1_MAXK && (p.Cout % 32) == 0 && p.Cout == p.CoutP;
}
// the 32-channel slices a workgroup takes (its weights <= 48 KB of LDS); 0 = the launch is not for these kernels
int q1_slices_per_block(const ConvParams& p, const ConvDims& d) {
  int sb = 49152 / (d.Cin * 64);
  const int nsl = p.Cout / 32;
  while (sb > 1 && nsl % sb) --sb;
  return sb < 1 ? 0 : sb;
}
// conv1x1_qkv_bf16_kernel: the qkv convolution of an AttentionBlock (bf16 storage) writing the packed operands of
// flash_attn_bf16v2_kernel (ConvParams::qkv_*) instead of fp32 qkv
bool conv_qkv_can_run(const ConvParams& p, const ConvDims& d) {
  return p.qkv_q && q1_operands_ok(p, d) && !p.residual && !p.stats && p.qkv_CH % 32 == 0 && p.Cout == 3 * p.qkv_CH * p.qkv_H &&
         p.qkv_T % 128 == 0 && d.M == (int64_t)p.N * p.qkv_T && q1_slices_per_block(p, d) > 0;
}
// conv1x1_bf16_stream_kernel: the same streaming GEMM with a plain [M][Cout] bf16 output (+ bias, + residual, GroupNorm
// slabs: one per workgroup row block)
bool conv_bf16_stream1x1_can_run(const ConvParams& p, const ConvDims& d) {
  return !p.qkv_q && q1_operands_ok(p, d) && p.out_bf16 && (!p.residual || p.res_bf16) && d.same_grid && d.V >= 4096 &&
         (d.V % 128) == 0 && d.V < LIM31 && q1_slices_per_block(p, d) > 0 && q1_slices_per_block(p, d) <= Q1_MAXSB;
}
// conv1x1_stream_kernel: a raw-input exact-fp32 1x1x1 convolution, every wave walks 16-row tiles; NCH = Cin / 32 in 1..8;
// no statistics
bool conv_stream1x1_can_run(const ConvParams& p, const ConvDims& d) {
  return p.ksz == 1 && p.stride == 1 && !p.ups && !p.coef && !p.residual && !p.skip_w && !p.stats && p.bf16 == 0 && !p.in_bf16 &&
         !p.out_bf16 && (p.Cout % 64) == 0 && (d.Cin % 32) == 0 && d.Cin >= 32 && d.Cin <= 256 && (d.M % 16) == 0 && d.same_grid;
}
// conv1x1_small_kernel: an exact-fp32 1x1x1 convolution of a small grid (16 .. 4096 voxels per sample, 32 .. 256 input
// channels in 32-channel chunks: NCH = Cin / 32 in 1..8, 64-channel output blocks, one source) whose input is normalised
// without an activation (an AttentionBlock's qkv) or that adds a residual (its proj_out).  Raw-input 1x1x1 convolutions
// (ResBlock skips) keep their kernels.
bool conv_small1x1_can_run(const ConvParams& p, const ConvDims& d) {
  return p.ksz == 1 && p.stride == 1 && p.pad == 0 && !p.ups && p.bf16 == 0 && !p.in_bf16 && !p.out_bf16 && !p.res_bf16 &&
         !p.skip_w && !p.src1 && p.C1 == 0 && !p.qkv_q && ((p.coef && !p.act) || p.residual) && (d.Cin % 32) == 0 &&
         d.Cin >= 32 && d.Cin <= 256 && p.CinP == d.Cin && (p.Cout % 64) == 0 && p.CoutP == p.Cout && d.same_grid &&
         (d.V % 16) == 0 && d.V <= 4096 && p.N * d.V * (d.Cin > p.Cout ? d.Cin : p.Cout) < LIM31;
}
// conv_s2_bf16_kernel: the stride-2 3x3x3 convolution of a Downsample block on bf16 activation storage (raw input, 2 x 8 x 8
// output tiles x 64 output channels)
bool conv_s2_bf16_can_run(const ConvParams& p, const ConvDims& d) {
  return p.ksz == 3 && p.stride == 2 && p.pad == 1 && !p.ups && p.bf16 == 1 && p.in_bf16 && p.out_bf16 && p.w_bft && !p.coef &&
         !p.residual && !p.skip_w && p.C1 == 0 && (d.Cin % 16) == 0 && (p.Cout % 64) == 0 && p.ID == 2 * p.OD && p.IH == 2 * p.OH &&
         p.IW == 2 * p.OW && (p.OD % 2) == 0 && (p.OH % 8) == 0 && (p.OW % 8) == 0 && d.src_vox * d.Cin < LIM31;
}
// conv_bf16t_kernel (8^3 voxels x 64 | 32 output channels per workgroup) on bf16 storage; a fused skip only in its 64-wide form
bool conv_bf16_wide_can_run(const ConvParams& p, const ConvDims& d) {
  return d.halo && p.bf16 == 1 && p.in_bf16 && (!p.residual || p.res_bf16) && p.w_bft && (!p.skip_w || p.skip_w_bft) &&
         (p.OD % 8) == 0 && (p.OH % 8) == 0 && (p.OW % 8) == 0 && (p.Cout % 32) == 0 && (p.C0 % 8) == 0 && (p.skip_C0 % 8) == 0 &&
         ((p.skip_C0 + p.skip_C1) % 8) == 0 && (p.Cout >= 64 || !p.skip_w);
}
// conv_bf16p_kernel, its persistent wave-specialised form
bool conv_bf16_persistent_can_run(const ConvParams& p, const ConvDims& d) {
  return conv_bf16_wide_can_run(p, d) && (p.C1 == 0 || (p.C0 % 16) == 0) &&  // (a 16-channel chunk / a 32-channel skip step lies in ONE source)
         (!p.skip_w || ((d.SCin % 32) == 0 && (p.skip_C1 == 0 || (p.skip_C0 % 32) == 0))) &&
         d.src_vox < LIM24;  // (24-bit voxel indices in the producers' address arithmetic)
}
// conv_wino3_kernel, the F(2x2x2, 3x3x3) form (kernels_conv3.hip): exact fp32 on fp32 storage, 64-channel output blocks, its
// staging applies the affine and SiLU together, buffer addressing of whole source tensors.  (What its epilogue addresses
// depends on the split: wino3_split_fits.)
bool conv_wino3_can_run(const ConvParams& p, const ConvDims& d) {
  return d.halo && p.w_wino3 && p.bf16 == 0 && !p.in_bf16 && !p.out_bf16 && p.Cout >= 64 && (p.Cout % 64) == 0 &&
         (!p.skip_w || (p.skip_w_wino3 && (p.skip_C0 % 16) == 0 && (p.skip_C1 % 4) == 0)) && (!p.coef || p.act) &&
         p.N * d.src_vox * d.cmax * 4 < LIM32;
}
// ... out / residual and every split's partial sums lie within 4 GB of their base (the statistics records, an eighth of the
// output's bytes, then do too)
bool wino3_split_fits(const ConvParams& p, const ConvDims& d, int nsplit) { return nsplit * d.M * p.Cout * 4 < LIM32; }
// conv_wino2_kernel, the (z,y) Winograd form of the 128-voxel halo tile: exact fp32 on fp32 storage, where its weights were
// prepared; 64-channel output blocks, or (without a fused skip) exactly 32 output channels: two wave rows
bool conv_wino2_can_run(const ConvParams& p, const ConvDims& d) {
  return d.halo && p.w_wino2 && p.bf16 == 0 && !p.in_bf16 && !p.out_bf16 && !(p.residual && p.res_bf16) &&
         (p.Cout >= 64 ? (p.Cout % 64) == 0 && (!p.skip_w || p.skip_w_wino2) : p.Cout == 32 && !p.skip_w);
}
// conv_halo_kernel: its bf16-product form (conv_halo_bf16) goes with bf16 storage, its fp32 form with fp32 storage; a fused
// skip only with 64-wide output tiles.  conv_halo_split_kernel (conv_halo_bf16x3): fp32 storage.
bool conv_halo_can_run(const ConvParams& p, const ConvDims& d) {
  if (!d.halo) return false;
  if (conv_halo_bf16x3(p)) return !p.in_bf16 && !p.out_bf16 && !(p.residual && p.res_bf16);
  const bool bf = conv_halo_bf16(p);
  return (p.in_bf16 != 0) == bf && (!p.residual || (p.res_bf16 != 0) == bf) && (p.Cout >= 64 || !p.skip_w);
}
// conv_small_kernel: 64 rows x 64 output channels (the weights are padded to the 64-wide tile from 64 output channels on), 32-bit
// output voxel indices; a fused skip's chunks follow the (tap, chunk) list: at stride 1 without upsampling only
bool conv_row_tile_can_run(const ConvParams& p, const ConvDims& d) {
  return p.Cout >= 64 && d.M < LIM31 &&
         (!p.skip_w || (p.stride == 1 && !p.ups && p.ID == p.OD && !(p.bf16 == 1 && p.w_bf && !p.skip_w_bf)));
}
// conv_igemm_kernel: any shape, no fused skip
bool conv_gather_can_run(const ConvParams& p, const ConvDims&) { return !p.skip_w; }

bool can_run(ConvKernel kernel, const ConvParams& p, const ConvDims& d) {
  switch (kernel) {
    case ConvKernel::Qkv: return conv_qkv_can_run(p, d);
    case ConvKernel::Bf16Stream1x1: return conv_bf16_stream1x1_can_run(p, d);
    case ConvKernel::Stream1x1: return conv_stream1x1_can_run(p, d);
    case ConvKernel::Small1x1: return conv_small1x1_can_run(p, d);
    case ConvKernel::S2Bf16: return conv_s2_bf16_can_run(p, d);
    case ConvKernel::Bf16Persistent: return conv_bf16_persistent_can_run(p, d);
    case ConvKernel::Bf16Wide: return conv_bf16_wide_can_run(p, d);
    case ConvKernel::Wino3: return conv_wino3_can_run(p, d);
    case ConvKernel::Wino2: return conv_wino2_can_run(p, d);
    case ConvKernel::Halo: return conv_halo_can_run(p, d);
    case ConvKernel::RowTile: return conv_row_tile_can_run(p, d);
    case ConvKernel::Gather: return conv_gather_can_run(p, d);
  }
  return false;
}

// ---- split-K

struct KSplit {
  int n, cps;  // splits, chunks per split
};
// split-K over `chunks` chunks: `want` splits, at most `max_split` (<= chunks), the chunks dealt evenly (the last split
// may get fewer)
KSplit ksplit(int64_t want, int max_split, int chunks) {
  const int cps = (int)cdiv(chunks, want < max_split ? want : max_split);
  return {(int)cdiv(chunks, cps), cps};
}

// what the chooser weighs: the work items each tiling makes of the rows the choices are made for (plan_n samples; M, all
// samples, sizes the grids and the scratch.  The capabilities stay on p.N: a batch past an addressing limit takes another
// kernel - the batch-invariant planner checks for that.)
struct ConvFill {
  int64_t Mc, tiles, t8, t3, target;
  ConvFill(const ConvParams& p, const ConvDims& d, int num_cus, int plan_n) {
    Mc = (plan_n > 0 ? plan_n : p.N) * d.V;
    tiles = cdiv(Mc, BM) * cdiv(p.Cout, d.bn);
    t8 = (Mc / 512) * cdiv(p.Cout, d.bn);  // wide-tile kernels: 8^3 tiles x Cout slices
    t3 = (Mc / 128) * (p.Cout / 64);       // F(2x2x2) form: 2 x 8 x 8 tiles x 64-Cout blocks
    target = 2 * (int64_t)num_cus;
  }
};

KSplit bf16t_split(const ConvParams& p, const ConvDims& d, const ConvFill& f, int num_cus) {
  const int64_t tgt = (int64_t)num_cus * (p.OD >= 32 && p.coef ? BF16T_SPLIT_WGS_PER_CU_TOP : BF16T_SPLIT_WGS_PER_CU);
  return ksplit(f.t8 < tgt ? cdiv(tgt, f.t8) : 1, d.ncc16, d.ncc16);
}

// F(2x2x2, 3x3x3) form: ONE persistent 4-wave workgroup per CU walks (tile, 64-Cout block, split) items, so the chip is
// full from num_cus items on; split-K only up to that
KSplit wino3_split(const ConvDims& d, const ConvFill& f, int num_cus) {
  return ksplit(f.t3 < num_cus ? cdiv(num_cus, f.t3) : 1, d.ncc, d.ncc);
}

// bf16 1x1x1 streaming kernels: 32-channel slices per workgroup, and its rows: a multiple of 128 that divides the sample, about
// two workgroups per CU.  (The plain form shares ConvParams::qkv_T / qkv_sb / qkv_rows with the fused qkv form.)
void q1_plan(ConvParams& p, const ConvDims& d, int num_cus) {
  if (p.kernel == ConvKernel::Bf16Stream1x1) p.qkv_T = (int)d.V;
  p.qkv_sb = q1_slices_per_block(p, d);
  const int nby = (p.Cout / 32) / p.qkv_sb;
  int rows = 128;
  while (rows * 2 <= p.qkv_T && (p.qkv_T % (rows * 2)) == 0 && ((int64_t)p.N * p.qkv_T / (rows * 2)) * nby >= 2 * (int64_t)num_cus) rows *= 2;
  p.qkv_rows = rows;
}

}  // namespace

bool conv_can_run(ConvKernel kernel, const ConvParams& p) {
  const ConvDims d(p);
  return conv_channels_ok(p, d) && can_run(kernel, p, d);
}

// The geometry each kernel reads: split-K only where the kernel can split (and then with its scratch), the grid and tile depth
// of the halo forms, the slices and rows of the bf16 1x1x1 streaming kernels.
bool conv_can_launch(const ConvParams& p) {
  const ConvDims d(p);
  if (!conv_channels_ok(p, d) || !can_run(p.kernel, p, d)) return false;
  if (p.nsplit < 1 || p.chunks_per_split < 1 || (p.nsplit > 1 && !p.partial)) return false;
  switch (p.kernel) {
    case ConvKernel::Gather:
    case ConvKernel::RowTile:
      return true;
    case ConvKernel::Halo:
      return p.grid_x >= 1 && (p.tz == 1 || p.tz == 2);
    case ConvKernel::Wino2:
      return p.grid_x >= 1 && p.tz == 2;
    case ConvKernel::Bf16Wide:
      return p.grid_x >= 1;
    case ConvKernel::Bf16Persistent:
      return p.grid_x >= 1 && p.nsplit == 1;
    case ConvKernel::Wino3:  // every split owns at least one chunk (the stage loop tests at its end); the upsampling form
                             // takes raw x2 input without a fused skip
      return p.grid_x >= 1 && p.tz == 2 && (int64_t)(p.nsplit - 1) * p.chunks_per_split < d.ncc && wino3_split_fits(p, d, p.nsplit) &&
             (!p.wino3_up || (p.ups && !p.coef && !p.skip_w));
    case ConvKernel::Qkv:
    case ConvKernel::Bf16Stream1x1:
      return p.nsplit == 1 && p.qkv_sb >= 1 && p.qkv_rows >= 128;
    case ConvKernel::Stream1x1:
    case ConvKernel::Small1x1:
    case ConvKernel::S2Bf16:
      return p.nsplit == 1;
  }
  return false;
}

const char* conv_kernel_name(ConvKernel k) {
  switch (k) {
    case ConvKernel::Gather: return "conv_igemm_kernel";
    case ConvKernel::Halo: return "conv_halo_kernel";
    case ConvKernel::RowTile: return "conv_small_kernel";
    case ConvKernel::Wino2: return "conv_wino2_kernel";
    case ConvKernel::Bf16Wide: return "conv_bf16t_kernel";
    case ConvKernel::Wino3: return "conv_wino3_kernel";
    case ConvKernel::Stream1x1: return "conv1x1_stream_kernel";
    case ConvKernel::Bf16Persistent: return "conv_bf16p_kernel";
    case ConvKernel::S2Bf16: return "conv_s2_bf16_kernel";
    case ConvKernel::Qkv: return "conv1x1_qkv_bf16_kernel";
    case ConvKernel::Bf16Stream1x1: return "conv1x1_bf16_stream_kernel";
    case ConvKernel::Small1x1: return "conv1x1_small_kernel";
  }
  return "?";
}

size_t conv_plan(ConvParams& p, int num_cus, const Knobs& k, int plan_n) {
  const ConvDims d(p);
  const ConvFill f(p, d, num_cus, plan_n);
  const int Cout = p.Cout;
  // the halo forms' tile depth: 128-voxel tiles, or on an under-filled chip 64-voxel tiles that double the workgroups before
  // resorting to split-K.  Exact-fp32 launches whose (z,y) Winograd weights exist for 64-channel output blocks keep the
  // 128-voxel tile on under-filled levels too: the Winograd kernels do 4/9 (8/27) of the MFMAs per voxel, which buys more
  // than the doubled workgroup count of 64-voxel tiles; the chip is filled by split-K over the channel chunks instead.
  // HOLO_CONV_WINO_SMALL=0 turns that off, HOLO_CONV_FORCE_TZ2=1 (tests) takes 128-voxel tiles (hence the Winograd kernels)
  // on small grids
  const bool wino_small = k.conv_wino_small != 0 && Cout >= 64 && conv_wino2_can_run(p, d) && d.ncc >= 2;
  const int tz = f.tiles < f.target && k.conv_force_tz2 != 1 && !wino_small ? 1 : 2;

  // ---- the kernel: the first of these that can run and is wanted here
  const ConvKernel kernel = [&] {
    // the qkv convolution of an AttentionBlock, fused with the operand packing of the bf16 attention (the planner offers it by
    // setting qkv_q; HOLO_CONV_QKV_FUSED=0 keeps the row-tile kernel + attn_pack_kernel)
    if (p.qkv_q) {
      if (conv_qkv_can_run(p, d) && k.conv_qkv_fused != 0) return ConvKernel::Qkv;
      p.qkv_q = nullptr;  // (not this launch: the caller packs)
    }
    // any other 1x1x1 convolution of a large grid on bf16 storage (the attention's proj_out): the same streaming GEMM with a
    // plain output (HOLO_CONV1X1_BF16_STREAM=0 keeps the row-tile kernel)
    if (conv_bf16_stream1x1_can_run(p, d) && k.conv1x1_bf16_stream != 0) return ConvKernel::Bf16Stream1x1;
    // a 1x1x1 convolution of raw input over a LARGE grid (a ResBlock's skip_connection on the 64^3 level): the streaming
    // GEMM (HOLO_CONV1X1_STREAM_MIN_M=<rows>: development knob, default 131 072 rows; 0 = off)
    if (conv_stream1x1_can_run(p, d) && k.conv1x1_stream_min_m > 0 && f.Mc >= k.conv1x1_stream_min_m)
      return ConvKernel::Stream1x1;
    // an attention block's qkv / proj_out in exact fp32 (16^3, 8^3): one 16-row tile per workgroup, K split over its
    // waves (HOLO_CONV1X1_SMALL=0 keeps the row-tile kernel)
    if (conv_small1x1_can_run(p, d) && k.conv1x1_small != 0) return ConvKernel::Small1x1;
    // the stride-2 convolution of a Downsample block in the bf16 storage mode, where its 128-voxel tiles give the chip at
    // least a workgroup per four CUs (128^3 net: 128^3 -> 64^3 540 -> ~100 us, and the two levels below; deeper the row-tile
    // kernel's split-K fills the chip better).  HOLO_CONV_S2T=0 keeps the row-tile kernel, =1 takes this one wherever it is
    // defined (tests)
    if (conv_s2_bf16_can_run(p, d) && k.conv_s2t != 0 && ((f.Mc / 128) * (Cout / 64) >= num_cus / 4 || k.conv_s2t == 1))
      return ConvKernel::S2Bf16;
    // bf16 wide-tile kernel: where it fills the chip without split-K, and on the under-filled levels once the K extent is
    // long (BF16T_LONG_K).  HOLO_CONV_BF16T=0 disables it, =1 forces it everywhere (tests)
    if (conv_bf16_wide_can_run(p, d) && k.conv_bf16t != 0 &&
        (f.t8 >= f.target || d.Cin + d.SCin >= BF16T_LONG_K || k.conv_bf16t == 1)) {
      // the filled levels (every CU gets whole tiles without split-K): the persistent wave-specialised form
      // (kernels_conv_bf16p.hip) - by default only for launches that stage their input RAW (no GroupNorm / SiLU on load: the
      // input convolution, the Upsample convolutions): there its producer waves keep up with the consumers (tools/bf16p_probe:
      // 128^3 32 -> 64 282 vs 293 us); with the activation arithmetic they do not yet (540 vs 479 us) and conv_bf16t_kernel
      // stays.  HOLO_CONV_BF16P=0 keeps conv_bf16t_kernel everywhere, =2 takes the persistent form for activated input too,
      // =1 forces it onto every wide-tile launch, without split-K (tests: small grids)
      const int64_t bp = k.conv_bf16p;
      const int wgs = num_cus & ~7;
      if (conv_bf16_persistent_can_run(p, d) && bp != 0 && (bp == 1 || bp == 2 || !p.coef) &&
          ((bf16t_split(p, d, f, num_cus).n == 1 && wgs >= 8 && f.t8 >= wgs) || bp == 1))
        return ConvKernel::Bf16Persistent;
      return ConvKernel::Bf16Wide;
    }
    // F(2x2x2, 3x3x3) form (kernels_conv3.hip) from HOLO_CONV_WINO3_MIN_ITEMS work items on (default num_cus / 2: the (z,y)
    // form needs 2 workgroups per CU).  HOLO_CONV_WINO3=0 disables it
    if (conv_wino3_can_run(p, d) && tz == 2 && k.conv_wino3 != 0) {
      const int n = wino3_split(d, f, num_cus).n;
      if (wino3_split_fits(p, d, n) && f.t3 * n >= (k.conv_wino3_min_items != KNOB_UNSET ? k.conv_wino3_min_items : num_cus / 2))
        return ConvKernel::Wino3;
    }
    // exact-fp32 128-voxel tiles: the (z,y) Winograd form when its weights were prepared
    if (conv_wino2_can_run(p, d) && tz == 2) return ConvKernel::Wino2;
    if (conv_halo_can_run(p, d)) return ConvKernel::Halo;
    // 1x1x1, strided and deepest-level convs: row-tile kernel (also for the 32^3 stride-2 convolution with its 32 768 rows:
    // the per-tap gather kernel takes 118 us there, this one 95); under 64 output channels the per-tap gather kernel
    return conv_row_tile_can_run(p, d) ? ConvKernel::RowTile : ConvKernel::Gather;
  }();
  p.kernel = kernel;
  // the upsampling form of the three-axis Winograd kernel (kernels_conv3.hip): nearest x2 input read raw, no fused skip.
  // HOLO_CONV_WINO3_UP=0 keeps the generic form.  (No shape criterion: measured per launch, the form pays on every shape of
  // the plan, the split-K 16^3 one included - profiles/r14_wino3_upsample.txt)
  p.wino3_up = kernel == ConvKernel::Wino3 && p.ups && !p.coef && !p.skip_w && k.conv_wino3_up != 0 ? 1 : 0;

  // ---- its geometry
  switch (kernel) {
    case ConvKernel::Qkv:
    case ConvKernel::Bf16Stream1x1:
      q1_plan(p, d, num_cus);
      [[fallthrough]];
    case ConvKernel::Stream1x1:
    case ConvKernel::Small1x1:
      p.nsplit = 1;
      p.chunks_per_split = d.ncc;
      break;
    case ConvKernel::S2Bf16:
      p.nsplit = 1;
      p.chunks_per_split = d.Cin / 16;
      break;
    case ConvKernel::RowTile: {
      const int64_t t2 = cdiv(f.Mc, SM_ROWS) * cdiv(Cout, 64);
      const int64_t tgt = SM_SPLIT_WGS_PER_CU * (int64_t)num_cus;
      const int nall = d.nchunks + d.nsk;
      const int max_split = nall / SG > 1 ? nall / SG : 1;  // a split below one full staging group only adds a reduce launch
      const KSplit s = ksplit(t2 < tgt ? cdiv(tgt, t2) : 1, max_split, nall);
      p.nsplit = s.n;
      p.chunks_per_split = s.cps;
      break;
    }
    case ConvKernel::Gather: {
      const int max_split = d.nchunks / 4 > 1 ? d.nchunks / 4 : 1;  // keep >= 4 chunks per block
      const KSplit s = ksplit(f.tiles < f.target ? cdiv(f.target, f.tiles) : 1, max_split, d.nchunks);
      p.nsplit = s.n;
      p.chunks_per_split = s.cps;
      break;
    }
    case ConvKernel::Bf16Wide: {
      const KSplit s = bf16t_split(p, d, f, num_cus);
      p.tz = 8;
      p.nsplit = s.n;
      p.chunks_per_split = s.cps;
      p.skip_chunks_per_split = (int)cdiv(d.nsk16, s.n);
      p.grid_x = (int)(d.M / 512);
      break;
    }
    case ConvKernel::Bf16Persistent: {  // no split-K: grid_x persistent workgroups, a multiple of 8 up to the CUs' multiple of 8
      const int64_t wcap = (num_cus & ~7) >= 8 ? (num_cus & ~7) : 8;
      const int64_t t8a = (d.M / 512) * cdiv(Cout, d.bn);  // (the tiles of all samples)
      int64_t g = t8a < wcap ? ((t8a + 7) & ~(int64_t)7) : wcap;
      const int64_t max_wgs = k.conv_bf16p_wgs;  // test knob: at most this many persistent workgroups
      if (max_wgs > 0 && max_wgs < g) g = max_wgs;
      p.tz = 8;
      p.nsplit = 1;
      p.chunks_per_split = d.ncc16;
      p.skip_chunks_per_split = d.nsk16;
      p.grid_x = (int)g;
      break;
    }
    case ConvKernel::Wino3: {
      const KSplit s = wino3_split(d, f, num_cus);
      const int64_t items = (d.M / 128) * (Cout / 64) * s.n;
      p.tz = 2;
      p.nsplit = s.n;
      p.chunks_per_split = s.cps;
      p.skip_chunks_per_split = (int)cdiv(d.nsk, s.n);
      // every workgroup gets the same number of items when the list allows it (the last round is then full)
      p.grid_x = (int)cdiv(items, cdiv(items, num_cus));
      break;
    }
    case ConvKernel::Halo:
    case ConvKernel::Wino2: {  // split over 32-channel chunks (each split walks all 27 taps)
      const int64_t htiles = tz == 2 ? f.tiles : (f.Mc / 64) * cdiv(Cout, d.bn);
      const KSplit s = ksplit(htiles < f.target ? cdiv(f.target, htiles) : 1, d.ncc, d.ncc);
      p.tz = tz;
      p.nsplit = s.n;
      p.chunks_per_split = s.cps;
      p.skip_chunks_per_split = (int)cdiv(d.nsk, s.n);
      // One workgroup per tile.  (The kernel can also walk several tiles per workgroup - grid_x < tiles - with the
      // next tile's halo prefetched under the last tap; measured on MI355X that is no faster than letting the
      // dispatcher refill the slots, which also balances the load dynamically: tools/conv_timeline.cpp.)
      p.grid_x = (int)(d.M / (64 * tz));
      break;
    }
  }
  const size_t scratch = p.nsplit > 1 ? (size_t)p.nsplit * d.M * Cout * sizeof(float) : 0;
  if (k.debug_plan)
    fprintf(stderr, "[plan] conv %d->%d k%d s%d @%d^3 batch %d%s: %s, tz %d, split-K %d x %d chunks (skip %d), grid_x %d, qkv %d rows x %d slices, scratch %zu bytes\n",
            d.Cin, Cout, p.ksz, p.stride, p.OD, p.N, p.skip_w ? " +skip" : "", conv_kernel_name(kernel), p.tz, p.nsplit,
            p.chunks_per_split, p.skip_chunks_per_split, p.grid_x, p.qkv_rows, p.qkv_sb, scratch);
  return scratch;
}

// slab decomposition shared by the planner (buffer sizes) and the launchers (gn_stats_launch, conv_launch's split-K reduce)
void gn_stats_geometry(int C, int64_t V, int* n_blocks, int* vox_per_block) {
  const int cq = C >> 2;
  const int rows = 256 / cq;
  int64_t B = cdiv(V, rows);
  if (B > 256) B = 256;
  int64_t vpb = cdiv(cdiv(V, B), rows) * rows;
  *n_blocks = (int)cdiv(V, vpb);
  *vox_per_block = (int)vpb;
}

// Number of GroupNorm-statistics slabs per sample the launch of `p` writes into p.stats (0 = this launch cannot
// produce them: un-split gather kernel; use gn_stats_launch on the output instead).
int conv_stats_slabs(const ConvParams& p) {
  const int64_t V = (int64_t)p.OD * p.OH * p.OW;
  if (p.nsplit > 1) {
    int B, vpb;
    gn_stats_geometry(p.Cout < 1024 ? p.Cout : 1024, V, &B, &vpb);
    return B;
  }
  switch (p.kernel) {
    case ConvKernel::Bf16Wide:
    case ConvKernel::Bf16Persistent:
      return (int)(V / 512);  // one slab per tile
    case ConvKernel::Halo:
      if (conv_halo_bf16x3(p)) return (int)(V / 32);  // bf16x3 kernel: per half 8x8 slab
      [[fallthrough]];
    case ConvKernel::Wino2:
    case ConvKernel::Wino3:
      return (int)(V / (64 * p.tz)) * (p.Cout >= 64 ? 1 : 2);
    case ConvKernel::RowTile:
      return V % SM_ROWS == 0 ? (int)(V / SM_ROWS) : 0;
    case ConvKernel::S2Bf16:
      return (int)(V / 128);  // one slab per 2 x 8 x 8 tile
    case ConvKernel::Bf16Stream1x1:
      return p.qkv_rows > 0 ? p.qkv_T / p.qkv_rows : 0;  // one slab per workgroup row block
    case ConvKernel::Small1x1:
      return (int)(V / 16);  // one slab per workgroup
    default:
      return 0;
  }
}

double conv_flops(const ConvParams& p) {
  const double M = (double)p.N * p.OD * p.OH * p.OW;
  return 2.0 * M * p.Cout * ((double)(p.C0 + p.C1) * p.ksz * p.ksz * p.ksz + (p.skip_w ? p.skip_C0 + p.skip_C1 : 0));
}

// multiply-adds actually issued to the matrix pipe (x2): the Winograd kernels spend 64 pseudo-taps per 2 x 2 x 2 outputs
// (F(2x2x2)) or 48 per 2 x 2 outputs ((z,y) form) where the direct form spends 27 per output; the fused skip costs the
// same in all forms (F(2x2x2): accumulated directly; (z,y): 4 pseudo-taps per 4 outputs)
double conv_exec_flops(const ConvParams& p) {
  // (the upsampling form of the F(2x2x2) kernel issues the 27 of 64 pseudo-taps whose operands are not identically zero)
  const double wino3_taps = p.wino3_up ? 27.0 / 8.0 : 8.0;
  const double taps = p.kernel == ConvKernel::Wino3 ? wino3_taps : p.kernel == ConvKernel::Wino2 ? 12.0 : 0.0;
  if (taps == 0.0) return conv_flops(p);
  const double M = (double)p.N * p.OD * p.OH * p.OW;
  return 2.0 * M * p.Cout * ((double)(p.C0 + p.C1) * taps + (p.skip_w ? p.skip_C0 + p.skip_C1 : 0));
}

}  // namespace holo
