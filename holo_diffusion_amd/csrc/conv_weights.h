// conv_weights.h — the packed format of one convolution's weights: padding, the size of every device copy, which copies a
// weight gets, and the set of pointers that goes with them.  Host-only arithmetic (no HIP header), shared by unet_plan.cpp,
// unet_exec.cpp, the repack launchers and tools/.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "holo_knobs.h"

namespace holo {

// F(2x2x2, 3x3x3) pack (conv_wino3_kernel, kernels_conv3.hip): floats per (32-channel chunk, 16-Cout slice) of a 3x3x3 weight
// - 64 pseudo-taps x 2 halves x 1 KB - and of a fused 1x1x1 skip - 8 destinations x 2 halves x 1 KB
constexpr int WINO3_CHUNK_FLOATS = 32 * 1024, WINO3_SKIP_FLOATS = 4 * 1024;
inline int64_t conv_wino3_weight_floats(int CoutP, int CinP, int src_taps) {
  return (int64_t)(CinP >> 5) * (CoutP >> 4) * (src_taps == 27 ? WINO3_CHUNK_FLOATS : WINO3_SKIP_FLOATS);
}

// every copy starts on a 64-element boundary of its store
inline int64_t round64(int64_t n) { return (n + 63) & ~(int64_t)63; }

// Packed conv weights are zero padded to [taps][CoutP][CinP].  THE rounding rule: CoutP is a multiple of the kernels' Cout
// tile (64 when Cout >= 64, else 32: 36 .. 60 channels - an in / out width of the net - are two 32-wide tiles), CinP a
// multiple of the 32-channel K chunk.
inline int conv_cout_tile(int Cout) { return Cout >= 64 ? 64 : 32; }  // conv_launch's grids walk Cout in tiles of this width
struct ConvWeightLayout {
  int Cout = 0, Cin = 0, taps = 0;  // as in the OIDHW source: taps 27 (3x3x3) or 1
  int CoutP = 0, CinP = 0;
  int64_t f32_floats() const { return (int64_t)taps * CoutP * CinP; }  // ConvParams::w
  // the bf16 buffer: four planes of f32_floats() elements back to back, as repack_conv_weight_bf16_kernel writes them -
  // hi, mid, lo (ConvParams::w_bf) and plane 3, hi packed for the wide-tile kernels (ConvParams::w_bft)
  int64_t bf16_elems() const { return 4 * round64(f32_floats()); }
  int64_t bft_offset() const { return 3 * f32_floats(); }
  // (z,y) Winograd pack: 48 pseudo-taps of a 3x3x3 weight, 4 of a fused 1x1x1 skip (ConvParams::w_wino2)
  int64_t wino2_floats() const { return (int64_t)(taps == 27 ? 48 : 4) * CoutP * CinP; }
  int64_t wino3_floats() const { return conv_wino3_weight_floats(CoutP, CinP, taps); }  // F(2x2x2) pack (ConvParams::w_wino3)
};
inline ConvWeightLayout conv_weight_layout(int Cout, int Cin, int taps) {
  const int tile = conv_cout_tile(Cout);
  return {Cout, Cin, taps, (Cout + tile - 1) / tile * tile, (Cin + 31) / 32 * 32};
}

// Which copies a weight gets besides the fp32 pack.  Two rules ON PURPOSE: the forward rule follows the levels whose
// convolutions can land on 128-voxel tiles (up to 256 output channels); the transposed convolution of the backward has the
// forward's INPUT channels as its outputs, up to 768 with the skip concat, so the dgrad rule admits 512- and 768-wide
// outputs for the (z,y) form that the forward rule does not.  Merging the two would change which kernels run.
struct ConvCopies {
  bool bf16 = false, wino2 = false, wino3 = false;
};
// forward weights (holo_unet_create): bf16 planes always (the compute mode may change after the weights were set).
// (z,y) Winograd pack: the convolutions that can land on 128-voxel tiles - a 3x3x3 weight, or a ResBlock's 1x1x1
// skip_connection (`skip`) that rides inside one, of the levels with 8-divisible planes: up to 256 output channels, up to
// 768 input channels with the skip concat.  F(2x2x2) pack (64 pseudo-taps / 8 signed skip copies): the levels whose
// workgroup list can fill the chip, 64-channel output blocks up to 256 (64^3 .. 8^3 in the released nets).
// HOLO_CONV_WINO=0: no Winograd copy, HOLO_CONV_WINO3=0: no F(2x2x2) copy
inline ConvCopies forward_copies(const ConvWeightLayout& l, bool skip, const Knobs& k) {
  ConvCopies c;
  const bool c3 = l.taps == 27;
  c.bf16 = true;
  c.wino2 = k.conv_wino != 0 && (c3 || skip) && l.Cout <= 256 && l.Cin <= 768 && (l.Cout % 64 == 0 || (c3 && l.Cout == 32));
  c.wino3 = c.wino2 && k.conv_wino3 != 0 && l.Cout % 64 == 0;
  return c;
}
// transposed weights (holo_unet_set_dgrad_weight; `l` is the TRANSPOSED layout: l.Cout the forward's Cin): the backward runs
// in the exact-fp32 mode only, so no bf16 planes, and Winograd packs only when that mode is on at the call
inline ConvCopies dgrad_copies(const ConvWeightLayout& l, int compute_mode, const Knobs& k) {
  ConvCopies c;
  c.wino2 = k.conv_wino != 0 && compute_mode == 0 && l.taps == 27 && l.Cout % 64 == 0 && l.Cout <= 768 && l.Cin <= 768;
  c.wino3 = c.wino2 && k.conv_wino3 != 0 && l.Cout <= 256;
  return c;
}

// Every device copy of one convolution's weights and the layout they all share (host-side bookkeeping; null = not prepared
// for this conv).  Planner::emit_conv hands the ones the compute mode uses to ConvParams, and conv_plan picks kernels from
// those.
struct ConvWeights {
  float* f32 = nullptr;     // repacked fp32 copy
  uint16_t* bf = nullptr;   // bf16 (RNE) planes hi, mid, lo packed for v_mfma_f32_16x16x32_bf16
  uint16_t* bft = nullptr;  // plane 3 of the same buffer: hi packed for the wide-tile kernel (conv_bf16t_kernel)
  float* wino2 = nullptr;   // the wide top levels: (z,y) Winograd pseudo-taps (conv_wino2_kernel)
  float* wino3 = nullptr;   // ... and the F(2x2x2, 3x3x3) pseudo-taps (conv_wino3_kernel)
  ConvWeightLayout layout;
};
// OIDHW [Cout][Cin][taps] fp32 -> every copy of `dst` that exists (unet_exec.cpp); 0 or the failing launcher's code
int pack_conv_weights(const float* src_oidhw, const ConvWeights& dst, void* stream);

}  // namespace holo
