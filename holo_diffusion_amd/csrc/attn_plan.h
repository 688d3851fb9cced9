// attn_plan.h — the launch descriptions of the attention kernels (GemmParams, AttnParams) and the sizing rules their
// launchers (kernels_gemm.hip, kernels_attn_bf16.hip) share with the denoiser's planner (unet_plan.cpp): which shapes a kernel
// takes, how the key range is split, how large its workspace is and how it is laid out.  Host-only arithmetic, no HIP
// header: ONE definition of each rule, reachable from a plain C++ program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "holo_knobs.h"

namespace holo {

// ---------------------------------------------------------------------------------------------
// batched GEMM on fp32 MFMA (kernels_gemm.hip):  C[b] = alpha * A[b] * B[b]^T
//   A[b][m][k] at A + b*sa + m*lda + k            (k contiguous)
//   B[b][n][k] at B + b*sb + n*ldb + k            (b_kmajor = 0, k contiguous)
//              at B + b*sb + k*ldb + n            (b_kmajor = 1, n contiguous)
//   C[b][m][n] at C + b*sc + m*ldc + n
// batch index b = b0*nb1 + b1 with separate strides for the two levels (sample, head).
// ---------------------------------------------------------------------------------------------
struct GemmParams {
  const float* A;
  const float* B;
  float* C;
  int M, Nn, K;
  int lda, ldb, ldc;
  int nb0, nb1;
  int64_t sa0, sa1, sb0, sb1, sc0, sc1;
  int b_kmajor;
  float alpha;
};

// Flash-style attention over the token-major qkv buffer [N][T][3C] (head-major channel order: q,k,v blocks of
// C/H channels per head, unet.py:448); out is token-major [N][T][C].  scale2 = 1/sqrt(head channels).
struct AttnParams {
  const float* qkv;
  float* out;
  int N, T, C, H;
  float scale2;
  // fp32 kernel: key splits (flash_attn_splits) and, when > 1, the workspace of their partials
  // (flash_attn_workspace_bytes): part [nsplit][N][T][C] unnormalised O, part_ml [nsplit][N][H][T][2] (m, l)
  int nsplit;
  float* part;
  float* part_ml;
};
inline bool flash_attn_supported(int T, int ch) { return (T % 128) == 0 && (ch == 16 || ch == 32 || ch == 64 || ch == 128); }
// Key splits: enough workgroups for one per CU, at most one key tile per wave.  Measured on MI355X (profiles/r07_attn_*):
// T = 512, two heads of 128 channels: 32 workgroups -> 128 with four splits; at T = 4096 the un-split grid has 256
// workgroups already.  HOLO_FLASH_SPLIT=<n> sets the split count (clamped to [1, T/128]; tests, A/B).
inline int flash_attn_splits(int N, int T, int H, int num_cus, const Knobs& k) {
  const int max_split = T / 128;
  const int64_t base = (int64_t)N * H * (T / 32);
  int64_t s = k.flash_split;
  if (s <= 0) s = base < num_cus ? (num_cus + base - 1) / base : 1;
  return (int)(s < 1 ? 1 : s > max_split ? max_split : s);
}
inline size_t flash_attn_workspace_bytes(const AttnParams& p) {
  if (p.nsplit <= 1) return 0;
  return (size_t)p.nsplit * ((size_t)p.N * p.T * p.C + (size_t)p.N * p.H * p.T * 2) * sizeof(float);
}

// bf16-product variant (shared K/V tiles in LDS, v_mfma_f32_16x16x32_bf16), for the opt-in bf16 mode
// Second form of the bf16 attention (bf16 storage mode, long sequences): a pre-pass rewrites qkv once per call as
// bf16 Q (pre-scaled) / K per head and V TRANSPOSED per head, so that the main kernel stages plain 16-byte rows;
// 64-key blocks, 64 queries per wave, v_mfma_f32_32x32x16_bf16, exp2-domain softmax; the key range is split across
// workgroups (and recombined) when one workgroup per 256 queries would leave half of the chip's wave slots empty.
// `work` (flash_attn_bf16v2_workspace_bytes) holds the packed operands and the split partials; out_bf16: `out` is bf16.
// The plan decides ONCE how the key range is split (flash_attn_bf16v2_ksplit) and whether the LAZY pass runs before the exact
// kernel (`lazy`; head channels 32 / 64 only); the workspace is sized and laid out from that same split count.
inline bool flash_attn_bf16v2_supported(int T, int ch) { return (T % 256) == 0 && (ch == 32 || ch == 64 || ch == 128); }
inline int flash_attn_bf16v2_ksplit(const AttnParams& p, int num_cus, const Knobs& k) {
  const int64_t wgs = (int64_t)p.N * p.H * (p.T / (p.C / p.H == 128 ? 128 : 256));
  int ks = 1;
  // two workgroups per CU for the kernels that run two waves per SIMD; the LAZY kernel (head channels 32 / 64) runs one
  const int per_cu = 2;
  while (wgs * ks < per_cu * (int64_t)num_cus && ks < 8 && (p.T / (ks * 2)) % 128 == 0) ks *= 2;  // (an even number of 64-key blocks per split: the LAZY loop takes two per trip)
  const int64_t v = k.flash_v2_ksplit;  // development knob
  if (v >= 1 && v <= 8 && (p.T / v) % 128 == 0) ks = (int)v;
  return ks;
}
inline size_t flash_attn_bf16v2_workspace_bytes(const AttnParams& p, int ks) {
  const size_t ntc = (size_t)p.N * p.T * p.C;
  size_t b = 3 * ntc * sizeof(uint16_t);
  if (ks > 1) b += (size_t)ks * ntc * sizeof(float) + (size_t)ks * p.N * p.H * p.T * 2 * sizeof(float);
  b += (size_t)p.N * p.H * ks * (p.T / 128) * sizeof(int);  // the LAZY kernel's redo flags, one per workgroup
  return b;
}
inline void flash_attn_bf16v2_operands(const AttnParams& p, void* work, uint16_t** q, uint16_t** k, uint16_t** vt, float* qscale) {
  const size_t ntc = (size_t)p.N * p.T * p.C;
  uint16_t* w16 = reinterpret_cast<uint16_t*>(work);
  *q = w16, *k = w16 + ntc, *vt = w16 + 2 * ntc;
  *qscale = p.scale2 * 1.4426950408889634f;  // softmax in the exp2 domain
}

}  // namespace holo
