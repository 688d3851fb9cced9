// holo_kernels.h — host-side launchers of the gfx950 kernels (definitions in kernels_*.hip).
// All pointers are device pointers; `stream` is a hipStream_t as void*.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/holo_abi.h"
#include "attn_plan.h"
#include "bwd_plan.h"
#include "conv_plan.h"
#include "conv_weights.h"
#include "holo_knobs.h"
#include "render_plan.h"

// per-device context of the C ABI (holo_ctx_create)
struct HoloCtx {
  int device;
  int num_cus;
  int deterministic = 0;  // holo_ctx_set_deterministic: scatter-adds of the backward entries in fixed point (order-independent)
};

namespace holo {

// conv3d (ConvParams, conv_plan: conv_plan.h).  conv_launch runs the kernel conv_plan chose; the launchers of the kernels
// that live in files of their own pick the instantiation only (conv_can_launch has checked the launch).
int conv_launch(const ConvParams& p, void* stream);
int conv_s2_bf16_launch(const ConvParams& p, void* stream);         // kernels_conv_s2.hip
int conv1x1_qkv_bf16_launch(const ConvParams& p, void* stream);     // kernels_conv1x1_bf16.hip
int conv1x1_bf16_stream_launch(const ConvParams& p, void* stream);  // kernels_conv1x1_bf16.hip
int conv_wino3_launch(const ConvParams& p, void* stream);           // kernels_conv3.hip
int conv_bf16p_launch(const ConvParams& p, void* stream);           // kernels_conv_bf16p.hip
// kernels_conv3.hip (conv_wino3_weight_floats and the pack constants behind it: conv_weights.h)
int repack_conv_weight_wino3_launch(const float* w, float* out, int Cout, int Cin, int src_taps, int CoutP, int CinP,
                                    void* stream);

// batched GEMM on fp32 MFMA (kernels_gemm.hip; GemmParams: attn_plan.h)
int gemm_launch(const GemmParams& p, void* stream);
// nb products C[b] (M x N, ldc) = A[b] (M x K, lda) . B[b] (b_kmajor ? K x N : N x K; ldb), strides sa / sb / sc between them
inline int gemm_batch_launch(const float* A, int lda, const float* B, int ldb, int b_kmajor, float* C, int ldc, int M, int N,
                             int K, int nb, int64_t sa, int64_t sb, int64_t sc, void* stream) {
  GemmParams g;
  memset(&g, 0, sizeof g);
  g.A = A, g.B = B, g.C = C;
  g.M = M, g.Nn = N, g.K = K;
  g.lda = lda, g.ldb = ldb, g.ldc = ldc;
  g.nb0 = nb, g.nb1 = 1;
  g.sa0 = sa, g.sb0 = sb, g.sc0 = sc;
  g.b_kmajor = b_kmajor;
  g.alpha = 1.f;
  return gemm_launch(g, stream);
}

// attention (AttnParams and the sizing rules the planner shares with these launchers: attn_plan.h)
int flash_attn_launch(const AttnParams& p, void* stream);
// packed != 0: the operands in `work` have been written already (the fused qkv convolution), the packing pre-pass is skipped;
// flash_attn_bf16v2_operands: where they go and the scale folded into Q
int flash_attn_bf16v2_launch(const AttnParams& p, void* work, int out_bf16, int ksplit, int lazy, void* stream, int packed = 0);

// in-place row softmax over `rows` rows of length `cols` (unet.py:453, fp32)
int softmax_rows_launch(float* s, int64_t rows, int cols, void* stream);

// ---------------------------------------------------------------------------------------------
// misc (kernels_misc.hip)
// ---------------------------------------------------------------------------------------------
int ncdhw_to_ndhwc_launch(const float* in, float* out, int N, int C, int64_t V, int tanh_flag, void* stream,
                          int out_bf16 = 0);  // out_bf16 / in_bf16 / x_bf16: the channels-last tensor is bf16
int ndhwc_to_ncdhw_launch(const float* in, float* out, int N, int C, int64_t V, void* stream, int in_bf16 = 0);
int f32_to_bf16_launch(const float* in, float* out_bf16, int64_t n, void* stream);  // element-wise, n % 8 == 0

// GroupNorm statistics, stage 1: partial[n][b][c] = (sum, sumsq) in double over voxel slab b (deterministic,
// no atomics).  gn_stats_geometry (conv_plan.h) gives the slab count B(C, V) the buffers must be sized for.
int gn_stats_launch(const float* x, double* partial, int N, int C, int64_t V, void* stream, int x_bf16 = 0);

// stage 2: GroupNorm(32 groups, eps) folded to per-channel (a,b), optionally composed with FiLM
// (unet.py:248-250): y = GN(x)*(1+scale)+shift.  Channels [0,C0) use part0 (B0 slabs), [C0,C0+C1) part1.
int gn_finalize_launch(const double* part0, int C0, int B0, const double* part1, int C1, int B1, int N, int64_t V,
                       int groups, float eps, const float* gamma, const float* beta, const float* film,
                       int film_stride, int film_cout, float* coef, void* stream, float* moments = nullptr,
                       const float* x0 = nullptr, const float* x1 = nullptr, float* act = nullptr, int act_silu = 0);
// moments (training forward): [N][C0 + C1][2] = (mean, rstd) of the channel's group, for the backward pass
// act (optional): the launch also writes act[n][v][c] = a*x + b (act_silu: SiLU of it) over the virtual concat x = [x0 | x1],
// channels-last fp32 of C0 / C1 channels, with the arithmetic of the row-tile convolution's staging: the one convolution
// that would apply (a, b) on load reads `act` as raw input instead.  Needs (C0 + C1) / groups % 4 == 0 and C0 % 4 == 0.

// emb = Linear2(SiLU(Linear1(timestep_embedding(t, mc))));  writes silu(emb) (all consumers apply SiLU first:
// unet.py:199-205) and emb itself.  load_kind: the HOLO_DEBUG_TIMESTEP_LOAD of the plan (0 in production, see the kernel).
int time_embed_launch(const int64_t* t, int N, int mc, int ted, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* emb, float* emb_silu, int load_kind, void* stream);

// out[n][r] = bias[r] + sum_k W[r][k] * in[n][k]      (all ResBlock emb_layers concatenated)
int rows_linear_launch(const float* in, const float* w, const float* bias, float* out, int N, int rows, int K,
                       void* stream);

int ddpm_step_launch(const float* tables, int T, const int64_t* timesteps, int batch, int64_t per, const float* x_t,
                     const float* model_out, const float* noise, int clip, float* sample, float* pred_xstart,
                     void* stream);
// The Philox steps (include/holo_abi.h).  row_streams null: holo_*_step_philox, `offset` is the 64-bit stream offset;
// non-null: holo_*_step_philox_rows, one stream per row and `offset` is the 32-bit timestep index.
int ddpm_step_philox_launch(const float* tables, int T, const int64_t* timesteps, int batch, int64_t per, const float* x_t,
                            const float* model_out, uint64_t seed, const uint32_t* row_streams, uint64_t offset, int clip,
                            float* sample, float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream);
// DDIM step: coefs is (batch, 8) fp32, one row per sample (include/holo_abi.h, holo_ddim_step)
int ddim_step_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                     const float* noise, int clip, float* sample, float* pred_xstart, void* stream);
int ddim_step_philox_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                            uint64_t seed, const uint32_t* row_streams, uint64_t offset, int clip, float* sample,
                            float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream);
// The guided steps (include/holo_abi.h, holo_ddpm_step_guided / holo_ddim_step_guided): `grad` is the cond_fn gradient,
// `variances` the (T,) posterior_variance table, slot 5 of a DDIM row sqrt(1 - abar_t); the Philox forms as above
int ddpm_step_guided_launch(const float* tables, int T, const int64_t* timesteps, const float* variances, int batch,
                            int64_t per, const float* x_t, const float* model_out, const float* grad, const float* noise,
                            int clip, float* sample, float* pred_xstart, void* stream);
int ddpm_step_guided_philox_launch(const float* tables, int T, const int64_t* timesteps, const float* variances, int batch,
                                   int64_t per, const float* x_t, const float* model_out, const float* grad, uint64_t seed,
                                   const uint32_t* row_streams, uint64_t offset, int clip, float* sample,
                                   float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream);
int ddim_step_guided_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                            const float* grad, const float* noise, int clip, float* sample, float* pred_xstart,
                            void* stream);
int ddim_step_guided_philox_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                                   const float* grad, uint64_t seed, const uint32_t* row_streams, uint64_t offset, int clip,
                                   float* sample, float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream);
// DPM-Solver++ multistep step: coefs is (batch, 8) fp32, rows {a, b0, b1, b2, 0...}; hist1 / hist2 may be null
// (include/holo_abi.h, holo_dpm_step)
int dpm_step_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                    const float* hist1, const float* hist2, int clip, float* sample, float* pred_xstart, void* stream);
// The masked (inpainting) DDPM step and forward noising (include/holo_abi.h, holo_ddpm_step_inpaint / holo_q_sample):
// known_coefs / coefs are (batch, 2) fp32 rows {a, b}; mask is (batch, voxels); `ncdhw` says where an element's voxel is
// (0: element / channels, 1: element % voxels); the Philox forms as above
int ddpm_step_inpaint_launch(const float* tables, int T, const int64_t* timesteps, const float* known_coefs, int batch,
                             int64_t per, int channels, int ncdhw, const float* x_t, const float* model_out,
                             const float* x0_known, const float* mask, const float* noise, const float* noise_known,
                             int clip, float* sample, float* pred_xstart, void* stream);
int ddpm_step_inpaint_philox_launch(const float* tables, int T, const int64_t* timesteps, const float* known_coefs, int batch,
                                    int64_t per, int channels, int ncdhw, const float* x_t, const float* model_out,
                                    const float* x0_known, const float* mask, uint64_t seed, const uint32_t* row_streams,
                                    uint64_t offset, int clip, float* sample, float* pred_xstart, float* noise_out,
                                    float* noise_known_out, void* stream);
int q_sample_launch(const float* coefs, int batch, int64_t per, const float* x, const float* noise, float* out, void* stream);
int q_sample_philox_launch(const float* coefs, int batch, int64_t per, const float* x, uint64_t seed,
                           const uint32_t* row_streams, uint64_t offset, float* out, float* noise_out, int ncdhw_channels,
                           void* stream);
// Diffusion losses and the variational bound's terms (include/holo_abi.h, holo_diffusion_loss / holo_vb_terms).  A workgroup
// owns kLossTile elements of one sample and leaves one double per term in `partial` (loss_partials(batch, per) doubles: a
// function of the shapes alone); a one-workgroup finalize launch writes `terms` ((batch, 2) / (batch, 3) doubles)
constexpr int kLossTile = 2048;
int64_t loss_partials(int batch, int64_t per);
int diffusion_loss_launch(int batch, int64_t per, const float* target, const float* model_out, const float* row_scale,
                          double* terms, float* grad_out, double* partial, void* stream);
int vb_terms_launch(const float* coefs, int batch, int64_t per, const float* x_start, const float* x_t, const float* noise,
                    const float* model_out, int clip, double* terms, double* partial, void* stream);
int tanh_launch(const float* x, float* y, int64_t n, void* stream);
// dst = src for a SMALL caller-provided tensor, read with system-scope loads (holo_ld_sys, holo_common.h)
int copy_sys_launch(const float* src, float* dst, int64_t n, void* stream);
// ---- shared by the host files (*_exec.cpp, host_params.h)
// returns HOLO_E_HIP from the calling function, with the failed call in the error text
#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      holo::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return HOLO_E_HIP;                                                                     \
    }                                                                                        \
  } while (0)
// every part of a workspace starts on a 256-byte boundary
inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// 0.5 * (R - 1) * voxel_size: the VolumeLocator's local -> world scale of an R^3 grid
inline float grid_half_extent(int resol, float volume_extent) {
  return 0.5f * (float)(resol - 1) * (volume_extent / (float)resol);
}
// Host -> device upload of a packed parameter image into a buffer that kernels have been reading (a re-commit after a
// parameter update): the bytes land in a staging buffer that only copy_sys_kernel ever reads (system-scope loads), which
// then writes `dst` like any kernel - so no kernel can meet a stale cached line of `dst` (holo_ld_sys).  Synchronises.
// Returns 0 or the hipError_t.
inline int upload_via_stage(float** stage, size_t* stage_floats, float* dst, const float* host, size_t n, void* stream) {
  if (*stage_floats < n) {
    if (*stage) (void)hipFree(*stage);
    *stage = nullptr;
    *stage_floats = 0;
    hipError_t e = hipMalloc((void**)stage, n * sizeof(float));
    if (e != hipSuccess) return (int)e;
    *stage_floats = n;
  }
  hipError_t e = hipMemcpyAsync(*stage, host, n * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (copy_sys_launch(*stage, dst, (int64_t)n, stream)) return -1;
  e = hipStreamSynchronize((hipStream_t)stream);
  return e == hipSuccess ? 0 : (int)e;
}
int clip_launch(const float* x, float* y, float lo, float hi, int64_t n, void* stream);

// ---------------------------------------------------------------------------------------------
// Parameter update (kernels_optim.hip): multi-tensor Adam and the global gradient norm.  The tensor list travels by value in
// the kernel arguments: a table of kAdamTensors descriptors and kAdamBlocks (tensor, chunk) entries per launch, a chunk =
// kAdamChunk elements split over kAdamSplit workgroups.
// ---------------------------------------------------------------------------------------------
constexpr int kAdamTensors = 40;
constexpr int kAdamBlocks = 320;
constexpr int kAdamChunk = 65536;
constexpr int kAdamSplit = 8;
struct AdamTable {
  float* param[kAdamTensors];
  const float* grad[kAdamTensors];
  float* exp_avg[kAdamTensors];
  float* exp_avg_sq[kAdamTensors];
  float* copy[kAdamTensors];  // optional second destination of the updated parameter
  int64_t numel[kAdamTensors];
  uint16_t chunk[kAdamBlocks];  // entry -> chunk of its tensor
  uint8_t tensor[kAdamBlocks];  // entry -> slot in the arrays above
};
// the step's scalars, formed on the host in double like torch (adam_scalars, unet_exec.cpp) and rounded once
struct AdamScalars {
  float w1;             // 1 - beta1
  float beta2, w2;      // beta2, 1 - beta2
  float eps;
  float neg_step_size;  // -lr / (1 - beta1^step)
  float bc2_sqrt;       // sqrt(1 - beta2^step)
  float weight_decay;
  float decay;          // 1 - lr * weight_decay (adamw)
  int32_t adamw;
};
// copies: n optional second destinations (or null).  Stream-ordered, no allocation, no synchronisation.
int adam_step_launch(const HoloAdamTensor* t, float* const* copies, int n, const AdamScalars& s, const float* clip_coef,
                     void* stream);
int64_t grad_norm_partials(const HoloAdamTensor* t, int n);  // doubles of workspace grad_norm_launch needs
int grad_norm_launch(const HoloAdamTensor* t, int n, float max_norm, double* partial, float* total_norm, float* clip_coef,
                     void* stream);

int repack_conv_weight_bf16_launch(const float* w, uint16_t* out, int Cout, int Cin, int taps, int CoutP, int CinP,
                                   void* stream);
// OIDHW [Cout][Cin][taps] -> zero padded MFMA-fragment-packed layout (see ConvParams::w)
// OIDHW 3x3x3 (src_taps = 27) -> 48 (z,y) Winograd pseudo-taps, or a 1x1x1 skip weight (src_taps = 1) -> its 4
// pseudo-taps; same packed layout as repack_conv_weight_launch
int repack_conv_weight_wino2_launch(const float* w, float* out, int Cout, int Cin, int src_taps, int CoutP, int CinP,
                                    void* stream);
int repack_conv_weight_launch(const float* w, float* out, int Cout, int Cin, int taps, int CoutP, int CinP,
                              void* stream);

// ---------------------------------------------------------------------------------------------
// renderer (kernels_render.hip)
// ---------------------------------------------------------------------------------------------
// packed RenderMLP (built by render_exec.cpp::holo_renderer_commit)
struct MlpParams {
  const float* w_feat;  // [Hd][C]   folded density-net rows 0..Hd-1 (hidden features)
  const float* b_feat;  // [Hd]
  const float* w_dens;  // [C]       folded density row
  float b_dens;
  const float* w_rad;   // [3][Hd]   radiance weights on the hidden features
  const float* u_rad;   // [3][C]    0.6 * W_eff[:Hd]^T w_rad[c]  (linear part of LeakyReLU folded)
  const float* w_dir;   // [3][27]   radiance weights on the direction embedding
  float b_rad[3];
  float k_rad[3];       // 0.6 * w_rad[c] . b_eff[:Hd]
  int Hd;
};

struct RenderKernelParams {
  const float* grid_cl;  // (R,R,R,C) channels-last voxel features
  int R, C;
  float half_extent;  // 0.5*(R-1)*voxel_size (VolumeLocator local->world scale)
  MlpParams mlp;
  // cameras of this launch: gridDim.y = n_cams frames are rendered by ONE launch (outputs of camera i at
  // rgb + i*3*H*W, depth + i*H*W, ...): a single 400^2 frame is only 1.6 waves of workgroups on 256 CUs, so
  // per-frame launches leave the chip half empty for the second half of every frame
  struct Cam {
    float Rm[9], T[3], focal[2], pp[2];
    float zmin, zmax;
  };
  static constexpr int MAX_CAMS = 32;
  Cam cams[MAX_CAMS];
  int n_cams;
  int H, W;
  float range_x, range_y;  // NDC half ranges
  int n_coarse, n_fine;
  float bg[3];
  float background_opacity;
  float pdf_eps;
  // persistent launch: n_tiles = n_cams * ceil(H*W/32) wave tiles, walked by gridDim.x * (waves per workgroup) resident
  // waves; xcd > 1: XCD-aware tile order (workgroup b is taken to sit on XCD b % xcd)
  int64_t n_tiles;
  int xcd;
  // scratch, one slot per RESIDENT wave: val_ws 64*32 float4 (sigma, rgb of the coarse samples); nrm_ws the same for
  // their normals (null: normals are not rendered)
  float* val_ws;
  float* nrm_ws;
  const float* dens_field;  // render2_kernel with normals: S[v] = w_dens . F[v] per voxel (density_field_launch); else null
  // outputs (per camera): CHW planes
  float* rgb;
  float* depth;
  float* mask;
  float* rgb_c;  // may be null
  float* depth_c;
  float* mask_c;
  float* nrm;    // rendered normals sum_i w_i n_i (n_cams,3,H,W), fine / coarse pass; may be null
  float* nrm_c;
  unsigned long long* dbg;  // optional per-slot phase clocks [slot][8] (HOLO_RENDER_TIMELINE=1); null in production
  int split3;  // 1: RenderMLP products on the bf16 matrix cores from an exact 3-term bf16 split (feature_size 32 only)
  int* tile_ctr;  // render2_kernel: 8 zeroed counters (one per XCD range) for the dynamic tile hand-out; null = static stride
  int tail_quads;  // render2_kernel, dynamic hand-out: this many LAST 4-ray tiles of every XCD range go out as single-ray items
  // training-mode rendering (n_rays > 0; render2_kernel only): every camera renders the SAME number of rays given as NDC
  // coordinates; outputs are (n_cams, 3, n_rays) / (n_cams, n_rays) planes.  Optional injected random streams (null =
  // deterministic): stratified coarse depths, stratified importance samples, density noise of both passes.
  struct Train {
    int n_rays;
    const float* xys;           // (n_cams, n_rays, 2) NDC x, y of every ray (PyTorch3D convention: +x left, +y up)
    const float* u_coarse;      // (n_cams, n_rays, n_coarse) uniforms in [0,1): stratified depths (_jiggle_within_stratas)
    const float* u_fine;        // (n_cams, n_rays, n_fine) uniforms: sample_pdf(det = False)
    const float* noise_coarse;  // (n_cams, n_rays, n_coarse) standard normals: density noise of the coarse pass
    const float* noise_fine;    // (n_cams, n_rays, n_coarse + n_fine) standard normals of the fine pass, in DEPTH ORDER
    float noise_std;            // density_noise_std_train
    float* z_merged;            // optional out (n_cams, n_rays, n_coarse + n_fine): the fine pass's depths, in depth order
    unsigned char* new_flags;   // optional out, same shape: 1 where the merged position holds an importance sample
  } train;
};

// ---- backward of the training-mode renderer (kernels_render_bwd.hip) ----
// per ray record (36 floats): origin 3 | direction 3 | W_dir e(dir) + b_rad 3 | harmonic embedding of the normalised direction 27
constexpr int RBWD_REC = 36;      // floats per ray record
constexpr int RBWD_REC_DIR = 3;   // offset of the direction
constexpr int RBWD_REC_RDIR = 6;  // offset of the radiance direction term
constexpr int RBWD_REC_EMB = 9;   // offset of the 27 embedding entries
struct RenderBwdRays {
  RenderKernelParams::Cam cams[RenderKernelParams::MAX_CAMS];
  int n_cams, n_rays;
  int64_t ray0;        // global index of the first ray of this camera group
  const float* xys;    // (all cameras, n_rays, 2)
  float* rays;         // (all rays, 36)
  const float* w_dir;  // [3][27]
  float b_rad[3];
};
// one chunk of whole rays; feature-major buffers have `ld` (= chunk capacity, a multiple of 64) columns
struct RenderBwdChunk {
  const float* grid_cl;
  float* ggrid_cl;
  int R, C;
  float half_extent;
  int Hd, Hp;
  int nm, n_coarse, rays_per_cam;
  int64_t ray0;      // global index of the chunk's first ray
  int n_rays_chunk;
  int64_t n, n_pad, ld;
  const float* rays;
  const float* z_merged;           // (all rays, nm) merged depths in depth order
  const unsigned char* new_flags;  // (all rays, nm) 1 = importance sample, 0 = coarse sample
  float* F;    // [n_pad][C]
  float* YT;   // [Hp][ld]
  float* AT;   // [Hp][ld]
  float* GFT;  // [C][ld]
  float4* val;
  float4* drad;
  float4* gval;
  float4* GR;
  double* tmp;    // [n][4]
  float* gr_ray;  // (all rays, 4)
  const float* be;     // [Hp]
  const float* w_rad;  // [3][Hd]
  const float* noise_fine;
  const float* noise_coarse;
  float noise_std;
  const float *g_rgb, *g_depth, *g_mask, *g_rgb_c, *g_depth_c, *g_mask_c;  // any may be null (= zero)
  float bg[3];
  float background_opacity;
  // deterministic mode (null otherwise): the scatter adds fixed-point integers into gfix [voxel][C], scaled from *gfix_max =
  // bits of max |GFT| of the chunk (rbwd_absmax_launch), and rbwd_fix_flush_launch adds the chunk's sums to ggrid_cl
  long long* gfix;
  uint32_t* gfix_max;
};
int rbwd_absmax_launch(const RenderBwdChunk& p, void* stream);
int rbwd_fix_flush_launch(const RenderBwdChunk& p, void* stream);
int rbwd_rays_launch(const RenderBwdRays& p, void* stream);
int rbwd_gather_launch(const RenderBwdChunk& p, void* stream);
int rbwd_point_fwd_launch(const RenderBwdChunk& p, void* stream);
int rbwd_composite_launch(const RenderBwdChunk& p, void* stream);
int rbwd_point_bwd_launch(const RenderBwdChunk& p, void* stream);
int rbwd_dir_grad_launch(const float* gr_ray, const float* rays, int64_t n_rays_total, float* out, void* stream);
int rbwd_rowsum_launch(const float* YT, int64_t ld, int64_t n, int rows, float* out, int accumulate, void* stream);
int rbwd_scatter_launch(const RenderBwdChunk& p, void* stream);
// dw[i] (+)= sum_s partial[s][i] (kernels_bwd.hip)
int partial_reduce_launch(const float* partial, float* dw, int64_t n, int splits, int accumulate, void* stream);

// stand-alone implicit function: densities[P], colours[P][3] at world points pts[P][3];
// direction of point i is dirs[i / pts_per_dir] (pts_per_dir = 1: one direction per point)
struct ImplicitEvalParams {
  const float* grid_cl;
  int R, C;
  float half_extent;
  MlpParams mlp;
  const float* pts;
  const float* dirs;
  float* rdir;  // scratch [ceil(n_points / pts_per_dir)][3]: radiance direction term per direction
  int64_t n_points;     // end of the point range of this launch
  int64_t point0;       // first point of this launch (implicit_points_launch); hidden rows are relative to it
  int64_t pts_per_dir;
  float* densities;
  float* colours;
  float* hidden;  // optional [n_points][Hd]: hidden features after the LeakyReLU (input of the feature head); null = off
};
int bias_leaky_launch(float* y, const float* bias, int64_t rows, int cols, void* stream);
// view pooling (kernels_viewpool.hip): source-view feature maps -> voxel feature grid
struct ViewPoolParams {
  static constexpr int MAX_VIEWS = 16, MAX_FEATS = 8, MAX_AGG = 512;
  struct Cam {
    float Rm[9], T[3], focal[2], pp[2], centre[3];
  };
  struct Feat {
    const float* data;  // (n_views, H, W, Cp) channels-last, Cp = C rounded up to 4
    int C, Cp, H, W;
    int quad0;          // first channel quad of this map in the concatenated quad list
    int out0;           // first aggregated feature of this key: [AVG (C) | STD (C)]
  };
  Cam cams[MAX_VIEWS];
  Feat feat[MAX_FEATS];
  int n_views, n_feats, n_quads;
  int R;
  float half_extent;
  float gamma, min_weight, proj_eps;
  int A, F;           // aggregated features (2 sum C), output features
  const float* wt;    // (A, F) transposed mapper weight
  const float* bias;  // (F) or null
  float* out;         // (1, F, R, R, R)
};
int view_pool_launch(const ViewPoolParams& p, void* stream);
// holo_view_coverage (include/holo_abi.h): per voxel centre the number of views that see it; H / W are each view's map size
struct ViewCoverageParams {
  ViewPoolParams::Cam cams[ViewPoolParams::MAX_VIEWS];
  int H[ViewPoolParams::MAX_VIEWS], W[ViewPoolParams::MAX_VIEWS];
  int n_views, R;
  float half_extent, proj_eps;
  float* out;  // (1, 1, R, R, R)
};
int view_coverage_launch(const ViewCoverageParams& p, void* stream);
// backward of view_pool_kernel (kernels_viewpool_bwd.hip): fwd as for the forward launch (feature maps channels-last in the
// workspace, transposed mapper weight), gout = d loss / d voxel_features (1, F, R, R, R)
struct ViewPoolBwdParams {
  ViewPoolParams fwd;
  const float* gout;
  float* gfeat[ViewPoolParams::MAX_FEATS];  // zeroed (n_views, H, W, Cp) gradient maps, or null per key
  int want_feats;
  float* partial;  // [n_wgs][A * F + F]
  float* dW;       // (F, A) or null
  float* dbias;    // (F) or null
  // deterministic mode (holo_ctx_set_deterministic; null otherwise): zeroed 64-bit fixed-point images of the gradient maps
  // and one word per map for the bits of its largest addend (the launch runs twice: measure, then add)
  long long* gfix[ViewPoolParams::MAX_FEATS];
  uint32_t* fix_max;  // [MAX_FEATS], zeroed
};
int view_pool_bwd_launch(const ViewPoolBwdParams& b, int n_wgs, const Knobs& k, void* stream);
int nhwc_pad_to_nchw_launch(const float* in, float* out, int n, int C, int Cp, int64_t HW, void* stream);
// deterministic mode: in (+)= value of the fixed-point image (binary point from *maxbits), the image zeroed again
int fix_flush_launch(long long* fix, const uint32_t* maxbits, float* out, int64_t n, void* stream);
// MLPMeanFeatureAggregator path (kernels_viewpool.hip): the folded aggregator + mapper (viewpool_exec.cpp); vp carries the
// views, the feature maps (quad0 = first quad in the kernel's padded channel order), R, F, proj_eps and the output
struct MlpMeanParams {
  ViewPoolParams vp;
  const float* a;    // [128][dp]  W1 Ws in the padded channel order
  const float* am;   // [128][dp]  W1 Wm
  const float* cb;   // [128]      W1 (bs + bm) + b1
  const float* g;    // [F][128]   M Wl
  const float* g0;   // [F]        M bl + mapper bias
  const float* l;    // [128]      Wl[0]
  float l0;          // bl[0]
  int dp;            // padded input width (multiple of 8): sum of the maps' padded channels + padded embedding
  int emb0;          // first column of the ray-direction embedding
  int n_harmonic;
};
int mlp_mean_pool_launch(const MlpMeanParams& p, int num_cus, void* stream);
// backward of the MLPMeanFeatureAggregator path (kernels_viewpool_bwd.hip): the row buffers live in the workspace,
// rows = view * P + voxel; NRp / Pp = row counts padded for the split-K products (the padding rows are zero)
struct MlpMeanBwdParams {
  MlpMeanParams fwd;
  const float* gout;  // (1, F, R, R, R)
  int FW;             // width of a DUL row: F values of du, dlogit at column F, zero padding to a multiple of 4
  int64_t NRp, Pp;
  // the row buffers hold ONE chunk of voxels [p0, p0 + Pc) of the Pall = R^3 (rows = view * Pc + local voxel): the workspace
  // does not grow with the grid (holo_mlp_mean_backward walks the chunks, the parameter gradients add up in chunk order)
  int64_t p0, Pc, Pall;
  float *X, *MEAN, *CM, *PRE, *H, *U, *DUL, *DULT, *DPRET, *DC, *DCT, *DX, *DCA;
  float* gfeat[ViewPoolParams::MAX_FEATS];
  long long* gfix[ViewPoolParams::MAX_FEATS];  // deterministic mode, as in ViewPoolBwdParams (per chunk of voxels)
  uint32_t* fix_max;
};
int mm_bwd_step_launch(const MlpMeanBwdParams& b, int step, void* stream);
int mm_colsum_launch(const float* src, int64_t rows, int cols, int ld, float* partial, int n_blocks, float* out, void* stream,
                     int accumulate = 0);
int mm_sum_partials_launch(const float* partial, int S, int64_t n, float* out, void* stream, int accumulate = 0);
int nchw_to_nhwc_pad_launch(const float* in, float* out, int n, int C, int Cp, int64_t HW, void* stream);
int transpose_small_launch(const float* in, float* out, int rows, int cols, void* stream);
// ---------------------------------------------------------------------------------------------
// backward of the denoiser (kernels_bwd.hip)
// ---------------------------------------------------------------------------------------------
// (WgradParams, WgradPlan, GnBwdParams and the sizing rules the training planner shares with these launchers: bwd_plan.h)
int conv_wgrad_launch(const WgradParams& p, const WgradPlan& g, float* dw, int accumulate, void* stream);
int flip_transpose_weight_launch(const float* in, float* out, int Co, int Ci, int T, void* stream);
int weight_tco_ci_launch(const float* in, float* out, int Co, int Ci, int T, void* stream);
int colsum_launch(const float* g, int64_t M, int C, double* scratch, float* out, int accumulate, void* stream);
int gn_bwd_launch(const GnBwdParams& p, void* stream);
int add_launch(float* dst, const float* src, int64_t n, int accumulate, void* stream);
int split_cat_launch(const float* g, float* g0, float* g1, int64_t M, int C0, int C1, int acc0, int acc1, void* stream);
int sumpool2_launch(const float* gup, float* gin, int N, int R, int C, int accumulate, void* stream);
int zero_insert2_launch(const float* gy, float* out, int N, int Rs, int C, void* stream);  // (Rs = the coarse edge, out: (2 Rs)^3)
int conv_dgrad_s2_launch(const float* gy, const float* wt, float* gx, int N, int RI, int RO, int Ci, int Co, int accumulate,
                         void* stream);
int attn_ds_launch(const float* P, float* dP, int64_t rows, int cols, void* stream);
int transpose_launch(const float* in, float* out, int batch, int T, void* stream);
int film_bwd_launch(const float* dfilm, const float* embs, const float* w, float* dw, float* db, float* gembs, int N, int rows,
                    int K, void* stream);
int time_embed_bwd_launch(const int64_t* t, int N, int mc, int ted, const float* w1, const float* b1, const float* w2,
                          const float* b2, const float* gembs, float* dw1, float* db1, float* dw2, float* db2, void* stream);
int fill_launch(float* dst, float v, int64_t n, void* stream);

int implicit_eval_launch(const ImplicitEvalParams& p, void* stream);   // = dirs + points
int implicit_dirs_launch(const ImplicitEvalParams& p, void* stream);
int implicit_points_launch(const ImplicitEvalParams& p, void* stream);
int implicit_normals_launch(const ImplicitEvalParams& p, float* normals, void* stream);  // uses grid_cl, pts, n_points, mlp
int density_field_launch(const float* grid_cl, const float* w_dens, int C, int64_t nvox, float* out, void* stream);
// ---- mesh export (kernels_mesh.hip): the density on a lattice of m^3 points and surface nets on a lattice field
// 2h / (m - 1), rounded once from double: the float32 spacing every lattice coordinate is formed with
inline float lattice_spacing(float half_extent, int m) { return (float)(2.0 * (double)half_extent / (double)(m - 1)); }
// field [m][m][m] = LeakyReLU(trilerp(S)(p) + b_dens); S [R][R][R] from density_field_launch
int density_lattice_launch(const float* S, int R, float half_extent, float b_dens, int m, float* field, void* stream);
size_t surface_workspace_bytes(int m);
int surface_count_launch(const float* field, int m, float level, int64_t* counts, void* workspace, void* stream);
// verts / faces null: that pass is not launched
int surface_emit_launch(const float* field, int m, float level, float half_extent, float* verts, int64_t verts_capacity,
                        int32_t* faces, int64_t tris_capacity, void* workspace, void* stream);
// one launch of a planned call (render_plan.h: render_plan, render_launches)
int render_launch(const RenderKernelParams& p, const RenderPlan& plan, const RenderLaunch& launch, void* stream);

}  // namespace holo
