// kernels_misc.hip — HBM-bound kernels around the MFMA ops of the denoiser.
//
//   layout     NCDHW (plugin boundary) <-> channels-last (kernel layout); optional tanh
//              (holo_diffusion_model.py:425)
//   gn_stats   per-(sample, channel) sum / sum-of-squares of GroupNorm32's input (nn.py:23-25), in double
//   gn_finalize GroupNorm(32, C, eps=1e-5) folded with affine and FiLM (unet.py:248-252) into (a,b)/channel
//   time_embed timestep_embedding + time_embed MLP (nn.py:109-127, unet.py:645-650)
//   rows_linear all ResBlock emb_layers Linear(SiLU(emb)) at once (unet.py:199-205,245)
//   ddpm_step  clamp + posterior mean + noise (gaussian_diffusion.py:314-343,237-240,499-506)
//   ddim_step  clamp + DDIM update (Equation 12) + noise, and its reverse (gaussian_diffusion.py:645-727)
//   dpm_step   clamp + DPM-Solver++ multistep update from the two previous predictions (build-side extension)
#include <stdlib.h>

#include "holo_common.h"
#include "holo_kernels.h"
#include "rowtile_silu.h"

namespace holo {
namespace {

// ---------------------------------------------------------------------------------------------
// [N][C][V] -> [N][V][C] through a 32x33 LDS tile.  grid = (V/32, C/32, N), block = (32, 8)
// ---------------------------------------------------------------------------------------------
// out_bf16 / in_bf16: the channels-last side is a bf16 tensor (bf16 storage mode of the denoiser)
__global__ __launch_bounds__(256) void ncdhw_to_ndhwc_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             int C, int64_t V, int tanh_flag, int out_bf16) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int64_t v0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  in += (int64_t)n * C * V;
  const int64_t obase = (int64_t)n * C * V;
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j;
    const int64_t v = v0 + tx;
    float x = 0.f;
    if (c < C && v < V) x = in[(int64_t)c * V + v];
    if (tanh_flag) x = tanhf(x);
    tile[j][tx] = x;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int64_t v = v0 + j;
    const int c = c0 + tx;
    if (c < C && v < V) {
      if (out_bf16)
        reinterpret_cast<uint16_t*>(out)[obase + v * C + c] = (uint16_t)(pack_bf16x2(tile[tx][j], 0.f) & 0xffffu);
      else
        out[obase + v * C + c] = tile[tx][j];
    }
  }
}

// fp32 -> bf16 of a tensor that already is channels-last (the bf16 storage mode's input on the channels-last entry,
// holo_unet_forward_cl): 8 elements per thread, 2 x 16 bytes in, 16 bytes out
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float4* __restrict__ in, float4* __restrict__ out, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = in[2 * i], b = in[2 * i + 1];
    out[i] = make_float4(__uint_as_float(pack_bf16x2(a.x, a.y)), __uint_as_float(pack_bf16x2(a.z, a.w)),
                         __uint_as_float(pack_bf16x2(b.x, b.y)), __uint_as_float(pack_bf16x2(b.z, b.w)));
  }
}

__global__ __launch_bounds__(256) void ndhwc_to_ncdhw_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             int C, int64_t V, int in_bf16) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int64_t v0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t ibase = (int64_t)n * C * V;
  out += (int64_t)n * C * V;
  for (int j = ty; j < 32; j += 8) {
    const int64_t v = v0 + j;
    const int c = c0 + tx;
    float x = 0.f;
    if (c < C && v < V)
      x = in_bf16 ? __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(in)[ibase + v * C + c] << 16)
                  : in[ibase + v * C + c];
    tile[j][tx] = x;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j;
    const int64_t v = v0 + tx;
    if (c < C && v < V) out[(int64_t)c * V + v] = tile[tx][j];
  }
}

// ---------------------------------------------------------------------------------------------
// GroupNorm statistics, two deterministic stages (no atomics, fixed summation order):
//   stage 1 (gn_stats):    partial[n][b][c] = (sum, sum of squares) over voxel slab b, in double.
//                          x: [N][V][C] channels-last, C % 4 == 0, C/4 <= 256.  block = 256 threads:
//                          cq = C/4 threads across channels, rows = 256/cq voxels per pass; grid = (B, N).
//   stage 2 (gn_finalize): one block per (group, sample) reduces the partials of its channels over all
//                          slabs, then folds GroupNorm(eps) + affine (+ FiLM) into per-channel (a, b).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                       int C, int64_t V, int vox_per_block, int x_bf16) {
  __shared__ double red[256 * 8];
  const int n = blockIdx.y;
  const int cq = C >> 2;
  const int rows = 256 / cq;
  const int tid = threadIdx.x;
  const int c4 = tid % cq;
  const int vr = tid / cq;
  const int64_t vbeg = (int64_t)blockIdx.x * vox_per_block;
  int64_t vend = vbeg + vox_per_block;
  if (vend > V) vend = V;
  const int64_t xbase = (int64_t)n * V * C;
  double ds[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
  if (vr < rows) {
    float fs[4] = {0, 0, 0, 0}, fq[4] = {0, 0, 0, 0};
    int cnt = 0;
#pragma unroll 4
    for (int64_t v = vbeg + vr; v < vend; v += rows) {
      float4 t;
      if (x_bf16) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(x) + xbase + v * C + c4 * 4);
        t = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                        __uint_as_float(u.y & 0xffff0000u));
      } else {
        t = *reinterpret_cast<const float4*>(x + xbase + v * C + c4 * 4);
      }
      fs[0] += t.x;
      fs[1] += t.y;
      fs[2] += t.z;
      fs[3] += t.w;
      fq[0] += t.x * t.x;
      fq[1] += t.y * t.y;
      fq[2] += t.z * t.z;
      fq[3] += t.w * t.w;
      if (++cnt == 32) {  // fp32 partial sums stay short; long sums are carried in double
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ds[e] += fs[e];
          dq[e] += fq[e];
          fs[e] = 0.f;
          fq[e] = 0.f;
        }
        cnt = 0;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ds[e] += fs[e];
      dq[e] += fq[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[tid * 8 + e] = ds[e];
    red[tid * 8 + 4 + e] = dq[e];
  }
  __syncthreads();
  if (tid < cq) {
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < rows; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += red[(r * cq + tid) * 8 + e];
    double* dst = partial + (((int64_t)n * gridDim.x + blockIdx.x) * C + tid * 4) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dst[e * 2 + 0] = s[e];
      dst[e * 2 + 1] = s[4 + e];
    }
  }
}

__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  const float lo = __shfl_xor(__uint_as_float((uint32_t)(b & 0xffffffffull)), mask);
  const float hi = __shfl_xor(__uint_as_float((uint32_t)(b >> 32)), mask);
  b = (unsigned long long)__float_as_uint(lo) | ((unsigned long long)__float_as_uint(hi) << 32);
  double r;
  memcpy(&r, &b, 8);
  return r;
}

// The pre-activated form (PRE, gn_finalize_act_kernel): the block that has just computed its group's (a, b) also writes
// act[n][v][c] = silu(fma(x, a, b)) (or the affine alone) for its cpg channels over all V voxels of its sample, so that the
// ONE convolution reading the tensor takes it as raw input instead of repeating the activation per (tap, Cout tile)
// (unetplan::preactivate_rowtile).  x is the virtual concat [x0 | x1], channels-last fp32; cpg % 4 == 0 and C0 % 4 == 0, so a
// 4-channel quad has one source.  The arithmetic is the row-tile kernel's `commit` (kernels_conv.hip) on the same fp32
// (a, b): one fused multiply-add, then silu_f - the quotient that its shortened division equals wherever it is taken
// (rowtile_silu.h) - so the convolution's results are bit-identical either way.
struct GnPreact {
  const float *x0, *x1;
  float* act;
  int silu;
};
constexpr int GN_PRE_TOP = 2;  // quads per thread up to which x is requested at the top, to come back under the reduction

// coef[n][c] = (a, b) with GN(x)*(1+scale)+shift = a*x + b.  grid = (groups, N), block = 256
// (rs, rq: 4 doubles each of LDS; s_ab: 2 x 256 floats of it in the PRE form, else unused)
template <bool PRE>
__device__ __forceinline__ void gn_finalize_body(double* rs, double* rq, float* s_ab, const double* __restrict__ part0, int C0,
                                                 int B0, const double* __restrict__ part1, int C1, int B1, int64_t V,
                                                 int groups, float eps, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ film,
                                                 int film_stride, int film_cout, float* __restrict__ coef,
                                                 float* __restrict__ moments, const GnPreact& pre) {
  const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int Cin = C0 + C1;
  const int cpg = Cin / groups;
  // PRE: item i of the block is quad i % qpg of voxel i / qpg (items < 2^31: gn_finalize_launch)
  const unsigned qpg = (unsigned)cpg >> 2, items = PRE ? (unsigned)V * qpg : 0u;
  auto item_at = [&](unsigned i, int64_t& row, int& c) {
    const unsigned v = i / qpg;
    c = g * cpg + 4 * (int)(i - v * qpg);
    row = (int64_t)n * V + v;
  };
  auto item_src = [&](int64_t row, int c) { return c < C0 ? pre.x0 + row * C0 + c : pre.x1 + row * C1 + (c - C0); };
  float4 xr[GN_PRE_TOP];
  const bool x_at_top = PRE && items <= (unsigned)GN_PRE_TOP * 256u;
  if (PRE && x_at_top) {
#pragma unroll
    for (int u = 0; u < GN_PRE_TOP; ++u) {
      const unsigned i = (unsigned)tid + (unsigned)u * 256u;
      xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < items) {
        int64_t row;
        int c;
        item_at(i, row, c);
        xr[u] = *reinterpret_cast<const float4*>(item_src(row, c));
      }
    }
  }
  // the channel's affine / FiLM rows are requested FIRST: they come back under the reduction instead of after it (this
  // kernel is nothing but dependent round trips: ~66 launches per forward)
  float pg = 0.f, pb = 0.f, psc = 0.f, psh = 0.f;
  if (tid < cpg) {
    const int c = g * cpg + tid;
    pg = gamma[c];
    pb = beta[c];
    if (film) {
      psc = film[(int64_t)n * film_stride + c];
      psh = film[(int64_t)n * film_stride + film_cout + c];
    }
  }
  // Every (slab, channel-of-the-group) pair is one 16-byte (sum, sumsq) record; consecutive channels of a slab are
  // contiguous, so the threads walk the pairs with the channel index fastest (coalesced runs of cpg records) and keep
  // eight independent loads in flight.  The summation order depends on nothing but the launch geometry: deterministic.
  double s = 0.0, sq = 0.0;
  {
    const int c_lo = g * cpg, c_hi = c_lo + cpg;
    // the group may straddle the seam of the virtual concat: channels [c_lo, c_mid) come from part0, [c_mid, c_hi) from part1
    const int c_mid = c_lo < C0 ? (c_hi < C0 ? c_hi : C0) : c_lo;
    for (int half = 0; half < 2; ++half) {
      const int ca = half == 0 ? c_lo : c_mid, cb = half == 0 ? c_mid : c_hi;
      const int nch = cb - ca;
      if (nch <= 0) continue;
      const double* p = half == 0 && ca < C0 ? part0 : part1;
      const int Cs = p == part0 ? C0 : C1, B = p == part0 ? B0 : B1;
      const int cs0 = p == part0 ? ca : ca - C0;
      const int64_t total = (int64_t)B * nch;
      const double* base = p + ((int64_t)n * B * Cs + cs0) * 2;
      // record j of the run -> (slab j / nch, channel j % nch): 32-bit, and a shift / mask when the run is a power of two wide
      // (it is, except where a group straddles the seam of a concat): the 64-bit division this was costs ~150 instructions,
      // twice per record, in a kernel that is nothing but latency
      const bool pow2 = (nch & (nch - 1)) == 0;
      const int sh = 31 - __builtin_clz((unsigned)nch);
      auto rec = [&](int64_t j64) -> int64_t {
        const unsigned j = (unsigned)j64;  // (total < 2^31: gn_finalize_launch)
        const unsigned q = pow2 ? (j >> sh) : j / (unsigned)nch;
        const unsigned r = pow2 ? (j & (unsigned)(nch - 1)) : j - q * (unsigned)nch;
        return ((int64_t)q * Cs + r) * 2;
      };
      int64_t i = tid;
      // (sixteen loads in flight: the 2 048 x 2 records of a 64^3 tensor of the north-star net - 16 per thread - are ONE round
      //  trip instead of two; a thread adds its records in the same order whatever the batch width: bit-identical sums)
      for (; i + 15 * 256 < total; i += 16 * 256) {
        double2 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int64_t j = i + u * 256;
          v[u] = *reinterpret_cast<const double2*>(base + rec(j));
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          s += v[u].x;
          sq += v[u].y;
        }
      }
      for (; i + 7 * 256 < total; i += 8 * 256) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t j = i + u * 256;
          v[u] = *reinterpret_cast<const double2*>(base + rec(j));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          s += v[u].x;
          sq += v[u].y;
        }
      }
      for (; i < total; i += 256) {
        const double2 v = *reinterpret_cast<const double2*>(base + rec(i));
        s += v.x;
        sq += v.y;
      }
    }
  }
  // fixed-order butterfly inside each wave (no barrier), then the four wave totals in wave order: one barrier in all
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s += shfl_xor_f64(s, o);
    sq += shfl_xor_f64(sq, o);
  }
  if ((tid & 63) == 0) {
    rs[tid >> 6] = s;
    rq[tid >> 6] = sq;
  }
  __syncthreads();
  if (tid < cpg) {
    const int c = g * cpg + tid;
    const double cnt = (double)cpg * (double)V;
    const double mean = (((rs[0] + rs[1]) + rs[2]) + rs[3]) / cnt;
    double var = (((rq[0] + rq[1]) + rq[2]) + rq[3]) / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    double a = rstd * (double)pg;
    double b = (double)pb - mean * a;
    if (film) {
      const double sc = 1.0 + (double)psc;
      const double sh = (double)psh;
      a *= sc;
      b = b * sc + sh;
    }
    coef[((int64_t)n * Cin + c) * 2 + 0] = (float)a;
    coef[((int64_t)n * Cin + c) * 2 + 1] = (float)b;
    if (moments) {  // training forward: the backward needs the group's mean and 1/std
      moments[((int64_t)n * Cin + c) * 2 + 0] = (float)mean;
      moments[((int64_t)n * Cin + c) * 2 + 1] = (float)rstd;
    }
    if (PRE) {  // the fp32 (a, b) the convolution would have read from coef
      s_ab[tid * 2 + 0] = (float)a;
      s_ab[tid * 2 + 1] = (float)b;
    }
  }
  if (PRE) {
    __syncthreads();
    auto apply = [&](unsigned i, float4 x) {
      int64_t row;
      int c;
      item_at(i, row, c);
      const float4* ab = reinterpret_cast<const float4*>(s_ab + (c - g * cpg) * 2);
      const float4 c01 = ab[0], c23 = ab[1];  // (a, b) of channels 0, 1 | 2, 3
      float4 y = make_float4(__builtin_fmaf(x.x, c01.x, c01.y), __builtin_fmaf(x.y, c01.z, c01.w),
                             __builtin_fmaf(x.z, c23.x, c23.y), __builtin_fmaf(x.w, c23.z, c23.w));
      if (pre.silu) y = make_float4(silu_f(y.x), silu_f(y.y), silu_f(y.z), silu_f(y.w));
      *reinterpret_cast<float4*>(pre.act + row * Cin + c) = y;
    };
    if (x_at_top) {
#pragma unroll
      for (int u = 0; u < GN_PRE_TOP; ++u) {
        const unsigned i = (unsigned)tid + (unsigned)u * 256u;
        if (i < items) apply(i, xr[u]);
      }
    } else {
      for (unsigned i = (unsigned)tid; i < items; i += 256u) {
        int64_t row;
        int c;
        item_at(i, row, c);
        apply(i, *reinterpret_cast<const float4*>(item_src(row, c)));
      }
    }
  }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ part0, int C0, int B0,
                                                          const double* __restrict__ part1, int C1, int B1, int64_t V,
                                                          int groups, float eps, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ film, int film_stride,
                                                          int film_cout, float* __restrict__ coef,
                                                          float* __restrict__ moments) {
  __shared__ double rs[4], rq[4];
  gn_finalize_body<false>(rs, rq, nullptr, part0, C0, B0, part1, C1, B1, V, groups, eps, gamma, beta, film, film_stride,
                          film_cout, coef, moments, GnPreact{nullptr, nullptr, nullptr, 0});
}
__global__ __launch_bounds__(256) void gn_finalize_act_kernel(const double* __restrict__ part0, int C0, int B0,
                                                              const double* __restrict__ part1, int C1, int B1, int64_t V,
                                                              int groups, float eps, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ film, int film_stride,
                                                              int film_cout, float* __restrict__ coef,
                                                              float* __restrict__ moments, GnPreact pre) {
  __shared__ double rs[4], rq[4];
  __shared__ __attribute__((aligned(16))) float s_ab[512];
  gn_finalize_body<true>(rs, rq, s_ab, part0, C0, B0, part1, C1, B1, V, groups, eps, gamma, beta, film, film_stride, film_cout,
                         coef, moments, pre);
}

// ---------------------------------------------------------------------------------------------
// time embedding: one block per sample.  dynamic-free: mc <= 256, ted <= 1024
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void time_embed_kernel(const int64_t* __restrict__ t, int mc, int ted,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         float* __restrict__ emb, float* __restrict__ emb_silu,
                                                         int load_kind) {
  __shared__ float te[256];
  __shared__ float h1[1024];
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  // the caller's tensor, possibly just copied from the host: system-scope load (holo_ld_sys).  load_kind != 0 is a
  // DEVELOPMENT knob (HOLO_DEBUG_TIMESTEP_LOAD, scripts/h2d_stress_kinds.py) that reads it the two ways a compiler would:
  // 1 = wave-uniform address (s_load_dwordx2, through the scalar cache), 2 = per-lane address (global_load_dwordx2)
  float tv;
  if (load_kind == 1) {
    tv = (float)t[n];
  } else if (load_kind == 2) {
    const int64_t* tp = t + n;
    HOLO_LAUNDER(tp);  // the address in vector registers
    tv = (float)*tp;
  } else {
    tv = (float)holo_ld_sys(t + n);
  }
  const int half = mc / 2;
  for (int i = tid; i < mc; i += 256) {
    float v = 0.f;
    if (i < 2 * half) {
      const int k = i < half ? i : i - half;
      const float freq = expf((-9.210340371976184f * (float)k) / (float)half);
      const float arg = tv * freq;
      v = i < half ? cosf(arg) : sinf(arg);
    }
    te[i] = v;
  }
  __syncthreads();
  for (int j = tid; j < ted; j += 256) {
    float acc = 0.f;
    const float* w = w1 + (int64_t)j * mc;
    for (int k = 0; k < mc; ++k) acc = fmaf(w[k], te[k], acc);
    acc += b1[j];
    h1[j] = acc / (1.0f + expf(-acc));
  }
  __syncthreads();
  for (int j = tid; j < ted; j += 256) {
    float acc = 0.f;
    const float* w = w2 + (int64_t)j * ted;
    for (int k = 0; k < ted; ++k) acc = fmaf(w[k], h1[k], acc);
    acc += b2[j];
    emb[(int64_t)n * ted + j] = acc;
    emb_silu[(int64_t)n * ted + j] = acc / (1.0f + expf(-acc));
  }
}

// out[n][r] = bias[r] + W[r][:] . in[n][:]   one wave per (r, n)
__global__ __launch_bounds__(256) void rows_linear_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out,
                                                          int rows, int K) {
  const int n = blockIdx.y;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* wr = w + (int64_t)r * K;
  const float* x = in + (int64_t)n * K;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = fmaf(wr[k], x[k], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) out[(int64_t)n * rows + r] = acc + bias[r];
}

// ---------------------------------------------------------------------------------------------
// Sampler step kernels (DDPM, DDIM, DPM-Solver++): float4 per thread, grid = (blocks over per/4, batch).  Each sampler keeps
// its own arithmetic; what they share is below: the clamp, the float4 access of the two layouts, and the in-kernel noise draw.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 clamp4(float4 m) {
  return make_float4(fminf(fmaxf(m.x, -1.f), 1.f), fminf(fmaxf(m.y, -1.f), 1.f), fminf(fmaxf(m.z, -1.f), 1.f),
                     fminf(fmaxf(m.w, -1.f), 1.f));
}
// A thread's four elements from `o` on: STRIDED = false, consecutive floats (one 16-byte access); STRIDED = true, `es` apart
template <bool STRIDED = false>
__device__ __forceinline__ float4 ld4(const float* p, int64_t o, int64_t es = 1) {
  if (STRIDED) return make_float4(p[o], p[o + es], p[o + 2 * es], p[o + 3 * es]);
  return *reinterpret_cast<const float4*>(p + o);
}
template <bool STRIDED = false>
__device__ __forceinline__ void st4(float* p, int64_t o, float4 v, int64_t es = 1) {
  if (STRIDED)
    p[o] = v.x, p[o + es] = v.y, p[o + 2 * es] = v.z, p[o + 3 * es] = v.w;
  else
    *reinterpret_cast<float4*>(p + o) = v;
}

// ---------------------------------------------------------------------------------------------
// The noise drawn IN the kernel (perf mode; gaussian_diffusion.py:498 `th.randn_like(x)`, :604): a thread's four elements
// take the four outputs of ONE Philox4x32-10 block - counter (element quad low, high, sample, stream offset), key (seed
// low, seed high) - turned into standard normals by two Box-Muller pairs.  A draw depends on nothing but (seed, offset,
// sample, element): bit-reproducible whatever the launch geometry; no generator state, no separate randn launch, and the
// 4 B / element of noise never cross HBM (optionally written out for tests).
// "Element" is the LOGICAL element: the quads are numbered in channels-last order (voxel, channel / 4).  NCDHW = 0: the
// tensors are in that order in memory (the sampler's channels-last chain) - quad = four consecutive floats.  NCDHW = 1:
// the tensors are (C, voxels) planes - a thread takes the same quad's four channels of one voxel from four planes
// (consecutive threads = consecutive voxels: coalesced), so both layouts of a chain draw the same noise.
// ROWS (holo_*_step_philox_rows): row b draws what a batch-1 launch draws for stream row_streams[b] - counter slot 2 is 0
// and the key's high word is seed_hi ^ row_streams[b] - so a chain's noise does not depend on the row it runs in.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
// two uniforms -> two standard normals; u1 in (0, 1): 24 bits + half a step, so the logarithm is finite (|z| <= 5.9)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}
// the four normals of canonical quad `qd` (written in place, as box_muller does: returned by value, the DDPM update after it
// compiles to fewer packed instructions)
__device__ __forceinline__ void draw4(int64_t qd, uint32_t slot, uint32_t offset, uint32_t seed_lo, uint32_t key_hi,
                                      float4& e) {
  uint32_t rnd[4];
  philox4x32_10((uint32_t)qd, (uint32_t)((uint64_t)qd >> 32), slot, offset, seed_lo, key_hi, rnd);
  box_muller(rnd[0], rnd[1], e.x, e.y);
  box_muller(rnd[2], rnd[3], e.z, e.w);
}
// the key's high word of row b (its counter slot 2 is ROWS ? 0 : b)
template <bool ROWS>
__device__ __forceinline__ uint32_t row_key(uint32_t seed_hi, const uint32_t* __restrict__ row_streams, int b) {
  return ROWS ? seed_hi ^ holo_ld_sys(row_streams + b) : seed_hi;  // (a small table from the host)
}
// Thread `tid` of sample b: the canonical (channels-last) quad it draws for, where the quad's first element lives, and the
// distance between its elements in memory
struct StepQuad {
  int64_t qd, o, es;
};
template <bool NCDHW>
__device__ __forceinline__ StepQuad step_quad(int64_t tid, int b, int64_t per, int channels) {
  StepQuad q = {tid, (int64_t)b * per + tid * 4, 1};
  if (NCDHW) {
    const int64_t V = per / channels;
    const int64_t cq = tid / V, v = tid - cq * V;
    q.qd = v * (channels >> 2) + cq;
    q.o = (int64_t)b * per + cq * 4 * V + v;
    q.es = V;
  }
  return q;
}

// ---------------------------------------------------------------------------------------------
// DDPM ancestral update (gaussian_diffusion.py:314-343,237-240,499-506): sample = c1*pred + c2*x + [t != 0]*sigma*noise with
// c1, c2, log-variance read by timestep index from the device table.
// ---------------------------------------------------------------------------------------------
struct DdpmCoefs {
  float c1, c2, sig;
};
// sample b's timestep, clamped into the table
__device__ __forceinline__ int64_t ddpm_timestep(int T, const int64_t* __restrict__ timesteps, int b) {
  int64_t tt = holo_ld_sys(timesteps + b);
  if (tt < 0) tt = 0;
  if (tt >= T) tt = T - 1;
  return tt;
}
__device__ __forceinline__ DdpmCoefs ddpm_coefs(const float* __restrict__ tables, int T,
                                                const int64_t* __restrict__ timesteps, int b) {
  const int64_t tt = ddpm_timestep(T, timesteps, b);
  const float c1 = holo_ld_sys(tables + tt * 4 + 0);  // (a 16 KB table uploaded from the host: see holo_ld_sys)
  const float c2 = holo_ld_sys(tables + tt * 4 + 1);
  const float lv = holo_ld_sys(tables + tt * 4 + 2);
  return {c1, c2, tt != 0 ? expf(0.5f * lv) : 0.f};
}
// The reference rounds each product, (c1*pred + c2*x) + sigma*noise; this kernel rounds c1*pred only and fuses the other two
// into the sums: fma(sigma, noise, fma(c2, x, c1*pred)).  Spelled out so that the source says what runs (hipcc's
// __fmul_rn / __fadd_rn are plain operators that contract after inlining); contract(off) keeps it at exactly this.
__device__ __forceinline__ float ddpm_mean(float x, float m, DdpmCoefs c) {
#pragma clang fp contract(off)
  return fmaf(c.c2, x, c.c1 * m);
}
__device__ __forceinline__ float ddpm_update(float x, float m, float e, DdpmCoefs c) {
#pragma clang fp contract(off)
  return fmaf(c.sig, e, ddpm_mean(x, m, c));
}
__device__ __forceinline__ float4 ddpm_update4(float4 x, float4 m, float4 e, DdpmCoefs c) {
  return make_float4(ddpm_update(x.x, m.x, e.x, c), ddpm_update(x.y, m.y, e.y, c), ddpm_update(x.z, m.z, e.z, c),
                     ddpm_update(x.w, m.w, e.w, c));
}

__global__ __launch_bounds__(256) void ddpm_step_kernel(const float* __restrict__ tables, int T,
                                                        const int64_t* __restrict__ timesteps, int64_t per,
                                                        const float* __restrict__ x_t,
                                                        const float* __restrict__ model_out,
                                                        const float* __restrict__ noise, int clip,
                                                        float* __restrict__ sample, float* __restrict__ pred) {
  const int b = blockIdx.y;
  const DdpmCoefs c = ddpm_coefs(tables, T, timesteps, b);
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= per) return;
  const int64_t o = (int64_t)b * per + i;
  const float4 x = ld4(x_t, o);
  float4 m = ld4(model_out, o);
  const float4 e = ld4(noise, o);
  if (clip) m = clamp4(m);
  st4(sample, o, ddpm_update4(x, m, e, c));
  st4(pred, o, m);
}

// The same update with the noise drawn in the kernel (draw4)
template <bool NCDHW, bool ROWS = false>
__global__ __launch_bounds__(256) void ddpm_step_philox_kernel(const float* __restrict__ tables, int T,
                                                               const int64_t* __restrict__ timesteps, int64_t per,
                                                               const float* __restrict__ x_t,
                                                               const float* __restrict__ model_out, uint32_t seed_lo,
                                                               uint32_t seed_hi, uint32_t offset, int clip,
                                                               float* __restrict__ sample, float* __restrict__ pred,
                                                               float* __restrict__ noise_out, int channels,
                                                               const uint32_t* __restrict__ row_streams) {
  const int b = blockIdx.y;
  const uint32_t key_hi = row_key<ROWS>(seed_hi, row_streams, b);
  const DdpmCoefs c = ddpm_coefs(tables, T, timesteps, b);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const StepQuad q = step_quad<NCDHW>(tid, b, per, channels);
  const float4 x = ld4<NCDHW>(x_t, q.o, q.es);
  float4 m = ld4<NCDHW>(model_out, q.o, q.es);
  float4 e;
  draw4(q.qd, ROWS ? 0u : (uint32_t)b, offset, seed_lo, key_hi, e);
  if (clip) m = clamp4(m);
  st4<NCDHW>(sample, q.o, ddpm_update4(x, m, e, c), q.es);
  if (pred) st4<NCDHW>(pred, q.o, m, q.es);
  if (noise_out) st4<NCDHW>(noise_out, q.o, e, q.es);
}

// ---------------------------------------------------------------------------------------------
// Guided DDPM update (condition_mean, gaussian_diffusion.py:429-433, inside p_sample :499-506): the posterior mean is moved
// by variance * grad before the noise is added; pred_xstart stays the clamped model output.  v = variances[t] is
// posterior_variance as its own (T,) table (slot 3 of `tables` stays 0).  Per element
//   mean = ddpm_mean ;  mean_g = mean + v*grad (product rounded, sum rounded) ;  sample = fma(sigma, noise, mean_g)
// so that grad == 0 gives ddpm_update's bits.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ddpm_guided_update(float x, float m, float g, float e, DdpmCoefs c, float v) {
#pragma clang fp contract(off)
  const float mean_g = ddpm_mean(x, m, c) + v * g;
  return fmaf(c.sig, e, mean_g);
}
__device__ __forceinline__ float4 ddpm_guided_update4(float4 x, float4 m, float4 g, float4 e, DdpmCoefs c, float v) {
  return make_float4(ddpm_guided_update(x.x, m.x, g.x, e.x, c, v), ddpm_guided_update(x.y, m.y, g.y, e.y, c, v),
                     ddpm_guided_update(x.z, m.z, g.z, e.z, c, v), ddpm_guided_update(x.w, m.w, g.w, e.w, c, v));
}

__global__ __launch_bounds__(256) void ddpm_step_guided_kernel(const float* __restrict__ tables, int T,
                                                               const int64_t* __restrict__ timesteps,
                                                               const float* __restrict__ variances, int64_t per,
                                                               const float* __restrict__ x_t,
                                                               const float* __restrict__ model_out,
                                                               const float* __restrict__ grad,
                                                               const float* __restrict__ noise, int clip,
                                                               float* __restrict__ sample, float* __restrict__ pred) {
  const int b = blockIdx.y;
  const DdpmCoefs c = ddpm_coefs(tables, T, timesteps, b);
  const float v = holo_ld_sys(variances + ddpm_timestep(T, timesteps, b));
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= per) return;
  const int64_t o = (int64_t)b * per + i;
  const float4 x = ld4(x_t, o);
  float4 m = ld4(model_out, o);
  const float4 g = ld4(grad, o);
  const float4 e = ld4(noise, o);
  if (clip) m = clamp4(m);
  st4(sample, o, ddpm_guided_update4(x, m, g, e, c, v));
  if (pred) st4(pred, o, m);
}

// The same update with the noise drawn in the kernel: the draw of ddpm_step_philox_kernel
template <bool NCDHW, bool ROWS = false>
__global__ __launch_bounds__(256) void ddpm_step_guided_philox_kernel(
    const float* __restrict__ tables, int T, const int64_t* __restrict__ timesteps, const float* __restrict__ variances,
    int64_t per, const float* __restrict__ x_t, const float* __restrict__ model_out, const float* __restrict__ grad,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t offset, int clip, float* __restrict__ sample, float* __restrict__ pred,
    float* __restrict__ noise_out, int channels, const uint32_t* __restrict__ row_streams) {
  const int b = blockIdx.y;
  const uint32_t key_hi = row_key<ROWS>(seed_hi, row_streams, b);
  const DdpmCoefs c = ddpm_coefs(tables, T, timesteps, b);
  const float v = holo_ld_sys(variances + ddpm_timestep(T, timesteps, b));
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const StepQuad q = step_quad<NCDHW>(tid, b, per, channels);
  const float4 x = ld4<NCDHW>(x_t, q.o, q.es);
  float4 m = ld4<NCDHW>(model_out, q.o, q.es);
  const float4 g = ld4<NCDHW>(grad, q.o, q.es);
  float4 e;
  draw4(q.qd, ROWS ? 0u : (uint32_t)b, offset, seed_lo, key_hi, e);
  if (clip) m = clamp4(m);
  st4<NCDHW>(sample, q.o, ddpm_guided_update4(x, m, g, e, c, v), q.es);
  if (pred) st4<NCDHW>(pred, q.o, m, q.es);
  if (noise_out) st4<NCDHW>(noise_out, q.o, e, q.es);
}

// ---------------------------------------------------------------------------------------------
// Masked (inpainting) DDPM update and forward noising (RePaint, Lugmayr et al. 2022; include/holo_abi.h).  Per element
//   unk = ddpm_update ;  known = a*x0_known + b*e_k (q_lin: q_sample's arithmetic) ;  sample = m*known + (1 - m)*unk
// every product and sum of the last two rounded, so that m == 0 gives ddpm_update's bits and m == 1 gives `known`'s.  The mask
// is per VOXEL (batch, voxels).  MODE says how a thread finds the voxels of its four elements:
//   MASK_QUAD     channels-last tensors, C a multiple of 4: four consecutive floats of one voxel
//   MASK_QUAD_PL  NCDHW tensors, C a multiple of 4 (Philox only): the same quad from four channel planes (step_quad<true>)
//   MASK_ELEMS    anything else: four consecutive floats in memory, each with its own voxel (`ncdhw`: element % voxels, else
//                 element / C)
// Philox draw domains, by a tag in counter slot 2 (the row, or 0 with per-row streams): none - the step's noise, the draw of
// ddpm_step_philox_kernel; DRAW_KNOWN - e_k; DRAW_QSAMPLE - q_sample_philox_kernel.  No other kernel sets these bits.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t DRAW_KNOWN = 0x80000000u, DRAW_QSAMPLE = 0x40000000u;
constexpr int MASK_QUAD = 0, MASK_QUAD_PL = 1, MASK_ELEMS = 2;

__device__ __forceinline__ float q_lin(float a, float x, float b, float e) {
#pragma clang fp contract(off)
  return a * x + b * e;
}
__device__ __forceinline__ float4 q_lin4(float a, float4 x, float b, float4 e) {
  return make_float4(q_lin(a, x.x, b, e.x), q_lin(a, x.y, b, e.y), q_lin(a, x.z, b, e.z), q_lin(a, x.w, b, e.w));
}
__device__ __forceinline__ float inpaint_blend(float m, float known, float unk) {
#pragma clang fp contract(off)
  const float om = 1.f - m;
  return m * known + om * unk;
}
__device__ __forceinline__ float4 inpaint_blend4(float4 m, float4 known, float4 unk) {
  return make_float4(inpaint_blend(m.x, known.x, unk.x), inpaint_blend(m.y, known.y, unk.y),
                     inpaint_blend(m.z, known.z, unk.z), inpaint_blend(m.w, known.w, unk.w));
}
// the mask values of the four elements of thread `tid` of sample b (tid * 4 < per; channels divides per)
template <int MODE>
__device__ __forceinline__ float4 mask4(const float* __restrict__ mask, int b, int64_t tid, int64_t per, int channels,
                                        int ncdhw) {
  const int64_t V = per / channels;
  const float* mb = mask + (int64_t)b * V;
  if (MODE == MASK_QUAD || MODE == MASK_QUAD_PL) {
    const float m = mb[MODE == MASK_QUAD ? tid * 4 / channels : tid % V];
    return make_float4(m, m, m, m);
  }
  const int64_t i = tid * 4;
  auto vox = [&](int64_t e) { return ncdhw ? e % V : e / channels; };
  return make_float4(mb[vox(i)], mb[vox(i + 1)], mb[vox(i + 2)], mb[vox(i + 3)]);
}
__device__ __forceinline__ bool all4(float4 m, float v) { return m.x == v && m.y == v && m.z == v && m.w == v; }

template <int MODE>
__global__ __launch_bounds__(256) void ddpm_step_inpaint_kernel(
    const float* __restrict__ tables, int T, const int64_t* __restrict__ timesteps, const float* __restrict__ known_coefs,
    int64_t per, const float* __restrict__ x_t, const float* __restrict__ model_out, const float* __restrict__ x0_known,
    const float* __restrict__ mask, const float* __restrict__ noise, const float* __restrict__ noise_known, int clip,
    float* __restrict__ sample, float* __restrict__ pred, int channels, int ncdhw) {
  const int b = blockIdx.y;
  const DdpmCoefs c = ddpm_coefs(tables, T, timesteps, b);
  const float ka = holo_ld_sys(known_coefs + b * 2), kb = holo_ld_sys(known_coefs + b * 2 + 1);  // (a small host table)
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const int64_t o = (int64_t)b * per + tid * 4;
  const float4 x = ld4(x_t, o);
  float4 m = ld4(model_out, o);
  const float4 e = ld4(noise, o);
  const float4 k0 = ld4(x0_known, o);
  const float4 ek = noise_known ? ld4(noise_known, o) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 mk = mask4<MODE>(mask, b, tid, per, channels, ncdhw);
  if (clip) m = clamp4(m);
  st4(sample, o, inpaint_blend4(mk, q_lin4(ka, k0, kb, ek), ddpm_update4(x, m, e, c)));
  if (pred) st4(pred, o, m);
}

// The same update with both noises drawn in the kernel.  A draw that cannot reach the sample is skipped unless its output is
// wanted (two Philox blocks and four Box-Muller pairs per thread would make the kernel ALU-bound): e_k where b == 0 or the
// mask is 0 on the whole quad, e_u where it is 1 on the whole quad; the skipped noise enters as 0
template <int MODE, bool ROWS>
__global__ __launch_bounds__(256) void ddpm_step_inpaint_philox_kernel(
    const float* __restrict__ tables, int T, const int64_t* __restrict__ timesteps, const float* __restrict__ known_coefs,
    int64_t per, const float* __restrict__ x_t, const float* __restrict__ model_out, const float* __restrict__ x0_known,
    const float* __restrict__ mask, uint32_t seed_lo, uint32_t seed_hi, uint32_t offset, int clip, float* __restrict__ sample,
    float* __restrict__ pred, float* __restrict__ noise_out, float* __restrict__ noise_known_out, int channels, int ncdhw,
    const uint32_t* __restrict__ row_streams) {
  constexpr bool PL = MODE == MASK_QUAD_PL;
  const int b = blockIdx.y;
  const uint32_t key_hi = row_key<ROWS>(seed_hi, row_streams, b);
  const DdpmCoefs c = ddpm_coefs(tables, T, timesteps, b);
  const float ka = holo_ld_sys(known_coefs + b * 2), kb = holo_ld_sys(known_coefs + b * 2 + 1);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const StepQuad q = step_quad<PL>(tid, b, per, channels);
  const float4 x = ld4<PL>(x_t, q.o, q.es);
  float4 m = ld4<PL>(model_out, q.o, q.es);
  const float4 k0 = ld4<PL>(x0_known, q.o, q.es);
  const float4 mk = mask4<MODE>(mask, b, tid, per, channels, ncdhw);
  const uint32_t slot = ROWS ? 0u : (uint32_t)b;
  float4 e = make_float4(0.f, 0.f, 0.f, 0.f), ek = e;
  if (noise_out || !all4(mk, 1.f)) draw4(q.qd, slot, offset, seed_lo, key_hi, e);
  if (noise_known_out || (kb != 0.f && !all4(mk, 0.f))) draw4(q.qd, slot | DRAW_KNOWN, offset, seed_lo, key_hi, ek);
  if (clip) m = clamp4(m);
  st4<PL>(sample, q.o, inpaint_blend4(mk, q_lin4(ka, k0, kb, ek), ddpm_update4(x, m, e, c)), q.es);
  if (pred) st4<PL>(pred, q.o, m, q.es);
  if (noise_out) st4<PL>(noise_out, q.o, e, q.es);
  if (noise_known_out) st4<PL>(noise_known_out, q.o, ek, q.es);
}

// q_sample (gaussian_diffusion.py:189-204) and the composed forward jump of a resampling schedule: out = a*x + b*noise with
// the row (a, b) of sample b; elementwise, any layout
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ coefs, int64_t per,
                                                       const float* __restrict__ x, const float* __restrict__ noise,
                                                       float* __restrict__ out) {
  const int b = blockIdx.y;
  const float ka = holo_ld_sys(coefs + b * 2), kb = holo_ld_sys(coefs + b * 2 + 1);
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= per) return;
  const int64_t o = (int64_t)b * per + i;
  st4(out, o, q_lin4(ka, ld4(x, o), kb, ld4(noise, o)));
}
// the same with the noise drawn in the kernel, in the DRAW_QSAMPLE domain
template <bool NCDHW, bool ROWS = false>
__global__ __launch_bounds__(256) void q_sample_philox_kernel(const float* __restrict__ coefs, int64_t per,
                                                              const float* __restrict__ x, uint32_t seed_lo,
                                                              uint32_t seed_hi, uint32_t offset, float* __restrict__ out,
                                                              float* __restrict__ noise_out, int channels,
                                                              const uint32_t* __restrict__ row_streams) {
  const int b = blockIdx.y;
  const float ka = holo_ld_sys(coefs + b * 2), kb = holo_ld_sys(coefs + b * 2 + 1);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const StepQuad q = step_quad<NCDHW>(tid, b, per, channels);
  float4 e;
  draw4(q.qd, (ROWS ? 0u : (uint32_t)b) | DRAW_QSAMPLE, offset, seed_lo, row_key<ROWS>(seed_hi, row_streams, b), e);
  st4<NCDHW>(out, q.o, q_lin4(ka, ld4<NCDHW>(x, q.o, q.es), kb, e), q.es);
  if (noise_out) st4<NCDHW>(noise_out, q.o, e, q.es);
}

// ---------------------------------------------------------------------------------------------
// DDIM update (gaussian_diffusion.py:645-727: ddim_sample, and ddim_reverse_sample with c4 = 0).  Sample b reads its row
// coefs[b*8 + 0..4] = (sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t], sqrt(abar_prev),
// sqrt(1 - abar_prev - sigma^2), [t != 0] * sigma), computed on the host in float32 in the reference's order, so strided
// schedules and the reverse step need nothing else here.  Per element, in the reference's order and each operation rounded
// (no fma contraction, see ddim_mean):
//   eps = (c0*x - pred) / c1 ;  mean = pred*c2 + c3*eps ;  sample = mean + c4*noise
// ---------------------------------------------------------------------------------------------
// Plain operators under contract(off): hipcc's __fmul_rn / __fadd_rn are plain operators compiled with the header's default
// fp-contract, so after inlining they fuse into fmas (that costs the bit-exactness the DDIM tests check)
__device__ __forceinline__ float ddim_mean(float x, float m, float c0, float c1, float c2, float c3) {
#pragma clang fp contract(off)
  const float eps = (c0 * x - m) / c1;
  return m * c2 + c3 * eps;
}
__device__ __forceinline__ float4 ddim_mean4(float4 x, float4 m, const float (&c)[5]) {
  return make_float4(ddim_mean(x.x, m.x, c[0], c[1], c[2], c[3]), ddim_mean(x.y, m.y, c[0], c[1], c[2], c[3]),
                     ddim_mean(x.z, m.z, c[0], c[1], c[2], c[3]), ddim_mean(x.w, m.w, c[0], c[1], c[2], c[3]));
}
__device__ __forceinline__ float4 add_noise4(float4 s, float c4, float4 e) {
#pragma clang fp contract(off)
  return make_float4(s.x + c4 * e.x, s.y + c4 * e.y, s.z + c4 * e.z, s.w + c4 * e.w);
}

__global__ __launch_bounds__(256) void ddim_step_kernel(const float* __restrict__ coefs, int64_t per,
                                                        const float* __restrict__ x_t,
                                                        const float* __restrict__ model_out,
                                                        const float* __restrict__ noise, int clip,
                                                        float* __restrict__ sample, float* __restrict__ pred) {
  const int b = blockIdx.y;
  float c[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) c[k] = holo_ld_sys(coefs + b * 8 + k);  // (a small table uploaded from the host: see holo_ld_sys)
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= per) return;
  const int64_t o = (int64_t)b * per + i;
  const float4 x = ld4(x_t, o);
  float4 m = ld4(model_out, o);
  if (clip) m = clamp4(m);
  float4 s = ddim_mean4(x, m, c);
  if (noise && c[4] != 0.f) s = add_noise4(s, c[4], ld4(noise, o));
  st4(sample, o, s);
  if (pred) st4(pred, o, m);
}

// The same update with the noise drawn in the kernel: the draw of ddpm_step_philox_kernel (same counter, key and logical
// element numbering), so a DDIM step at timestep t draws the noise a DDPM step at t would.  Samples whose c4 is 0 skip the
// draw unless noise_out asks for it.
template <bool NCDHW, bool ROWS = false>
__global__ __launch_bounds__(256) void ddim_step_philox_kernel(const float* __restrict__ coefs, int64_t per,
                                                               const float* __restrict__ x_t,
                                                               const float* __restrict__ model_out, uint32_t seed_lo,
                                                               uint32_t seed_hi, uint32_t offset, int clip,
                                                               float* __restrict__ sample, float* __restrict__ pred,
                                                               float* __restrict__ noise_out, int channels,
                                                               const uint32_t* __restrict__ row_streams) {
  const int b = blockIdx.y;
  float c[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) c[k] = holo_ld_sys(coefs + b * 8 + k);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const StepQuad q = step_quad<NCDHW>(tid, b, per, channels);
  const float4 x = ld4<NCDHW>(x_t, q.o, q.es);
  float4 m = ld4<NCDHW>(model_out, q.o, q.es);
  if (clip) m = clamp4(m);
  float4 s = ddim_mean4(x, m, c);
  float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c[4] != 0.f || noise_out) {
    draw4(q.qd, ROWS ? 0u : (uint32_t)b, offset, seed_lo, row_key<ROWS>(seed_hi, row_streams, b), e);
    if (c[4] != 0.f) s = add_noise4(s, c[4], e);
  }
  st4<NCDHW>(sample, q.o, s, q.es);
  if (pred) st4<NCDHW>(pred, q.o, m, q.es);
  if (noise_out) st4<NCDHW>(noise_out, q.o, e, q.es);
}

// ---------------------------------------------------------------------------------------------
// Guided DDIM update (condition_score, gaussian_diffusion.py:445-453, then ddim_sample :674-693): the score is moved by
// sqrt(1 - abar_t) * grad, the prediction is re-derived from it (and NOT clamped again), then the DDIM update runs on that
// prediction.  The row of holo_ddim_step with c5 = sqrt(1 - abar_t) in slot 5.  Per element, each operation rounded:
//   eps0 = (c0*x - pred) / c1 ;  eps1 = eps0 - c5*grad ;  predg = c0*x - c1*eps1 ;  eps = (c0*x - predg) / c1
//   sample = predg*c2 + c3*eps + c4*noise ;  pred_xstart = predg
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ddim_guided_mean(float x, float m, float g, const float (&c)[6], float& predg) {
#pragma clang fp contract(off)
  const float eps0 = (c[0] * x - m) / c[1];
  const float eps1 = eps0 - c[5] * g;
  predg = c[0] * x - c[1] * eps1;
  return ddim_mean(x, predg, c[0], c[1], c[2], c[3]);
}
__device__ __forceinline__ float4 ddim_guided_mean4(float4 x, float4 m, float4 g, const float (&c)[6], float4& predg) {
  return make_float4(ddim_guided_mean(x.x, m.x, g.x, c, predg.x), ddim_guided_mean(x.y, m.y, g.y, c, predg.y),
                     ddim_guided_mean(x.z, m.z, g.z, c, predg.z), ddim_guided_mean(x.w, m.w, g.w, c, predg.w));
}

__global__ __launch_bounds__(256) void ddim_step_guided_kernel(const float* __restrict__ coefs, int64_t per,
                                                               const float* __restrict__ x_t,
                                                               const float* __restrict__ model_out,
                                                               const float* __restrict__ grad,
                                                               const float* __restrict__ noise, int clip,
                                                               float* __restrict__ sample, float* __restrict__ pred) {
  const int b = blockIdx.y;
  float c[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = holo_ld_sys(coefs + b * 8 + k);  // (a small table uploaded from the host: see holo_ld_sys)
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= per) return;
  const int64_t o = (int64_t)b * per + i;
  const float4 x = ld4(x_t, o);
  float4 m = ld4(model_out, o);
  const float4 g = ld4(grad, o);
  if (clip) m = clamp4(m);
  float4 pg;
  float4 s = ddim_guided_mean4(x, m, g, c, pg);
  if (noise && c[4] != 0.f) s = add_noise4(s, c[4], ld4(noise, o));
  st4(sample, o, s);
  if (pred) st4(pred, o, pg);
}

// The same update with the noise drawn in the kernel: the draw of ddim_step_philox_kernel
template <bool NCDHW, bool ROWS = false>
__global__ __launch_bounds__(256) void ddim_step_guided_philox_kernel(
    const float* __restrict__ coefs, int64_t per, const float* __restrict__ x_t, const float* __restrict__ model_out,
    const float* __restrict__ grad, uint32_t seed_lo, uint32_t seed_hi, uint32_t offset, int clip,
    float* __restrict__ sample, float* __restrict__ pred, float* __restrict__ noise_out, int channels,
    const uint32_t* __restrict__ row_streams) {
  const int b = blockIdx.y;
  float c[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = holo_ld_sys(coefs + b * 8 + k);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid * 4 >= per) return;
  const StepQuad q = step_quad<NCDHW>(tid, b, per, channels);
  const float4 x = ld4<NCDHW>(x_t, q.o, q.es);
  float4 m = ld4<NCDHW>(model_out, q.o, q.es);
  const float4 g = ld4<NCDHW>(grad, q.o, q.es);
  if (clip) m = clamp4(m);
  float4 pg;
  float4 s = ddim_guided_mean4(x, m, g, c, pg);
  float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c[4] != 0.f || noise_out) {
    draw4(q.qd, ROWS ? 0u : (uint32_t)b, offset, seed_lo, row_key<ROWS>(seed_hi, row_streams, b), e);
    if (c[4] != 0.f) s = add_noise4(s, c[4], e);
  }
  st4<NCDHW>(sample, q.o, s, q.es);
  if (pred) st4<NCDHW>(pred, q.o, pg, q.es);
  if (noise_out) st4<NCDHW>(noise_out, q.o, e, q.es);
}

// ---------------------------------------------------------------------------------------------
// DPM-Solver++ multistep update (Lu et al. 2022, data prediction).  The host expands the order-1/2/3 update into one row per
// sample, coefs[b*8 + 0..3] = (a, b0, b1, b2), formed in float64 and rounded once (ImplicitronGaussianDiffusion.dpm_coefs);
// hist1 / hist2 are the clipped predictions of the two steps before this one.  Per element, each product and each sum
// rounded, in this order (no fma contraction):
//   pred = clip ? clamp(model_out, -1, 1) : model_out ;  sample = ((a*x + b0*pred) + b1*hist1) + b2*hist2
// A null history pointer drops its term: it is neither read nor added.  No noise, so the kernel is layout-agnostic.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 dpm_lin4(float4 x, float4 m, float a, float b0) {
#pragma clang fp contract(off)
  return make_float4(a * x.x + b0 * m.x, a * x.y + b0 * m.y, a * x.z + b0 * m.z, a * x.w + b0 * m.w);
}

__global__ __launch_bounds__(256) void dpm_step_kernel(const float* __restrict__ coefs, int64_t per,
                                                       const float* __restrict__ x_t,
                                                       const float* __restrict__ model_out,
                                                       const float* __restrict__ hist1,
                                                       const float* __restrict__ hist2, int clip,
                                                       float* __restrict__ sample, float* __restrict__ pred) {
  const int b = blockIdx.y;
  float c[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = holo_ld_sys(coefs + b * 8 + k);  // (a small table uploaded from the host: see holo_ld_sys)
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= per) return;
  const int64_t o = (int64_t)b * per + i;
  const float4 x = ld4(x_t, o);
  float4 m = ld4(model_out, o);
  if (clip) m = clamp4(m);
  float4 s = dpm_lin4(x, m, c[0], c[1]);
  if (hist1) s = add_noise4(s, c[2], ld4(hist1, o));  // (s + c*h, each operation rounded)
  if (hist2) s = add_noise4(s, c[3], ld4(hist2, o));
  st4(sample, o, s);
  if (pred) st4(pred, o, m);
}

// ---------------------------------------------------------------------------------------------
// Diffusion losses and the terms of the variational bound (include/holo_abi.h: holo_diffusion_loss, holo_vb_terms;
// gaussian_diffusion.py:817-850, :941-952, :1027-1029, losses.py:18-83).  Bandwidth kernels like the steps above: a float4 per
// lane and round, any layout.  A workgroup owns kLossTile consecutive elements of ONE sample: per-lane double accumulators, a
// fixed-order LDS tree, one partial per (sample, term, workgroup) in the caller's workspace; loss_finalize_kernel (one
// workgroup) adds a sample's partials in a fixed order and scales.  No atomics, no last-block trick: the number of partials
// depends on (batch, elems_per_sample) alone, so the bits depend on neither the run nor the CU count, and a sample's
// terms depend on neither the batch nor the row it runs in.
// ---------------------------------------------------------------------------------------------
constexpr int kLossRounds = kLossTile / 1024;  // 256 lanes x 16 bytes per round
static_assert(kLossTile % 1024 == 0, "whole rounds of 256 float4");

// fixed-order sums of a workgroup's 256 x K doubles (block_sum256 of kernels_optim.hip, K sums behind one set of barriers)
template <int K>
__device__ __forceinline__ void block_sums256(double (&acc)[K], double* red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[k * 256 + tid] = acc[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * 256 + tid] += red[k * 256 + tid + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = red[k * 256];
}
__device__ __forceinline__ double sum4d(float4 v) { return ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w); }

// mean_flat((target - model_out)**2) and mean_flat(_huber(.., scaling=0.001)) (gaussian_diffusion.py:949-952, :1062-1076):
// every operation rounded, in the reference's order; sqrtf and the division are the correctly rounded ones
__device__ __forceinline__ float loss_sq(float t, float m) {
#pragma clang fp contract(off)
  const float d = t - m;
  return d * d;
}
__device__ __forceinline__ float loss_huber(float sq) {
#pragma clang fp contract(off)
  const float s = 0.001f;
  const float a = 1.f + sq / (float)(0.001 * 0.001);
  return (sqrtf(fmaxf(a, 0.f) + 1e-4f) - 1.f) * s;  // (_safe_sqrt(a, eps=1e-4) - 1) * scaling
}
// the cotangent of w_b * mse_b: (model_out - target) * s_b with s_b = float(2 * w_b / n)
__device__ __forceinline__ float4 loss_grad4(float4 t, float4 m, float s) {
#pragma clang fp contract(off)
  return make_float4((m.x - t.x) * s, (m.y - t.y) * s, (m.z - t.z) * s, (m.w - t.w) * s);
}

// grid = (cdiv(per, kLossTile), batch).  partial[(b * 2 + k) * gridDim.x + blockIdx.x], k = 0: sum sq, 1: sum huber
template <bool TERMS, bool GRAD>
__global__ __launch_bounds__(256) void diffusion_loss_kernel(int64_t per, const float* __restrict__ target,
                                                             const float* __restrict__ model_out,
                                                             const float* __restrict__ row_scale, float unit_scale,
                                                             double* __restrict__ partial, float* __restrict__ grad_out) {
  __shared__ double red[TERMS ? 2 * 256 : 1];
  const int b = blockIdx.y;
  const float s = !GRAD ? 0.f : row_scale ? holo_ld_sys(row_scale + b) : unit_scale;
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int r = 0; r < kLossRounds; ++r) {
    const int64_t i = (int64_t)blockIdx.x * kLossTile + (int64_t)(r * 256 + (int)threadIdx.x) * 4;
    if (i < per) {
      const int64_t o = (int64_t)b * per + i;
      const float4 t = ld4(target, o), m = ld4(model_out, o);
      if (TERMS) {
        const float4 sq = make_float4(loss_sq(t.x, m.x), loss_sq(t.y, m.y), loss_sq(t.z, m.z), loss_sq(t.w, m.w));
        acc[0] += sum4d(sq);
        acc[1] += sum4d(make_float4(loss_huber(sq.x), loss_huber(sq.y), loss_huber(sq.z), loss_huber(sq.w)));
      }
      if (GRAD) st4(grad_out, o, loss_grad4(t, m, s));
    }
  }
  if (TERMS) {
    block_sums256<2>(acc, red);
    if (threadIdx.x == 0) {
      partial[((int64_t)b * 2 + 0) * gridDim.x + blockIdx.x] = acc[0];
      partial[((int64_t)b * 2 + 1) * gridDim.x + blockIdx.x] = acc[1];
    }
  }
}

// One sample's row of holo_vb_terms: coefs[b*8 + 0..7] = (posterior_mean_coef1, posterior_mean_coef2, logvar, exp(-logvar),
// exp(-0.5*logvar), sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, [t == 0]) with logvar =
// posterior_log_variance_clipped[t]; every transcendental of a per-row scalar was taken on the host
struct VbRow {
  float c1, c2, einv, istd, sr, srm1;
  bool t0;
};
// losses.py:48-53 in float32, th.pow(x, 3) as (x*x)*x
__device__ __forceinline__ float approx_normal_cdf(float x) {
#pragma clang fp contract(off)
  return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * ((x * x) * x))));
}
// losses.py:56-83: log-likelihood of the Gaussian (mean, 1 / istd) discretised to bins of 2/255 around x in [-1, 1]
__device__ __forceinline__ float discretized_log_likelihood(float x, float mean, float istd) {
#pragma clang fp contract(off)
  const float centered = x - mean;
  const float cdf_plus = approx_normal_cdf(istd * (centered + (float)(1.0 / 255.0)));
  const float cdf_min = approx_normal_cdf(istd * (centered - (float)(1.0 / 255.0)));
  const float p = x < -0.999f ? cdf_plus : x > 0.999f ? 1.0f - cdf_min : cdf_plus - cdf_min;
  return logf(fmaxf(p, 1e-12f));
}
// One element: acc[0] += the bound's term in nats (t > 0: normal_kl of two Gaussians that share the FIXED_SMALL
// log-variance, whose -1 + lv2 - lv1 + exp(lv1 - lv2) is 0 and is NOT evaluated - see holo_abi.h; t == 0: the decoder's
// negative log-likelihood), acc[1] += (pred - x_start)^2, acc[2] += (eps - noise)^2 (gaussian_diffusion.py:409-413)
template <bool NOISE>
__device__ __forceinline__ void vb_element(float x0, float xt, float pred, float e, const VbRow& c, float (&v)[3]) {
#pragma clang fp contract(off)
  if (c.t0) {
    const float mean_p = c.c1 * pred + c.c2 * xt;  // q_posterior_mean_variance(pred, x_t, t): products rounded, sum rounded
    v[0] = -discretized_log_likelihood(x0, mean_p, c.istd);
  } else {
    // mean_q - mean_p = (c1*x_start + c2*x_t) - (c1*pred + c2*x_t): the c2*x_t terms cancel exactly, and are left out - in
    // float32 they leave 2^-24 * |c2*x_t| of rounding in a difference of c1 * |x_start - pred| ~ 1e-4 at t = 999 (1e-3 relative)
    const float dm = c.c1 * (x0 - pred);
    v[0] = 0.5f * ((dm * dm) * c.einv);
  }
  const float dx = pred - x0;
  v[1] = dx * dx;
  if (NOISE) {
    const float de = (c.sr * xt - pred) / c.srm1 - e;
    v[2] = de * de;
  } else {
    v[2] = 0.f;
  }
}

// grid = (cdiv(per, kLossTile), batch).  partial[(b * 3 + k) * gridDim.x + blockIdx.x], k = 0: vb (nats), 1: xstart, 2: eps
template <bool NOISE>
__global__ __launch_bounds__(256) void vb_terms_kernel(const float* __restrict__ coefs, int64_t per,
                                                       const float* __restrict__ x_start, const float* __restrict__ x_t,
                                                       const float* __restrict__ noise,
                                                       const float* __restrict__ model_out, int clip,
                                                       double* __restrict__ partial) {
  __shared__ double red[3 * 256];
  const int b = blockIdx.y;
  float k[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = holo_ld_sys(coefs + b * 8 + j);  // (a small table uploaded from the host: see holo_ld_sys)
  const VbRow c = {k[0], k[1], k[3], k[4], k[5], k[6], k[7] != 0.f};
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < kLossRounds; ++r) {
    const int64_t i = (int64_t)blockIdx.x * kLossTile + (int64_t)(r * 256 + (int)threadIdx.x) * 4;
    if (i < per) {
      const int64_t o = (int64_t)b * per + i;
      const float4 x0 = ld4(x_start, o), xt = ld4(x_t, o);
      float4 m = ld4(model_out, o);
      const float4 e = NOISE ? ld4(noise, o) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (clip) m = clamp4(m);
      float vx[3], vy[3], vz[3], vw[3];
      vb_element<NOISE>(x0.x, xt.x, m.x, e.x, c, vx);
      vb_element<NOISE>(x0.y, xt.y, m.y, e.y, c, vy);
      vb_element<NOISE>(x0.z, xt.z, m.z, e.z, c, vz);
      vb_element<NOISE>(x0.w, xt.w, m.w, e.w, c, vw);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] += sum4d(make_float4(vx[j], vy[j], vz[j], vw[j]));
    }
  }
  block_sums256<3>(acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) partial[((int64_t)b * 3 + j) * gridDim.x + blockIdx.x] = acc[j];
  }
}

// One workgroup.  Per sample, a lane adds every 256th partial of each of the K terms (the K x 8 loads of an unrolled round
// are independent: the launch is a latency chain, not a bandwidth one), then the tree: a fixed order.  out[b*K + k] = sum / n,
// and / ln 2 more for k == bits_term (the bound's term in bits; -1: none)
template <int K>
__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* __restrict__ partial, int batch, int64_t nblk,
                                                            int bits_term, int64_t n, double* __restrict__ out) {
  __shared__ double red[K * 256];
  for (int b = 0; b < batch; ++b) {
    const double* __restrict__ p = partial + (int64_t)b * K * nblk;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += p[k * nblk + i];
    }
    block_sums256<K>(acc, red);
    if (threadIdx.x < K) {
      const double mean = red[threadIdx.x * 256] / (double)n;
      out[b * K + threadIdx.x] = (int)threadIdx.x == bits_term ? mean / 0.6931471805599453 : mean;
    }
    __syncthreads();  // (red is written again in the next round)
  }
}

// copy of a SMALL caller-provided tensor (biases, GroupNorm affine parameters, ...) with system-scope loads (holo_ld_sys)
__global__ __launch_bounds__(256) void copy_sys_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = holo_ld_sys(src + i);
}
__global__ __launch_bounds__(256) void tanh_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = tanhf(x[i]);
}
__global__ __launch_bounds__(256) void clip_kernel(const float* __restrict__ x, float* __restrict__ y, float lo,
                                                   float hi, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = fminf(fmaxf(x[i], lo), hi);
}

// OIDHW [Cout][Cin][taps] -> zero padded packed layout [tap][CinP/32][CoutP/16][half][kq][lj][4]
// (see wpack_block in kernels_conv.hip): element (tap, co, ci) with k = ci % 32 goes to
//   block(tap, ci/32, co/16) + (k>>2 & 1)*256 + ((k>>3)*16 + co%16)*4 + (k & 3)
__global__ __launch_bounds__(256) void repack_conv_weight_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                                 int Cout, int Cin, int taps, int CoutP, int CinP) {
  const int64_t total = (int64_t)CoutP * CinP * taps;
  const int ncc = CinP >> 5, nsl = CoutP >> 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i & 3);
    const int lj = (int)((i >> 2) & 15);
    const int kq = (int)((i >> 6) & 3);
    const int half = (int)((i >> 8) & 1);
    int64_t blk = i >> 9;
    const int slice = (int)(blk % nsl);
    blk /= nsl;
    const int cc = (int)(blk % ncc);
    const int tap = (int)(blk / ncc);
    const int co = slice * 16 + lj;
    const int ci = cc * 32 + kq * 8 + half * 4 + e;
    out[i] = (ci < Cin && co < Cout) ? holo_ld_sys(w + ((int64_t)co * Cin + ci) * taps + tap) : 0.f;  // (caller's tensor: holo_ld_sys)
  }
}

// (z,y) Winograd weights (conv_wino2_kernel): pseudo-tap pt = (xi_z*4 + xi_y)*3 + kx of a 3x3x3 kernel is
// U[xi_z][xi_y][kx] = sum_kz,ky G[xi_z][kz] G[xi_y][ky] w[kz][ky][kx] with G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
// (formed in double, rounded once); a 1x1x1 skip weight (centre tap) has the four non-zero pseudo-taps xi_z, xi_y in
// {1, 2}: +-w/4.  Packed layout as above.
__global__ __launch_bounds__(256) void repack_conv_weight_wino2_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                                       int Cout, int Cin, int src_taps, int CoutP, int CinP) {
  const int taps = src_taps == 27 ? 48 : 4;
  const int64_t total = (int64_t)CoutP * CinP * taps;
  const int ncc = CinP >> 5, nsl = CoutP >> 4;
  const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i & 3);
    const int lj = (int)((i >> 2) & 15);
    const int kq = (int)((i >> 6) & 3);
    const int half = (int)((i >> 8) & 1);
    int64_t blk = i >> 9;
    const int slice = (int)(blk % nsl);
    blk /= nsl;
    const int cc = (int)(blk % ncc);
    const int pt = (int)(blk / ncc);
    const int co = slice * 16 + lj;
    const int ci = cc * 32 + kq * 8 + half * 4 + e;
    float v = 0.f;
    if (ci < Cin && co < Cout) {
      const float* src = w + ((int64_t)co * Cin + ci) * src_taps;
      if (src_taps == 27) {  // pt = (xi_z*4 + xi_y)*3 + kx
        const int kx = pt % 3, xy = (pt / 3) & 3, xz = pt / 12;
        double u = 0.0;
        for (int kz = 0; kz < 3; ++kz)
          for (int ky = 0; ky < 3; ++ky) u += G[xz][kz] * G[xy][ky] * (double)holo_ld_sys(src + kz * 9 + ky * 3 + kx);
        v = (float)u;
      } else {  // pt = (xi_z-1)*2 + (xi_y-1): G[xi][1] = +.5 (xi = 1), -.5 (xi = 2)
        v = ((pt >> 1) == (pt & 1) ? 0.25f : -0.25f) * holo_ld_sys(src);
      }
    }
    out[i] = v;
  }
}

// OIDHW [Cout][Cin][taps] -> FOUR bf16 planes: (hi, mid, lo with w = hi + mid + lo exactly: hi = rne(w),
// mid = rne(w - hi), lo = rne(w - hi - mid)), each packed [tap][CinP/32][CoutP/16][lane = 16*kq + lj][8]: lane's 8
// values are channels 8*kq .. 8*kq+7 of the chunk for output channel 16*slice + lj (B operand of
// v_mfma_f32_16x16x32_bf16).  Plane 0 alone is the plain bf16 rounding used by the bf16 mode.
__global__ __launch_bounds__(256) void repack_conv_weight_bf16_kernel(const float* __restrict__ w,
                                                                      uint16_t* __restrict__ out, int Cout, int Cin,
                                                                      int taps, int CoutP, int CinP) {
  const int64_t total = (int64_t)CoutP * CinP * taps / 2;  // pairs per plane
  const int ncc = CinP >> 5, nsl = CoutP >> 4;
  uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e2 = (int)(i & 3);  // pair index inside the lane's 8 values
    const int lane = (int)((i >> 2) & 63);
    int64_t blk = i >> 8;
    const int slice = (int)(blk % nsl);
    blk /= nsl;
    const int cc = (int)(blk % ncc);
    const int tap = (int)(blk / ncc);
    const int co = slice * 16 + (lane & 15);
    const int ci = cc * 32 + (lane >> 4) * 8 + e2 * 2;
    const float v0 = (ci < Cin && co < Cout) ? holo_ld_sys(w + ((int64_t)co * Cin + ci) * taps + tap) : 0.f;
    const float v1 = (ci + 1 < Cin && co < Cout) ? holo_ld_sys(w + ((int64_t)co * Cin + ci + 1) * taps + tap) : 0.f;
    const uint32_t h = pack_bf16x2(v0, v1);
    const float r0 = v0 - __uint_as_float(h << 16), r1 = v1 - __uint_as_float(h & 0xffff0000u);
    const uint32_t m = pack_bf16x2(r0, r1);
    const uint32_t l = pack_bf16x2(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
    o32[i] = h;
    o32[total + i] = m;
    o32[2 * total + i] = l;
    // plane 3: the bf16 rounding again, packed for v_mfma_f32_32x32x16_bf16 (conv_bf16t_kernel):
    // [tap][CinP/16][CoutP/32][lane][8], lane's 8 values = channels 8*(lane>>5) .. +7 of the chunk, output channel lane&31
    {
      const int nc16 = CinP >> 4, ns32 = CoutP >> 5;
      int64_t b2 = i >> 8;
      const int sl2 = (int)(b2 % ns32);
      b2 /= ns32;
      const int cc2 = (int)(b2 % nc16);
      const int tap2 = (int)(b2 / nc16);
      const int co2 = sl2 * 32 + (lane & 31);
      const int ci2 = cc2 * 16 + (lane >> 5) * 8 + e2 * 2;
      const float u0 = (ci2 < Cin && co2 < Cout) ? w[((int64_t)co2 * Cin + ci2) * taps + tap2] : 0.f;
      const float u1 = (ci2 + 1 < Cin && co2 < Cout) ? w[((int64_t)co2 * Cin + ci2 + 1) * taps + tap2] : 0.f;
      o32[3 * total + i] = pack_bf16x2(u0, u1);
    }
  }
}

}  // namespace

int ncdhw_to_ndhwc_launch(const float* in, float* out, int N, int C, int64_t V, int tanh_flag, void* stream, int out_bf16) {
  dim3 grid((unsigned)cdiv(V, 32), (unsigned)cdiv(C, 32), (unsigned)N);
  HOLO_LAUNCH(ncdhw_to_ndhwc_kernel, grid, dim3(256), stream, in, out, C, V, tanh_flag, out_bf16);
  return 0;
}
int ndhwc_to_ncdhw_launch(const float* in, float* out, int N, int C, int64_t V, void* stream, int in_bf16) {
  dim3 grid((unsigned)cdiv(V, 32), (unsigned)cdiv(C, 32), (unsigned)N);
  HOLO_LAUNCH(ndhwc_to_ncdhw_kernel, grid, dim3(256), stream, in, out, C, V, in_bf16);
  return 0;
}

int gn_stats_launch(const float* x, double* partial, int N, int C, int64_t V, void* stream, int x_bf16) {
  if ((C & 3) || (C >> 2) > 256) {
    set_error("gn_stats: unsupported C=%d", C);
    return -1;
  }
  int B, vpb;
  gn_stats_geometry(C, V, &B, &vpb);
  dim3 grid((unsigned)B, (unsigned)N);
  HOLO_LAUNCH(gn_stats_kernel, grid, dim3(256), stream, x, partial, C, V, vpb, x_bf16);
  return 0;
}

int gn_finalize_launch(const double* part0, int C0, int B0, const double* part1, int C1, int B1, int N, int64_t V,
                       int groups, float eps, const float* gamma, const float* beta, const float* film,
                       int film_stride, int film_cout, float* coef, void* stream, float* moments, const float* x0,
                       const float* x1, float* act, int act_silu) {
  const int Cin = C0 + C1;
  if (Cin % groups || Cin / groups > 256) {
    set_error("gn_finalize: C=%d not compatible with %d groups", Cin, groups);
    return -1;
  }
  const int cpg = Cin / groups;
  // the kernel numbers the (slab, channel) records of a run in 32 bits
  if ((int64_t)(B0 > B1 ? B0 : B1) * cpg >= ((int64_t)1 << 31)) {
    set_error("gn_finalize: %d slabs of %d channels per group: more than 2^31 records per run", B0 > B1 ? B0 : B1, cpg);
    return -1;
  }
  dim3 grid((unsigned)groups, (unsigned)N);
  if (act) {
    // quads of one source each, numbered in 32 bits
    if ((cpg & 3) || (C0 & 3) || !x0 || (C1 > 0 && !x1) || V * (cpg >> 2) >= ((int64_t)1 << 31)) {
      set_error("gn_finalize: the activated tensor needs whole 4-channel quads per group and source (%d + %d channels, %d groups) "
                "and fewer than 2^31 of them per group (%lld voxels)", C0, C1, groups, (long long)V);
      return -1;
    }
    HOLO_LAUNCH(gn_finalize_act_kernel, grid, dim3(256), stream, part0, C0, B0, part1, C1, B1, V, groups, eps, gamma, beta,
                film, film_stride, film_cout, coef, moments, GnPreact{x0, x1, act, act_silu});
    return 0;
  }
  HOLO_LAUNCH(gn_finalize_kernel, grid, dim3(256), stream, part0, C0, B0, part1, C1, B1, V, groups, eps, gamma, beta,
              film, film_stride, film_cout, coef, moments);
  return 0;
}

int time_embed_launch(const int64_t* t, int N, int mc, int ted, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* emb, float* emb_silu, int load_kind, void* stream) {
  if (mc > 256 || ted > 1024) {
    set_error("time_embed: model_channels=%d too large", mc);
    return -1;
  }
  HOLO_LAUNCH(time_embed_kernel, dim3((unsigned)N), dim3(256), stream, t, mc, ted, w1, b1, w2, b2, emb, emb_silu, load_kind);
  return 0;
}

int rows_linear_launch(const float* in, const float* w, const float* bias, float* out, int N, int rows, int K,
                       void* stream) {
  dim3 grid((unsigned)cdiv(rows, 4), (unsigned)N);
  HOLO_LAUNCH(rows_linear_kernel, grid, dim3(256), stream, in, w, bias, out, rows, K);
  return 0;
}

// The sampler step launchers.  What every step kernel needs of the shapes: elems_per_sample a multiple of 4 (a float4 per
// thread) and, for the Philox kernels, ncdhw_channels 0 or a multiple of 4 that divides it (a quad = four channels of a voxel)
static bool step_shape_ok(const char* name, int64_t per, int ncdhw_channels = 0) {
  if (per & 3) {
    set_error("%s: elems_per_sample must be a multiple of 4", name);
    return false;
  }
  if (ncdhw_channels < 0 || (ncdhw_channels & 3) || (ncdhw_channels > 0 && per % ncdhw_channels)) {
    set_error("%s: ncdhw_channels must be 0 (channels-last tensors) or a multiple of 4 that divides elems_per_sample",
              name);
    return false;
  }
  return true;
}
static dim3 step_grid(int64_t per, int batch) { return dim3((unsigned)cdiv(per / 4, 256), (unsigned)batch); }
// A Philox step kernel's instance for the layout and the stream form.  Counter slot 3 is the offset's low half, and its high
// half goes into the key, so counters stay distinct for any 64-bit stream offset; with row_streams the offset is the
// 32-bit timestep index (high half 0) and the kernel folds each row's stream into the key instead.
#define HOLO_LAUNCH_PHILOX_STEP(kernel, ncdhw_channels, row_streams, ...) \
  do {                                                                    \
    if (ncdhw_channels && row_streams)                                    \
      HOLO_LAUNCH((kernel<true, true>), __VA_ARGS__);                     \
    else if (ncdhw_channels)                                              \
      HOLO_LAUNCH((kernel<true, false>), __VA_ARGS__);                    \
    else if (row_streams)                                                 \
      HOLO_LAUNCH((kernel<false, true>), __VA_ARGS__);                    \
    else                                                                  \
      HOLO_LAUNCH((kernel<false, false>), __VA_ARGS__);                   \
  } while (0)

int ddpm_step_launch(const float* tables, int T, const int64_t* timesteps, int batch, int64_t per, const float* x_t,
                     const float* model_out, const float* noise, int clip, float* sample, float* pred_xstart,
                     void* stream) {
  if (!step_shape_ok("ddpm_step", per)) return -1;
  HOLO_LAUNCH(ddpm_step_kernel, step_grid(per, batch), dim3(256), stream, tables, T, timesteps, per, x_t, model_out, noise,
              clip, sample, pred_xstart);
  return 0;
}

int ddpm_step_philox_launch(const float* tables, int T, const int64_t* timesteps, int batch, int64_t per, const float* x_t,
                            const float* model_out, uint64_t seed, const uint32_t* row_streams, uint64_t offset, int clip,
                            float* sample, float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  if (!step_shape_ok(row_streams ? "ddpm_step_philox_rows" : "ddpm_step_philox", per, ncdhw_channels)) return -1;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);
  HOLO_LAUNCH_PHILOX_STEP(ddpm_step_philox_kernel, ncdhw_channels, row_streams, step_grid(per, batch), dim3(256), stream,
                          tables, T, timesteps, per, x_t, model_out, k0, k1, (uint32_t)offset, clip, sample, pred_xstart,
                          noise_out, ncdhw_channels, row_streams);
  return 0;
}

int ddim_step_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                     const float* noise, int clip, float* sample, float* pred_xstart, void* stream) {
  if (!step_shape_ok("ddim_step", per)) return -1;
  HOLO_LAUNCH(ddim_step_kernel, step_grid(per, batch), dim3(256), stream, coefs, per, x_t, model_out, noise, clip, sample,
              pred_xstart);
  return 0;
}

int ddim_step_philox_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                            uint64_t seed, const uint32_t* row_streams, uint64_t offset, int clip, float* sample,
                            float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  if (!step_shape_ok(row_streams ? "ddim_step_philox_rows" : "ddim_step_philox", per, ncdhw_channels)) return -1;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);  // (as ddpm_step_philox)
  HOLO_LAUNCH_PHILOX_STEP(ddim_step_philox_kernel, ncdhw_channels, row_streams, step_grid(per, batch), dim3(256), stream,
                          coefs, per, x_t, model_out, k0, k1, (uint32_t)offset, clip, sample, pred_xstart, noise_out,
                          ncdhw_channels, row_streams);
  return 0;
}

// The guided steps (include/holo_abi.h): one Philox launcher per sampler, row_streams null or not as above
int ddpm_step_guided_launch(const float* tables, int T, const int64_t* timesteps, const float* variances, int batch,
                            int64_t per, const float* x_t, const float* model_out, const float* grad, const float* noise,
                            int clip, float* sample, float* pred_xstart, void* stream) {
  if (!step_shape_ok("ddpm_step_guided", per)) return -1;
  HOLO_LAUNCH(ddpm_step_guided_kernel, step_grid(per, batch), dim3(256), stream, tables, T, timesteps, variances, per, x_t,
              model_out, grad, noise, clip, sample, pred_xstart);
  return 0;
}

int ddpm_step_guided_philox_launch(const float* tables, int T, const int64_t* timesteps, const float* variances, int batch,
                                   int64_t per, const float* x_t, const float* model_out, const float* grad, uint64_t seed,
                                   const uint32_t* row_streams, uint64_t offset, int clip, float* sample,
                                   float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  if (!step_shape_ok("ddpm_step_guided_philox", per, ncdhw_channels)) return -1;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);  // (as ddpm_step_philox)
  HOLO_LAUNCH_PHILOX_STEP(ddpm_step_guided_philox_kernel, ncdhw_channels, row_streams, step_grid(per, batch), dim3(256),
                          stream, tables, T, timesteps, variances, per, x_t, model_out, grad, k0, k1, (uint32_t)offset,
                          clip, sample, pred_xstart, noise_out, ncdhw_channels, row_streams);
  return 0;
}

// The masked steps (include/holo_abi.h): the mask is per voxel, so the launcher needs the channel count in every layout
static bool inpaint_shape_ok(const char* name, int64_t per, int channels, int ncdhw) {
  if (!step_shape_ok(name, per)) return false;
  if (channels < 1 || per % channels || (ncdhw != 0 && ncdhw != 1)) {
    set_error("%s: channels must be >= 1 and divide elems_per_sample, layout 0 (channels-last) or 1 (NCDHW)", name);
    return false;
  }
  return true;
}

int ddpm_step_inpaint_launch(const float* tables, int T, const int64_t* timesteps, const float* known_coefs, int batch,
                             int64_t per, int channels, int ncdhw, const float* x_t, const float* model_out,
                             const float* x0_known, const float* mask, const float* noise, const float* noise_known,
                             int clip, float* sample, float* pred_xstart, void* stream) {
  if (!inpaint_shape_ok("ddpm_step_inpaint", per, channels, ncdhw)) return -1;
  if (!ncdhw && !(channels & 3))
    HOLO_LAUNCH(ddpm_step_inpaint_kernel<MASK_QUAD>, step_grid(per, batch), dim3(256), stream, tables, T, timesteps,
                known_coefs, per, x_t, model_out, x0_known, mask, noise, noise_known, clip, sample, pred_xstart, channels,
                ncdhw);
  else
    HOLO_LAUNCH(ddpm_step_inpaint_kernel<MASK_ELEMS>, step_grid(per, batch), dim3(256), stream, tables, T, timesteps,
                known_coefs, per, x_t, model_out, x0_known, mask, noise, noise_known, clip, sample, pred_xstart, channels,
                ncdhw);
  return 0;
}

int ddpm_step_inpaint_philox_launch(const float* tables, int T, const int64_t* timesteps, const float* known_coefs, int batch,
                                    int64_t per, int channels, int ncdhw, const float* x_t, const float* model_out,
                                    const float* x0_known, const float* mask, uint64_t seed, const uint32_t* row_streams,
                                    uint64_t offset, int clip, float* sample, float* pred_xstart, float* noise_out,
                                    float* noise_known_out, void* stream) {
  if (!inpaint_shape_ok("ddpm_step_inpaint_philox", per, channels, ncdhw)) return -1;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);  // (as ddpm_step_philox)
  const int mode = (channels & 3) ? MASK_ELEMS : ncdhw ? MASK_QUAD_PL : MASK_QUAD;
#define HOLO_LAUNCH_INPAINT(MODE)                                                                                          \
  do {                                                                                                                     \
    if (row_streams)                                                                                                       \
      HOLO_LAUNCH((ddpm_step_inpaint_philox_kernel<MODE, true>), step_grid(per, batch), dim3(256), stream, tables, T,      \
                  timesteps, known_coefs, per, x_t, model_out, x0_known, mask, k0, k1, (uint32_t)offset, clip, sample,     \
                  pred_xstart, noise_out, noise_known_out, channels, ncdhw, row_streams);                                  \
    else                                                                                                                   \
      HOLO_LAUNCH((ddpm_step_inpaint_philox_kernel<MODE, false>), step_grid(per, batch), dim3(256), stream, tables, T,     \
                  timesteps, known_coefs, per, x_t, model_out, x0_known, mask, k0, k1, (uint32_t)offset, clip, sample,     \
                  pred_xstart, noise_out, noise_known_out, channels, ncdhw, row_streams);                                  \
  } while (0)
  if (mode == MASK_QUAD) HOLO_LAUNCH_INPAINT(MASK_QUAD);
  else if (mode == MASK_QUAD_PL) HOLO_LAUNCH_INPAINT(MASK_QUAD_PL);
  else HOLO_LAUNCH_INPAINT(MASK_ELEMS);
#undef HOLO_LAUNCH_INPAINT
  return 0;
}

int q_sample_launch(const float* coefs, int batch, int64_t per, const float* x, const float* noise, float* out,
                    void* stream) {
  if (!step_shape_ok("q_sample", per)) return -1;
  HOLO_LAUNCH(q_sample_kernel, step_grid(per, batch), dim3(256), stream, coefs, per, x, noise, out);
  return 0;
}

int q_sample_philox_launch(const float* coefs, int batch, int64_t per, const float* x, uint64_t seed,
                           const uint32_t* row_streams, uint64_t offset, float* out, float* noise_out, int ncdhw_channels,
                           void* stream) {
  if (!step_shape_ok("q_sample_philox", per, ncdhw_channels)) return -1;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);  // (as ddpm_step_philox)
  HOLO_LAUNCH_PHILOX_STEP(q_sample_philox_kernel, ncdhw_channels, row_streams, step_grid(per, batch), dim3(256), stream,
                          coefs, per, x, k0, k1, (uint32_t)offset, out, noise_out, ncdhw_channels, row_streams);
  return 0;
}

int ddim_step_guided_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                            const float* grad, const float* noise, int clip, float* sample, float* pred_xstart,
                            void* stream) {
  if (!step_shape_ok("ddim_step_guided", per)) return -1;
  HOLO_LAUNCH(ddim_step_guided_kernel, step_grid(per, batch), dim3(256), stream, coefs, per, x_t, model_out, grad, noise,
              clip, sample, pred_xstart);
  return 0;
}

int ddim_step_guided_philox_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                                   const float* grad, uint64_t seed, const uint32_t* row_streams, uint64_t offset, int clip,
                                   float* sample, float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  if (!step_shape_ok("ddim_step_guided_philox", per, ncdhw_channels)) return -1;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);  // (as ddpm_step_philox)
  HOLO_LAUNCH_PHILOX_STEP(ddim_step_guided_philox_kernel, ncdhw_channels, row_streams, step_grid(per, batch), dim3(256),
                          stream, coefs, per, x_t, model_out, grad, k0, k1, (uint32_t)offset, clip, sample, pred_xstart,
                          noise_out, ncdhw_channels, row_streams);
  return 0;
}

int dpm_step_launch(const float* coefs, int batch, int64_t per, const float* x_t, const float* model_out,
                    const float* hist1, const float* hist2, int clip, float* sample, float* pred_xstart, void* stream) {
  if (!step_shape_ok("dpm_step", per)) return -1;
  HOLO_LAUNCH(dpm_step_kernel, step_grid(per, batch), dim3(256), stream, coefs, per, x_t, model_out, hist1, hist2, clip,
              sample, pred_xstart);
  return 0;
}

int f32_to_bf16_launch(const float* in, float* out_bf16, int64_t n, void* stream) {
  if (n & 7) {
    set_error("f32_to_bf16: the element count must be a multiple of 8");
    return -1;
  }
  int64_t blocks = cdiv(n >> 3, 256);
  if (blocks > 16384) blocks = 16384;
  HOLO_LAUNCH(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), stream, reinterpret_cast<const float4*>(in),
              reinterpret_cast<float4*>(out_bf16), n >> 3);
  return 0;
}

// The loss launchers: `partial` holds loss_partials(batch, per) doubles; the terms come out of the finalize launch
int64_t loss_partials(int batch, int64_t per) { return (int64_t)batch * 3 * cdiv(per, kLossTile); }
static dim3 loss_grid(int64_t per, int batch) { return dim3((unsigned)cdiv(per, kLossTile), (unsigned)batch); }

int diffusion_loss_launch(int batch, int64_t per, const float* target, const float* model_out, const float* row_scale,
                          double* terms, float* grad_out, double* partial, void* stream) {
  if (!step_shape_ok("diffusion_loss", per)) return -1;
  const dim3 grid = loss_grid(per, batch);
  const float unit = (float)(2.0 / (double)per);  // row_scale == NULL: every w_b is 1
  if (terms && grad_out)
    HOLO_LAUNCH((diffusion_loss_kernel<true, true>), grid, dim3(256), stream, per, target, model_out, row_scale, unit, partial,
                grad_out);
  else if (terms)
    HOLO_LAUNCH((diffusion_loss_kernel<true, false>), grid, dim3(256), stream, per, target, model_out, row_scale, unit,
                partial, grad_out);
  else
    HOLO_LAUNCH((diffusion_loss_kernel<false, true>), grid, dim3(256), stream, per, target, model_out, row_scale, unit,
                partial, grad_out);
  if (terms)
    HOLO_LAUNCH(loss_finalize_kernel<2>, dim3(1), dim3(256), stream, (const double*)partial, batch, (int64_t)grid.x, -1, per,
                terms);
  return 0;
}

int vb_terms_launch(const float* coefs, int batch, int64_t per, const float* x_start, const float* x_t, const float* noise,
                    const float* model_out, int clip, double* terms, double* partial, void* stream) {
  if (!step_shape_ok("vb_terms", per)) return -1;
  const dim3 grid = loss_grid(per, batch);
  if (noise)
    HOLO_LAUNCH(vb_terms_kernel<true>, grid, dim3(256), stream, coefs, per, x_start, x_t, noise, model_out, clip, partial);
  else
    HOLO_LAUNCH(vb_terms_kernel<false>, grid, dim3(256), stream, coefs, per, x_start, x_t, noise, model_out, clip, partial);
  HOLO_LAUNCH(loss_finalize_kernel<3>, dim3(1), dim3(256), stream, (const double*)partial, batch, (int64_t)grid.x, 0, per,
              terms);
  return 0;
}

int copy_sys_launch(const float* src, float* dst, int64_t n, void* stream) {
  int64_t blocks = cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  HOLO_LAUNCH(copy_sys_kernel, dim3((unsigned)blocks), dim3(256), stream, src, dst, n);
  return 0;
}
int tanh_launch(const float* x, float* y, int64_t n, void* stream) {
  int64_t blocks = cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  HOLO_LAUNCH(tanh_kernel, dim3((unsigned)blocks), dim3(256), stream, x, y, n);
  return 0;
}
int clip_launch(const float* x, float* y, float lo, float hi, int64_t n, void* stream) {
  int64_t blocks = cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  HOLO_LAUNCH(clip_kernel, dim3((unsigned)blocks), dim3(256), stream, x, y, lo, hi, n);
  return 0;
}
int repack_conv_weight_bf16_launch(const float* w, uint16_t* out, int Cout, int Cin, int taps, int CoutP, int CinP,
                                   void* stream) {
  int64_t total = (int64_t)CoutP * CinP * taps / 2;
  int64_t blocks = cdiv(total, 256);
  if (blocks > 8192) blocks = 8192;
  HOLO_LAUNCH(repack_conv_weight_bf16_kernel, dim3((unsigned)blocks), dim3(256), stream, w, out, Cout, Cin, taps, CoutP,
              CinP);
  return 0;
}
int repack_conv_weight_wino2_launch(const float* w, float* out, int Cout, int Cin, int src_taps, int CoutP, int CinP,
                                    void* stream) {
  if (src_taps != 27 && src_taps != 1) {
    set_error("repack_conv_weight_wino2: 27 or 1 source taps");
    return -1;
  }
  const ConvWeightLayout l = conv_weight_layout(Cout, Cin, src_taps);
  if (l.CoutP != CoutP || l.CinP != CinP) {  // (the kernel indexes with the arguments, the grid is sized from the layout)
    set_error("repack_conv_weight_wino2: paddings %d x %d are not the layout's %d x %d", CoutP, CinP, l.CoutP, l.CinP);
    return -1;
  }
  int64_t total = l.wino2_floats();
  int64_t blocks = cdiv(total, 256);
  if (blocks > 8192) blocks = 8192;
  HOLO_LAUNCH(repack_conv_weight_wino2_kernel, dim3((unsigned)blocks), dim3(256), stream, w, out, Cout, Cin, src_taps,
              CoutP, CinP);
  return 0;
}
int repack_conv_weight_launch(const float* w, float* out, int Cout, int Cin, int taps, int CoutP, int CinP,
                              void* stream) {
  int64_t total = (int64_t)CoutP * CinP * taps;
  int64_t blocks = cdiv(total, 256);
  if (blocks > 8192) blocks = 8192;
  HOLO_LAUNCH(repack_conv_weight_kernel, dim3((unsigned)blocks), dim3(256), stream, w, out, Cout, Cin, taps, CoutP,
              CinP);
  return 0;
}

}  // namespace holo
