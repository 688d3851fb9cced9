// kernels_optim.hip — the parameter update of a training step (include/holo_abi.h: holo_adam_step, holo_grad_norm,
// holo_unet_adam_step).  Replaces torch.optim.Adam(foreach=True).step() and torch.nn.utils.clip_grad_norm_ of the reference's
// training loop (trainer/optimizer_factory.py:78-149, trainer/training_loop.py:544-556).
//
//   adam_multi   one launch updates MANY tensors: the tensor descriptors and a (tensor, chunk) entry per workgroup column
//                travel BY VALUE in the kernel arguments (AdamTable, the scheme of torch's multi_tensor_apply) - no device
//                table, no upload, no allocation; a list longer than one table takes several launches
//   grad_sumsq   the same table walk, per-workgroup partial sums of squares of the gradients (double) into a workspace
//   grad_norm_finalize  one workgroup adds the partials in a fixed order: total_norm and the clip coefficient, which
//                adam_multi reads from the device (clipping costs no host round trip, the norm no atomics)
//
// Geometry: an entry of the table is a chunk of kAdamChunk elements of one tensor; blockIdx.x walks the entries and
// blockIdx.y splits an entry into kAdamSplit slices of 8 192 elements - 256 lanes x 8 rounds of 16 bytes.  A 64-element bias
// therefore costs one entry whose 7 spare workgroups leave at their first comparison, beside ~2 800 entries of real work
// in a 165 M parameter net; a launch holds up to 320 x 8 = 2 560 workgroups (ten per CU: the streaming grid of a
// memory-bound op).  Arithmetic: torch/optim/adam.py::_single_tensor_adam, non-capturable path, operation by operation.
#include "../../include/holo_abi.h"
#include "holo_common.h"
#include "holo_kernels.h"

namespace holo {

static_assert(sizeof(AdamTable) + sizeof(AdamScalars) + 16 <= 3072, "the kernel arguments stay well under the 4 KB limit");
static_assert(kAdamTensors <= 256 && kAdamChunk % (kAdamSplit * 4) == 0, "uint8 tensor slots; slices keep 16-byte alignment");

namespace {

constexpr int kSlice = kAdamChunk / kAdamSplit;

// One element.  Every operation rounds on its own, as the reference's tensor-at-a-time passes do: no contraction by the
// compiler, the one fused multiply-add is the one torch's lerp kernel issues.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamScalars& s, float clip) {
#pragma clang fp contract(off)
  g = g * clip;  // clip_grad_norm_: g.mul_(clip_coef_clamped)
  if (s.weight_decay != 0.f) {
    if (s.adamw)
      p = p * s.decay;  // param.mul_(1 - lr * weight_decay)
    else
      g = g + s.weight_decay * p;  // grad.add(param, alpha=weight_decay)
  }
  const float d = g - m;  // exp_avg.lerp_(grad, 1 - beta1): both branches of torch's lerp, a fused multiply-add there too
  m = s.w1 < 0.5f ? fmaf(s.w1, d, m) : fmaf(d, s.w1 - 1.f, g);
  v = v * s.beta2 + (s.w2 * g) * g;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p + (s.neg_step_size * m) / denom;  // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// the slice [lo, hi) of its tensor this workgroup owns; false: nothing (a spare workgroup of a short tensor)
__device__ __forceinline__ bool adam_slice(const AdamTable& tab, int& t, int64_t& lo, int64_t& hi) {
  t = tab.tensor[blockIdx.x];
  const int64_t n = tab.numel[t];
  lo = (int64_t)tab.chunk[blockIdx.x] * kAdamChunk + (int64_t)blockIdx.y * kSlice;
  hi = lo + kSlice < n ? lo + kSlice : n;
  return lo < n;
}
__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d, const void* e) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

// grid = (entries, kAdamSplit), block = 256.  4 reads + 3 writes (4 with a second destination) of 4 bytes per element.
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamTable tab, const AdamScalars s,
                                                         const float* __restrict__ clip_coef) {
  int t;
  int64_t lo, hi;
  if (!adam_slice(tab, t, lo, hi)) return;
  float* __restrict__ p = tab.param[t];
  const float* __restrict__ g = tab.grad[t];
  float* __restrict__ m = tab.exp_avg[t];
  float* __restrict__ v = tab.exp_avg_sq[t];
  float* __restrict__ cp = tab.copy[t];  // the library's private plain copy of the parameter, or null
  const float clip = clip_coef ? *clip_coef : 1.f;
  const int tid = threadIdx.x;
  if (!aligned16(p, g, m, v, cp)) {  // (a view at an odd storage offset: element by element)
    for (int64_t i = lo + tid; i < hi; i += 256) {
      float pi = p[i], mi = m[i], vi = v[i];
      adam_update(pi, g[i], mi, vi, s, clip);
      p[i] = pi, m[i] = mi, v[i] = vi;
      if (cp) cp[i] = pi;
    }
    return;
  }
  const int n4 = (int)((hi - lo) >> 2);  // (lo is a multiple of the slice: the alignment of the bases carries over)
  float4* p4 = reinterpret_cast<float4*>(p + lo);
  const float4* g4 = reinterpret_cast<const float4*>(g + lo);
  float4* m4 = reinterpret_cast<float4*>(m + lo);
  float4* v4 = reinterpret_cast<float4*>(v + lo);
  float4* c4 = cp ? reinterpret_cast<float4*>(cp + lo) : nullptr;
  for (int i = tid; i < n4; i += 256) {
    float4 pv = p4[i], mv = m4[i], vv = v4[i];
    const float4 gv = g4[i];
    adam_update(pv.x, gv.x, mv.x, vv.x, s, clip);
    adam_update(pv.y, gv.y, mv.y, vv.y, s, clip);
    adam_update(pv.z, gv.z, mv.z, vv.z, s, clip);
    adam_update(pv.w, gv.w, mv.w, vv.w, s, clip);
    p4[i] = pv, m4[i] = mv, v4[i] = vv;
    if (c4) c4[i] = pv;
  }
  const int64_t i = lo + 4 * (int64_t)n4 + tid;  // the tensor's last 1..3 elements
  if (i < hi) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update(pi, g[i], mi, vi, s, clip);
    p[i] = pi, m[i] = mi, v[i] = vi;
    if (cp) cp[i] = pi;
  }
}

// fixed-order sum of a workgroup's 256 doubles (no atomics anywhere on this path: bit-identical from run to run)
__device__ __forceinline__ double block_sum256(double x, double* red) {
  const int tid = threadIdx.x;
  red[tid] = x;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// partial[blockIdx.y * gridDim.x + blockIdx.x] = sum of squares of the workgroup's slice (0 for a spare workgroup)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamTable tab, double* __restrict__ partial) {
  __shared__ double red[256];
  int t;
  int64_t lo, hi;
  double acc = 0.0;
  if (adam_slice(tab, t, lo, hi)) {
    const float* __restrict__ g = tab.grad[t];
    const int tid = threadIdx.x;
    if (((uintptr_t)g & 15) != 0) {
      for (int64_t i = lo + tid; i < hi; i += 256) acc += (double)g[i] * (double)g[i];
    } else {
      const int n4 = (int)((hi - lo) >> 2);
      const float4* g4 = reinterpret_cast<const float4*>(g + lo);
      for (int i = tid; i < n4; i += 256) {
        const float4 q = g4[i];
        acc += ((double)q.x * (double)q.x + (double)q.y * (double)q.y) + ((double)q.z * (double)q.z + (double)q.w * (double)q.w);
      }
      const int64_t i = lo + 4 * (int64_t)n4 + tid;
      if (i < hi) acc += (double)g[i] * (double)g[i];
    }
  }
  const double total = block_sum256(acc, red);
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// One workgroup.  torch.nn.utils.clip_grad_norm_: clip_coef = min(1, max_norm / (total_norm + 1e-6)), in float.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ partial, int64_t n, float max_norm,
                                                                 float* __restrict__ total_norm, float* __restrict__ clip_coef) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const double total = block_sum256(acc, red);
  if (threadIdx.x == 0) {
    const float tn = (float)sqrt(total);
    *total_norm = tn;
    const float c = max_norm / (tn + 1e-6f);
    *clip_coef = max_norm > 0.f && c < 1.f ? c : 1.f;
  }
}

// Walks the tensor list into tables of at most kAdamTensors tensors / kAdamBlocks entries and hands each full table to
// `emit(table, entries)`; a tensor too long for the room left continues in the next table.
template <class Emit>
int for_each_table(const HoloAdamTensor* t, float* const* copies, int n, Emit emit) {
  AdamTable tab{};
  int nt = 0, nb = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t chunks = cdiv(t[i].numel, kAdamChunk);
    for (int64_t c = 0; c < chunks;) {
      if (nt == kAdamTensors || nb == kAdamBlocks) {
        if (const int rc = emit(tab, nb)) return rc;
        nt = nb = 0;
      }
      tab.param[nt] = t[i].param, tab.grad[nt] = t[i].grad, tab.exp_avg[nt] = t[i].exp_avg, tab.exp_avg_sq[nt] = t[i].exp_avg_sq;
      tab.copy[nt] = copies ? copies[i] : nullptr;
      tab.numel[nt] = t[i].numel;
      for (; c < chunks && nb < kAdamBlocks; ++c, ++nb) {
        tab.tensor[nb] = (uint8_t)nt;
        tab.chunk[nb] = (uint16_t)c;
      }
      ++nt;
    }
  }
  return nb ? emit(tab, nb) : 0;
}

int check_list(const char* who, const HoloAdamTensor* t, int n, bool need_state) {
  for (int i = 0; i < n; ++i) {
    if (t[i].numel < 0 || t[i].numel > (int64_t)kAdamChunk * 65535) {
      set_error("%s: tensor %d has %lld elements (0 .. %lld)", who, i, (long long)t[i].numel, (long long)kAdamChunk * 65535);
      return -1;
    }
    if (t[i].numel && (!t[i].grad || (need_state && (!t[i].param || !t[i].exp_avg || !t[i].exp_avg_sq)))) {
      set_error("%s: tensor %d has a null pointer", who, i);
      return -1;
    }
  }
  return 0;
}

}  // namespace

int adam_step_launch(const HoloAdamTensor* t, float* const* copies, int n, const AdamScalars& s, const float* clip_coef,
                     void* stream) {
  if (check_list("adam_step", t, n, true)) return -1;
  return for_each_table(t, copies, n, [&](const AdamTable& tab, int entries) {
    HOLO_LAUNCH(adam_multi_kernel, dim3((unsigned)entries, kAdamSplit), dim3(256), stream, tab, s, clip_coef);
    return 0;
  });
}

int64_t grad_norm_partials(const HoloAdamTensor* t, int n) {
  int64_t entries = 0;
  for (int i = 0; i < n; ++i) entries += t[i].numel > 0 ? cdiv(t[i].numel, kAdamChunk) : 0;
  return entries * kAdamSplit;
}

int grad_norm_launch(const HoloAdamTensor* t, int n, float max_norm, double* partial, float* total_norm, float* clip_coef,
                     void* stream) {
  if (check_list("grad_norm", t, n, false)) return -1;
  int64_t base = 0;
  const int rc = for_each_table(t, nullptr, n, [&](const AdamTable& tab, int entries) {
    HOLO_LAUNCH(grad_sumsq_kernel, dim3((unsigned)entries, kAdamSplit), dim3(256), stream, tab, partial + base);
    base += (int64_t)entries * kAdamSplit;
    return 0;
  });
  if (rc) return rc;
  HOLO_LAUNCH(grad_norm_finalize_kernel, dim3(1), dim3(256), stream, (const double*)partial, base, max_norm, total_norm,
              clip_coef);
  return 0;
}

}  // namespace holo
