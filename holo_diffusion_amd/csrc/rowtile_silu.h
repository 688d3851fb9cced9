// rowtile_silu.h — SiLU with the correctly rounded quotient, as the row-tile convolution applies it while staging
// (kernels_conv.hip), in a header of its own so that tools/silu_div_check.cpp can run both forms over every float.
//
//   silu(v) = v / d,  d = 1 + exp(-v)
//
// silu_f is the plain expression: hipcc expands the division into the IEEE sequence - v_div_scale x 2, v_rcp, six
// multiply-adds (a Newton step on the reciprocal, the quotient, two residual corrections), v_div_fmas, v_div_fixup: 11
// instructions.  The two scale steps and the fix-up only act outside a range: v_div_scale leaves numerator and denominator
// alone unless one of them is zero, infinite, NaN or denormal, the exponents differ by 96 or more, the reciprocal or the
// quotient is denormal, or the numerator is below 2^-103; v_div_fmas with no scale pending is a plain multiply-add, and
// v_div_fixup passes a finite quotient of normal operands through.  With 2^-60 <= |v| <= 64 the denominator lies in
// [1, 2^93) and the quotient above 2^-94, so none of that applies: the multiply-adds alone compute the same bits.  On this
// range the second residual correction never changes the quotient either - that is no theorem, it is the count of
// tools/silu_div_check.cpp over all 2^32 inputs (0 differing, on gfx950's v_rcp_f32 and v_exp_f32), which
// tests/test_gpu_rowtile_bits.py repeats with every run of the suite - so silu_div_core is reciprocal, Newton step, quotient
// and ONE residual correction: 6 instructions.  silu_in_range is the range test, made on the whole wave by the caller, with
// silu_f as the other path.
#pragma once

#include "holo_common.h"

namespace holo {

constexpr float SILU_FAST_MIN = 8.6736174e-19f;  // 2^-60
constexpr float SILU_FAST_MAX = 64.0f;

__device__ __forceinline__ float silu_den(float v) { return 1.0f + __expf(-v); }
__device__ __forceinline__ float silu_f(float v) { return v / silu_den(v); }

// v / d for 2^-60 <= |v| <= 64, d = silu_den(v): the multiply-adds of the IEEE sequence up to the first residual correction
__device__ __forceinline__ float silu_div_core(float v, float d) {
#ifdef HOLO_EMU
  return v / d;
#else
  float r = __builtin_amdgcn_rcpf(d);
  const float e = __builtin_fmaf(-d, r, 1.0f);
  r = __builtin_fmaf(e, r, r);
  const float q = v * r;
  return __builtin_fmaf(__builtin_fmaf(-d, q, v), r, q);
#endif
}
// (as the kernel folds it over a chunk's values with v_max3 / v_min3, which skip a NaN: a NaN goes either way and stays one)
__device__ __forceinline__ bool silu_in_range(float v) {
  return fmaxf(fabsf(v), 0.f) <= SILU_FAST_MAX && fminf(fabsf(v), SILU_FAST_MAX) >= SILU_FAST_MIN;
}

}  // namespace holo
