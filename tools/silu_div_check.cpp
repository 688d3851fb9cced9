// silu_div_check — the row-tile convolution's SiLU over ALL 2^32 bit patterns of its argument: the form the kernel runs
// (rowtile_silu.h: inside the range test the shortened division, outside it the IEEE sequence) against the plain expression
// v / (1 + exp(-v)), bit for bit, a NaN equal to any NaN.  Prints the number of differing inputs; exit status 1 if there is
// one.  tests/test_gpu_rowtile_bits.py builds and runs it.
// Build: hipcc -O3 --offload-arch=gfx950 -Iholo_diffusion_amd/csrc tools/silu_div_check.cpp -o tools/silu_div_check
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "rowtile_silu.h"

using namespace holo;

__device__ __forceinline__ bool same_bits(float a, float b) {
  return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

__global__ __launch_bounds__(256) void check_kernel(unsigned long long* out) {
  // out[0] differing inputs, out[1] inputs inside the range, out[2] a differing bit pattern + 1
  unsigned long long diff = 0, inside = 0, first = 0;
  const unsigned base = (blockIdx.x * 256u + threadIdx.x) * 256u;
  for (unsigned i = 0; i < 256u; ++i) {
    const unsigned bits = base + i;
    const float v = __uint_as_float(bits);
    const float want = silu_f(v);
    const bool in = silu_in_range(v);
    const float got = in ? silu_div_core(v, silu_den(v)) : silu_f(v);
    if (!same_bits(got, want)) {
      ++diff;
      if (!first) first = (unsigned long long)bits + 1;
    }
    if (in) ++inside;
  }
  if (diff) atomicAdd(out + 0, diff);
  if (inside) atomicAdd(out + 1, inside);
  if (first) atomicMax(out + 2, first);
}

int main() {
  unsigned long long* d = nullptr;
  unsigned long long h[3] = {0, 0, 0};
  if (hipMalloc(&d, sizeof(h)) != hipSuccess || hipMemset(d, 0, sizeof(h)) != hipSuccess) {
    printf("no device memory\n");
    return 2;
  }
  hipLaunchKernelGGL(check_kernel, dim3(65536), dim3(256), 0, nullptr, d);  // 65536 x 256 x 256 = 2^32 inputs
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) {
    printf("the check kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
    return 2;
  }
  printf("inputs 4294967296 inside_range %llu differing %llu", h[1], h[0]);
  if (h[2]) printf(" a_differing_input 0x%08llx", h[2] - 1);
  printf("\n");
  return h[0] ? 1 : 0;
}
