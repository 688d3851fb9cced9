// rowtile_probe — where a launch of conv_small_kernel (the row-tile convolution) spends its time (development probe, not part
// of the library).  Two launches of the north-star denoiser:
//   * the 4^3 512 -> 512 3x3x3 convolution with GroupNorm + SiLU on load (split-K, 432 workgroups, cold weights cycled);
//   * the 64^3 -> 32^3 Downsample convolution, 64 -> 64, stride 2, raw input (512 workgroups, 7 staging groups each).
// Linked against the production kernels_conv.o it times the launches (hipEvents, conv + reduce where split).  Linked against
// a kernels_conv.o built with -DHOLO_ROWTILE_PROBE (and itself built with -DROWTILE_STAMPS) it reads the kernel's phase
// stamps instead: shader cycles of wave 0 per workgroup and phase, as mean over the workgroups.  The stamps fence the
// scheduler: read that build's SHARES, never its run time.
// Build (from the repository root, after `make -C holo_diffusion_amd/csrc`):
//   O=holo_diffusion_amd/csrc; H="hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950"
//   L="$O/kernels_conv3.o $O/kernels_conv_bf16p.o $O/kernels_conv_s2.o $O/kernels_conv1x1_bf16.o $O/kernels_misc.o $O/conv_plan.o"
//   $H -c tools/rowtile_probe.cpp -o /tmp/rt.o && hipcc --offload-arch=gfx950 /tmp/rt.o $O/kernels_conv.o $L -o tools/rowtile_probe
//   $H -DHOLO_ROWTILE_PROBE -I$O -c $O/kernels_conv.hip -o /tmp/kc_stamps.o && $H -DROWTILE_STAMPS -c tools/rowtile_probe.cpp -o /tmp/rts.o
//   hipcc --offload-arch=gfx950 /tmp/rts.o /tmp/kc_stamps.o $L -o tools/rowtile_probe_stamps
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../holo_diffusion_amd/csrc/holo_kernels.h"
namespace holo {
void set_error(const char* fmt, ...) {
  va_list a;
  va_start(a, fmt);
  vprintf(fmt, a);
  va_end(a);
  printf("\n");
}
}  // namespace holo
using namespace holo;
#define CK(x)                                                         \
  do {                                                                \
    hipError_t e = (x);                                               \
    if (e != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

static float* dev_random(size_t n, float scale) {
  std::vector<float> h(n);
  for (auto& x : h) x = (rand() % 2001 - 1000) * 1e-3f * scale;
  float* d;
  CK(hipMalloc(&d, n * 4));
  CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}

static void run(const char* name, int Cin, int Cout, int RI, int stride, bool act, int iters) {
  const int RO = RI / stride;
  const ConvWeightLayout L = conv_weight_layout(Cout, Cin, 27);
  const size_t wfloats = (size_t)L.f32_floats();
  const int NW = (wfloats * 4 > (1u << 20)) ? 16 : 1;  // large weight sets are cycled past the memory-side cache
  std::vector<float*> w(NW);
  for (int i = 0; i < NW; ++i) w[i] = dev_random(wfloats, 0.1f);
  float* src = dev_random((size_t)RI * RI * RI * Cin, 1.f);
  float* bias = dev_random(Cout, 0.1f);
  float* coef = nullptr;
  if (act) {
    std::vector<float> hc((size_t)Cin * 2);
    for (int c = 0; c < Cin; ++c) hc[2 * c] = 1.f + 0.01f * (c % 7), hc[2 * c + 1] = 0.01f * (c % 5) - 0.02f;
    CK(hipMalloc(&coef, hc.size() * 4));
    CK(hipMemcpy(coef, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
  }
  float* out;
  CK(hipMalloc(&out, (size_t)RO * RO * RO * Cout * 4));
  ConvParams p{};
  p.src0 = src, p.C0 = Cin, p.N = 1, p.ID = p.IH = p.IW = RI, p.OD = p.OH = p.OW = RO, p.stride = stride, p.pad = 1, p.ksz = 3;
  p.Cout = Cout, p.w = w[0], p.CoutP = L.CoutP, p.CinP = L.CinP, p.out = out, p.coef = coef, p.act = act ? 1 : 0, p.bias = bias;
  Knobs k = Knobs::from_env();
  const size_t sb = conv_plan(p, 256, k);
  if (sb) CK(hipMalloc((void**)&p.partial, sb));
  const int64_t M = (int64_t)RO * RO * RO;
  const int wgs = (int)((M + 63) / 64) * ((Cout + 63) / 64) * p.nsplit;
  printf("%s: %d^3 -> %d^3, %d -> %d channels%s: kernel %s, split-K %d x %d chunks, %d workgroups\n", name, RI, RO, Cin, Cout,
         act ? ", GroupNorm + SiLU on load" : ", raw input", conv_kernel_name(p.kernel), p.nsplit, p.chunks_per_split, wgs);
  if (p.kernel != ConvKernel::RowTile) {
    printf("  not planned on the row-tile kernel: skipped\n");
    return;
  }
#ifdef ROWTILE_STAMPS
  (void)iters;
  CK(hipMalloc((void**)&p.dbg, (size_t)wgs * 64));
  for (int i = 0; i < 4; ++i) {
    p.w = w[i % NW];
    CK(hipMemset(p.dbg, 0, (size_t)wgs * 64));
    if (conv_launch(p, nullptr)) exit(1);
    CK(hipDeviceSynchronize());
  }
  std::vector<unsigned long long> d((size_t)wgs * 8);
  CK(hipMemcpy(d.data(), p.dbg, d.size() * 8, hipMemcpyDeviceToHost));
  static const char* seg[7] = {"prologue", "issue of the requests", "wait for the activations", "activation + commit",
                               "barrier + weights' arrival", "MFMAs", "epilogue"};
  double mean[8] = {0}, total = 0;
  for (int b = 0; b < wgs; ++b)
    for (int s = 0; s < 8; ++s) mean[s] += (double)d[(size_t)b * 8 + s] / wgs;
  for (int s = 0; s < 7; ++s) total += mean[s];
  printf("  shader cycles of wave 0, mean over %d workgroups (%.2f staging groups each); about 40 per stamp are the stamp's own\n", wgs,
         mean[7]);
  for (int s = 0; s < 7; ++s)
    printf("    %-28s %9.0f  %5.1f %%%s\n", seg[s], mean[s], 100.0 * mean[s] / total,
           s >= 1 && s <= 5 && mean[7] > 0 ? "" : "");
  printf("    %-28s %9.0f\n", "sum", total);
  if (mean[7] > 0)
    printf("  per staging group: requests %.0f | wait %.0f | activation + commit %.0f | barrier + weights %.0f | MFMAs %.0f\n",
           mean[1] / mean[7], mean[2] / mean[7], mean[3] / mean[7], mean[4] / mean[7], mean[5] / mean[7]);
#else
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int i = 0; i < 8; ++i) {
    p.w = w[i % NW];
    if (conv_launch(p, nullptr)) exit(1);
  }
  CK(hipDeviceSynchronize());
  float best = 1e30f, sum = 0.f;
  const int reps = 5;
  for (int r = 0; r < reps; ++r) {
    CK(hipEventRecord(e0));
    for (int i = 0; i < iters; ++i) {
      p.w = w[i % NW];
      conv_launch(p, nullptr);
    }
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    best = ms < best ? ms : best;
    sum += ms;
  }
  printf("  %.2f us per launch%s (best of %d x %d launches; mean %.2f)\n", best * 1e3 / iters, p.nsplit > 1 ? " + reduce" : "", reps,
         iters, sum * 1e3 / iters / reps);
#endif
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  const int iters = argc > 1 ? atoi(argv[1]) : 64;
  run("deep level", 512, 512, 4, 1, true, iters);
  run("Downsample", 64, 64, 64, 2, false, iters);
  return 0;
}
