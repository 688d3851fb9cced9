// conv_plan_check.cpp — the convolution planner (holo_diffusion_amd/csrc/conv_plan.cpp) swept on the CPU.
//
// A stand-alone program (its own main, no HIP, nothing loaded into Python), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_conv_plan_cpu.py:
//   conv_plan_check <golden table>      checks (a), (b), (c) below and that every kernel is chosen at least 20 times
//   conv_plan_check                     prints the table only
// It builds launches the way the denoiser's planner does (unet_plan.cpp: Planner::plan_conv / hand_over) over
//   compute mode 0 / 1 / 2 with the weight copies hand_over gives each mode; 1x1x1 stride 1, 3x3x3 stride 1 and 2; nearest x2
//   upsampling; grid edges 2 .. 64; 4 .. 384 channels of the first source alone and with an equal concat half; 4 .. 256
//   output channels; GroupNorm affine, SiLU, residual, fused 1x1x1 skip, offered qkv packing; batch 1 and 3, planned for the
//   batch and batch-invariant; 8 / 20 / 32 / 256 CUs; the default knobs and every forcing knob the GPU tests use,
// thinned by a fixed hash to a table below 256 KB, and prints one line per case: the inputs, then the plan
//   kernel tz nsplit chunks_per_split skip_chunks_per_split grid_x wino3_up qkv_sb qkv_rows scratch slabs exec_flops
// It asserts
//   (a) the lines equal the golden table (recorded from the commit BEFORE the planner moved here: see the recipe in
//       tests/test_conv_plan_cpu.py; a trailing " *" marks the launches that commit's launcher refused and that plan anew),
//   (b) conv_can_launch - what conv_launch asks before it launches anything - accepts every plan,
//   (c) the statistics slabs follow the chosen kernel's slab rule, and the scratch is nsplit * M * Cout * 4 bytes exactly when
//       the launch is split.
// What is NOT generated is what no caller may ask of any kernel (ConvParams): a concat whose seam is off a 32-channel chunk,
// SiLU without the affine, a fused skip anywhere but where the denoiser fuses one (3x3x3, stride 1, no upsampling, at least 64
// output channels, activated input, no residual, not the bf16x3 mode), upsampling other than of a 3x3x3 stride-1 convolution.
//
// -DCONV_PLAN_RECORD builds the same generator against a tree that still has the planner behind holo_kernels.h (with
// -DHOLO_EMU and that tree's tests/emu on the include path, linked to its libholo_emu.so); it prints the table only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#ifdef CONV_PLAN_RECORD
#include "holo_common.h"
#include "holo_kernels.h"
#else
#include "conv_plan.h"
#endif
#include "conv_weights.h"

using namespace holo;

namespace {

Knobs default_knobs() {
  Knobs k;
#define HOLO_KNOB_DEFAULT(field, env, kind, dflt, when, doc) k.field = knob_##kind(nullptr, dflt);
  HOLO_KNOBS(HOLO_KNOB_DEFAULT)
#undef HOLO_KNOB_DEFAULT
  return k;
}

struct KnobSet {
  const char* name;
  int64_t Knobs::*field;
  int64_t value;
  int mode, kind;  // the launches it bears on: compute mode (-1: all), kind (below)
};
// kinds: 0 = 1x1x1 stride 1, 1 = 3x3x3 stride 1, 2 = 3x3x3 stride 2
const KnobSet KNOBS[] = {
    {"-", nullptr, 0, -1, -1},
    {"bf16t0", &Knobs::conv_bf16t, 0, 1, 1},
    {"bf16t1", &Knobs::conv_bf16t, 1, 1, 1},
    {"bf16p0", &Knobs::conv_bf16p, 0, 1, 1},
    {"bf16p1", &Knobs::conv_bf16p, 1, 1, 1},
    {"bf16p2", &Knobs::conv_bf16p, 2, 1, 1},
    {"s2t0", &Knobs::conv_s2t, 0, 1, 2},
    {"s2t1", &Knobs::conv_s2t, 1, 1, 2},
    {"tz2", &Knobs::conv_force_tz2, 1, -1, 1},
    {"winosmall0", &Knobs::conv_wino_small, 0, 0, 1},
    {"wino3-0", &Knobs::conv_wino3, 0, 0, 1},
    {"wino3up0", &Knobs::conv_wino3_up, 0, 0, 1},
    {"small0", &Knobs::conv1x1_small, 0, 0, 0},
    {"stream0", &Knobs::conv1x1_stream_min_m, 0, 0, 0},
    {"qkv0", &Knobs::conv_qkv_fused, 0, 1, 0},
    {"bf16stream0", &Knobs::conv1x1_bf16_stream, 0, 1, 0},
};

struct Case {
  int mode, kind, ups, R, C0, C1, Cout, coef, act, residual, skip, qkv, N, plan_n, cus, knob;
};

uint32_t mix(uint32_t x) {  // (a fixed integer hash: the thinning is the same everywhere)
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x;
}

template <class T>
T* fake(uintptr_t a) {  // never dereferenced: the planner looks at which operands EXIST
  return reinterpret_cast<T*>(a);
}

// the launch as Planner::plan_conv / hand_over (unet_plan.cpp) build it
ConvParams make_params(const Case& c, const Knobs& k) {
  ConvParams p;
  memset(&p, 0, sizeof p);
  const int ksz = c.kind == 0 ? 1 : 3, stride = c.kind == 2 ? 2 : 1;
  const int Cin = c.C0 + c.C1;
  const bool bfs = c.mode == 1;  // bf16 storage of the activations
  const int64_t V = (int64_t)(c.R / stride) * (c.R / stride) * (c.R / stride);
  // (the attention internals stay fp32: qkv is written fp32, and below 1024 tokens the fp32 attention feeds proj_out; so does
  // the head convolution's output)
  const bool out_f32 = (c.kind == 0 && c.coef && !c.act && !c.residual) || (c.kind == 1 && c.Cout < 32);
  const bool in_f32 = c.kind == 0 && c.residual && !c.coef && V < 1024;
  p.in_bf16 = bfs && !in_f32, p.res_bf16 = bfs, p.out_bf16 = bfs && !out_f32;
  p.src0 = fake<const float>(0x1000);
  p.src1 = c.C1 ? fake<const float>(0x2000) : nullptr;
  p.C0 = c.C0, p.C1 = c.C1;
  p.N = c.N;
  p.ID = p.IH = p.IW = c.R;
  p.ups = c.ups;
  p.OD = p.OH = p.OW = c.R / stride;
  p.stride = stride, p.pad = ksz == 3 ? 1 : 0, p.ksz = ksz;
  p.Cout = c.Cout;
  auto hand_over = [&](const ConvWeightLayout& l, bool skip) {
    const ConvCopies cc = forward_copies(l, skip, k);
    const bool bf = c.mode != 0, wino = c.mode == 0;
    (skip ? p.skip_w : p.w) = fake<const float>(0x3000);
    (skip ? p.skip_w_bf : p.w_bf) = bf && cc.bf16 ? fake<const uint16_t>(0x4000) : nullptr;
    (skip ? p.skip_w_bft : p.w_bft) = bf && cc.bf16 ? fake<const uint16_t>(0x5000) : nullptr;
    (skip ? p.skip_w_wino2 : p.w_wino2) = wino && cc.wino2 ? fake<const float>(0x6000) : nullptr;
    (skip ? p.skip_w_wino3 : p.w_wino3) = wino && cc.wino3 ? fake<const float>(0x7000) : nullptr;
    (skip ? p.skip_CinP : p.CinP) = l.CinP;
  };
  const ConvWeightLayout l = conv_weight_layout(c.Cout, Cin, ksz * ksz * ksz);
  p.CoutP = l.CoutP;
  hand_over(l, false);
  p.bf16 = c.mode;
  p.coef = c.coef ? fake<const float>(0x8000) : nullptr;
  p.act = c.act;
  p.bias = fake<const float>(0x9000);
  p.residual = c.residual ? fake<const float>(0xa000) : nullptr;
  p.out = fake<float>(0xb000);
  if (c.skip) {  // the block input [x0 | x1] of a ResBlock whose second convolution this is: as wide as this launch's input is not
    p.skip_src0 = fake<const float>(0xc000);
    p.skip_C0 = c.C0 == c.Cout ? c.C0 / 2 : c.C0;  // (a skip connection exists where the widths differ)
    p.skip_src1 = c.C1 ? fake<const float>(0xd000) : nullptr;
    p.skip_C1 = c.C1 ? p.skip_C0 : 0;
    hand_over(conv_weight_layout(c.Cout, p.skip_C0 + p.skip_C1, 1), true);
    p.skip_bias = fake<const float>(0xe000);
    // (the launch's own input is the first convolution's output: one source of Cout channels)
    p.C0 = c.Cout, p.C1 = 0, p.src1 = nullptr;
    const ConvWeightLayout l2 = conv_weight_layout(c.Cout, c.Cout, 27);
    hand_over(l2, false);
  }
  if (c.qkv) {
    const int CH = (c.C0 % 64) == 0 && (c.R & 8) ? 64 : 32;
    p.qkv_q = fake<uint16_t>(0xf000), p.qkv_k = fake<uint16_t>(0xf100), p.qkv_vt = fake<uint16_t>(0xf200);
    p.qkv_scale = 1.f, p.qkv_T = (int)V, p.qkv_CH = CH, p.qkv_H = c.C0 / CH;
  }
  return p;
}

int failures = 0;
void fail(const std::string& line, const char* what) {
  if (++failures <= 20) printf("FAIL %s: %s\n", what, line.c_str());
}

}  // namespace

int main(int argc, char** argv) {
  const int Rs[] = {2, 4, 6, 8, 12, 16, 24, 32, 64};
  const int C0s[] = {4, 32, 36, 64, 96, 128, 160, 192, 256, 384};
  const int Couts[] = {4, 32, 36, 64, 96, 128, 192, 256};
  const int CUs[] = {8, 20, 32, 256};
  const Knobs dflt = default_knobs();
  std::vector<std::string> lines;
  std::map<int, int> chosen;
  uint32_t counter = 0;
  for (int mode = 0; mode < 3; ++mode)
    for (int kind = 0; kind < 3; ++kind)
      for (int ups = 0; ups <= (kind == 1 ? 1 : 0); ++ups)
        for (int R : Rs)
          for (int C0 : C0s)
            for (int cat = 0; cat <= ((C0 % 32) == 0 ? 1 : 0); ++cat)
              for (int Cout : Couts)
                for (int flags = 0; flags < 32; ++flags) {
                  Case c;
                  c.mode = mode, c.kind = kind, c.ups = ups, c.R = R, c.C0 = C0, c.C1 = cat ? C0 : 0, c.Cout = Cout;
                  c.coef = flags & 1, c.act = (flags >> 1) & 1, c.residual = (flags >> 2) & 1, c.skip = (flags >> 3) & 1;
                  c.qkv = (flags >> 4) & 1;
                  if (c.act && !c.coef) continue;
                  if (c.skip && !(kind == 1 && !ups && Cout >= 64 && mode != 2 && c.act && !c.residual)) continue;
                  if (c.qkv && !(kind == 0 && mode == 1 && c.coef && !c.act && !c.residual && !cat && (C0 % 32) == 0)) continue;
                  if (c.qkv) c.Cout = 3 * C0;
                  if (c.qkv && Cout != Couts[0]) continue;  // (one qkv width per input width)
                  for (int N : {1, 3})
                    for (int plan_n = 0; plan_n <= (N > 1 ? 1 : 0); ++plan_n)
                      for (int cus : CUs)
                        for (int kn = 0; kn < (int)(sizeof KNOBS / sizeof KNOBS[0]); ++kn) {
                          const KnobSet& ks = KNOBS[kn];
                          if ((ks.mode >= 0 && ks.mode != mode) || (ks.kind >= 0 && ks.kind != kind)) continue;
                          // thinning: one case in `keep`, more of the launches only few kernels take (large raw 1x1x1 grids,
                          // offered qkv packing, stride 2 on bf16 storage, exact-fp32 attention convolutions)
                          int keep = kn == 0 ? 9000 : 7000;
                          const bool plain = !c.coef && !c.residual && !cat, c32 = (C0 % 32) == 0 && (Cout % 32) == 0;
                          if (kind == 1 && (R % 8) == 0 && (C0 % 16) == 0) keep = kn == 0 ? 1200 : 950;  // (the halo forms)
                          if (kind == 0 && mode == 0 && R == 64 && plain) keep = 16;
                          if (c.qkv) keep = 6;
                          if (kind == 2 && mode == 1 && R >= 16 && plain && (C0 % 16) == 0 && (Cout % 64) == 0) keep = 20;
                          if (kind == 0 && mode != 2 && (R % 8) == 0 && R <= 32 && !cat && c32 && (c.residual || (c.coef && !c.act)) && !c.qkv)
                            keep = 110;
                          if (mix(counter++) % keep) continue;
                          c.N = N, c.plan_n = plan_n, c.cus = cus, c.knob = kn;
                          Knobs k = dflt;
                          if (ks.field) k.*(ks.field) = ks.value;
                          ConvParams p = make_params(c, k);
                          const bool offered = p.qkv_q != nullptr;
                          const size_t scratch = conv_plan(p, cus, k, plan_n);
                          if (scratch) p.partial = fake<float>(0x10000);
                          const int slabs = conv_stats_slabs(p);
                          if (slabs > 0) p.stats = fake<double>(0x20000);  // (as Planner::emit_conv: only where the launch writes them)
                          char buf[256];
                          snprintf(buf, sizeof buf, "m%d k%ds%du%d R%d c%d+%d>%d f%d%d%d%d%d n%dp%d cu%d %s | %d %d %d %d %d %d %d %d %d %zu %d %.17g",
                                   mode, p.ksz, p.stride, ups, R, c.C0, c.C1, c.Cout, c.coef, c.act, c.residual, c.skip, c.qkv, N, plan_n,
                                   cus, ks.name, (int)p.kernel, p.tz, p.nsplit, p.chunks_per_split, p.skip_chunks_per_split, p.grid_x,
                                   p.wino3_up, p.qkv_sb, p.qkv_rows, scratch, slabs, conv_exec_flops(p));
                          const std::string line = buf;
                          lines.push_back(line);
                          ++chosen[(int)p.kernel];
                          // (c) scratch and slabs
                          const int64_t V = (int64_t)p.OD * p.OH * p.OW, M = p.N * V;
                          if (p.nsplit < 1 || scratch != (p.nsplit > 1 ? (size_t)p.nsplit * M * p.Cout * 4 : 0)) fail(line, "scratch");
                          if (offered && p.kernel != ConvKernel::Qkv && p.qkv_q) fail(line, "qkv packing left offered");
                          int64_t want = 0;  // slabs per sample of an un-split launch: V over the voxels of one slab, when that divides
                          int64_t per = 0;
                          switch (p.kernel) {
                            case ConvKernel::Bf16Wide:
                            case ConvKernel::Bf16Persistent: per = 512; break;
                            case ConvKernel::Halo:
                            case ConvKernel::Wino2:
                            case ConvKernel::Wino3: per = 64 * p.tz; break;
                            case ConvKernel::RowTile: per = 64; break;
                            case ConvKernel::S2Bf16: per = 128; break;
                            case ConvKernel::Bf16Stream1x1: per = p.qkv_rows; break;
                            case ConvKernel::Small1x1: per = 16; break;
                            default: break;
                          }
                          if (per > 0 && V % per == 0) want = V / per;
                          if (p.kernel == ConvKernel::Halo && p.bf16 == 2 && p.Cout >= 64) want = V / 32;  // (bf16x3: per half 8 x 8 slab)
                          else if ((p.kernel == ConvKernel::Halo || p.kernel == ConvKernel::Wino2) && p.Cout < 64) want *= 2;  // (two wave rows)
                          if (per > 0 && p.kernel != ConvKernel::RowTile && V % per) fail(line, "slab does not divide the sample");
                          if (p.nsplit > 1 ? (slabs < 1 || slabs > 256) : slabs != want) fail(line, "slabs");
#ifndef CONV_PLAN_RECORD
                          // (b) the launcher's one check
                          if (!conv_can_run(p.kernel, p)) fail(line, "the chosen kernel cannot run the launch");
                          else if (!conv_can_launch(p)) fail(line, "the launcher refuses the plan");
#endif
                        }
                }
  if (argc < 2) {
    for (const std::string& l : lines) puts(l.c_str());
    return failures ? 1 : 0;
  }
#ifndef CONV_PLAN_RECORD
  // (a) the golden table
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    printf("cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<std::string> golden;
  char row[512];
  while (fgets(row, sizeof row, f)) {
    std::string s = row;
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    golden.push_back(s);
  }
  fclose(f);
  int marked = 0;
  if (golden.size() != lines.size()) {
    printf("FAIL: %zu cases, the golden table has %zu\n", lines.size(), golden.size());
    ++failures;
  } else {
    for (size_t i = 0; i < lines.size(); ++i) {
      const bool star = golden[i].size() > 2 && golden[i].compare(golden[i].size() - 2, 2, " *") == 0;
      marked += star;
      if ((star ? golden[i].substr(0, golden[i].size() - 2) : golden[i]) != lines[i]) {
        fail(lines[i], "differs from the golden table");
        if (failures <= 20) printf("     golden: %s\n", golden[i].c_str());
      }
    }
  }
  const ConvKernel all[] = {ConvKernel::Gather, ConvKernel::Halo, ConvKernel::RowTile, ConvKernel::Wino2, ConvKernel::Bf16Wide,
                            ConvKernel::Wino3, ConvKernel::Stream1x1, ConvKernel::Bf16Persistent, ConvKernel::S2Bf16,
                            ConvKernel::Qkv, ConvKernel::Bf16Stream1x1, ConvKernel::Small1x1};
  for (ConvKernel kk : all) {
    printf("%-28s %5d cases\n", conv_kernel_name(kk), chosen[(int)kk]);
    if (chosen[(int)kk] < 20) {
      printf("FAIL: %s chosen fewer than 20 times\n", conv_kernel_name(kk));
      ++failures;
    }
  }
  printf("%zu cases, %d marked as planned anew\n", lines.size(), marked);
  if (failures) {
    printf("conv_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  printf("conv_plan_check: OK\n");
#endif
  return 0;
}
