// unet_plan_check.cpp — the denoiser's planners (holo_diffusion_amd/csrc/unet_plan.cpp, unet_train_plan.cpp) swept on the CPU:
// what a plan launches, that no launch reads memory another launch was allowed to overwrite, and that the backward of a
// training plan neither overwrites nor forgets a gradient.
//
// A stand-alone program (its own main, no HIP, nothing loaded into Python), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_unet_plan_cpu.py:
//   unet_plan_check <forward table> <training table>   checks (a) .. (f) and the coverage conditions below
//   unet_plan_check                   prints the table of the forward plans only
//   unet_plan_check --train           prints the table of the training plans only
//   unet_plan_check --self-test       damages one good forward plan and one good training plan in two ways each and asserts that
//                                     (c), (d) and (f) name exactly the damaged ops
// The workspace and the three parameter stores are made-up addresses that are never dereferenced, so 128^3 nets cost nothing.
//
// THE SWEEP: the nets of tests/test_gpu_unet.py (with the north-star and the plumb net), test_gpu_unet_grid_sizes.py,
// test_gpu_unet_channel_widths.py, test_gpu_cu_counts.py and the 128^3 bf16 side workload's net, crossed with compute mode
// 0 / 1 / 2, batch 1 / 2 / 4, batch-invariant on / off (exact fp32), 8 / 20 / 32 / 256 CUs, the default knobs and the
// planner-level knobs the tests force (KNOBS below), and the forward of a training plan (tape set, arena keeping everything);
// thinned by a fixed hash, but for every knob set on nets where it bites, to about 210 plans and a table of about 60 KB.  Every plan of the sweep prints one line
//   <case> | bytes n_joins first_conv last_conv cl_refusal err n_ops <FNV-1a hash of its op lines> | block_outputs offsets
// and one small plan (the one-level net c4-to-36, exact fp32) prints its op lines too: kind, side / fork / join and every field of the op's parameter struct,
// pointers as offsets into the workspace (w+) or the f32 / bf16 / Winograd parameter store (f+ / b+ / v+).
//
// It asserts
//   (a) the lines equal the golden table (recorded from the commit BEFORE the planner moved into unet_plan.cpp: the recipe
//       is in tests/test_unet_plan_cpu.py);
//   (b) releasing memory changes nobody's producer: every inference plan is built a second time with the arena keeping
//       everything; the two op lists agree in everything but addresses, and for every operand an op reads the ops that last
//       wrote it are the same in both (in the keeping plan every buffer has an address of its own, so there they are
//       unambiguous);
//   (c) one launch's buffers: what an op writes (partial, stats, out, ...) is pairwise disjoint and disjoint from what it
//       reads; residual == out is the one allowed alias;
//   (d) the side lane: no main-lane op between the fork and the consumer that waits for a side op's join writes a range that
//       side op touches or reads a range it writes;
//   (e) every workspace range an op reads is covered by the writes of earlier ops, every range lies in [0, plan.bytes), and
//       the small region stays inside small_cap;
//   every plan is also built on NO workspace, as a sizing pass (under UBSan: no arithmetic on a null pointer): Plan::sizing is
//   set there alone, and bytes and the ops but for their addresses equal the placed plan's; and every knob set of KNOBS
//   changes at least one plan of the sweep against the default knobs.  When a plan line differs from the golden table, the
//   plan's op lines are printed.
// The footprint of an op - the ranges it reads and writes - is derived from the op's own fields (footprint()), never from
// the planner's Act records; a conv's statistics slabs come from conv_stats_slabs and its scratch from conv_plan re-run on a
// copy of its parameters.  The program fails on an op kind without a footprint and on a non-null workspace pointer of an op
// that lies in none of its declared ranges.
// COVERAGE is a condition: the sweep must hold plans with a side lane, the packed bf16 attention, the GEMM / softmax
// attention, split key ranges in the fp32 flash kernel, a split-K convolution that writes statistics, a fused skip, a
// separate 1x1x1 skip, an Upsample, a Downsample, a batch-invariant batch > 1 and a tape.
//
// TRAINING PLANS (TrainPlanner, fp32 only): the nets of tests/test_gpu_backward.py (tiny, wide = u8, deep), the plumbing and
// north-star nets, g12-6-3, g24-12 and two nets of the channel-width file, crossed with batch 1 / 2, 256 / 8 / 20 / 32 CUs and
// the default knobs, HOLO_DGRAD_S2_DIRECT=1, HOLO_WGRAD_TILES=1 and HOLO_WGRAD_REDUCE_TILE_MIN=1: 288 plans, a table of about
// 90 KB.  The transposed weights are a table on made-up addresses as holo_unet_set_dgrad_weight makes it (make_dgrad).  Every
// plan prints
//   train <case> | bytes gy_off gx_off <hash of grad_off> n_bops <hash of its backward op lines> err
// every (net, batch) also the line of its sizing pass on NO transposed weights (what holo_unet_backward_workspace_bytes
// plans before any was supplied; every pointer masked), and one small plan (c36-to-4) its backward op lines: the name of
// the launcher and every argument it is called with (bl_*).  A training plan is checked as ONE timeline: its taped forward
// ops, a pseudo-op that writes gy_off (the layout pass of grad_out), the backward ops, a pseudo-op that reads gx_off.  Each
// backward kind has a footprint from its own fields (bwd_footprint; wgrad_plan is re-run on the op's parameters).  Declared
// in-place aliases: a conv with residual == out, the acc* destinations (read and written), softmax and attn_ds.  Asserted:
//   (a) the lines equal the second golden table (recorded from the commit whose backward launches were closures: recipe in
//       tests/test_unet_plan_cpu.py);
//   (c) as above, over the whole timeline: e.g. wgrad partial vs gy vs sources, gn_bwd part / grp / gx0 / gx1 / ga;
//   (e) as above: every range a backward op reads was written by an earlier op of the forward or the backward (an
//       accumulating op reads its destination), inside [0, bytes);
//   (f) gradient accounting: a non-accumulating write is the first backward write to its range (declared exceptions: the
//       attention's one transposition scratch, and the q / k / v gradient GEMMs that interleave in one tensor, whose rows are
//       compared exactly); no backward op writes what a forward op wrote; by the end every parameter's
//       [grad_off, + numel * 4) and the input gradient are written (emb_layers rows through the concatenated matrices);
//   the sizing pass with the same transposed weights gives the same bytes, offsets and ops but for addresses; every knob set
//   changes some training plan; and the sweep holds a concat ResBlock with a conv skip (split_cat), a ResBlock with an
//   identity skip, an attention block, a Downsample on the zero-insert route and one on conv_dgrad_s2, an Upsample, the head,
//   both wgrad kernels and the tile reduce, a split-K dgrad and a dgrad on a Winograd copy.
// What it cannot see: data.  A kernel that ignores its acc flag, or a launcher that reads other fields than the footprint
// assumes, passes here; the GPU parity tests are for that.
//
// -DUNET_PLAN_RECORD: the including file has brought a tree's planner in already (a `Desc` type that Planner takes, and
// set_cus; for the training plans record_train and recording stand-ins of the backward's launchers); the program then runs
// on that planner and prints tables only.  That is how the golden tables are recorded from the parent commit.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#ifndef UNET_PLAN_RECORD
#include "unet_train_plan.h"
typedef holo::unetplan::UnetDesc Desc;
static void set_cus(Desc& d, int cus) { d.num_cus = cus; }
using namespace holo::unetplan;
#endif

using namespace holo;

namespace {

// ---- the sweep -------------------------------------------------------------------------------------------------------
struct NetCfg {
  const char* name;
  int R, cin, cout, mc, nrb;
  std::vector<int> mult, attn;
  int heads;
};
const NetCfg NETS[] = {
    // tests/test_gpu_unet.py
    {"u8", 8, 16, 16, 64, 2, {1, 2}, {2}, 2},
    {"u16", 16, 16, 16, 64, 2, {1, 2, 2}, {4}, 2},
    {"u16n", 16, 16, 16, 32, 2, {1, 1}, {}, 2},
    {"u16p", 16, 16, 16, 64, 2, {1, 2}, {}, 2},
    {"u8d", 8, 16, 16, 64, 2, {1, 2, 2}, {2}, 2},
    {"u16s", 16, 16, 16, 64, 1, {1, 2}, {}, 2},
    {"u16a", 16, 16, 16, 64, 2, {1, 2, 2}, {1, 2}, 2},
    {"u16w", 16, 16, 16, 128, 2, {1, 2}, {2}, 2},
    {"u16h", 16, 16, 16, 128, 1, {1, 2}, {2}, 4},
    {"u16t", 16, 16, 16, 64, 1, {1, 2}, {1}, 2},
    {"u32", 32, 16, 16, 64, 2, {1, 2, 2}, {}, 2},
    {"dflt", 32, 128, 128, 128, 2, {1, 2, 4, 8}, {8, 16}, 2},
    {"u64l", 64, 32, 32, 64, 1, {1, 1, 1}, {}, 2},
    {"u16k", 16, 16, 16, 256, 1, {1, 2}, {}, 2},
    {"tiny", 8, 32, 32, 32, 2, {1, 2}, {1, 2}, 2},
    {"plumb", 32, 16, 16, 64, 2, {1, 1, 2, 4, 8}, {4, 8}, 2},
    {"north", 64, 32, 32, 64, 2, {1, 1, 2, 4, 8}, {4, 8}, 2},
    {"donut128", 128, 32, 32, 64, 2, {1, 1, 2, 4, 8}, {4, 8}, 2},  // the 128^3 bf16 side workload
    // tests/test_gpu_unet_grid_sizes.py
    {"g12-6", 12, 16, 16, 32, 2, {1, 2}, {2}, 2},
    {"g12-6-wide", 12, 16, 16, 64, 2, {1, 2}, {1, 2}, 2},
    {"g12-6-3", 12, 16, 16, 32, 2, {1, 1, 2}, {2, 4}, 2},
    {"g20-10-5", 20, 16, 16, 32, 2, {1, 1, 2}, {4}, 2},
    {"g24-12", 24, 16, 16, 64, 2, {1, 2}, {}, 2},
    {"g24-12-6", 24, 16, 16, 64, 2, {1, 2, 2}, {1, 4}, 2},
    {"g40-20", 40, 16, 16, 64, 2, {1, 2}, {}, 2},
    {"g48-24-12", 48, 16, 16, 64, 2, {1, 1, 2}, {4}, 2},
    {"g96", 96, 32, 32, 64, 2, {1, 1, 2, 4}, {4, 8}, 2},
    // tests/test_gpu_unet_channel_widths.py
    {"c96-192", 16, 12, 20, 96, 2, {1, 2}, {2}, 3},
    {"c96-heads2", 8, 12, 20, 96, 2, {1, 2}, {1, 2}, 2},
    {"c160", 16, 4, 8, 160, 2, {1}, {}, 2},
    {"c224", 8, 8, 4, 224, 2, {1}, {1}, 7},
    {"c36-to-4", 8, 36, 4, 32, 2, {1, 3}, {2}, 2},
    {"c4-to-36", 8, 4, 36, 32, 2, {1}, {}, 2},
    {"c3-1", 32, 4, 4, 32, 1, {3, 1}, {}, 1},
    // tests/test_gpu_backward.py (its `tiny` and `wide` are tiny and u8 above): the training sweep only
    {"deep", 16, 16, 16, 32, 1, {1, 2, 3}, {4}, 2},
};
const int N_FWD_NETS = 34;  // the forward sweep's nets: the table of the forward plans is recorded for these
// (tests/test_gpu_cu_counts.py runs u16 and u8 above under 8 / 20 / 32 CUs)
const int FULL_NET = 32;  // c4-to-36: its default exact-fp32 plan prints every op line
const int CUS[] = {256, 8, 20, 32};
const int BATCHES[] = {1, 2, 4};

struct Env {
  const char *name, *value;
};
struct KnobSet {
  const char* tag;
  std::vector<Env> env;
};
const KnobSet KNOBS[] = {
    {"-", {}},
    {"side0", {{"HOLO_SIDE_LANE_CUS", "0"}}},
    {"sidelow", {{"HOLO_SIDE_LANE_CUS", "4"}, {"HOLO_SIDE_LANE_MIN_R", "8"}, {"HOLO_SIDE_LANE_FORK_R", "4"}}},
    {"noskipfusion", {{"HOLO_NO_SKIP_FUSION", "1"}}},
    {"noflash", {{"HOLO_NO_FLASH_ATTN", "1"}}},
    {"fusebelow8", {{"HOLO_SKIP_FUSION_BELOW_R", "8"}}},
    {"fusebelow1000", {{"HOLO_SKIP_FUSION_BELOW_R", "1000"}}},
    {"bf16flash0", {{"HOLO_BF16_FLASH_MIN_T", "0"}}},
    {"bf16flash256", {{"HOLO_BF16_FLASH_MIN_T", "256"}}},
    {"keep", {{"HOLO_KEEP_INTERMEDIATES", "1"}}},
};

uint32_t mix(uint32_t x) {  // (a fixed integer hash: the thinning is the same everywhere)
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x;
}

// ---- made-up addresses -----------------------------------------------------------------------------------------------
const uintptr_t WS = (uintptr_t)1 << 44, ST_F32 = (uintptr_t)2 << 44, ST_BF = (uintptr_t)3 << 44, ST_WINO = (uintptr_t)4 << 44;
const uintptr_t ST_DGRAD = (uintptr_t)5 << 44;  // the transposed weights of a training plan (holo_unet_set_dgrad_weight's buffers)
const uintptr_t REGION = (uintptr_t)1 << 44;    // no store and no workspace is as large

struct Case {
  int net, mode, batch, bi, cus, knob, tape;
};

// One built plan with what the checks need of its planner
struct Built {
  Plan plan;
  std::string err;
  size_t small_top = 0, small_cap = 0;
  int ted = 0, emb_rows = 0;
  Knobs knobs;  // the planner's snapshot
  int cus = 0, plan_n = 0;
};

void make_desc(Desc& d, const Case& c) {
  const NetCfg& n = NETS[c.net];
  memset(&d.cfg, 0, sizeof d.cfg);
  d.cfg.image_size = n.R, d.cfg.in_channels = n.cin, d.cfg.out_channels = n.cout, d.cfg.model_channels = n.mc;
  d.cfg.num_res_blocks = n.nrb, d.cfg.num_heads = n.heads, d.cfg.homogeneous_resample = 1;
  d.cfg.n_channel_mult = (int)n.mult.size();
  for (size_t i = 0; i < n.mult.size(); ++i) d.cfg.channel_mult[i] = n.mult[i];
  d.cfg.n_attention_resolutions = (int)n.attn.size();
  for (size_t i = 0; i < n.attn.size(); ++i) d.cfg.attention_resolutions[i] = n.attn[i];
  set_cus(d, c.cus);
  build_structure(&d);
  enumerate_params(&d);
  d.knobs = Knobs::from_env();
  d.compute_mode = c.mode;
  d.batch_invariant = c.bi != 0;
  carve_params(&d, nullptr, nullptr, nullptr);  // (the sizing pass of holo_unet_create)
  carve_params(&d, reinterpret_cast<float*>(ST_F32), reinterpret_cast<uint16_t*>(ST_BF), reinterpret_cast<float*>(ST_WINO));
}

// the plan of `c` as holo_unet_forward builds it (`keep`: with the arena keeping everything), or as the training planner
// builds its forward (c.tape); ws = 0: the sizing pass of holo_unet_workspace_bytes
void build_plan(const Case& c, bool keep, Built& b, uintptr_t ws = WS) {
  for (const Env& e : KNOBS[c.knob].env) setenv(e.name, e.value, 1);
  {
    Desc d;
    make_desc(d, c);
    if (keep) d.knobs.keep_intermediates = true;
    std::vector<Tape> tape;
    Planner pl(&d, c.batch, reinterpret_cast<void*>(ws), b.plan);
    if (c.tape) pl.arena.keep = true, pl.tape = &tape;
    pl.build();
    b.err = pl.err;
    b.small_top = pl.small_top, b.small_cap = pl.small_cap;
    b.ted = d.ted, b.emb_rows = d.emb_rows;
    b.knobs = pl.knobs;
    b.cus = c.cus, b.plan_n = pl.plan_n();
  }
  for (const Env& e : KNOBS[c.knob].env) unsetenv(e.name);
}

// ---- the table -------------------------------------------------------------------------------------------------------
bool g_null_ws = false;  // the plan was built on no workspace: its workspace pointers are bare offsets (printed masked)
bool g_mask_ws = false;  // print workspace pointers without their offset: (b) compares op lists "in everything but addresses"
bool g_mask_all = false;  // print every pointer as null or not: a sizing pass on no transposed weights assumes addresses for them
int failures = 0;
void fail(const std::string& where, const std::string& what) {
  if (++failures <= 30) printf("FAIL %s: %s\n", where.c_str(), what.c_str());
}

std::string addr(const void* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  char buf[40];
  if (!a) return "0";
  if (g_mask_all) return "p";
  if (g_null_ws && a < WS) return "w";
  const char* tag = a >= WS && a < WS + REGION ? "w" : a >= ST_F32 && a < ST_F32 + REGION ? "f" : a >= ST_BF && a < ST_BF + REGION ? "b" :
                    a >= ST_WINO && a < ST_WINO + REGION ? "v" : a >= ST_DGRAD && a < ST_DGRAD + REGION ? "d" : nullptr;
  if (!tag) return "?";
  if (tag[0] == 'w' && g_mask_ws) return "w";
  snprintf(buf, sizeof buf, "%s+%llu", tag, (unsigned long long)(a & (REGION - 1)));
  return buf;
}
struct Line {
  std::string s;
  Line& i(const char* k, long long v) {
    s += ' ', s += k, s += '=', s += std::to_string(v);
    return *this;
  }
  Line& f(const char* k, double v) {
    char buf[40];
    snprintf(buf, sizeof buf, " %s=%.9g", k, v);
    s += buf;
    return *this;
  }
  Line& p(const char* k, const void* v) {
    s += ' ', s += k, s += '=', s += addr(v);
    return *this;
  }
};

void conv_fields(Line& l, const ConvParams& c) {
  l.p("src0", c.src0).p("src1", c.src1).i("C0", c.C0).i("C1", c.C1).i("N", c.N).i("ID", c.ID).i("IH", c.IH).i("IW", c.IW).i("ups", c.ups)
      .i("OD", c.OD).i("OH", c.OH).i("OW", c.OW).i("stride", c.stride).i("pad", c.pad).i("ksz", c.ksz).i("Cout", c.Cout).p("w", c.w)
      .i("CoutP", c.CoutP).i("CinP", c.CinP).p("coef", c.coef).i("act", c.act).p("bias", c.bias).p("residual", c.residual).p("out", c.out)
      .p("skip_src0", c.skip_src0).p("skip_src1", c.skip_src1).i("skip_C0", c.skip_C0).i("skip_C1", c.skip_C1).p("skip_w", c.skip_w)
      .p("w_bf", c.w_bf).p("skip_w_bf", c.skip_w_bf).i("bf16", c.bf16).i("skip_CinP", c.skip_CinP).p("skip_bias", c.skip_bias)
      .p("stats", c.stats).p("partial", c.partial).i("nsplit", c.nsplit).i("cps", c.chunks_per_split).i("scps", c.skip_chunks_per_split)
      .i("tz", c.tz).i("grid_x", c.grid_x).i("stagger", c.stagger_ticks).p("dbg", c.dbg).i("kernel", (int)c.kernel).p("w_wino2", c.w_wino2)
      .p("skip_w_wino2", c.skip_w_wino2).p("w_wino3", c.w_wino3).p("skip_w_wino3", c.skip_w_wino3).i("wino3_up", c.wino3_up)
      .p("w_bft", c.w_bft).p("skip_w_bft", c.skip_w_bft).i("in_bf16", c.in_bf16).i("res_bf16", c.res_bf16).i("out_bf16", c.out_bf16)
      .p("qkv_q", c.qkv_q).p("qkv_k", c.qkv_k).p("qkv_vt", c.qkv_vt).f("qkv_scale", c.qkv_scale).i("qkv_T", c.qkv_T).i("qkv_CH", c.qkv_CH)
      .i("qkv_H", c.qkv_H).i("qkv_sb", c.qkv_sb).i("qkv_rows", c.qkv_rows);
}
void gemm_fields(Line& l, const GemmParams& g) {
  l.p("A", g.A).p("B", g.B).p("C", g.C).i("M", g.M).i("Nn", g.Nn).i("K", g.K).i("lda", g.lda).i("ldb", g.ldb).i("ldc", g.ldc).i("nb0", g.nb0)
      .i("nb1", g.nb1).i("sa0", g.sa0).i("sa1", g.sa1).i("sb0", g.sb0).i("sb1", g.sb1).i("sc0", g.sc0).i("sc1", g.sc1)
      .i("b_kmajor", g.b_kmajor).f("alpha", g.alpha);
}

std::string op_line(const Op& op) {
  Line l;
  l.s = "  op";
  l.i("kind", op.kind).i("side", op.side).i("fork", op.fork).i("join", op.join);
  switch (op.kind) {
    case OP_IN: l.p("dst", op.in.dst).i("C", op.in.C).i("V", op.in.V).i("dst_bf16", op.in.dst_bf16); break;
    case OP_OUT: l.p("src", op.out.src).i("C", op.out.C).i("V", op.out.V); break;
    case OP_TEMB:
      l.p("w1", op.temb.w1).p("b1", op.temb.b1).p("w2", op.temb.w2).p("b2", op.temb.b2).p("emb", op.temb.emb).p("emb_silu", op.temb.emb_silu)
          .i("load_kind", op.temb.load_kind);
      break;
    case OP_EMBLIN: l.p("emb_silu", op.emblin.emb_silu).p("w", op.emblin.w).p("b", op.emblin.b).p("out", op.emblin.out); break;
    case OP_STATS: l.p("x", op.stats.x).p("part", op.stats.part).i("C", op.stats.C).i("x_bf16", op.stats.x_bf16).i("V", op.stats.V); break;
    case OP_FINAL: {
      const GnFinalize& f = op.fin;
      l.p("part0", f.part0).p("part1", f.part1).i("C0", f.C0).i("B0", f.B0).i("C1", f.C1).i("B1", f.B1).i("V", f.V).p("gamma", f.gamma)
          .p("beta", f.beta).p("film", f.film).i("film_stride", f.film_stride).i("film_cout", f.film_cout).p("coef", f.coef)
          .p("moments", f.moments).i("groups", f.groups);
      break;
    }
    case OP_CONV: conv_fields(l, op.conv); break;
    case OP_GEMM: gemm_fields(l, op.gemm); break;
    case OP_SOFTMAX: l.p("S", op.softmax.S).i("rows", op.softmax.rows).i("cols", op.softmax.cols); break;
    case OP_FLASH: {
      const Flash& f = op.flash;
      l.p("qkv", f.attn.qkv).p("out", f.attn.out).i("N", f.attn.N).i("T", f.attn.T).i("C", f.attn.C).i("H", f.attn.H).f("scale2", f.attn.scale2)
          .i("nsplit", f.attn.nsplit).p("part", f.attn.part).p("part_ml", f.attn.part_ml).i("form", f.form).p("packed", f.packed)
          .i("out_bf16", f.out_bf16).i("operands_packed", f.operands_packed).i("ksplit", f.ksplit).i("lazy", f.lazy);
      break;
    }
    default: l.s += " UNKNOWN"; break;
  }
  return l.s;
}

uint64_t fnv(uint64_t h, const std::string& s) {
  for (unsigned char ch : s) h = (h ^ ch) * 0x100000001b3ull;
  return h;
}
std::vector<std::string> op_lines(const Plan& plan) {
  std::vector<std::string> v;
  for (const Op& op : plan.ops) v.push_back(op_line(op));
  return v;
}
std::string case_name(const Case& c) {
  char buf[128];
  snprintf(buf, sizeof buf, "%s m%d n%d bi%d cu%d %s%s", NETS[c.net].name, c.mode, c.batch, c.bi, c.cus, KNOBS[c.knob].tag, c.tape ? " tape" : "");
  return buf;
}
std::string plan_line(const Case& c, const Built& b, const std::vector<std::string>& ops) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (const std::string& s : ops) h = fnv(h, s + "\n");
  char buf[256];
  snprintf(buf, sizeof buf, "%s | %zu %d %d %d %d %d %zu %016llx |", case_name(c).c_str(), b.plan.bytes, b.plan.n_joins, b.plan.first_conv,
           b.plan.last_conv, b.plan.cl_refusal ? 1 : 0, b.err.empty() ? 0 : 1, b.plan.ops.size(), (unsigned long long)h);
  std::string s = buf;
  for (const auto& kv : b.plan.block_outputs) s += ' ' + std::to_string(kv.second.off);
  return s;
}

// ---- footprints ------------------------------------------------------------------------------------------------------
struct Range {
  const char* name;
  size_t off, bytes;  // workspace offsets
  bool rd, wr;
  bool scratch;  // read and written, and filled by the launch itself before it reads it
  size_t end() const { return off + bytes; }
};
bool overlap(const Range& a, const Range& b) { return a.bytes && b.bytes && a.off < b.end() && b.off < a.end(); }

struct Footprint {
  std::vector<Range> r;
  std::vector<const void*> pointers;  // every pointer field of the op: the workspace ones must lie in a declared range
  void add(const char* name, const void* p, size_t bytes, bool rd, bool wr, bool scratch = false) {
    pointers.push_back(p);
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a >= WS && a < WS + REGION && bytes) r.push_back({name, (size_t)(a - WS), bytes, rd, wr, scratch});
  }
  void rd(const char* n, const void* p, size_t b) { add(n, p, b, true, false); }
  void wr(const char* n, const void* p, size_t b) { add(n, p, b, false, true); }
  void rw(const char* n, const void* p, size_t b) { add(n, p, b, true, true); }
  void scratch(const char* n, const void* p, size_t b) { add(n, p, b, true, true, true); }
  // a parameter store pointer (read-only memory no launch of a plan writes): it must not point into the workspace
  void param(std::initializer_list<const void*> ps) { pointers.insert(pointers.end(), ps); }
};

// a convolution launch (of the forward, or a dgrad of the backward) from its parameters
bool conv_footprint(const ConvParams& c, bool side, const Built& b, Footprint& fp, std::string& why) {
  const size_t N = (size_t)b.plan.batch;
  const size_t in_e = c.in_bf16 ? 2 : 4, sd = c.ups ? 2 : 1;
  const size_t Vin = (size_t)(c.ID / sd) * (c.IH / sd) * (c.IW / sd), Vout = (size_t)c.OD * c.OH * c.OW;
  fp.rd("src0", c.src0, N * Vin * c.C0 * in_e);
  fp.rd("src1", c.src1, N * Vin * c.C1 * in_e);
  fp.rd("skip_src0", c.skip_src0, N * Vout * c.skip_C0 * in_e);
  fp.rd("skip_src1", c.skip_src1, N * Vout * c.skip_C1 * in_e);
  fp.rd("coef", c.coef, N * ((size_t)c.C0 + c.C1) * 2 * 4);
  fp.rd("residual", c.residual, N * Vout * c.Cout * (c.res_bf16 ? 2 : 4));
  if (c.kernel == ConvKernel::Qkv) {  // (`out` is then NOT written: conv_plan.h)
    const size_t ntc = N * (size_t)c.qkv_T * c.qkv_CH * c.qkv_H * sizeof(uint16_t);
    fp.wr("qkv_q", c.qkv_q, ntc), fp.wr("qkv_k", c.qkv_k, ntc), fp.wr("qkv_vt", c.qkv_vt, ntc);
    fp.pointers.push_back(c.out);
    fp.r.push_back({"out(unwritten)", (size_t)(reinterpret_cast<uintptr_t>(c.out) - WS), N * Vout * c.Cout * (c.out_bf16 ? 2 : 4), false, false, false});
  } else {
    fp.wr("out", c.out, N * Vout * c.Cout * (c.out_bf16 ? 2 : 4));
    if (c.qkv_q) {
      why = "qkv packing left offered on another kernel";
      return false;
    }
  }
  const int slabs = c.stats ? conv_stats_slabs(c) : 0;
  if (c.stats && slabs <= 0) {
    why = "statistics on a launch that writes none";
    return false;
  }
  fp.wr("stats", c.stats, N * slabs * c.Cout * 2 * sizeof(double));
  ConvParams again = c;  // the scratch: conv_plan on a copy of the op's parameters
  const size_t sb = conv_plan(again, side ? (int)b.knobs.side_lane_cus : b.cus, b.knobs, b.plan_n);
  if (again.kernel != c.kernel || again.nsplit != c.nsplit || (sb != 0) != (c.partial != nullptr)) {
    why = "conv_plan re-run on the op's parameters chooses another launch";
    return false;
  }
  fp.scratch("partial", c.partial, sb);
  fp.param({c.w, c.bias, c.skip_w, c.skip_bias, c.w_bf, c.skip_w_bf, c.w_wino2, c.skip_w_wino2, c.w_wino3, c.skip_w_wino3, c.w_bft,
            c.skip_w_bft, c.dbg});
  return true;
}
void gemm_footprint(const GemmParams& g, Footprint& fp) {  // strided operands: the smallest enclosing range
  const size_t ba = (size_t)(g.nb0 - 1) * g.sa0 + (size_t)(g.nb1 - 1) * g.sa1, bb = (size_t)(g.nb0 - 1) * g.sb0 + (size_t)(g.nb1 - 1) * g.sb1,
               bc = (size_t)(g.nb0 - 1) * g.sc0 + (size_t)(g.nb1 - 1) * g.sc1;
  fp.rd("A", g.A, (ba + (size_t)(g.M - 1) * g.lda + g.K) * 4);
  fp.rd("B", g.B, (bb + (g.b_kmajor ? (size_t)(g.K - 1) * g.ldb + g.Nn : (size_t)(g.Nn - 1) * g.ldb + g.K)) * 4);
  fp.wr("C", g.C, (bc + (size_t)(g.M - 1) * g.ldc + g.Nn) * 4);
}

// the ranges op `op` of a plan of `b` reads and writes, from its own fields; false: no footprint for this kind
bool footprint(const Op& op, const Built& b, Footprint& fp, std::string& why) {
  const size_t N = (size_t)b.plan.batch;
  switch (op.kind) {
    case OP_IN: fp.wr("dst", op.in.dst, N * op.in.V * op.in.C * (op.in.dst_bf16 ? 2 : 4)); return true;
    case OP_OUT: fp.rd("src", op.out.src, N * op.out.V * op.out.C * 4); return true;
    case OP_TEMB:
      fp.wr("emb", op.temb.emb, N * b.ted * 4), fp.wr("emb_silu", op.temb.emb_silu, N * b.ted * 4);
      fp.param({op.temb.w1, op.temb.b1, op.temb.w2, op.temb.b2});
      return true;
    case OP_EMBLIN:
      fp.rd("emb_silu", op.emblin.emb_silu, N * b.ted * 4), fp.wr("out", op.emblin.out, N * b.emb_rows * 4);
      fp.param({op.emblin.w, op.emblin.b});
      return true;
    case OP_STATS: {
      int B, vpb;
      gn_stats_geometry(op.stats.C, op.stats.V, &B, &vpb);
      fp.rd("x", op.stats.x, N * op.stats.V * op.stats.C * (op.stats.x_bf16 ? 2 : 4));
      fp.wr("part", op.stats.part, N * B * op.stats.C * 2 * sizeof(double));
      return true;
    }
    case OP_FINAL: {
      const GnFinalize& f = op.fin;
      const size_t C = (size_t)f.C0 + f.C1;
      fp.rd("part0", f.part0, N * f.B0 * f.C0 * 2 * sizeof(double));
      fp.rd("part1", f.part1, N * f.B1 * f.C1 * 2 * sizeof(double));
      // sample n reads the rows [n * film_stride, + 2 * film_cout) (scale, shift) behind `film`: the smallest enclosing range
      fp.rd("film", f.film, f.film ? ((N - 1) * f.film_stride + 2 * (size_t)f.film_cout) * 4 : 0);
      fp.wr("coef", f.coef, N * C * 2 * 4);
      fp.wr("moments", f.moments, N * C * 2 * 4);
      fp.param({f.gamma, f.beta});
      return true;
    }
    case OP_CONV: return conv_footprint(op.conv, op.side != 0, b, fp, why);
    case OP_GEMM: gemm_footprint(op.gemm, fp); return true;
    case OP_SOFTMAX: fp.rw("S", op.softmax.S, (size_t)op.softmax.rows * op.softmax.cols * 4); return true;
    case OP_FLASH: {
      const Flash& f = op.flash;
      const size_t ntc = (size_t)f.attn.N * f.attn.T * f.attn.C;
      if (f.form == 2) {
        if (!f.operands_packed) fp.rd("qkv", f.attn.qkv, ntc * 3 * 4);  // (the packing pre-pass)
        else fp.pointers.push_back(f.attn.qkv);
        // the packed operands (written by the qkv convolution, else by this launch's own pre-pass), behind them the split
        // partials and redo flags this launch fills itself
        uint16_t *q, *k, *vt;
        float qs;
        flash_attn_bf16v2_operands(f.attn, f.packed, &q, &k, &vt, &qs);
        const size_t operands = (size_t)((const char*)(vt + ntc) - (const char*)f.packed);
        if (f.operands_packed) fp.rd("packed", f.packed, operands);
        else fp.scratch("packed", f.packed, operands);
        fp.scratch("packed_work", (const char*)f.packed + operands, flash_attn_bf16v2_workspace_bytes(f.attn, f.ksplit) - operands);
        fp.wr("out", f.attn.out, ntc * (f.out_bf16 ? 2 : 4));
        if (f.operands_packed) fp.r.push_back({"qkv(unread)", (size_t)(reinterpret_cast<uintptr_t>(f.attn.qkv) - WS), ntc * 3 * 4, false, false, false});
      } else if (f.form == 0) {
        fp.rd("qkv", f.attn.qkv, ntc * 3 * 4);
        fp.scratch("part", f.attn.part, flash_attn_workspace_bytes(f.attn));
        fp.pointers.push_back(f.attn.part_ml);  // (inside `part`)
        fp.wr("out", f.attn.out, ntc * 4);
      } else {
        why = "unknown form of the flash op";
        return false;
      }
      return true;
    }
  }
  why = "no footprint for op kind " + std::to_string((int)op.kind);
  return false;
}

// ---- the checks on one op list ------------------------------------------------------------------------------------------
struct Prints {
  std::vector<Footprint> fp;
  bool ok = true;
};
Prints footprints(const std::vector<Op>& ops, const Built& b, const std::string& where) {
  Prints p;
  p.fp.resize(ops.size());
  for (size_t i = 0; i < ops.size(); ++i) {
    std::string why;
    Footprint& fp = p.fp[i];
    if (!footprint(ops[i], b, fp, why)) {
      fail(where + " op " + std::to_string(i), why);
      p.ok = false;
      continue;
    }
    for (const void* q : fp.pointers) {  // a workspace pointer outside every declared range
      const uintptr_t a = reinterpret_cast<uintptr_t>(q);
      if (a < WS || a >= WS + REGION) continue;
      bool in = false;
      for (const Range& r : fp.r) in = in || (a - WS >= r.off && a - WS < r.end());
      if (!in) fail(where + " op " + std::to_string(i), "a workspace pointer in no declared range of the op"), p.ok = false;
    }
  }
  return p;
}

// (c): the ops whose own buffers collide
std::set<int> check_one_launch(const Prints& p) {
  std::set<int> bad;
  for (size_t i = 0; i < p.fp.size(); ++i) {
    const std::vector<Range>& r = p.fp[i].r;
    for (size_t a = 0; a < r.size(); ++a)
      for (size_t c = 0; c < r.size(); ++c) {
        if (a == c || !r[a].wr || !(r[c].rd || r[c].wr) || !overlap(r[a], r[c])) continue;
        const bool alias_ok = !strcmp(r[a].name, "out") && !strcmp(r[c].name, "residual") && r[a].off == r[c].off && r[a].bytes == r[c].bytes;
        if (!alias_ok) bad.insert((int)i);
      }
  }
  return bad;
}

// (d): the side ops a main-lane op between the fork and their consumer's join collides with
std::set<int> check_side_lane(const std::vector<Op>& ops, const Prints& p, std::string* what = nullptr) {
  std::set<int> bad;
  int fork_at = -1;
  for (size_t i = 0; i < ops.size(); ++i)
    if (ops[i].fork) fork_at = (int)i;
  for (size_t s = 0; s < ops.size(); ++s) {
    if (!ops[s].side) continue;
    // the join behind this side op: its own, or that of the next side op (the side stream runs in order)
    int join = -1;
    for (size_t j = s; j < ops.size() && join < 0; ++j)
      if (ops[j].side) join = ops[j].join;
    int consumer = -1;
    for (size_t j = 0; j < ops.size(); ++j)
      if (!ops[j].side && ops[j].join == join && join >= 0) consumer = (int)j;
    if (fork_at < 0 || fork_at > (int)s || consumer < 0) {
      bad.insert((int)s);
      if (what) *what = "a side op without a fork in front of it or a consumer waiting for its join";
      continue;
    }
    for (int m = fork_at; m < consumer; ++m) {
      if (ops[m].side) continue;
      for (const Range& a : p.fp[m].r)
        for (const Range& c : p.fp[s].r)
          if (overlap(a, c) && ((a.wr && (c.rd || c.wr)) || (a.rd && c.wr))) {
            bad.insert((int)s);
            if (what) *what = "main-lane op " + std::to_string(m) + " (" + a.name + ") against " + c.name;
          }
    }
  }
  return bad;
}

// the ops that last wrote some byte of [off, off + bytes) in front of op i, latest first
std::vector<int> latest_writers(const Prints& p, int i, size_t off, size_t bytes, bool* covered) {
  std::vector<std::pair<size_t, size_t>> open{{off, off + bytes}};  // what no op has been found for yet
  std::vector<int> w;
  for (int j = i - 1; j >= 0 && !open.empty(); --j) {
    bool hit = false;
    for (const Range& r : p.fp[j].r) {
      if (!r.wr) continue;
      std::vector<std::pair<size_t, size_t>> rest;
      for (const auto& o : open) {
        if (r.off >= o.second || r.end() <= o.first) {
          rest.push_back(o);
          continue;
        }
        hit = true;
        if (o.first < r.off) rest.push_back({o.first, r.off});
        if (r.end() < o.second) rest.push_back({r.end(), o.second});
      }
      open.swap(rest);
    }
    if (hit) w.push_back(j);
  }
  *covered = open.empty();
  return w;
}

// (e) and the bounds of one plan
void check_reads_and_bounds(const Built& b, const Prints& p, const std::string& where) {
  if (b.small_top > b.small_cap) fail(where, "the small region overflows small_cap");
  for (size_t i = 0; i < p.fp.size(); ++i)
    for (const Range& r : p.fp[i].r) {
      const std::string at = where + " op " + std::to_string(i) + " " + r.name;
      if (r.end() > b.plan.bytes) fail(at, "outside [0, plan.bytes)");
      if (r.off < b.small_cap && r.end() > b.small_cap) fail(at, "straddles the end of the small region");
      if (r.off < b.small_cap && r.end() > b.small_top) fail(at, "in the small region but beyond what was handed out");
      if (!r.rd) continue;
      bool covered = false;
      latest_writers(p, (int)i, r.off, r.bytes, &covered);
      if (!covered && !r.scratch) fail(at, "read before it is written");  // (scratch a launch fills itself first is exempt)
    }
}

// (b): the releasing plan against the keeping plan of the same case
void check_producers(const Built& rel, const Prints& prel, const Built& keep, const Prints& pkeep, const std::string& where) {
  g_mask_ws = true;
  const std::vector<std::string> a = op_lines(rel.plan), k = op_lines(keep.plan);
  g_mask_ws = false;
  if (a != k) {
    fail(where, "the keeping plan's ops differ from the releasing plan's in more than addresses");
    return;
  }
  for (size_t i = 0; i < a.size(); ++i) {
    const std::vector<Range>&r = prel.fp[i].r, &q = pkeep.fp[i].r;
    if (r.size() != q.size()) {
      fail(where + " op " + std::to_string(i), "the two plans' footprints differ");
      continue;
    }
    for (size_t x = 0; x < r.size(); ++x) {
      if (!r[x].rd) continue;
      bool c0, c1;
      const std::vector<int> wk = latest_writers(pkeep, (int)i, q[x].off, q[x].bytes, &c1);
      if (r[x].wr && wk.empty()) continue;  // (scratch the launch fills itself: in the keeping plan nobody wrote it before)
      if (latest_writers(prel, (int)i, r[x].off, r[x].bytes, &c0) != wk)
        fail(where + " op " + std::to_string(i) + " " + r[x].name, "released memory changed the operand's producers");
    }
  }
}

struct Coverage {
  int side = 0, bf16_attn = 0, gemm_attn = 0, flash_split = 0, split_stats = 0, fused_skip = 0, own_skip = 0, ups = 0, down = 0, bi = 0,
      tape = 0;
  void count(const Case& c, const Plan& plan) {
    bool f[9] = {};
    for (const Op& op : plan.ops) {
      if (op.kind == OP_FLASH) f[0] |= op.flash.form == 2, f[2] |= op.flash.form == 0 && op.flash.attn.nsplit > 1;
      if (op.kind == OP_SOFTMAX) f[1] = true;
      if (op.kind != OP_CONV) continue;
      const ConvParams& p = op.conv;
      f[3] |= p.nsplit > 1 && p.stats, f[4] |= p.skip_w != nullptr, f[5] |= p.ksz == 1 && !p.coef && !p.residual;
      f[6] |= p.ups != 0, f[7] |= p.stride == 2;
    }
    side += plan.n_joins > 0, bf16_attn += f[0], gemm_attn += f[1], flash_split += f[2], split_stats += f[3], fused_skip += f[4];
    own_skip += f[5], ups += f[6], down += f[7], bi += c.bi && c.batch > 1, tape += c.tape;
  }
};

std::vector<Case> sweep() {
  std::vector<Case> v;
  uint32_t counter = 0;
  const int n_nets = N_FWD_NETS, n_knobs = (int)(sizeof KNOBS / sizeof KNOBS[0]);
  for (int net = 0; net < n_nets; ++net)
    for (int mode = 0; mode < 3; ++mode)
      for (int batch : BATCHES)
        for (int bi = 0; bi <= (mode == 0 ? 1 : 0); ++bi)
          for (int cus : CUS)
            for (int knob = 0; knob < n_knobs; ++knob)
              for (int tape = 0; tape <= (mode == 0 && !bi && knob == 0 ? 1 : 0); ++tape) {
                // thinning: every net at batch 1 on 256 CUs with the default knobs in every mode; one in `keep` of the rest
                const bool base = batch == 1 && cus == 256 && knob == 0 && !bi && !tape;
                const int keep = base ? 1 : knob == 0 ? 64 : 200;
                if (mix(counter++) % keep) continue;
                v.push_back(Case{net, mode, batch, bi, cus, knob, tape});
              }
  // ... and every knob set where it bites, whatever the hash kept: (knob set, net, compute mode), batch 1, 256 CUs
  const struct {
    const char *knob, *net;
    int mode;
  } forced[] = {{"side0", "u32", 0}, {"side0", "north", 0}, {"sidelow", "u16", 0}, {"sidelow", "plumb", 0}, {"noskipfusion", "u8", 0},
                {"noskipfusion", "north", 1}, {"noflash", "north", 0}, {"noflash", "u16w", 1}, {"fusebelow8", "u16", 0},
                {"fusebelow8", "u32", 0}, {"fusebelow1000", "u64l", 0}, {"fusebelow1000", "north", 0}, {"bf16flash0", "u16a", 1},
                {"bf16flash0", "u16w", 1}, {"bf16flash0", "c224", 1}, {"bf16flash256", "u16w", 1}, {"bf16flash256", "u16h", 1},
                {"keep", "u8", 0}, {"keep", "north", 1}};
  for (const auto& f : forced) {
    Case c{-1, f.mode, 1, 0, 256, -1, 0};
    for (int i = 0; i < n_nets; ++i)
      if (!strcmp(NETS[i].name, f.net)) c.net = i;
    for (int i = 0; i < n_knobs; ++i)
      if (!strcmp(KNOBS[i].tag, f.knob)) c.knob = i;
    bool have = c.net < 0 || c.knob < 0;  // (a name that does not exist fails below: its knob set bites nowhere)
    for (const Case& o : v) have = have || (o.net == c.net && o.mode == c.mode && o.batch == 1 && !o.bi && o.cus == 256 && o.knob == c.knob && !o.tape);
    if (!have) v.push_back(c);
  }
  return v;
}

// ---- training plans ------------------------------------------------------------------------------------------------------
// The backward of a training plan, checked as ONE timeline with its taped forward: the forward ops, a pseudo-op that writes
// gy_off (the layout pass of grad_out), the backward ops, a pseudo-op that reads gx_off.
const char* const TRAIN_NETS[] = {"tiny", "u8", "deep", "plumb", "north", "g12-6-3", "g24-12", "c96-192", "c36-to-4"};
const char* const TRAIN_FULL_NET = "c36-to-4";  // its batch-1 plan on 256 CUs under the default knobs prints every backward op line
const int TRAIN_BATCHES[] = {1, 2};
const KnobSet TRAIN_KNOBS[] = {
    {"-", {}},
    {"s2direct", {{"HOLO_DGRAD_S2_DIRECT", "1"}}},
    {"wgradtiles", {{"HOLO_WGRAD_TILES", "1"}}},
    {"reducetile1", {{"HOLO_WGRAD_REDUCE_TILE_MIN", "1"}}},  // (tests/test_gpu_backward.py, wide-tiled-reduce)
};
struct TrainCase {
  int net, batch, cus, knob;
};
typedef std::map<std::string, ConvWeights> Dgrad;

// the line of one backward launch, from the arguments of its launcher
std::string bl_conv(const ConvParams& c) {
  Line l;
  l.s = "  bop conv";
  conv_fields(l, c);
  return l.s;
}
std::string bl_wgrad(const WgradParams& w, const WgradPlan& g, const float* dw, int acc) {
  Line l;
  l.s = "  bop wgrad";
  l.p("gy", w.gy).p("src0", w.src0).p("src1", w.src1).i("C0", w.C0).i("C1", w.C1).i("N", w.N).i("ID", w.ID).i("IH", w.IH).i("IW", w.IW)
      .i("ups", w.ups).i("OD", w.OD).i("OH", w.OH).i("OW", w.OW).i("stride", w.stride).i("pad", w.pad).i("ksz", w.ksz).i("ntaps", w.ntaps)
      .i("Cout", w.Cout).p("coef", w.coef).i("act", w.act).p("partial", w.partial).i("rows", g.rows).i("splits", g.splits)
      .i("reduce_tile", g.reduce_tile).p("dw", dw).i("acc", acc);
  return l.s;
}
std::string bl_colsum(const float* g, int64_t M, int C, const double* scratch, const float* out, int acc) {
  Line l;
  l.s = "  bop colsum";
  l.p("g", g).i("M", M).i("C", C).p("scratch", scratch).p("out", out).i("acc", acc);
  return l.s;
}
std::string bl_gn(const GnBwdParams& g) {
  Line l;
  l.s = "  bop gn_bwd";
  l.p("x0", g.x0).p("x1", g.x1).i("C0", g.C0).i("C1", g.C1).i("N", g.N).i("V", g.V).p("ga", g.ga).p("coef", g.coef).p("mom", g.mom)
      .p("gamma", g.gamma).p("beta", g.beta).p("film", g.film).i("film_stride", g.film_stride).i("film_cout", g.film_cout).i("act", g.act)
      .p("part", g.part).p("grp", g.grp).p("dgamma", g.dgamma).p("dbeta", g.dbeta).p("dfilm", g.dfilm).i("acc_params", g.acc_params)
      .p("gx0", g.gx0).p("gx1", g.gx1).i("acc0", g.acc0).i("acc1", g.acc1);
  return l.s;
}
std::string bl_add(const float* dst, const float* src, int64_t n, int acc) {
  Line l;
  l.s = "  bop add";
  l.p("dst", dst).p("src", src).i("n", n).i("acc", acc);
  return l.s;
}
std::string bl_split(const float* g, const float* g0, const float* g1, int64_t M, int C0, int C1, int acc0, int acc1) {
  Line l;
  l.s = "  bop split_cat";
  l.p("g", g).p("g0", g0).p("g1", g1).i("M", M).i("C0", C0).i("C1", C1).i("acc0", acc0).i("acc1", acc1);
  return l.s;
}
std::string bl_pool(const float* gup, const float* gin, int N, int R, int C, int acc) {
  Line l;
  l.s = "  bop sumpool2";
  l.p("gup", gup).p("gin", gin).i("N", N).i("R", R).i("C", C).i("acc", acc);
  return l.s;
}
std::string bl_zins(const float* gy, const float* out, int N, int Rs, int C) {
  Line l;
  l.s = "  bop zero_insert2";
  l.p("gy", gy).p("out", out).i("N", N).i("Rs", Rs).i("C", C);
  return l.s;
}
std::string bl_s2(const float* gy, const float* wt, const float* gx, int N, int RI, int RO, int Ci, int Co, int acc) {
  Line l;
  l.s = "  bop dgrad_s2";
  l.p("gy", gy).p("wt", wt).p("gx", gx).i("N", N).i("RI", RI).i("RO", RO).i("Ci", Ci).i("Co", Co).i("acc", acc);
  return l.s;
}
std::string bl_gemm(const GemmParams& g) {
  Line l;
  l.s = "  bop gemm";
  gemm_fields(l, g);
  return l.s;
}
std::string bl_softmax(const float* S, int64_t rows, int cols) {
  Line l;
  l.s = "  bop softmax";
  l.p("S", S).i("rows", rows).i("cols", cols);
  return l.s;
}
std::string bl_ds(const float* P, const float* dP, int64_t rows, int cols) {
  Line l;
  l.s = "  bop attn_ds";
  l.p("P", P).p("dP", dP).i("rows", rows).i("cols", cols);
  return l.s;
}
std::string bl_transpose(const float* in, const float* out, int batch, int T) {
  Line l;
  l.s = "  bop transpose";
  l.p("in", in).p("out", out).i("batch", batch).i("T", T);
  return l.s;
}
std::string bl_film(const float* dfilm, const float* embs, const float* w, const float* dw, const float* db, const float* gembs, int N,
                    int rows, int K) {
  Line l;
  l.s = "  bop film_bwd";
  l.p("dfilm", dfilm).p("embs", embs).p("w", w).p("dw", dw).p("db", db).p("gembs", gembs).i("N", N).i("rows", rows).i("K", K);
  return l.s;
}
std::string bl_temb(int N, int mc, int ted, const float* w1, const float* b1, const float* w2, const float* b2, const float* gembs,
                    const float* dw1, const float* db1, const float* dw2, const float* db2) {  // (the timesteps are the running call's)
  Line l;
  l.s = "  bop time_embed_bwd";
  l.i("N", N).i("mc", mc).i("ted", ted).p("w1", w1).p("b1", b1).p("w2", w2).p("b2", b2).p("gembs", gembs).p("dw1", dw1).p("db1", db1)
      .p("dw2", dw2).p("db2", db2);
  return l.s;
}

// One built training plan with what the checks need of its planner and its description
struct TrainBuilt {
  Built b;  // b.plan: the taped forward (its bytes: the whole training plan's)
  size_t gy_off = 0, gx_off = 0, gy_bytes = 0, gx_bytes = 0;
  std::vector<size_t> grad_off, grad_bytes;
  std::vector<std::string> blines;
  size_t head_dw = 0;                          // gradient offset of the head's convolution weight
  int res_identity = 0, res_concat_conv = 0;  // ResBlocks with an identity skip / with a concat input and a conv skip
#ifndef UNET_PLAN_RECORD
  std::vector<BwdOp> bops;
#endif
};

#ifdef UNET_PLAN_RECORD
// the recorder's: builds the plan with the tree it brought in and calls every backward launch once on recording stand-ins
// of the launchers, which append their bl_* line to g_rec
std::vector<std::string> g_rec;
void record_train(const Desc& d, const Dgrad& table, int batch, uintptr_t ws, TrainBuilt& t);
#else
std::string bwd_op_line(const BwdOp& op) {
  switch (op.kind) {
    case BOP_CONV: return bl_conv(op.conv);
    case BOP_WGRAD: return bl_wgrad(op.wgrad.p, op.wgrad.plan, op.wgrad.dw, 0);
    case BOP_COLSUM: return bl_colsum(op.colsum.g, op.colsum.M, op.colsum.C, op.colsum.scratch, op.colsum.out, 0);
    case BOP_GN_BWD: return bl_gn(op.gn);
    case BOP_ADD: return bl_add(op.add.dst, op.add.src, op.add.n, op.add.acc);
    case BOP_SPLIT_CAT: return bl_split(op.split.g, op.split.g0, op.split.g1, op.split.M, op.split.C0, op.split.C1, op.split.acc0, op.split.acc1);
    case BOP_SUMPOOL2: return bl_pool(op.pool.gup, op.pool.gin, op.pool.N, op.pool.R, op.pool.C, op.pool.acc);
    case BOP_ZERO_INSERT2: return bl_zins(op.zins.gy, op.zins.out, op.zins.N, op.zins.Rs, op.zins.C);
    case BOP_DGRAD_S2: return bl_s2(op.s2.gy, op.s2.wt, op.s2.gx, op.s2.N, op.s2.RI, op.s2.RO, op.s2.Ci, op.s2.Co, op.s2.acc);
    case BOP_GEMM: return bl_gemm(op.gemm);
    case BOP_SOFTMAX: return bl_softmax(op.softmax.S, op.softmax.rows, op.softmax.cols);
    case BOP_ATTN_DS: return bl_ds(op.ds.P, op.ds.dP, op.ds.rows, op.ds.cols);
    case BOP_TRANSPOSE: return bl_transpose(op.tr.in, op.tr.out, op.tr.batch, op.tr.T);
    case BOP_FILM_BWD: return bl_film(op.film.dfilm, op.film.embs, op.film.w, op.film.dw, op.film.db, op.film.gembs, op.film.N, op.film.rows, op.film.K);
    case BOP_TEMB_BWD: {
      const TimeEmbedBwd& e = op.temb;
      return bl_temb(e.N, e.mc, e.ted, e.w1, e.b1, e.w2, e.b2, e.gembs, e.dw1, e.db1, e.dw2, e.db2);
    }
  }
  return "  bop UNKNOWN";
}
std::vector<std::string> bwd_op_lines(const std::vector<BwdOp>& bops) {
  std::vector<std::string> v;
  for (const BwdOp& op : bops) v.push_back(bwd_op_line(op));
  return v;
}
#endif

// the table of transposed weights as holo_unet_set_dgrad_weight makes it, on invented addresses: every convolution weight's
// ParamSlot::layout(true) with the copies of dgrad_copies; a Downsample weight has its [tap][co][ci] entry and "#s1"
Dgrad make_dgrad(const Desc& d) {
  Dgrad table;
  uintptr_t top = ST_DGRAD;
  auto take = [&](int64_t floats) {
    float* p = reinterpret_cast<float*>(top);
    top += ((uintptr_t)floats * sizeof(float) + 255) & ~(uintptr_t)255;
    return p;
  };
  for (const ParamSlot& s : d.params) {
    if (!s.is_conv()) continue;
    const bool down = is_downsample_weight(s.name);
    if (down) {
      table[s.name].f32 = take(s.numel);
      if ((s.shape[0] & 3) || (s.shape[1] & 3)) continue;
    }
    ConvWeights& dw = table[down ? s.name + "#s1" : s.name];
    const ConvWeightLayout l = dw.layout = s.layout(true);
    const ConvCopies c = dgrad_copies(l, d.compute_mode, d.knobs);
    dw.f32 = take(l.f32_floats());
    if (c.wino2 || c.wino3) dw.wino2 = take(l.wino2_floats());
    if (c.wino3) dw.wino3 = take(l.wino3_floats());
  }
  return table;
}

int net_index(const char* name) {
  for (int i = 0; i < (int)(sizeof NETS / sizeof NETS[0]); ++i)
    if (!strcmp(NETS[i].name, name)) return i;
  fail(name, "no such net");
  return 0;
}
std::string train_name(const TrainCase& c) {
  char buf[128];
  snprintf(buf, sizeof buf, "train %s n%d cu%d %s", NETS[c.net].name, c.batch, c.cus, TRAIN_KNOBS[c.knob].tag);
  return buf;
}

// the training plan of `c`; how: 0 on the workspace, 1 as a sizing pass with the same transposed weights, 2 as a sizing pass
// on no transposed weights (holo_unet_backward_workspace_bytes before any was supplied)
void build_train(const TrainCase& c, int how, TrainBuilt& t) {
  for (const Env& e : TRAIN_KNOBS[c.knob].env) setenv(e.name, e.value, 1);
  {
    Desc d;
    make_desc(d, Case{c.net, 0, c.batch, 0, c.cus, 0, 1});
    const Dgrad table = how == 2 ? Dgrad() : make_dgrad(d);
    const uintptr_t ws = how ? 0 : WS;
    g_null_ws = g_mask_ws = how == 1, g_mask_all = how == 2;
#ifdef UNET_PLAN_RECORD
    record_train(d, table, c.batch, ws, t);
#else
    TrainPlan tp;
    TrainPlanner pl(&d, table, c.batch, reinterpret_cast<void*>(ws), tp);
    pl.build();
    t.b.plan = tp.fwd, t.b.err = pl.err;
    t.b.small_top = pl.pl.small_top, t.b.small_cap = pl.pl.small_cap;
    t.b.knobs = pl.pl.knobs;
    t.gy_off = tp.gy_off, t.gx_off = tp.gx_off, t.grad_off = tp.grad_off;
    t.b.plan.bytes = tp.bytes;
    t.bops = tp.bops;
    t.blines = bwd_op_lines(t.bops);
#endif
    g_null_ws = g_mask_ws = g_mask_all = false;
    t.b.ted = d.ted, t.b.emb_rows = d.emb_rows, t.b.cus = c.cus, t.b.plan_n = c.batch;
    const size_t V = (size_t)d.cfg.image_size * d.cfg.image_size * d.cfg.image_size;
    t.gy_bytes = (size_t)c.batch * V * d.cfg.out_channels * 4, t.gx_bytes = (size_t)c.batch * V * d.cfg.in_channels * 4;
    for (const ParamSlot& s : d.params) t.grad_bytes.push_back((size_t)s.numel * 4);
    if (t.b.err.empty()) t.head_dw = t.grad_off[d.pindex.at("out.2.weight")];
    for (const std::vector<std::vector<Block>>* half : {&d.inputs, &d.outputs})
      for (const std::vector<Block>& level : *half)
        for (const Block& k : level) t.res_identity += k.kind == B_RES && k.cin == k.cout, t.res_concat_conv += half == &d.outputs && k.kind == B_RES && k.cin != k.cout;
    for (const Block& k : d.middle) t.res_identity += k.kind == B_RES && k.cin == k.cout;
  }
  for (const Env& e : TRAIN_KNOBS[c.knob].env) unsetenv(e.name);
}
std::string train_line(const std::string& name, const TrainBuilt& t) {
  uint64_t h = 0xcbf29ce484222325ull, hg = h;
  for (const std::string& s : t.blines) h = fnv(h, s + "\n");
  for (size_t off : t.grad_off) hg = fnv(hg, std::to_string(off) + ",");
  char buf[256];
  snprintf(buf, sizeof buf, "%s | %zu %zu %zu %016llx %zu %016llx %d", name.c_str(), t.b.plan.bytes, t.gy_off, t.gx_off, (unsigned long long)hg,
           t.blines.size(), (unsigned long long)h, t.b.err.empty() ? 0 : 1);
  return buf;
}

#ifndef UNET_PLAN_RECORD
// the ranges backward op `op` reads and writes, from its own fields.  An accumulating destination (acc*) is read and written;
// scratch is what the launch fills itself before it reads it.
bool bwd_footprint(const BwdOp& op, const Built& b, Footprint& fp, std::string& why) {
  const size_t N = (size_t)b.plan.batch;
  auto dst = [&](const char* n, const void* p, size_t bytes, int acc) { fp.add(n, p, bytes, acc != 0, true); };
  switch (op.kind) {
    case BOP_CONV: return conv_footprint(op.conv, false, b, fp, why);
    case BOP_WGRAD: {
      const WgradParams& w = op.wgrad.p;
      const size_t sd = w.ups ? 2 : 1, Vin = (size_t)(w.ID / sd) * (w.IH / sd) * (w.IW / sd), Vout = (size_t)w.OD * w.OH * w.OW, Cin = (size_t)w.C0 + w.C1;
      const WgradPlan g = wgrad_plan(w, b.cus, b.knobs);
      if (g.rows != op.wgrad.plan.rows || g.splits != op.wgrad.plan.splits || g.reduce_tile != op.wgrad.plan.reduce_tile || (size_t)w.N != N) {
        why = "wgrad_plan re-run on the op's parameters chooses another launch";
        return false;
      }
      fp.rd("gy", w.gy, N * Vout * w.Cout * 4);
      fp.rd("src0", w.src0, N * Vin * w.C0 * 4), fp.rd("src1", w.src1, N * Vin * w.C1 * 4);
      fp.rd("coef", w.coef, N * Cin * 2 * 4);
      fp.scratch("partial", w.partial, wgrad_partial_bytes(w, g));
      fp.wr("dw", op.wgrad.dw, (size_t)w.Cout * Cin * w.ntaps * 4);
      return true;
    }
    case BOP_COLSUM:
      fp.rd("g", op.colsum.g, (size_t)op.colsum.M * op.colsum.C * 4);
      fp.scratch("scratch", op.colsum.scratch, colsum_scratch_bytes(op.colsum.C));
      fp.wr("out", op.colsum.out, (size_t)op.colsum.C * 4);
      return true;
    case BOP_GN_BWD: {
      const GnBwdParams& g = op.gn;
      const size_t Cin = (size_t)g.C0 + g.C1, V = (size_t)g.V;
      if ((size_t)g.N != N) {
        why = "a GroupNorm backward of another batch";
        return false;
      }
      fp.rd("x0", g.x0, N * V * g.C0 * 4), fp.rd("x1", g.x1, N * V * g.C1 * 4);
      fp.rd("ga", g.ga, N * V * Cin * 4);
      fp.rd("coef", g.coef, N * Cin * 2 * 4), fp.rd("mom", g.mom, N * Cin * 2 * 4);
      fp.rd("film", g.film, g.film ? ((N - 1) * g.film_stride + 2 * (size_t)g.film_cout) * 4 : 0);
      fp.param({g.gamma, g.beta});
      fp.scratch("part", g.part, gn_bwd_scratch_bytes(g)), fp.scratch("grp", g.grp, N * Cin * 2 * 4);
      dst("dgamma", g.dgamma, Cin * 4, g.acc_params), dst("dbeta", g.dbeta, Cin * 4, g.acc_params);
      for (size_t n = 0; n < N && g.dfilm; ++n) fp.wr("dfilm", g.dfilm + n * g.film_stride, 2 * (size_t)g.film_cout * 4);  // sample n's (scale, shift) rows
      dst("gx0", g.gx0, N * V * g.C0 * 4, g.acc0), dst("gx1", g.gx1, N * V * g.C1 * 4, g.acc1);
      return true;
    }
    case BOP_ADD: dst("dst", op.add.dst, (size_t)op.add.n * 4, op.add.acc), fp.rd("src", op.add.src, (size_t)op.add.n * 4); return true;
    case BOP_SPLIT_CAT: {
      const SplitCat& s = op.split;
      fp.rd("g", s.g, (size_t)s.M * ((size_t)s.C0 + s.C1) * 4);
      dst("g0", s.g0, (size_t)s.M * s.C0 * 4, s.acc0), dst("g1", s.g1, (size_t)s.M * s.C1 * 4, s.acc1);
      return true;
    }
    case BOP_SUMPOOL2: {
      const SumPool2& s = op.pool;
      const size_t v = (size_t)s.R * s.R * s.R;
      fp.rd("gup", s.gup, (size_t)s.N * 8 * v * s.C * 4), dst("gin", s.gin, (size_t)s.N * v * s.C * 4, s.acc);
      return true;
    }
    case BOP_ZERO_INSERT2: {
      const ZeroInsert2& z = op.zins;
      const size_t v = (size_t)z.Rs * z.Rs * z.Rs;
      fp.rd("gy", z.gy, (size_t)z.N * v * z.C * 4), fp.wr("out", z.out, (size_t)z.N * 8 * v * z.C * 4);
      return true;
    }
    case BOP_DGRAD_S2: {
      const DgradS2& s = op.s2;
      fp.rd("gy", s.gy, (size_t)s.N * s.RO * s.RO * s.RO * s.Co * 4), dst("gx", s.gx, (size_t)s.N * s.RI * s.RI * s.RI * s.Ci * 4, s.acc);
      fp.param({s.wt});
      return true;
    }
    case BOP_GEMM: gemm_footprint(op.gemm, fp); return true;
    case BOP_SOFTMAX: fp.rw("S", op.softmax.S, (size_t)op.softmax.rows * op.softmax.cols * 4); return true;
    case BOP_ATTN_DS:
      fp.rd("P", op.ds.P, (size_t)op.ds.rows * op.ds.cols * 4), fp.rw("dP", op.ds.dP, (size_t)op.ds.rows * op.ds.cols * 4);
      return true;
    case BOP_TRANSPOSE: {
      const size_t bytes = (size_t)op.tr.batch * op.tr.T * op.tr.T * 4;
      fp.rd("in", op.tr.in, bytes), fp.wr("transposed", op.tr.out, bytes);
      return true;
    }
    case BOP_FILM_BWD: {
      const FilmBwd& f = op.film;
      fp.rd("dfilm", f.dfilm, (size_t)f.N * f.rows * 4), fp.rd("embs", f.embs, (size_t)f.N * f.K * 4);
      fp.param({f.w});
      fp.wr("dw", f.dw, (size_t)f.rows * f.K * 4), fp.wr("db", f.db, (size_t)f.rows * 4), fp.wr("gembs", f.gembs, (size_t)f.N * f.K * 4);
      return true;
    }
    case BOP_TEMB_BWD: {
      const TimeEmbedBwd& e = op.temb;
      fp.param({e.w1, e.b1, e.w2, e.b2});
      fp.rd("gembs", e.gembs, (size_t)e.N * e.ted * 4);
      fp.wr("dw1", e.dw1, (size_t)e.ted * e.mc * 4), fp.wr("db1", e.db1, (size_t)e.ted * 4);
      fp.wr("dw2", e.dw2, (size_t)e.ted * e.ted * 4), fp.wr("db2", e.db2, (size_t)e.ted * 4);
      return true;
    }
  }
  why = "no footprint for backward op kind " + std::to_string((int)op.kind);
  return false;
}

// the timeline of a training plan: entry i < n_fwd is forward op i, n_fwd the write of gy, n_fwd + 1 + k backward op k, the
// last one the read of gx
struct Timeline {
  Prints p;
  size_t n_fwd = 0;
  size_t at(int bop) const { return n_fwd + 1 + (size_t)bop; }
};
Timeline timeline(const TrainBuilt& t, const std::vector<BwdOp>& bops, const std::string& where) {
  Timeline tl;
  tl.n_fwd = t.b.plan.ops.size();
  tl.p = footprints(t.b.plan.ops, t.b, where);
  Footprint gy, gx;
  gy.wr("gy", reinterpret_cast<const void*>(WS + t.gy_off), t.gy_bytes);
  gx.rd("gx", reinterpret_cast<const void*>(WS + t.gx_off), t.gx_bytes);
  tl.p.fp.push_back(gy);
  for (size_t k = 0; k < bops.size(); ++k) {
    Footprint fp;
    std::string why;
    const std::string at = where + " backward op " + std::to_string(k);
    if (!bwd_footprint(bops[k], t.b, fp, why)) fail(at, why), tl.p.ok = false;
    for (const void* q : fp.pointers) {  // a workspace pointer outside every declared range
      const uintptr_t a = reinterpret_cast<uintptr_t>(q);
      if (a < WS || a >= WS + REGION) continue;
      bool in = false;
      for (const Range& r : fp.r) in = in || (a - WS >= r.off && a - WS < r.end());
      if (!in) fail(at, "a workspace pointer in no declared range of the op"), tl.p.ok = false;
    }
    tl.p.fp.push_back(fp);
  }
  tl.p.fp.push_back(gx);
  return tl;
}

// the rows [off, off + bytes) a batched GEMM writes, exactly (its footprint is the smallest enclosing range)
std::vector<std::pair<size_t, size_t>> gemm_rows(const GemmParams& g) {
  std::vector<std::pair<size_t, size_t>> v;
  for (int b0 = 0; b0 < g.nb0; ++b0)
    for (int b1 = 0; b1 < g.nb1; ++b1)
      for (int m = 0; m < g.M; ++m) {
        const size_t off = (size_t)(reinterpret_cast<uintptr_t>(g.C) - WS) + ((size_t)b0 * g.sc0 + (size_t)b1 * g.sc1 + (size_t)m * g.ldc) * 4;
        v.push_back({off, off + (size_t)g.Nn * 4});
      }
  std::sort(v.begin(), v.end());
  return v;
}
bool rows_disjoint(const std::vector<std::pair<size_t, size_t>>& a, const std::vector<std::pair<size_t, size_t>>& b) {
  size_t i = 0, j = 0;
  while (i < a.size() && j < b.size()) {
    if (a[i].second <= b[j].first) ++i;
    else if (b[j].second <= a[i].first) ++j;
    else return false;
  }
  return true;
}

// (f) gradient accounting: the backward ops that overwrite a gradient (a non-accumulating write that is not the first
// backward write to its range), or write what a forward op wrote; `missing`: the gradients nobody has written by the end.
// Two writes may meet a range twice by declaration: a transposition into the buffer an earlier transposition filled (the
// attention backward's one T x T scratch), and the three GEMMs that write q, k and v gradients into the interleaved thirds
// of one [M][3C] tensor - their rows are compared exactly.
std::set<int> check_gradients(const TrainBuilt& t, const std::vector<BwdOp>& bops, const Timeline& tl, std::vector<std::string>* missing = nullptr) {
  std::set<int> bad;
  const Prints& p = tl.p;
  for (size_t k = 0; k < bops.size(); ++k) {
    const Footprint& fp = p.fp[tl.at((int)k)];
    for (const Range& r : fp.r) {
      if (!r.wr) continue;
      for (size_t j = 0; j < tl.n_fwd; ++j)
        for (const Range& q : p.fp[j].r)
          if (q.wr && overlap(r, q)) bad.insert((int)k);
      bool accumulating = r.rd && !r.scratch;
      for (const Range& q : fp.r) accumulating = accumulating || (q.rd && !q.wr && q.off == r.off && q.bytes == r.bytes && !strcmp(q.name, "residual"));
      if (accumulating) continue;  // ((e) has checked that an earlier op wrote it)
      for (size_t j = tl.n_fwd; j < tl.at((int)k); ++j)
        for (const Range& q : p.fp[j].r) {
          if (!q.wr || !overlap(r, q)) continue;
          const BwdOp* other = j > tl.n_fwd ? &bops[j - tl.n_fwd - 1] : nullptr;
          const bool same = q.off == r.off && q.bytes == r.bytes;
          if (same && other && other->kind == BOP_TRANSPOSE && bops[k].kind == BOP_TRANSPOSE && !strcmp(r.name, "transposed")) continue;
          if (other && other->kind == BOP_GEMM && bops[k].kind == BOP_GEMM && !strcmp(r.name, "C") && !strcmp(q.name, "C") &&
              rows_disjoint(gemm_rows(other->gemm), gemm_rows(bops[k].gemm)))
            continue;
          bad.insert((int)k);
        }
    }
  }
  if (missing) {
    auto written = [&](size_t off, size_t bytes) {  // by the backward ops
      std::vector<std::pair<size_t, size_t>> open{{off, off + bytes}};
      for (size_t k = 0; k < bops.size() && !open.empty(); ++k)
        for (const Range& r : p.fp[tl.at((int)k)].r) {
          if (!r.wr) continue;
          std::vector<std::pair<size_t, size_t>> rest;
          for (const auto& o : open) {
            if (r.off >= o.second || r.end() <= o.first) {
              rest.push_back(o);
              continue;
            }
            if (o.first < r.off) rest.push_back({o.first, r.off});
            if (r.end() < o.second) rest.push_back({r.end(), o.second});
          }
          open.swap(rest);
        }
      return open.empty();
    };
    for (size_t i = 0; i < t.grad_off.size(); ++i)
      if (!written(t.grad_off[i], t.grad_bytes[i])) missing->push_back("the gradient of parameter " + std::to_string(i));
    if (!written(t.gx_off, t.gx_bytes)) missing->push_back("the gradient of the input");
  }
  return bad;
}

struct TrainCoverage {
  int split_cat = 0, res_identity = 0, attn = 0, zero_insert = 0, dgrad_s2 = 0, ups = 0, head = 0, wgrad_rows = 0, wgrad_tiles = 0, reduce_tile = 0,
      dgrad_splitk = 0, dgrad_wino = 0;
  void count(const TrainBuilt& t) {
    bool f[12] = {};
    for (const BwdOp& op : t.bops) {
      f[0] |= op.kind == BOP_SPLIT_CAT && t.res_concat_conv, f[2] |= op.kind == BOP_SOFTMAX, f[3] |= op.kind == BOP_ZERO_INSERT2, f[4] |= op.kind == BOP_DGRAD_S2;
      f[5] |= op.kind == BOP_SUMPOOL2;
      if (op.kind == BOP_WGRAD) {
        f[6] |= reinterpret_cast<uintptr_t>(op.wgrad.dw) == WS + t.head_dw;
        f[7] |= op.wgrad.plan.rows == 1, f[8] |= op.wgrad.plan.rows == 0, f[9] |= op.wgrad.plan.reduce_tile != 0;
      }
      if (op.kind == BOP_CONV) f[10] |= op.conv.nsplit > 1, f[11] |= op.conv.kernel == ConvKernel::Wino2 || op.conv.kernel == ConvKernel::Wino3;
    }
    f[1] = t.res_identity > 0;
    split_cat += f[0], res_identity += f[1], attn += f[2], zero_insert += f[3], dgrad_s2 += f[4], ups += f[5], head += f[6], wgrad_rows += f[7];
    wgrad_tiles += f[8], reduce_tile += f[9], dgrad_splitk += f[10], dgrad_wino += f[11];
  }
};

// checks (c), (e), (f) and the sizing passes of one training plan
void check_train(const TrainCase& c, const TrainBuilt& t) {
  const std::string where = train_name(c);
  const Timeline tl = timeline(t, t.bops, where);
  if (!tl.p.ok) return;
  for (int i : check_one_launch(tl.p)) fail(where + " timeline op " + std::to_string(i), "(c) the launch's own buffers overlap");
  check_reads_and_bounds(t.b, tl.p, where);
  std::vector<std::string> missing;
  for (int k : check_gradients(t, t.bops, tl, &missing))
    fail(where + " backward op " + std::to_string(k), "(f) overwrites a gradient an earlier op wrote, or writes the forward's tape");
  for (const std::string& m : missing) fail(where, "(f) nothing has written " + m);
  TrainBuilt z;  // the sizing pass with the same transposed weights: the same bytes and ops, up to addresses
  build_train(c, 1, z);
  g_mask_ws = true;
  const std::vector<std::string> placed = bwd_op_lines(t.bops);
  g_mask_ws = false;
  if (!z.b.plan.sizing || t.b.plan.sizing) fail(where, "Plan::sizing is not set by the sizing pass alone");
  if (z.b.plan.bytes != t.b.plan.bytes || z.b.err != t.b.err || z.gy_off != t.gy_off || z.gx_off != t.gx_off || z.grad_off != t.grad_off || z.blines != placed)
    fail(where, "the sizing pass plans something else than the placed plan");
}
#endif

std::vector<TrainCase> train_sweep() {
  std::vector<TrainCase> v;
  for (const char* net : TRAIN_NETS)
    for (int batch : TRAIN_BATCHES)
      for (int cus : CUS)
        for (int knob = 0; knob < (int)(sizeof TRAIN_KNOBS / sizeof TRAIN_KNOBS[0]); ++knob) v.push_back(TrainCase{net_index(net), batch, cus, knob});
  return v;
}

// the golden table at `path` against `lines`; ops_of: line -> the op lines of that plan (printed when the line differs)
int compare_table(const char* path, const std::vector<std::string>& lines, std::map<size_t, std::vector<std::string>>& ops_of) {
  FILE* f = fopen(path, "r");
  if (!f) {
    printf("cannot open %s\n", path);
    exit(2);
  }
  std::vector<std::string> golden;
  static char row[8192];
  while (fgets(row, sizeof row, f)) {
    std::string s = row;
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    golden.push_back(s);
  }
  fclose(f);
  int marked = 0, shown = 0;
  if (golden.size() != lines.size()) {
    printf("FAIL: %zu lines, the golden table %s has %zu\n", lines.size(), path, golden.size());
    ++failures;
    return 0;
  }
  for (size_t i = 0; i < lines.size(); ++i) {
    const bool star = golden[i].size() > 2 && golden[i].compare(golden[i].size() - 2, 2, " *") == 0;
    marked += star;
    if ((star ? golden[i].substr(0, golden[i].size() - 2) : golden[i]) != lines[i]) {
      fail(lines[i], "(a) differs from the golden table");
      if (failures <= 30) printf("     golden: %s\n", golden[i].c_str());
      if (++shown <= 3 && ops_of.count(i))  // (the hash moved: which op, which field?  this tree's op lines of that plan)
        for (const std::string& o : ops_of[i]) puts(o.c_str());
    }
  }
  return marked;
}

int self_test() {
  // the north-star net with the side lane on, exact fp32, batch 1: split-K convolutions with statistics and side launches
  const Case c{16, 0, 1, 0, 256, 0, 0};
  Built b;
  build_plan(c, false, b);
  const std::string where = "self-test";
  {
    const Prints p = footprints(b.plan.ops, b, where);
    if (!p.ok || !check_one_launch(p).empty() || !check_side_lane(b.plan.ops, p).empty() || !b.plan.n_joins) {
      printf("self-test: the undamaged plan does not pass, or has no side lane\n");
      return 1;
    }
  }
  int rc = 0;
  {  // 1. a split convolution's statistics pointed into its split-K scratch (the order of release and placement gone wrong)
    std::vector<Op> ops = b.plan.ops;
    int at = -1;
    for (size_t i = 0; i < ops.size() && at < 0; ++i)
      if (ops[i].kind == OP_CONV && ops[i].conv.nsplit > 1 && ops[i].conv.stats && ops[i].conv.partial) at = (int)i;
    if (at >= 0) ops[at].conv.stats = reinterpret_cast<double*>(ops[at].conv.partial);
    const Prints p = footprints(ops, b, where);
    const std::set<int> c_bad = check_one_launch(p), d_bad = check_side_lane(ops, p);
    const bool ok = at >= 0 && c_bad == std::set<int>{at} && d_bad.empty();
    printf("self-test 1: stats of op %d into its partial: (c) reports %zu op(s), (d) %zu: %s\n", at, c_bad.size(), d_bad.size(), ok ? "as planted" : "WRONG");
    rc |= !ok;
  }
  {  // 2. a side launch's output moved onto a buffer a main-lane op writes between the fork and the join
    std::vector<Op> ops = b.plan.ops;
    const Prints p0 = footprints(ops, b, where);
    int side = -1, consumer = -1, fork_at = -1;
    for (size_t i = 0; i < ops.size(); ++i) {
      if (ops[i].fork) fork_at = (int)i;
      if (ops[i].side && ops[i].kind == OP_CONV && side < 0) side = (int)i;
    }
    for (size_t i = 0; i < ops.size() && side >= 0; ++i)
      if (!ops[i].side && ops[i].join == ops[side].join) consumer = (int)i;
    const void* target = nullptr;
    for (int m = fork_at; m >= 0 && m < consumer && !target; ++m)
      if (!ops[m].side && ops[m].kind == OP_CONV) target = ops[m].conv.out;
    if (target) ops[side].conv.out = reinterpret_cast<float*>(const_cast<void*>(target));
    const Prints p = footprints(ops, b, where);
    const std::set<int> c_bad = check_one_launch(p), d_bad = check_side_lane(ops, p);
    const bool ok = target && d_bad == std::set<int>{side} && c_bad.empty();
    printf("self-test 2: output of side op %d onto a main-lane buffer: (d) reports %zu op(s), (c) %zu: %s\n", side, d_bad.size(), c_bad.size(),
           ok ? "as planted" : "WRONG");
    rc |= !ok;
  }
#ifndef UNET_PLAN_RECORD
  {  // the backward of `deep` at batch 1: three levels, attention, both Downsample routes' neighbours, concat ResBlocks
    const TrainCase tc{net_index("deep"), 1, 256, 0};
    TrainBuilt t;
    build_train(tc, 0, t);
    {
      const Timeline tl = timeline(t, t.bops, where);
      std::vector<std::string> missing;
      if (!tl.p.ok || !check_one_launch(tl.p).empty() || !check_gradients(t, t.bops, tl, &missing).empty() || !missing.empty()) {
        printf("self-test: the undamaged training plan does not pass\n");
        return 1;
      }
    }
    {  // 3. the accumulate flag of a second consumer cleared: it overwrites what the first consumer left
      std::vector<BwdOp> bops = t.bops;
      int at = -1;
      for (size_t k = 0; k < bops.size() && at < 0; ++k)
        if (bops[k].kind == BOP_GN_BWD && bops[k].gn.acc0) at = (int)k;
      if (at >= 0) bops[at].gn.acc0 = 0;
      const Timeline tl = timeline(t, bops, where);
      const std::set<int> c_bad = check_one_launch(tl.p), f_bad = check_gradients(t, bops, tl);
      const bool ok = at >= 0 && f_bad == std::set<int>{at} && c_bad.empty();
      printf("self-test 3: acc0 of backward op %d cleared: (f) reports %zu op(s), (c) %zu: %s\n", at, f_bad.size(), c_bad.size(), ok ? "as planted" : "WRONG");
      rc |= !ok;
    }
    {  // 4. a weight gradient's slab partials pointed at the gradient it reads
      std::vector<BwdOp> bops = t.bops;
      int at = -1;
      for (size_t k = 0; k < bops.size() && at < 0; ++k)
        if (bops[k].kind == BOP_WGRAD) at = (int)k;
      if (at >= 0) bops[at].wgrad.p.partial = const_cast<float*>(bops[at].wgrad.p.gy);
      const Timeline tl = timeline(t, bops, where);
      const std::set<int> c_bad = check_one_launch(tl.p);
      const bool ok = at >= 0 && c_bad == std::set<int>{(int)tl.at(at)};
      printf("self-test 4: partial of backward op %d onto its gy: (c) reports %zu op(s): %s\n", at, c_bad.size(), ok ? "as planted" : "WRONG");
      rc |= !ok;
    }
  }
#endif
  if (failures) rc = 1;
  printf(rc ? "unet_plan_check --self-test: FAILED\n" : "unet_plan_check --self-test: OK\n");
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--self-test")) return self_test();
  const bool train_only = argc > 1 && !strcmp(argv[1], "--train");
  if (argc == 2 && !train_only) {
    printf("usage: unet_plan_check [<forward table> <training table> | --train | --self-test]\n");
    return 2;
  }
  const std::vector<Case> cases = train_only ? std::vector<Case>() : sweep();
  std::vector<std::string> lines;
  std::map<size_t, std::vector<std::string>> ops_of;  // plan line -> that plan's op lines (printed when the line differs)
  const int n_knobs = (int)(sizeof KNOBS / sizeof KNOBS[0]);
  std::vector<int> knob_cases(n_knobs, 0), knob_bites(n_knobs, 0);
  Coverage cov;
  uint32_t n_full = 0, n_sizing = 0;
  for (size_t ci = 0; ci < cases.size(); ++ci) {
    const Case& c = cases[ci];
    Built b;
    build_plan(c, false, b);
    const std::vector<std::string> ops = op_lines(b.plan);
    lines.push_back(plan_line(c, b, ops));
    ops_of[lines.size() - 1] = ops;
    if (c.knob) {  // does the knob set change this plan?  (against the same case under the default knobs)
      Case c0 = c;
      c0.knob = 0;
      Built b0;
      build_plan(c0, false, b0);
      ++knob_cases[c.knob];
      knob_bites[c.knob] += b0.plan.bytes != b.plan.bytes || op_lines(b0.plan) != ops;
    }
#ifndef UNET_PLAN_RECORD
    {  // the sizing pass (no workspace, as holo_unet_workspace_bytes plans): flagged, the same bytes, the same ops but for addresses
      Built z;
      build_plan(c, false, z, 0);
      g_mask_ws = true;
      const std::vector<std::string> placed = op_lines(b.plan);
      g_null_ws = true;
      std::vector<std::string> sized = op_lines(z.plan);
      g_null_ws = g_mask_ws = false;
      for (std::string& l : sized) {  // (offset 0 of the workspace, the time embedding, is a null pointer there)
        const size_t at = l.find(" emb=0 ");
        if (at != std::string::npos) l.replace(at, 7, " emb=w ");
      }
      if (!z.plan.sizing || b.plan.sizing) fail(case_name(c), "Plan::sizing is not set by the sizing pass alone");
      if (z.plan.bytes != b.plan.bytes || z.err != b.err || sized != placed) fail(case_name(c), "the sizing pass plans something else than the placed plan");
      ++n_sizing;
    }
#endif
    if (c.net == FULL_NET && c.mode == 0 && c.batch == 1 && c.cus == 256 && !c.knob && !c.bi && !c.tape) {  // (one small plan in full)
      lines.insert(lines.end(), ops.begin(), ops.end());
      ++n_full;
    }
    if (!b.err.empty()) continue;  // (a plan the planner itself refuses - a batch-invariant batch it cannot keep - launches nothing)
    cov.count(c, b.plan);
    const std::string where = case_name(c);
    const Prints p = footprints(b.plan.ops, b, where);
    if (!p.ok) continue;
    for (int i : check_one_launch(p)) fail(where + " op " + std::to_string(i), "(c) the launch's own buffers overlap");
    std::string what;
    for (int i : check_side_lane(b.plan.ops, p, &what)) fail(where + " side op " + std::to_string(i), "(d) " + what);
    check_reads_and_bounds(b, p, where);
    if (!c.tape) {
      Built k;
      build_plan(c, true, k);
      const Prints pk = footprints(k.plan.ops, k, where + " (keeping)");
      if (pk.ok && k.err.empty()) check_producers(b, p, k, pk, where);
      else fail(where, "the keeping plan cannot be built");
    }
  }
  if (argc < 2) {
    for (const std::string& l : lines) puts(l.c_str());
    return failures ? 1 : 0;
  }
  // ---- the training plans: every net of TRAIN_NETS x batch x CU count x knob set, and per (net, batch) the sizing pass on no
  // transposed weights
  std::vector<std::string> tlines;
  std::map<size_t, std::vector<std::string>> tops_of;
  const int n_tknobs = (int)(sizeof TRAIN_KNOBS / sizeof TRAIN_KNOBS[0]);
  std::vector<int> tknob_cases(n_tknobs, 0), tknob_bites(n_tknobs, 0);
  uint32_t n_train = 0, n_train_full = 0;
#ifndef UNET_PLAN_RECORD
  TrainCoverage tcov;
#endif
  std::vector<std::string> default_lines;  // of the same case under the default knobs (the sweep's order: knob 0 first)
  size_t default_bytes = 0;
  for (const TrainCase& c : train_sweep()) {
    TrainBuilt t;
    build_train(c, 0, t);
    tlines.push_back(train_line(train_name(c), t));
    tops_of[tlines.size() - 1] = t.blines;
    ++n_train;
    if (!c.knob) default_lines = t.blines, default_bytes = t.b.plan.bytes;
    else ++tknob_cases[c.knob], tknob_bites[c.knob] += default_bytes != t.b.plan.bytes || default_lines != t.blines;
    if (!strcmp(NETS[c.net].name, TRAIN_FULL_NET) && c.batch == 1 && c.cus == 256 && !c.knob) {
      tlines.insert(tlines.end(), t.blines.begin(), t.blines.end());
      ++n_train_full;
    }
    if (c.cus == 256 && !c.knob) {
      TrainBuilt z;
      build_train(c, 2, z);
      tlines.push_back(train_line(train_name(c) + " sizing-empty", z));
    }
    if (!t.b.err.empty()) {
      fail(train_name(c), "the training plan cannot be built: " + t.b.err);
      continue;
    }
#ifndef UNET_PLAN_RECORD
    tcov.count(t);
    check_train(c, t);
#endif
  }
  if (train_only) {
    for (const std::string& l : tlines) puts(l.c_str());
    return failures ? 1 : 0;
  }
  // (a) the golden tables
  int marked = compare_table(argv[1], lines, ops_of);
  marked += compare_table(argv[2], tlines, tops_of);
  const struct {
    const char* what;
    int n;
  } need[] = {{"a side lane", cov.side}, {"the packed bf16 attention", cov.bf16_attn}, {"the GEMM / softmax attention", cov.gemm_attn},
              {"split key ranges in the fp32 flash kernel", cov.flash_split}, {"a split-K convolution that writes statistics", cov.split_stats},
              {"a fused skip", cov.fused_skip}, {"a separate 1x1x1 skip", cov.own_skip}, {"an Upsample", cov.ups}, {"a Downsample", cov.down},
              {"a batch-invariant batch > 1", cov.bi}, {"a tape", cov.tape}};
  for (const auto& n : need) {
    printf("%-48s %5d plans\n", n.what, n.n);
    if (n.n == 0) {
      printf("FAIL: no plan of the sweep has %s\n", n.what);
      ++failures;
    }
  }
  for (int k = 1; k < n_knobs; ++k) {  // a knob set that changes no plan of the sweep checks nothing
    printf("knob set %-14s changes %3d of its %3d plans\n", KNOBS[k].tag, knob_bites[k], knob_cases[k]);
    if (!knob_bites[k]) {
      printf("FAIL: knob set %s changes no plan against the default knobs\n", KNOBS[k].tag);
      ++failures;
    }
  }
#ifndef UNET_PLAN_RECORD
  const struct {
    const char* what;
    int n;
  } tneed[] = {{"a concat ResBlock with a conv skip (split_cat)", tcov.split_cat}, {"a ResBlock with an identity skip", tcov.res_identity},
               {"an attention block's backward", tcov.attn}, {"a Downsample on the zero-insert route", tcov.zero_insert},
               {"a Downsample on conv_dgrad_s2", tcov.dgrad_s2}, {"an Upsample's backward", tcov.ups}, {"the head's backward", tcov.head},
               {"the row-staged wgrad kernel", tcov.wgrad_rows}, {"the tile wgrad kernel", tcov.wgrad_tiles}, {"the tile reduce", tcov.reduce_tile},
               {"a split-K dgrad", tcov.dgrad_splitk}, {"a dgrad on a Winograd copy", tcov.dgrad_wino}};
  for (const auto& n : tneed) {
    printf("%-48s %5d training plans\n", n.what, n.n);
    if (n.n == 0) {
      printf("FAIL: no training plan of the sweep has %s\n", n.what);
      ++failures;
    }
  }
#endif
  for (int k = 1; k < n_tknobs; ++k) {
    printf("knob set %-14s changes %3d of its %3d training plans\n", TRAIN_KNOBS[k].tag, tknob_bites[k], tknob_cases[k]);
    if (!tknob_bites[k]) {
      printf("FAIL: knob set %s changes no training plan against the default knobs\n", TRAIN_KNOBS[k].tag);
      ++failures;
    }
  }
  printf("%zu plans, %u of them with their op lines, %u sizing passes; %u training plans, %u of them with their op lines, %d lines marked\n",
         cases.size(), n_full, n_sizing, n_train, n_train_full, marked);
  if (failures) {
    printf("unet_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  printf("unet_plan_check: OK\n");
  return 0;
}
