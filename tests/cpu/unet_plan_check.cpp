// unet_plan_check.cpp — the denoiser's planner (holo_diffusion_amd/csrc/unet_plan.cpp) swept on the CPU: what a plan launches,
// and that no launch reads memory another launch was allowed to overwrite.
//
// A stand-alone program (its own main, no HIP, nothing loaded into Python), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_unet_plan_cpu.py:
//   unet_plan_check <golden table>    checks (a) .. (e) and the coverage condition below
//   unet_plan_check                   prints the table only
//   unet_plan_check --self-test       damages one good plan in two ways and asserts that (c) and (d) name exactly the damaged ops
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
// -DUNET_PLAN_RECORD: the including file has brought a tree's planner in already (a `Desc` type that Planner takes, and
// set_cus); the program then runs on that planner.  That is how the golden table is recorded from the parent commit.
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
#include "unet_plan.h"
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
};
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
const uintptr_t REGION = (uintptr_t)1 << 44;  // no store and no workspace is as large

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
int failures = 0;
void fail(const std::string& where, const std::string& what) {
  if (++failures <= 30) printf("FAIL %s: %s\n", where.c_str(), what.c_str());
}

std::string addr(const void* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  char buf[40];
  if (!a) return "0";
  if (g_null_ws && a < WS) return "w";
  const char* tag = a >= WS && a < WS + REGION ? "w" : a >= ST_F32 && a < ST_F32 + REGION ? "f" : a >= ST_BF && a < ST_BF + REGION ? "b" :
                    a >= ST_WINO && a < ST_WINO + REGION ? "v" : nullptr;
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
    case OP_CONV: {
      const ConvParams& c = op.conv;
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
      break;
    }
    case OP_GEMM: {
      const GemmParams& g = op.gemm;
      l.p("A", g.A).p("B", g.B).p("C", g.C).i("M", g.M).i("Nn", g.Nn).i("K", g.K).i("lda", g.lda).i("ldb", g.ldb).i("ldc", g.ldc).i("nb0", g.nb0)
          .i("nb1", g.nb1).i("sa0", g.sa0).i("sa1", g.sa1).i("sb0", g.sb0).i("sb1", g.sb1).i("sc0", g.sc0).i("sc1", g.sc1)
          .i("b_kmajor", g.b_kmajor).f("alpha", g.alpha);
      break;
    }
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
  size_t end() const { return off + bytes; }
};
bool overlap(const Range& a, const Range& b) { return a.bytes && b.bytes && a.off < b.end() && b.off < a.end(); }

struct Footprint {
  std::vector<Range> r;
  std::vector<const void*> pointers;  // every pointer field of the op: the workspace ones must lie in a declared range
  void add(const char* name, const void* p, size_t bytes, bool rd, bool wr) {
    pointers.push_back(p);
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a >= WS && a < WS + REGION && bytes) r.push_back({name, (size_t)(a - WS), bytes, rd, wr});
  }
  void rd(const char* n, const void* p, size_t b) { add(n, p, b, true, false); }
  void wr(const char* n, const void* p, size_t b) { add(n, p, b, false, true); }
  void rw(const char* n, const void* p, size_t b) { add(n, p, b, true, true); }
  // a parameter store pointer (read-only memory no launch of a plan writes): it must not point into the workspace
  void param(std::initializer_list<const void*> ps) { pointers.insert(pointers.end(), ps); }
};

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
    case OP_CONV: {
      const ConvParams& c = op.conv;
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
        fp.r.push_back({"out(unwritten)", (size_t)(reinterpret_cast<uintptr_t>(c.out) - WS), N * Vout * c.Cout * (c.out_bf16 ? 2 : 4), false, false});
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
      const size_t sb = conv_plan(again, op.side ? (int)b.knobs.side_lane_cus : b.cus, b.knobs, b.plan_n);
      if (again.kernel != c.kernel || again.nsplit != c.nsplit || (sb != 0) != (c.partial != nullptr)) {
        why = "conv_plan re-run on the op's parameters chooses another launch";
        return false;
      }
      fp.rw("partial", c.partial, sb);
      fp.param({c.w, c.bias, c.skip_w, c.skip_bias, c.w_bf, c.skip_w_bf, c.w_wino2, c.skip_w_wino2, c.w_wino3, c.skip_w_wino3, c.w_bft,
                c.skip_w_bft, c.dbg});
      return true;
    }
    case OP_GEMM: {
      const GemmParams& g = op.gemm;  // strided operands: the smallest enclosing range
      const size_t ba = (size_t)(g.nb0 - 1) * g.sa0 + (size_t)(g.nb1 - 1) * g.sa1, bb = (size_t)(g.nb0 - 1) * g.sb0 + (size_t)(g.nb1 - 1) * g.sb1,
                   bc = (size_t)(g.nb0 - 1) * g.sc0 + (size_t)(g.nb1 - 1) * g.sc1;
      fp.rd("A", g.A, (ba + (size_t)(g.M - 1) * g.lda + g.K) * 4);
      fp.rd("B", g.B, (bb + (g.b_kmajor ? (size_t)(g.K - 1) * g.ldb + g.Nn : (size_t)(g.Nn - 1) * g.ldb + g.K)) * 4);
      fp.wr("C", g.C, (bc + (size_t)(g.M - 1) * g.ldc + g.Nn) * 4);
      return true;
    }
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
        fp.add("packed", f.packed, operands, true, !f.operands_packed);
        fp.rw("packed_work", (const char*)f.packed + operands, flash_attn_bf16v2_workspace_bytes(f.attn, f.ksplit) - operands);
        fp.wr("out", f.attn.out, ntc * (f.out_bf16 ? 2 : 4));
        if (f.operands_packed) fp.r.push_back({"qkv(unread)", (size_t)(reinterpret_cast<uintptr_t>(f.attn.qkv) - WS), ntc * 3 * 4, false, false});
      } else if (f.form == 0) {
        fp.rd("qkv", f.attn.qkv, ntc * 3 * 4);
        fp.rw("part", f.attn.part, flash_attn_workspace_bytes(f.attn));
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
std::set<int> check_one_launch(const std::vector<Op>& ops, const Prints& p) {
  std::set<int> bad;
  for (size_t i = 0; i < ops.size(); ++i) {
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
      if (!covered && !(r.wr && (!strcmp(r.name, "partial") || !strcmp(r.name, "part") || !strncmp(r.name, "packed", 6))))
        fail(at, "read before it is written");  // (scratch a launch fills itself before it reads it is read-write and exempt)
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
  const int n_nets = (int)(sizeof NETS / sizeof NETS[0]), n_knobs = (int)(sizeof KNOBS / sizeof KNOBS[0]);
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

int self_test() {
  // the north-star net with the side lane on, exact fp32, batch 1: split-K convolutions with statistics and side launches
  const Case c{16, 0, 1, 0, 256, 0, 0};
  Built b;
  build_plan(c, false, b);
  const std::string where = "self-test";
  {
    const Prints p = footprints(b.plan.ops, b, where);
    if (!p.ok || !check_one_launch(b.plan.ops, p).empty() || !check_side_lane(b.plan.ops, p).empty() || !b.plan.n_joins) {
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
    const std::set<int> c_bad = check_one_launch(ops, p), d_bad = check_side_lane(ops, p);
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
    const std::set<int> c_bad = check_one_launch(ops, p), d_bad = check_side_lane(ops, p);
    const bool ok = target && d_bad == std::set<int>{side} && c_bad.empty();
    printf("self-test 2: output of side op %d onto a main-lane buffer: (d) reports %zu op(s), (c) %zu: %s\n", side, d_bad.size(), c_bad.size(),
           ok ? "as planted" : "WRONG");
    rc |= !ok;
  }
  if (failures) rc = 1;
  printf(rc ? "unet_plan_check --self-test: FAILED\n" : "unet_plan_check --self-test: OK\n");
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--self-test")) return self_test();
  const std::vector<Case> cases = sweep();
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
    for (int i : check_one_launch(b.plan.ops, p)) fail(where + " op " + std::to_string(i), "(c) the launch's own buffers overlap");
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
  // (a) the golden table
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    printf("cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<std::string> golden;
  static char row[8192];
  while (fgets(row, sizeof row, f)) {
    std::string s = row;
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    golden.push_back(s);
  }
  fclose(f);
  int marked = 0;
  if (golden.size() != lines.size()) {
    printf("FAIL: %zu lines, the golden table has %zu\n", lines.size(), golden.size());
    ++failures;
  } else {
    for (size_t i = 0; i < lines.size(); ++i) {
      const bool star = golden[i].size() > 2 && golden[i].compare(golden[i].size() - 2, 2, " *") == 0;
      marked += star;
      if ((star ? golden[i].substr(0, golden[i].size() - 2) : golden[i]) != lines[i]) {
        fail(lines[i], "(a) differs from the golden table");
        if (failures <= 30) printf("     golden: %s\n", golden[i].c_str());
        if (failures <= 3 && ops_of.count(i))  // (the hash moved: which op, which field?  this tree's op lines of that plan)
          for (const std::string& o : ops_of[i]) puts(o.c_str());
      }
    }
  }
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
  printf("%zu plans, %u of them with their op lines, %u sizing passes, %d lines marked\n", cases.size(), n_full, n_sizing, marked);
  if (failures) {
    printf("unet_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  printf("unet_plan_check: OK\n");
  return 0;
}
