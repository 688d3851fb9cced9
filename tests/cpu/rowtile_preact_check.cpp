// rowtile_preact_check.cpp — unetplan::preactivate_rowtile (unet_plan.cpp) checked on the CPU: a stand-alone program, no HIP,
// nothing dereferenced.  It builds forward plans on made-up addresses as unet_plan_check.cpp does, runs the pass over a copy
// and compares the copy with what Planner::build() made.  tests/test_rowtile_preact_cpu.py compiles it with unet_plan.cpp,
// unet_train_plan.cpp and conv_plan.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.
//
// Per (net, batch), exact fp32, 256 CUs:
//   (a) WHICH pairs are rewritten: the north-star net (batch 1 and 4) exactly its fourteen 4^3 GroupNorm + SiLU 3x3x3
//       convolutions and the middle attention's 1x1x1 qkv convolution (affine only), nothing at 8^3 and above; the seam net (8^3,
//       256 model channels, attention at 4^3) fourteen, one of them over the (512 + 256) concat whose 24-channel group at the
//       seam straddles it; none with HOLO_ROWTILE_PREACT=0; none in a plan without an activated row-tile convolution (u64l);
//   (b) the scratch lies in [bytes of build(), bytes after the pass), is as large as the largest rewritten tensor, and the only
//       pointers into it are a rewritten finalize's `act` and its convolution's `src0`;
//   (c) between a finalize and its convolution no main-lane op stands (side-lane ops never touch the scratch: (b));
//   (d) the sizing pass (no workspace) and the placed pass rewrite the same ops, with the same offsets and the same bytes;
//   (e) every op the pass did not rewrite is byte-equal to build()'s, and a rewritten op differs in the named fields only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "unet_plan.h"

using namespace holo;
using namespace holo::unetplan;

namespace {

struct NetCfg {
  const char* name;
  int R, cin, cout, mc, nrb;
  std::vector<int> mult, attn;
  int heads;
};
const NetCfg NORTH = {"north", 64, 32, 32, 64, 2, {1, 1, 2, 4, 8}, {4, 8}, 2};
const NetCfg SEAM = {"seam", 8, 16, 16, 256, 1, {1, 2}, {2}, 2};
const NetCfg U64L = {"u64l", 64, 32, 32, 64, 1, {1, 1, 1}, {}, 2};

const uintptr_t WS = (uintptr_t)1 << 44, ST_F32 = (uintptr_t)2 << 44, ST_BF = (uintptr_t)3 << 44, ST_WINO = (uintptr_t)4 << 44;

int failures = 0;
void fail(const std::string& where, const std::string& what) {
  if (++failures <= 30) printf("FAIL %s: %s\n", where.c_str(), what.c_str());
}

void make_desc(UnetDesc& d, const NetCfg& n) {
  memset(&d.cfg, 0, sizeof d.cfg);
  d.cfg.image_size = n.R, d.cfg.in_channels = n.cin, d.cfg.out_channels = n.cout, d.cfg.model_channels = n.mc;
  d.cfg.num_res_blocks = n.nrb, d.cfg.num_heads = n.heads, d.cfg.homogeneous_resample = 1;
  d.cfg.n_channel_mult = (int)n.mult.size();
  for (size_t i = 0; i < n.mult.size(); ++i) d.cfg.channel_mult[i] = n.mult[i];
  d.cfg.n_attention_resolutions = (int)n.attn.size();
  for (size_t i = 0; i < n.attn.size(); ++i) d.cfg.attention_resolutions[i] = n.attn[i];
  d.num_cus = 256;
  build_structure(&d);
  enumerate_params(&d);
  d.knobs = Knobs::from_env();
  d.compute_mode = 0;
  carve_params(&d, nullptr, nullptr, nullptr);
  carve_params(&d, reinterpret_cast<float*>(ST_F32), reinterpret_cast<uint16_t*>(ST_BF), reinterpret_cast<float*>(ST_WINO));
}

struct Built {
  Plan before, after;  // build()'s plan, and a copy the pass ran over
  Preact pre;
  std::string err;
};
// as unet_exec.cpp does behind both of its Planner(...).build() sites
void build(const NetCfg& n, int batch, uintptr_t ws, Built& b) {
  UnetDesc d;
  make_desc(d, n);
  Planner pl(&d, batch, reinterpret_cast<void*>(ws), b.before);
  pl.build();
  b.err = pl.err;
  b.after = b.before;
  b.pre = preactivate_rowtile(b.after, pl.knobs);
}

bool same(const Op& a, const Op& b) { return memcmp(&a, &b, sizeof(Op)) == 0; }

// every pointer of an op that may lie in the workspace
std::vector<const void*> pointers(const Op& o) {
  switch (o.kind) {
    case OP_IN: return {o.in.dst};
    case OP_OUT: return {o.out.src};
    case OP_TEMB: return {o.temb.emb, o.temb.emb_silu};
    case OP_EMBLIN: return {o.emblin.emb_silu, o.emblin.out};
    case OP_STATS: return {o.stats.x, o.stats.part};
    case OP_FINAL: return {o.fin.part0, o.fin.part1, o.fin.film, o.fin.coef, o.fin.moments, o.fin.x0, o.fin.x1, o.fin.act};
    case OP_CONV:
      return {o.conv.src0, o.conv.src1, o.conv.coef, o.conv.residual, o.conv.out, o.conv.skip_src0, o.conv.skip_src1, o.conv.stats,
              o.conv.partial, o.conv.qkv_q, o.conv.qkv_k, o.conv.qkv_vt};
    case OP_GEMM: return {};  // (its operands are views of attention scratch inside build()'s arena: GEMM plans are not at 4^3 here)
    case OP_SOFTMAX: return {o.softmax.S};
    case OP_FLASH: return {o.flash.attn.qkv, o.flash.attn.out, o.flash.attn.part, o.flash.attn.part_ml, o.flash.packed};
  }
  return {};
}

struct Pair {
  size_t fin, conv;
};

// (b), (c), (e) on one built plan; returns the rewritten pairs
std::vector<Pair> check_plan(const std::string& where, const Built& b, int batch, uintptr_t ws) {
  std::vector<Pair> pairs;
  const Plan &p0 = b.before, &p1 = b.after;
  if (!b.err.empty()) fail(where, "planner error: " + b.err);
  if (p0.ops.size() != p1.ops.size()) {
    fail(where, "the pass changed the number of ops");
    return pairs;
  }
  const uintptr_t s_lo = ws + b.pre.scratch_off, s_hi = s_lo + b.pre.scratch_bytes;
  std::set<size_t> touched;
  for (size_t i = 0; i < p1.ops.size(); ++i) {
    const Op& o = p1.ops[i];
    if (o.kind != OP_FINAL || !o.fin.act) continue;
    size_t j = i + 1;
    while (j < p1.ops.size() && p1.ops[j].side) ++j;  // (c): the next op of the caller's stream is the consumer
    if (j == p1.ops.size() || p1.ops[j].kind != OP_CONV || p1.ops[j].conv.src0 != o.fin.act) {
      fail(where, "op " + std::to_string(i) + ": the next main-lane op behind a pre-activating finalize is not its convolution");
      continue;
    }
    pairs.push_back(Pair{i, j});
    touched.insert(i), touched.insert(j);
    // (e) the rewritten ops: build()'s with the named fields changed
    const ConvParams& c0 = p0.ops[j].conv;
    Op f = p0.ops[i], c = p0.ops[j];
    f.fin.x0 = c0.src0, f.fin.x1 = c0.src1, f.fin.act = reinterpret_cast<float*>(s_lo), f.fin.act_silu = c0.act;
    c.conv.src0 = reinterpret_cast<const float*>(s_lo), c.conv.C0 = c0.C0 + c0.C1, c.conv.src1 = nullptr, c.conv.C1 = 0;
    c.conv.coef = nullptr, c.conv.act = 0;
    if (!same(f, o)) fail(where, "op " + std::to_string(i) + ": the finalize differs from build()'s in more than its four new fields");
    if (!same(c, p1.ops[j])) fail(where, "op " + std::to_string(j) + ": the convolution differs in more than src0 / C0 / src1 / C1 / coef / act");
    if (c0.coef != p0.ops[i].fin.coef || !c0.coef) fail(where, "op " + std::to_string(j) + ": did not read that finalize's coefficients");
    if (c0.kernel != ConvKernel::RowTile || c0.bf16 || c0.in_bf16 || c0.ups) fail(where, "op " + std::to_string(j) + ": not an exact-fp32 row-tile launch");
    if (!conv_can_launch(p1.ops[j].conv)) fail(where, "op " + std::to_string(j) + ": the rewritten launch is refused by conv_can_launch");
    const size_t bytes = (size_t)batch * c0.ID * c0.IH * c0.IW * (c0.C0 + c0.C1) * sizeof(float);
    if (bytes > b.pre.scratch_bytes) fail(where, "op " + std::to_string(j) + ": its tensor is larger than the scratch");
    const PreactShape s{(c0.C0 + c0.C1) / p0.ops[i].fin.groups, c0.C0, (int64_t)c0.ID * c0.IH * c0.IW, c0.ksz * c0.ksz * c0.ksz * ((c0.Cout + 63) / 64)};
    if (preact_refusal(s)) fail(where, "op " + std::to_string(j) + ": rewritten against the predicate: " + preact_refusal(s));
  }
  // (e) everything else is build()'s, byte for byte; (b) and nothing else points into the scratch
  for (size_t i = 0; i < p1.ops.size(); ++i) {
    if (!touched.count(i) && !same(p0.ops[i], p1.ops[i])) fail(where, "op " + std::to_string(i) + " was not rewritten and differs from build()'s");
    const std::vector<const void*> ptrs = pointers(p1.ops[i]);
    for (size_t k = 0; k < ptrs.size(); ++k) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(ptrs[k]);
      if (!ptrs[k] || a < ws + p0.bytes || a >= ws + p0.bytes + ((uintptr_t)1 << 40)) continue;  // (weights and parameters lie elsewhere)
      const bool own = touched.count(i) && ((p1.ops[i].kind == OP_FINAL && ptrs[k] == p1.ops[i].fin.act) ||
                                            (p1.ops[i].kind == OP_CONV && ptrs[k] == p1.ops[i].conv.src0));
      if (!own) fail(where, "op " + std::to_string(i) + " points behind build()'s workspace without being one of a pair");
      if (a != s_lo) fail(where, "op " + std::to_string(i) + ": a pointer into the scratch that is not its start");
    }
  }
  // (b)
  if (pairs.empty()) {
    if (p1.bytes != p0.bytes) fail(where, "no pair, but the workspace grew");
  } else {
    size_t want = 0;
    for (const Pair& pr : pairs) {
      const ConvParams& c0 = p0.ops[pr.conv].conv;
      const size_t bytes = (size_t)batch * c0.ID * c0.IH * c0.IW * (c0.C0 + c0.C1) * sizeof(float);
      if (bytes > want) want = bytes;
    }
    if (b.pre.scratch_bytes != want) fail(where, "the scratch is not the largest rewritten tensor");
    if (b.pre.scratch_off < p0.bytes || (b.pre.scratch_off & 255) || b.pre.scratch_off + b.pre.scratch_bytes > p1.bytes)
      fail(where, "the scratch does not lie in [bytes of build(), reported bytes), aligned");
  }
  if ((int)pairs.size() != b.pre.pairs) fail(where, "the pass reports another number of pairs than the plan holds");
  return pairs;
}

// (d) + (b), (c), (e) of both passes
std::vector<Pair> check_net(const NetCfg& n, int batch, Built* placed_out = nullptr) {
  const std::string where = std::string(n.name) + " n" + std::to_string(batch);
  Built placed, sizing;
  build(n, batch, WS, placed);
  build(n, batch, 0, sizing);
  const std::vector<Pair> pp = check_plan(where, placed, batch, WS), ps = check_plan(where + " sizing", sizing, batch, 0);
  if (!sizing.before.sizing || placed.before.sizing) fail(where, "which pass is the sizing pass");
  if (pp.size() != ps.size() || placed.after.bytes != sizing.after.bytes || placed.pre.scratch_off != sizing.pre.scratch_off ||
      placed.pre.scratch_bytes != sizing.pre.scratch_bytes)
    fail(where, "the sizing pass and the placed pass disagree");
  for (size_t k = 0; k < pp.size() && k < ps.size(); ++k)
    if (pp[k].fin != ps[k].fin || pp[k].conv != ps[k].conv) fail(where, "the sizing pass rewrote other ops");
  printf("%s: %zu pairs, scratch %zu bytes at %zu, workspace %zu -> %zu\n", where.c_str(), pp.size(), placed.pre.scratch_bytes,
         placed.pre.scratch_off, placed.before.bytes, placed.after.bytes);
  if (placed_out) *placed_out = placed;
  return pp;
}

}  // namespace

int main() {
  unsetenv("HOLO_ROWTILE_PREACT");
  // (a) the north-star net
  for (int batch : {1, 4}) {
    Built b;
    const std::vector<Pair> pairs = check_net(NORTH, batch, &b);
    const std::string where = "north n" + std::to_string(batch);
    int n3 = 0, nqkv = 0;
    for (const Pair& pr : pairs) {
      const ConvParams& c0 = b.before.ops[pr.conv].conv;
      const GnFinalize& f = b.after.ops[pr.fin].fin;
      if (c0.ID != 4 || c0.OD != 4) fail(where, "a pair off the 4^3 level");
      if (c0.ksz == 3 && c0.act == 1 && f.act_silu == 1) ++n3;
      if (c0.ksz == 1 && c0.act == 0 && f.act_silu == 0 && c0.C0 == 512 && c0.Cout == 1536) ++nqkv;
    }
    if (pairs.size() != 15 || n3 != 14 || nqkv != 1)
      fail(where, "expected the fourteen 4^3 GroupNorm + SiLU 3x3x3 convolutions and the qkv convolution, got " + std::to_string(pairs.size()) +
                      " pairs (" + std::to_string(n3) + " + " + std::to_string(nqkv) + ")");
    if (b.pre.scratch_bytes != (size_t)batch * 64 * 1024 * 4) fail(where, "the scratch is not batch x 256 KB");
    int seam = 0;
    for (const Pair& pr : pairs) seam += b.after.ops[pr.fin].fin.x1 != nullptr;
    if (seam != 3) fail(where, "expected the three concat convolutions of the way up among the pairs");
  }
  // (a) a group across the concat seam
  {
    Built b;
    const std::vector<Pair> pairs = check_net(SEAM, 1, &b);
    int straddle = 0, qkv = 0;
    for (const Pair& pr : pairs) {
      const GnFinalize& f = b.after.ops[pr.fin].fin;
      const int cpg = (f.C0 + f.C1) / f.groups;
      straddle += f.x1 && f.C0 % cpg != 0;
      qkv += b.before.ops[pr.conv].conv.ksz == 1;
    }
    if (pairs.size() != 14 || straddle != 1 || qkv != 4)
      fail("seam n1", "expected 14 pairs, one with a group across the seam, four qkv convolutions; got " + std::to_string(pairs.size()) + ", " +
                          std::to_string(straddle) + ", " + std::to_string(qkv));
  }
  // (a) no activated row-tile convolution: nothing to rewrite
  if (!check_net(U64L, 1).empty()) fail("u64l n1", "a plan without an activated row-tile convolution was rewritten");
  // (a) the knob at 0
  setenv("HOLO_ROWTILE_PREACT", "0", 1);
  for (const NetCfg* n : {&NORTH, &SEAM})
    if (!check_net(*n, 1).empty()) fail(std::string(n->name) + " knob 0", "pairs were rewritten");
  unsetenv("HOLO_ROWTILE_PREACT");
  if (failures) {
    printf("rowtile_preact_check: %d FAILURES\n", failures);
    return 1;
  }
  printf("rowtile_preact_check: OK\n");
  return 0;
}
