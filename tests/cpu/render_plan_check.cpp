// render_plan_check.cpp — the renderer's launch plan (holo_diffusion_amd/csrc/render_plan.h) and the view-pool workspace
// layouts (viewpool_layout.h) swept on the CPU.
//
// A stand-alone program (its own main, no HIP, nothing loaded into Python), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_render_plan_cpu.py:
//   render_plan_check <golden table>    prints nothing but the verdict: the table equals the golden one, every check below holds
//   render_plan_check                   prints the table only (thinned, with the digest of the full one: see `kept`)
//   render_plan_check --full            prints the full table
//   render_plan_check --self-test       plants faults in good plans and launch lists; the checks must name exactly those
// The sweep (not a full cross product: the full table is 5 112 lines; the committed one is thinned to a tenth)
//   shapes   16 / 32 / 64 features; normals on / off; the bf16x3 split ACTIVE on / off (it can only be at 32 features);
//            evaluation and training mode (training mode as the library plans it: no normals, no split)
//   counts   the (coarse, fine) pairs of tests/test_gpu_render_sample_counts.py::COUNTS and (64, 64)
//   chips    8, 20, 32 CUs on an 8^3 grid, 256 CUs on a 64^3 grid; emu false / true
//   knobs    the defaults over all of the above; each HOLO_RENDER* knob at the value the GPU tests give it (HOLO_RENDER_WGS,
//            which no test sets, at 7) over the counts (64, 64) and (64, 128) at 8 and 256 CUs
// gives one `plan` line each: the inputs, then the workspace bytes, the kernel instantiation and its workgroup size.
// Launch lists (`list` lines: p = index of the plan line, then per launch first camera + cameras, tiles, workgroups, XCD
// ranges, dynamic hand-out, tail) are made for 1, 4, 30, 32, 33, 40, 65 cameras x frames of 6 x 7, 16 x 16, 400 x 400 pixels
// (ray lists of 13 and 4096 rays in training mode) for the default-knob plans at (9, 7) - and at (64, 128) for 16 features -,
// and for 4 and 40 cameras x the smallest and the largest frame (ray list) for the knob plans at (64, 64).
// `vp` lines: the totals of holo_view_pool_workspace_bytes / holo_view_pool_backward_workspace_bytes for 1 .. 8 maps with
// channel counts off the multiples of four, 1 and 16 views, 8 and 256 CUs, deterministic off / on.
//
// Checked from each plan's own fields (check_plan, check_list, check_view_pool below): the workspace regions are 256-aligned,
// disjoint and in order, total = the last end + the pad; the ray-per-column scratch holds workgroup cap x waves slots of
// 32 KB (and the same again with normals); the counter region holds eight ints; waves = the constexpr rule of the chosen
// instantiation, or exactly 8 where a knob (or emu, for the tiled normals) selects the 8-wave form; 64 x waves <= 1024;
// render_can_launch accepts the plan; every launch has 1 .. 32 cameras and 1 .. cap workgroups; the launches cover the
// cameras once, in order; evaluation groups differ in size by at most one; xcd > 1 only on a full launch whose workgroups
// divide by it; tail and counters only with dynamic hand-out; render_can_launch refuses the hand-made bad plans (what the
// launcher's switch used to refuse); every instantiation the launcher's switch holds is planned at least once.
// What this does NOT prove: that a kernel stays inside the slot and the rows it is given - the GPU tests remain that check.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "render_plan.h"
#include "viewpool_layout.h"

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
  void (*apply)(Knobs&);
};
const KnobSet KNOBS[] = {
    {"default", [](Knobs&) {}},
    {"v1", [](Knobs& k) { k.render_v1 = true; }},
    {"nw8", [](Knobs& k) { k.render2_nw = 8; }},
    {"nrm_nw8", [](Knobs& k) { k.render2_nrm_nw = 8; }},
    {"static", [](Knobs& k) { k.render_static_tiles = true; }},
    {"tail0", [](Knobs& k) { k.render_tail = 0; }},
    {"tail1000", [](Knobs& k) { k.render_tail = 1000; }},
    {"xcd1", [](Knobs& k) { k.render_xcd = 1; }},
    {"wgs7", [](Knobs& k) { k.render_wgs = 7; }},
};
const int N_KNOBS = sizeof(KNOBS) / sizeof(KNOBS[0]);

struct Case {
  bool emu;
  int C, nc, nf;
  bool nrm, sp, train;
  int R, cus, knob;
};

const int COUNTS[9][2] = {{3, 2}, {5, 3}, {9, 7}, {33, 65}, {63, 127}, {64, 63}, {17, 128}, {64, 128}, {64, 64}};
const int CUS[4] = {8, 20, 32, 256};
const int CAMS[7] = {1, 4, 30, 32, 33, 40, 65};
const int FRAMES[3][2] = {{6, 7}, {16, 16}, {400, 400}};
const int RAYS[2] = {13, 4096};
struct Shape {
  int C;
  bool nrm, sp, train;
};
const Shape SHAPES[11] = {{16, false, false, false}, {16, true, false, false}, {32, false, false, false}, {32, true, false, false},
                          {32, false, true, false},  {32, true, true, false},  {64, false, false, false}, {64, true, false, false},
                          {16, false, false, true},  {32, false, false, true}, {64, false, false, true}};

std::vector<Case> all_cases() {
  std::vector<Case> out;
  for (int emu = 0; emu < 2; ++emu)
    for (const Shape& s : SHAPES)
      for (int cus : CUS)
        for (int kn = 0; kn < N_KNOBS; ++kn)
          for (const auto& cnt : COUNTS) {
            if (kn != 0 && !((cnt[0] == 64 && (cnt[1] == 64 || cnt[1] == 128)) && (cus == 8 || cus == 256))) continue;
            out.push_back({emu != 0, s.C, cnt[0], cnt[1], s.nrm, s.sp, s.train, cus == 256 ? 64 : 8, cus, kn});
          }
  return out;
}
// the launch lists of a case: (cameras, rays per camera)
std::vector<std::pair<int, int64_t>> lists_of(const Case& c) {
  std::vector<std::pair<int, int64_t>> out;
  auto rays = [&](int i) { return c.train ? (int64_t)RAYS[i] : (int64_t)FRAMES[i][0] * FRAMES[i][1]; };
  const int n_sizes = c.train ? 2 : 3;
  if (c.knob == 0 && ((c.nc == 9 && c.nf == 7) || (c.C == 16 && c.nc == 64 && c.nf == 128))) {
    for (int cams : CAMS)
      for (int i = 0; i < n_sizes; ++i) out.push_back({cams, rays(i)});
  } else if (c.knob != 0 && c.nc == 64 && c.nf == 64) {
    for (int cams : {4, 40})
      for (int i : {0, n_sizes - 1}) out.push_back({cams, rays(i)});
  }
  return out;
}

RenderPlan plan_of(const Case& c) {
  Knobs k = default_knobs();
  KNOBS[c.knob].apply(k);
  return render_plan({c.C, c.nc, c.nf, c.nrm, c.sp, c.train, c.R, 256}, c.cus, k, c.emu);
}

std::string kernel_name(const RenderPlan& p) {
  char b[96];
  if (p.family == RenderFamily::Tiled) snprintf(b, sizeof b, "render2_kernel<%d,%d,%d,%d%s>", p.ch, p.z, (int)p.train, p.waves, p.nrm ? ",1" : "");
  else snprintf(b, sizeof b, "render_kernel<%d,%d,%d,%d>", p.ch, (int)p.sp, (int)p.nrm, p.z);
  return b;
}
// every instantiation render_launch's switch holds (kernels_render.hip: render_launch_t<8, false>, <16, false>, <16, true>,
// <32, false>)
std::set<std::string> all_instantiations() {
  std::set<std::string> s;
  char b[96];
  for (int ch : {8, 16, 32}) {
    for (int tr = 0; tr < 2; ++tr) {
      const int w64 = render2_waves(ch, 64), w128 = render2_waves(ch, 128);
      snprintf(b, sizeof b, "render2_kernel<%d,64,%d,%d>", ch, tr, w64), s.insert(b);
      snprintf(b, sizeof b, "render2_kernel<%d,64,%d,8>", ch, tr), s.insert(b);
      snprintf(b, sizeof b, "render2_kernel<%d,128,%d,%d>", ch, tr, w128), s.insert(b);
    }
    if (ch <= 16)
      for (int nw : {10, 8}) snprintf(b, sizeof b, "render2_kernel<%d,64,0,%d,1>", ch, nw), s.insert(b);
    for (int sp = 0; sp < (ch == 16 ? 2 : 1); ++sp)
      for (int nrm = 0; nrm < 2; ++nrm)
        for (int z : {64, 128}) snprintf(b, sizeof b, "render_kernel<%d,%d,%d,%d>", ch, sp, nrm, z), s.insert(b);
  }
  return s;
}

typedef std::vector<std::string> Errs;
void fail(Errs& e, const char* what) { e.push_back(what); }

void check_plan(const RenderPlan& p, const Knobs& k, Errs& e) {
  const RenderLayout& L = p.layout;
  const RenderRegion* regs[6] = {&L.grid_cl, &L.tile_ctr, &L.val_ws, &L.nrm_ws, &L.dens_field, &L.pad};
  size_t end = 0;
  for (const RenderRegion* r : regs) {
    if (r->off % 256 || r->bytes % 256) fail(e, "region not 256-aligned");
    if (r->off < end) fail(e, "regions overlap");
    if (r->off != end) fail(e, "gap between regions");
    end = r->end();
  }
  if (L.total != L.pad.end() || L.pad.bytes != 256) fail(e, "total is not the last end plus the pad");
  if (p.slots != (int64_t)p.wg_cap * p.waves) fail(e, "slot count is not cap x waves");
  if (p.family == RenderFamily::RayPerColumn) {
    const size_t need = (size_t)p.wg_cap * p.waves * 32768;
    if (L.val_ws.bytes < need) fail(e, "scratch smaller than cap x waves x 32 KB");
    if (p.nrm && L.nrm_ws.bytes < need) fail(e, "normals scratch smaller than cap x waves x 32 KB");
    if (p.dynamic) fail(e, "dynamic hand-out on the ray-per-column kernel");
  }
  if (p.dynamic && L.tile_ctr.bytes < 8 * sizeof(int)) fail(e, "counter region does not hold eight ints");
  if (p.family == RenderFamily::Tiled && !p.train && L.tile_ctr.bytes < 8 * sizeof(int)) fail(e, "counter region does not hold eight ints");
  const int rule = p.family == RenderFamily::Tiled ? render2_waves(p.ch, p.z, p.nrm) : render_waves(p.ch, p.z, p.nrm);
  const bool eight = p.family == RenderFamily::Tiled && (p.nrm ? (k.render2_nrm_nw == 8 || p.emu) : (k.render2_nw == 8 && rule == 12));
  if (p.waves != (eight ? 8 : rule)) fail(e, "waves differ from the instantiation's rule");
  if (64 * p.waves > 1024) fail(e, "workgroup above 1024 threads");
  if (k.render_wgs > 0 && p.wg_cap != (int)k.render_wgs) fail(e, "cap ignores HOLO_RENDER_WGS");
  if (!render_can_launch(p)) fail(e, "render_can_launch refuses the plan");
}

void check_list(const RenderPlan& p, const std::vector<RenderLaunch>& ls, int n_cameras, Errs& e) {
  int next = 0, lo = 1 << 30, hi = 0;
  for (const RenderLaunch& l : ls) {
    if (l.cam0 != next) fail(e, "launches do not cover the cameras once, in order");
    next = l.cam0 + l.n_cams;
    if (l.n_cams < 1 || l.n_cams > 32) fail(e, "camera group outside 1..32");
    if (l.n_wgs < 1 || l.n_wgs > p.wg_cap) fail(e, "workgroups outside 1..cap");
    if (l.xcd < 1 || (l.xcd > 1 && (l.n_wgs != p.wg_cap || l.n_wgs % l.xcd))) fail(e, "XCD split on a launch it does not divide");
    if (!l.dynamic && l.tail_quads != 0) fail(e, "tail without dynamic hand-out");
    if (l.dynamic != p.dynamic) fail(e, "hand-out differs from the plan's");
    if (p.train && (l.xcd != 1 || l.dynamic)) fail(e, "training mode with XCD split or dynamic hand-out");
    lo = l.n_cams < lo ? l.n_cams : lo, hi = l.n_cams > hi ? l.n_cams : hi;
  }
  if (next != n_cameras) fail(e, "launches do not cover the cameras once, in order");
  if (!p.train && !ls.empty() && hi - lo > 1) fail(e, "evaluation groups differ by more than one camera");
}

// ---- view pooling ----------------------------------------------------------------------------------------------------
struct VpCase {
  int n_feats, n_views, cus;
  bool backward, det;
};
const int VP_CH[8] = {3, 5, 64, 17, 128, 6, 33, 2}, VP_HW[8][2] = {{5, 7}, {9, 4}, {25, 25}, {13, 13}, {7, 7}, {50, 50}, {3, 11}, {100, 100}};
void vp_feats(int n, HoloViewFeature* f) {
  for (int k = 0; k < n; ++k) f[k] = {nullptr, VP_CH[k], VP_HW[k][0], VP_HW[k][1]};
}
const HoloViewPoolCfg VP_CFG = {16, 8.f, 32, 1.f, 0.1f, 1e-2f};

void check_view_pool(const ViewPoolLayout& L, const VpCase& c, Errs& e) {
  std::vector<std::pair<size_t, size_t>> regs;  // (offset, padded bytes), in order
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  for (int k = 0; k < c.n_feats; ++k) regs.push_back({L.map[k], pad(L.map_bytes[k])});
  regs.push_back({L.wt, 0});
  if (c.backward) {
    for (int k = 0; k < c.n_feats; ++k) regs.push_back({L.gmap[k], pad(L.map_bytes[k])});
    regs.push_back({L.partial, pad((size_t)L.n_wgs * 4)});
    if (c.det) {
      for (int k = 0; k < c.n_feats; ++k) regs.push_back({L.gfix[k], pad(2 * L.map_bytes[k])});
      regs.push_back({L.fix_max, 256});
      if (L.fix_end != L.fix_max + 256) fail(e, "view pool: zeroed range does not end behind the words");
    }
  }
  size_t end = 0;
  for (const auto& r : regs) {
    if (r.first % 256) fail(e, "view pool: region not 256-aligned");
    if (r.first < end) fail(e, "view pool: regions overlap");
    end = r.first + r.second;
  }
  if (L.total < end + L.pad || L.pad < 256) fail(e, "view pool: total does not hold the last region and the pad");
}

// ---- the table --------------------------------------------------------------------------------------------------------
// The committed table is thinned (every plan whose index hashes to 0 mod 16, with its lists; every fourth `vp` line) and ends
// in a digest of the FULL table - its lines, bytes and 64-bit FNV-1a -, so the whole sweep is still compared with the recording.
bool kept(unsigned index) { return ((index * 2654435761u) >> 16) % 16 == 0; }

std::string table(Errs& errs, std::set<std::string>* seen, bool full) {
  std::string out, all;
  char b[512];
  int index = 0;
  auto emit = [&](const std::string& block, bool keep) {
    all += block;
    if (keep) out += block;
  };
  for (const Case& c : all_cases()) {
    std::string block;
    Knobs k = default_knobs();
    KNOBS[c.knob].apply(k);
    const RenderPlan p = plan_of(c);
    Errs e;
    check_plan(p, k, e);
    const std::string kn = kernel_name(p);
    if (seen) seen->insert(kn);
    snprintf(b, sizeof b, "plan %d emu=%d C=%d nc=%d nf=%d nrm=%d sp=%d train=%d R=%d cus=%d knobs=%s ws=%zu kernel=%s block=%d\n", index,
             (int)c.emu, c.C, c.nc, c.nf, (int)c.nrm, (int)c.sp, (int)c.train, c.R, c.cus, KNOBS[c.knob].name, p.layout.total, kn.c_str(),
             64 * p.waves);
    block += b;
    for (const auto& l : lists_of(c)) {
      const std::vector<RenderLaunch> ls = render_launches(p, l.first, l.second);
      check_list(p, ls, l.first, e);
      snprintf(b, sizeof b, "list p=%d cams=%d rays=%lld", index, l.first, (long long)l.second);
      block += b;
      for (const RenderLaunch& x : ls) {
        snprintf(b, sizeof b, " | %d+%d tiles=%lld wgs=%d xcd=%d dyn=%d tail=%d", x.cam0, x.n_cams, (long long)x.n_tiles, x.n_wgs, x.xcd,
                 (int)x.dynamic, x.tail_quads);
        block += b;
      }
      block += "\n";
    }
    emit(block, kept((unsigned)index));
    for (const std::string& m : e) errs.push_back("plan " + std::to_string(index) + ": " + m);
    ++index;
  }
  int vp = 0;
  for (int back = 0; back < 2; ++back)
    for (int det = 0; det < (back ? 2 : 1); ++det)
      for (int cus : {8, 256})
        for (int views : {1, 16})
          for (int n = 1; n <= 8; ++n) {
            if (!back && cus != 8) continue;
            HoloViewFeature f[8];
            vp_feats(n, f);
            const VpCase c = {n, views, cus, back != 0, det != 0};
            const ViewPoolLayout L = view_pool_layout(VP_CFG, f, n, views, c.backward, cus, c.det);
            Errs e;
            check_view_pool(L, c, e);
            for (const std::string& m : e) errs.push_back("vp: " + m);
            snprintf(b, sizeof b, "vp bwd=%d det=%d cus=%d views=%d maps=%d total=%zu\n", back, det, cus, views, n, L.total);
            emit(b, vp++ % 4 == 0);
          }
  if (full) return all;
  uint64_t h = 1469598103934665603ull;
  size_t lines = 0;
  for (unsigned char ch : all) h = (h ^ ch) * 1099511628211ull, lines += ch == '\n';
  snprintf(b, sizeof b, "full table: %zu lines, %zu bytes, fnv1a64=%016llx\n", lines, all.size(), (unsigned long long)h);
  return out + b;
}

// the hand-made plans render_can_launch must refuse: what the launcher's switch used to find out at launch time
int check_refusals(Errs& errs) {
  const Knobs k = default_knobs();
  int n = 0;
  auto refused = [&](const char* what, RenderPlan p) {
    ++n;
    if (render_can_launch(p)) errs.push_back(std::string("render_can_launch accepts: ") + what);
  };
  auto good = [&](int C, int nf, bool nrm, bool sp, bool train) { return render_plan({C, 64, nf, nrm, sp, train, 8, 256}, 256, k, false); };
  RenderPlan p = good(16, 64, false, false, false);
  if (!render_can_launch(p)) errs.push_back("render_can_launch refuses the base plan of the refusal list");
  p.hidden = 128, refused("dnet_hidden_dim 128", p);
  p = good(16, 64, false, false, false), p.n_coarse = 2, refused("2 coarse samples", p);
  p = good(16, 64, false, false, false), p.n_coarse = 65, refused("65 coarse samples", p);
  p = good(16, 64, false, false, false), p.n_fine = 1, refused("1 new sample", p);
  refused("129 new samples", good(16, 129, false, false, false));
  refused("128 features", good(128, 64, false, false, false));
  refused("128 features, normals", good(128, 64, true, false, false));
  refused("normals in training mode", good(16, 64, true, false, true));
  p = good(64, 64, true, false, false), p.family = RenderFamily::Tiled, p.rays_per_tile = 4, refused("tiled normals of 64 features", p);
  p = good(16, 128, true, false, false), p.family = RenderFamily::Tiled, p.rays_per_tile = 4, refused("tiled normals of 128 new samples", p);
  p = good(32, 64, false, true, false), p.family = RenderFamily::Tiled, p.rays_per_tile = 4, refused("split arithmetic on the tiled kernel", p);
  p = good(16, 64, false, false, false), p.sp = true, refused("split arithmetic at 16 features", p);
  p = good(16, 64, false, false, false), p.waves = 10, refused("10 waves without normals", p);
  p = good(64, 64, false, false, false), p.waves = 12, refused("12 waves at 64 features", p);
  p = good(16, 64, false, false, false), p.z = 128, refused("128 rows for 64 new samples", p);
  p = good(16, 128, false, false, false), p.z = 64, refused("64 rows for 128 new samples", p);
  p = good(32, 64, false, true, false), p.slots -= 1, refused("a slot count one wave short", p);
  return n;
}

int self_test() {
  const Knobs k = default_knobs();
  int bad = 0;
  auto expect = [&](const char* what, const Errs& e, const char* needle) {
    bool found = false;
    for (const std::string& m : e) found |= m.find(needle) != std::string::npos;
    if (!found || e.size() != 1) {
      printf("self-test: fault '%s' gave %zu findings%s\n", what, e.size(), found ? "" : " and not the planted one");
      for (const std::string& m : e) printf("   %s\n", m.c_str());
      ++bad;
    }
  };
  const RenderPlan rpc = render_plan({32, 64, 64, true, true, false, 8, 256}, 256, k, false);
  const RenderPlan tiled = render_plan({16, 64, 64, false, false, false, 8, 256}, 256, k, false);
  {  // the good ones are clean
    Errs e;
    check_plan(rpc, k, e), check_plan(tiled, k, e);
    check_list(tiled, render_launches(tiled, 40, 160000), 40, e);
    if (!e.empty()) printf("self-test: the good plans give %zu findings\n", e.size()), ++bad;
  }
  {
    RenderPlan p = rpc;  // a scratch one wave short of the resident waves
    p.layout.val_ws.bytes -= 32768, p.layout.nrm_ws.off -= 32768, p.layout.dens_field.off -= 32768, p.layout.pad.off -= 32768, p.layout.total -= 32768;
    Errs e;
    check_plan(p, k, e);
    for (auto it = e.begin(); it != e.end();) it = it->find("render_can_launch") != std::string::npos ? e.erase(it) : it + 1;
    expect("slot count one wave short", e, "scratch smaller");
  }
  {
    RenderPlan p = rpc;  // the normals' scratch laid over the values'
    p.layout.nrm_ws.off -= 256;
    Errs e;
    check_plan(p, k, e);
    for (auto it = e.begin(); it != e.end();) it = it->find("gap between") != std::string::npos ? e.erase(it) : it + 1;
    expect("overlapping regions", e, "regions overlap");
  }
  {
    std::vector<RenderLaunch> ls = render_launches(tiled, 65, 42);  // 22 + 22 + 21 -> 33 + 11 + 21
    ls[0].n_cams = 33, ls[1].cam0 = 33, ls[1].n_cams = 11;
    Errs e;
    check_list(tiled, ls, 65, e);
    for (auto it = e.begin(); it != e.end();) it = it->find("differ by more") != std::string::npos ? e.erase(it) : it + 1;
    expect("a camera group of 33", e, "camera group outside 1..32");
  }
  {
    std::vector<RenderLaunch> ls = render_launches(tiled, 40, 160000);  // XCD ranges on a launch of cap - 1 workgroups
    ls[0].n_wgs -= 1;
    Errs e;
    check_list(tiled, ls, 40, e);
    expect("XCD split on a launch that is not full", e, "XCD split");
  }
  printf(bad ? "render_plan_check --self-test: FAILED\n" : "render_plan_check --self-test: OK (4 planted faults found, nothing else)\n");
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--self-test")) return self_test();
  Errs errs;
  std::set<std::string> seen;
  if (argc > 1 && !strcmp(argv[1], "--full")) {
    fputs(table(errs, nullptr, true).c_str(), stdout);
    return 0;
  }
  const std::string t = table(errs, &seen, false);
  if (argc < 2) {
    fputs(t.c_str(), stdout);
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    printf("render_plan_check: cannot open %s\n", argv[1]);
    return 2;
  }
  std::string golden;
  char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) golden.append(buf, n);
  fclose(f);
  if (golden != t) {
    size_t i = 0, line = 1;
    while (i < golden.size() && i < t.size() && golden[i] == t[i]) line += golden[i++] == '\n';
    errs.push_back("the table differs from the golden one, first at line " + std::to_string(line));
  }
  const int n_refused = check_refusals(errs);
  for (const std::string& inst : all_instantiations())
    if (!seen.count(inst)) errs.push_back("never planned: " + inst);
  for (const std::string& inst : seen)
    if (!all_instantiations().count(inst)) errs.push_back("planned but not in the launcher's switch: " + inst);
  size_t lines = 0;
  for (char ch : t) lines += ch == '\n';
  for (size_t i = 0; i < errs.size() && i < 40; ++i) printf("%s\n", errs[i].c_str());
  printf("%zu table lines, %zu instantiations planned, %d bad plans refused, %zu findings\n", lines, seen.size(), n_refused, errs.size());
  printf(errs.empty() ? "render_plan_check: OK\n" : "render_plan_check: FAILED\n");
  return errs.empty() ? 0 : 1;
}
