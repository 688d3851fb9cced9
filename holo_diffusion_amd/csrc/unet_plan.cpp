// unet_plan.cpp — the denoiser's planner (unet_plan.h): the structure of UNetModel (holo_diffusion/guided_diffusion/unet.py:645-798
// as configured by SimpleUnet3D, holo_diffusion/utils/diffusion_utils.py:56-75), its parameter table, and the static launch
// plan of UNetModel.forward (unet.py:800-837).  Everything is static for a given (description, batch): tensor shapes, workspace
// offsets, split-K factors, kernel parameters.  Host-only arithmetic: nothing here launches, allocates or includes HIP.
#include "unet_plan.h"

#include <stdio.h>

#include <algorithm>

namespace holo {
namespace unetplan {

void build_structure(UnetDesc* u) {
  const HoloUnetCfg& c = u->cfg;
  const int mc = c.model_channels;
  int ch = c.channel_mult[0] * mc;
  char buf[128];
  u->inputs.clear();
  u->outputs.clear();
  u->middle.clear();
  u->inputs.push_back({Block{B_CONV, "input_blocks.0.0", c.in_channels, ch}});
  std::vector<int> chans{ch};
  int ds = 1, idx = 1;
  auto has_attn = [&](int d) {
    for (int i = 0; i < c.n_attention_resolutions; ++i)
      if (c.attention_resolutions[i] == d) return true;
    return false;
  };
  for (int level = 0; level < c.n_channel_mult; ++level) {
    const int mult = c.channel_mult[level];
    for (int r = 0; r < c.num_res_blocks; ++r) {
      std::vector<Block> layers;
      snprintf(buf, sizeof buf, "input_blocks.%d.0", idx);
      layers.push_back(Block{B_RES, buf, ch, mult * mc});
      ch = mult * mc;
      if (has_attn(ds)) {
        snprintf(buf, sizeof buf, "input_blocks.%d.1", idx);
        layers.push_back(Block{B_ATTN, buf, ch, ch});
      }
      u->inputs.push_back(layers);
      chans.push_back(ch);
      ++idx;
    }
    if (level != c.n_channel_mult - 1) {
      snprintf(buf, sizeof buf, "input_blocks.%d.0", idx);
      u->inputs.push_back({Block{B_DOWN, buf, ch, ch}});
      chans.push_back(ch);
      ds *= 2;
      ++idx;
    }
  }
  u->middle.push_back(Block{B_RES, "middle_block.0", ch, ch});
  u->middle.push_back(Block{B_ATTN, "middle_block.1", ch, ch});
  u->middle.push_back(Block{B_RES, "middle_block.2", ch, ch});
  int oidx = 0;
  for (int level = c.n_channel_mult - 1; level >= 0; --level) {
    const int mult = c.channel_mult[level];
    for (int i = 0; i < c.num_res_blocks + 1; ++i) {
      const int ich = chans.back();
      chans.pop_back();
      std::vector<Block> layers;
      snprintf(buf, sizeof buf, "output_blocks.%d.0", oidx);
      layers.push_back(Block{B_RES, buf, ch + ich, mc * mult});
      ch = mc * mult;
      if (has_attn(ds)) {
        snprintf(buf, sizeof buf, "output_blocks.%d.%d", oidx, (int)layers.size());
        layers.push_back(Block{B_ATTN, buf, ch, ch});
      }
      if (level && i == c.num_res_blocks) {
        snprintf(buf, sizeof buf, "output_blocks.%d.%d", oidx, (int)layers.size());
        layers.push_back(Block{B_UP, buf, ch, ch});
        ds /= 2;
      }
      u->outputs.push_back(layers);
      ++oidx;
    }
  }
  u->final_ch = ch;
}

static void add_param(UnetDesc* u, const std::string& name, std::vector<int64_t> shape, ParamKind kind) {
  ParamSlot s;
  s.name = name;
  s.shape = shape;
  s.numel = 1;
  for (auto d : shape) s.numel *= d;
  s.kind = kind;
  s.set = false;
  u->pindex[name] = (int)u->params.size();
  u->params.push_back(s);
}

void enumerate_params(UnetDesc* u) {
  const HoloUnetCfg& c = u->cfg;
  const int64_t mc = c.model_channels, ted = 4 * mc;
  u->ted = (int)ted;
  add_param(u, "time_embed.0.weight", {ted, mc}, P_PLAIN);
  add_param(u, "time_embed.0.bias", {ted}, P_PLAIN);
  add_param(u, "time_embed.2.weight", {ted, ted}, P_PLAIN);
  add_param(u, "time_embed.2.bias", {ted}, P_PLAIN);
  u->emb_rows = 0;
  auto add_block = [&](const Block& b) {
    const std::string& p = b.prefix;
    const int64_t ci = b.cin, co = b.cout;
    switch (b.kind) {
      case B_CONV:
        add_param(u, p + ".weight", {co, ci, 3, 3, 3}, P_CONV3);
        add_param(u, p + ".bias", {co}, P_PLAIN);
        break;
      case B_RES:
        add_param(u, p + ".in_layers.0.weight", {ci}, P_PLAIN);
        add_param(u, p + ".in_layers.0.bias", {ci}, P_PLAIN);
        add_param(u, p + ".in_layers.2.weight", {co, ci, 3, 3, 3}, P_CONV3);
        add_param(u, p + ".in_layers.2.bias", {co}, P_PLAIN);
        add_param(u, p + ".emb_layers.1.weight", {2 * co, ted}, P_EMB_W);
        add_param(u, p + ".emb_layers.1.bias", {2 * co}, P_EMB_B);
        u->emb_row_off[p] = u->emb_rows;
        u->emb_rows += (int)(2 * co);
        add_param(u, p + ".out_layers.0.weight", {co}, P_PLAIN);
        add_param(u, p + ".out_layers.0.bias", {co}, P_PLAIN);
        add_param(u, p + ".out_layers.3.weight", {co, co, 3, 3, 3}, P_CONV3);
        add_param(u, p + ".out_layers.3.bias", {co}, P_PLAIN);
        if (ci != co) {
          add_param(u, p + ".skip_connection.weight", {co, ci, 1, 1, 1}, P_CONV1);
          add_param(u, p + ".skip_connection.bias", {co}, P_PLAIN);
        }
        break;
      case B_ATTN:
        add_param(u, p + ".norm.weight", {ci}, P_PLAIN);
        add_param(u, p + ".norm.bias", {ci}, P_PLAIN);
        add_param(u, p + ".qkv.weight", {3 * ci, ci, 1}, P_CONV1);
        add_param(u, p + ".qkv.bias", {3 * ci}, P_PLAIN);
        add_param(u, p + ".proj_out.weight", {ci, ci, 1}, P_CONV1);
        add_param(u, p + ".proj_out.bias", {ci}, P_PLAIN);
        break;
      case B_DOWN:
        add_param(u, p + ".op.weight", {co, ci, 3, 3, 3}, P_CONV3);
        add_param(u, p + ".op.bias", {co}, P_PLAIN);
        break;
      case B_UP:
        add_param(u, p + ".conv.weight", {co, ci, 3, 3, 3}, P_CONV3);
        add_param(u, p + ".conv.bias", {co}, P_PLAIN);
        break;
      case B_HEAD:
        break;
    }
  };
  for (auto& l : u->inputs)
    for (auto& b : l) add_block(b);
  for (auto& b : u->middle) add_block(b);
  for (auto& l : u->outputs)
    for (auto& b : l) add_block(b);
  add_param(u, "out.0.weight", {u->final_ch}, P_PLAIN);
  add_param(u, "out.0.bias", {u->final_ch}, P_PLAIN);
  add_param(u, "out.2.weight", {c.out_channels, u->final_ch, 3, 3, 3}, P_CONV3);
  add_param(u, "out.2.bias", {c.out_channels}, P_PLAIN);
}

StoreSizes carve_params(UnetDesc* u, float* f32, uint16_t* bf, float* wino) {
  StoreSizes n;
  auto take = [](auto* base, int64_t& top, int64_t count) {
    auto* p = base ? base + top : nullptr;
    top += round64(count);
    return p;
  };
  for (ParamSlot& s : u->params) {
    if (s.kind == P_EMB_W || s.kind == P_EMB_B) continue;  // rows of emb_w / emb_b (below)
    if (!s.is_conv()) {
      s.w.f32 = take(f32, n.f32, s.numel);
      continue;
    }
    const ConvWeightLayout l = s.w.layout = s.layout();
    const ConvCopies c = forward_copies(l, s.name.find("skip_connection") != std::string::npos, u->knobs);
    s.w.f32 = take(f32, n.f32, l.f32_floats());
    if (c.bf16) {
      s.w.bf = take(bf, n.bf, l.bf16_elems());
      s.w.bft = s.w.bf ? s.w.bf + l.bft_offset() : nullptr;
    }
    if (c.wino2) s.w.wino2 = take(wino, n.wino, l.wino2_floats());
    if (c.wino3) s.w.wino3 = take(wino, n.wino, l.wino3_floats());
  }
  u->emb_w = take(f32, n.f32, (int64_t)u->emb_rows * u->ted);
  u->emb_b = take(f32, n.f32, u->emb_rows);
  for (ParamSlot& s : u->params)
    if (f32 && (s.kind == P_EMB_W || s.kind == P_EMB_B)) {
      const int row = u->emb_row_off[s.name.substr(0, s.name.rfind(".emb_layers"))];
      s.w.f32 = s.kind == P_EMB_W ? u->emb_w + (int64_t)row * u->ted : u->emb_b + row;
    }
  return n;
}

ConvWeights W(const UnetDesc* u, const std::string& name) {
  auto it = u->pindex.find(name);
  return it == u->pindex.end() ? ConvWeights() : u->params[it->second].w;
}

// C = alpha A B^T ([T][T] out of two [T][ch] operands), or with b_kmajor C = alpha A B ([T][ch] out of [T][T] and [T][ch])
GemmParams attn_gemm(const AttnDims& d, AttnMat A, AttnMat B, bool b_kmajor, AttnMat C, float alpha) {
  GemmParams g;
  memset(&g, 0, sizeof g);
  g.A = A.p, g.lda = A.ld, g.sa0 = A.s0, g.sa1 = A.s1;
  g.B = B.p, g.ldb = B.ld, g.sb0 = B.s0, g.sb1 = B.s1;
  g.C = C.p, g.ldc = C.ld, g.sc0 = C.s0, g.sc1 = C.s1;
  g.M = (int)d.T;
  g.Nn = b_kmajor ? d.ch() : (int)d.T;
  g.K = b_kmajor ? (int)d.T : d.ch();
  g.nb0 = d.N;
  g.nb1 = d.H;
  g.b_kmajor = b_kmajor ? 1 : 0;
  g.alpha = alpha;
  return g;
}

// ---------------------------------------------------------------------------------------------
// plan builder
// ---------------------------------------------------------------------------------------------
Planner::Planner(const UnetDesc* u_, int N_, void* ws, Plan& plan_)
    : u(u_), N(N_), base(reinterpret_cast<uintptr_t>(ws)), sizing(ws == nullptr), plan(plan_), ops(plan_.ops) {
  // a generous fixed region for the small buffers
  small_cap = Arena::al((size_t)N * 8 * 1024 * 256 * 2 + (size_t)N * (u->emb_rows + 4 * u->ted) * 4 * 2 + 65536);
  arena_base = small_cap;
  arena.keep = u->knobs.keep_intermediates;
}

Act Planner::new_act(int C, int R, bool f32) {
  Act a;
  a.C = C;
  a.R = R;
  a.bytes = (size_t)N * vox(R) * C * ((bfs() && !f32) ? 2 : sizeof(float));
  a.off = guarded(arena_base + arena.alloc(a.bytes), a.bytes);
  return a;
}
// GroupNorm partial-sum buffer [N][slabs][C][2] doubles; the slab count depends on the producing kernel
void Planner::alloc_stats(Act& a, int slabs) {
  a.stats_B = slabs;
  a.stats_bytes = (size_t)N * slabs * a.C * 2 * sizeof(double);
  a.stats_off = guarded(arena_base + arena.alloc(a.stats_bytes), a.stats_bytes);
}
// LIFETIMES.  The first-fit arena relies on STREAM ORDER: memory released at one point of the plan may be handed to any
// launch planned later, because that launch runs behind the last user of the memory on the same stream.  Side-lane ops
// (plan_side_lane) run on a second stream between the fork and their consumer's join, in no order against the main ops of
// that stretch.  So everything a side op reads or writes - the skip tensor, its statistics records, the partial tensor P
// (its coefficients live in the bump-only small region) - is allocated BEFORE the fork in plan order and released only
// AFTER the consumer that waits for the join: nothing released after the fork is ever handed to a side op, and nothing a
// side op touches is handed out again before its join.  `side_live` holds those ranges while they are protected; every
// allocation is checked against them (guarded).
void Planner::release(Act& a) {
  arena.free(a.off - arena_base, a.bytes);
  if (a.stats_bytes) arena.free(a.stats_off - arena_base, a.stats_bytes);
}
size_t Planner::small_alloc(size_t bytes) {
  size_t off = small_top;
  small_top += Arena::al(bytes);
  return off;
}
size_t Planner::guarded(size_t off, size_t bytes) {
  for (const SideRange& r : side_live)
    if (off < r.off + r.bytes && r.off < off + bytes && err.empty())
      err = "internal: an allocation between the side lane's fork and join " + std::to_string(r.join) + " overlaps a buffer of that side op";
  return off;
}

void Planner::emit_stats(Act& a) {
  int B, vpb;
  gn_stats_geometry(a.C, vox(a.R), &B, &vpb);
  alloc_stats(a, B);
  Op op = make_op(OP_STATS);
  op.stats.x = ptr<float>(a.off);
  op.stats.part = ptr<double>(a.stats_off);
  op.stats.C = a.C;
  op.stats.V = vox(a.R);
  op.stats.x_bf16 = bfs() ? 1 : 0;
  ops.push_back(op);
}
// GroupNorm `norm` (its .weight / .bias) of [x0 | x1], folded with the FiLM rows when given; returns the coef offset
size_t Planner::emit_finalize(const Act& x0, const Act* x1, const std::string& norm, const float* film, int film_cout) {
  const int Cin = x0.C + (x1 ? x1->C : 0);
  size_t coef = small_alloc((size_t)N * Cin * 2 * sizeof(float));
  Op op = make_op(OP_FINAL);
  GnFinalize& f = op.fin;
  if (tape) {
    last_mom = small_alloc((size_t)N * Cin * 2 * sizeof(float));
    f.moments = ptr<float>(last_mom);
  }
  f.part0 = ptr<double>(x0.stats_off);
  f.C0 = x0.C;
  f.B0 = x0.stats_B;
  f.part1 = x1 ? ptr<double>(x1->stats_off) : nullptr;
  f.C1 = x1 ? x1->C : 0;
  f.B1 = x1 ? x1->stats_B : 0;
  f.V = vox(x0.R);
  f.gamma = P(u, norm + ".weight");
  f.beta = P(u, norm + ".bias");
  f.film = film;
  f.film_stride = u->emb_rows;
  f.film_cout = film_cout;
  f.coef = ptr<float>(coef);
  f.groups = 32;
  ops.push_back(op);
  return coef;
}
// The same GroupNorm of ONE half `x` of a virtual concat whose groups (cpg channels each) do not straddle the seam: the
// half's channels start at c_first of the norm's parameters, and the coefficients get a buffer [N][x.C][2] of their own
size_t Planner::emit_finalize_half(const Act& x, int c_first, int cpg, const std::string& norm) {
  size_t coef = small_alloc((size_t)N * x.C * 2 * sizeof(float));
  Op op = make_op(OP_FINAL);
  GnFinalize& f = op.fin;
  f.part0 = ptr<double>(x.stats_off);
  f.C0 = x.C;
  f.B0 = x.stats_B;
  f.V = vox(x.R);
  f.gamma = P(u, norm + ".weight") + c_first;
  f.beta = P(u, norm + ".bias") + c_first;
  f.film_stride = u->emb_rows;
  f.coef = ptr<float>(coef);
  f.groups = x.C / cpg;
  ops.push_back(op);
  return coef;
}
Tape& Planner::record(const Block& b, const Act& x0, const Act& out) {  // training: a layer onto the tape
  tape->emplace_back();
  Tape& t = tape->back();
  t.b = b;
  t.x0 = x0;
  t.out = out;
  return t;
}
// the convolution `layer` (its .weight / .bias) of x into the activation `out`
ConvDesc Planner::conv_of(const std::string& layer, const Act& x, const Act& out) {
  ConvDesc d;
  d.x0 = &x;
  d.w = W(u, layer + ".weight");
  d.bias = P(u, layer + ".bias");
  d.out = ptr<float>(out.off);
  d.Cout = out.C;
  return d;
}
// One weight's copies into the launch `p`: its main weight, or (`skip`) that of its fused 1x1x1 skip, whose sources are
// set.  conv_plan picks kernels from the weight pointers it finds, so which copies are handed over IS the compute mode:
// the bf16 ones off the exact mode (halo-path launches multiply on the bf16 matrix cores), the Winograd ones in it (where
// conv_plan finds 128-voxel tiles).  The padded extents are the ones the weight was PACKED with, so the weight must be
// this launch's own (Cin, Cout) and its CoutP must hold every Cout tile the launch walks: a tile outside it is memory that
// no repack wrote.
// (`cin0` >= 0: the launch is one half of a split concat convolution and sums the weight's input channels from cin0 on:
// whole 32-channel chunks, on conv_wino3_kernel only - its pack is chunk-major, [chunk][16-Cout slice]..., so the half is the
// same pack entered at chunk cin0 / 32; every other copy is handed over whole and must not be read: emit_conv checks)
void Planner::hand_over(const ConvWeights& cw, ConvParams& p, bool skip, int cin0) {
  const bool bf = u->compute_mode != 0, wino = u->compute_mode == 0;
  (skip ? p.skip_w : p.w) = cw.f32;
  (skip ? p.skip_w_bf : p.w_bf) = bf ? cw.bf : nullptr;
  (skip ? p.skip_w_bft : p.w_bft) = bf ? cw.bft : nullptr;
  (skip ? p.skip_w_wino2 : p.w_wino2) = wino ? cw.wino2 : nullptr;
  (skip ? p.skip_w_wino3 : p.w_wino3) = wino ? cw.wino3 : nullptr;
  (skip ? p.skip_CinP : p.CinP) = cw.layout.CinP;
  const ConvWeightLayout& l = cw.layout;
  const int Cin = skip ? p.skip_C0 + p.skip_C1 : p.C0 + p.C1;
  const int tile = conv_cout_tile(p.Cout);
  const bool slice_ok = cin0 >= 0 && !skip && wino && cw.wino3 && l.taps == 27 && (cin0 % 32) == 0 && (Cin % 32) == 0 && cin0 + Cin <= l.Cin;
  if (slice_ok) {
    p.w_wino3 = cw.wino3 + conv_wino3_weight_floats(l.CoutP, cin0, l.taps);
    p.CinP = Cin;
  }
  if (err.empty() && (l.Cout != p.Cout || (l.Cin != Cin && !slice_ok) || (cin0 >= 0 && !slice_ok) || (p.Cout + tile - 1) / tile * tile > l.CoutP || l.CoutP != p.CoutP))
    err = "internal: a " + std::to_string(Cin) + " -> " + std::to_string(p.Cout) + " convolution was handed weights packed for " +
          std::to_string(l.Cin) + " -> " + std::to_string(l.Cout) + " (padded to " + std::to_string(l.CinP) + " -> " +
          std::to_string(l.CoutP) + ")";
}
// the launch of `d` with its kernel and geometry chosen (conv_plan), its split-K scratch not yet placed; returns that scratch's bytes
size_t Planner::plan_conv(const ConvDesc& d, ConvParams& p) {
  if (const ConvParams* q = d.qkv_pack) {  // (conv_plan may fuse the attention's operand packing into the launch)
    p.qkv_q = q->qkv_q, p.qkv_k = q->qkv_k, p.qkv_vt = q->qkv_vt;
    p.qkv_scale = q->qkv_scale, p.qkv_T = q->qkv_T, p.qkv_CH = q->qkv_CH, p.qkv_H = q->qkv_H;
  }
  p.in_bf16 = bfs() && !d.in_f32;
  p.res_bf16 = bfs();
  p.out_bf16 = bfs() && !d.out_f32;
  p.src0 = ptr<float>(d.x0->off);
  p.src1 = d.x1 ? ptr<float>(d.x1->off) : nullptr;
  p.C0 = d.x0->C;
  p.C1 = d.x1 ? d.x1->C : 0;
  p.N = N;
  p.ID = p.IH = p.IW = d.in_size();
  p.ups = d.ups;
  p.OD = p.OH = p.OW = d.out_size();
  p.stride = d.stride;
  p.pad = d.ksz == 3 ? 1 : 0;
  p.ksz = d.ksz;
  p.Cout = d.Cout;
  p.CoutP = d.w.layout.CoutP;
  hand_over(d.w, p, false, d.w_slice ? d.w_cin0 : -1);
  p.bf16 = u->compute_mode;
  p.coef = d.coef ? ptr<float>(*d.coef) : nullptr;
  p.act = d.act;
  p.bias = d.bias;
  p.residual = d.residual;
  p.out = d.out;
  if (d.skip.w.f32) {  // halo kernel
    p.skip_src0 = ptr<float>(d.skip.x0->off);
    p.skip_src1 = d.skip.x1 ? ptr<float>(d.skip.x1->off) : nullptr;
    p.skip_C0 = d.skip.x0->C;
    p.skip_C1 = d.skip.x1 ? d.skip.x1->C : 0;
    hand_over(d.skip.w, p, true);
    p.skip_bias = d.skip.bias;
  }
  ConvParams one = p;
  const int cus = d.cus > 0 ? d.cus : u->num_cus;
  size_t sb = conv_plan(p, cus, knobs, plan_n());
  if (plan_n() != N) {  // the batch-invariant plan: the launch must compute each sample as the batch-1 launch does
    one.N = 1;
    conv_plan(one, cus, knobs);
    if (err.empty() && (one.kernel != p.kernel || one.tz != p.tz || one.nsplit != p.nsplit ||
                        one.chunks_per_split != p.chunks_per_split || one.skip_chunks_per_split != p.skip_chunks_per_split))
      err = "batch-invariant plan: at batch " + std::to_string(N) + " the " + std::to_string(p.C0 + p.C1) + " -> " +
            std::to_string(p.Cout) + " convolution at " + std::to_string(p.OD) + "^3 cannot keep its batch-1 choice (kernel " +
            std::to_string((int)one.kernel) + ", split-K " + std::to_string(one.nsplit) + " -> kernel " +
            std::to_string((int)p.kernel) + ", split-K " + std::to_string(p.nsplit) + "; an addressing limit of the batch)";
  }
  if (d.w_slice && err.empty() && p.kernel != ConvKernel::Wino3)  // (no other kernel can enter its weights at a chunk)
    err = "internal: one half of a split concat convolution left conv_wino3_kernel";
  return sb;
}
ConvParams Planner::place_conv(const ConvDesc& d, int* stats_slabs) {
  ConvParams p;
  memset(&p, 0, sizeof p);
  const size_t sb = plan_conv(d, p);
  size_t so = 0;
  if (sb) {
    so = scratch_alloc(sb);
    p.partial = ptr<float>(so);
  }
  // GroupNorm statistics of the output: from the conv / split-K-reduce epilogue when the launch can
  // produce them, else by a separate pass over the output
  const int slabs = d.stats_of ? conv_stats_slabs(p) : 0;
  if (slabs > 0) {
    alloc_stats(*d.stats_of, slabs);
    p.stats = ptr<double>(d.stats_of->stats_off);
  }
  // The split-K scratch is released only AFTER the statistics buffer has its place: the reduce kernel of this very
  // launch writes the statistics while other workgroups of it still read partial sums, so the two must not share memory.
  // (Released before, first fit could hand the scratch's own first bytes to the statistics: sample 0 of a split launch then
  // came out wrong in ~25 % of the runs of the bf16 mode at 32^3 - scripts/bf16_batch_check.py, found in round 4.)
  // Stream order protects the scratch against every LATER launch.
  if (sb) scratch_free(so, sb);
  if (stats_slabs) *stats_slabs = slabs;
  return p;
}
void Planner::emit_conv(const ConvDesc& d) {
  Op op = make_op(OP_CONV);
  int slabs = 0;
  op.conv = place_conv(d, &slabs);
  ops.push_back(op);
  if (d.stats_of && slabs == 0) emit_stats(*d.stats_of);
}

// ---- the side lane (exact-fp32 inference plans).  The first convolution of an up-path ResBlock sums over the virtual
// concat [h | encoder skip].  GroupNorm(32) over it has Cin / 32 channels per group; where no group straddles the seam, the
// skip half's statistics, coefficients and its chunks of the sum depend on the skip tensor alone, which exists since the
// descent.  plan_side_lane runs in front of the deep levels (build) and emits, for every such convolution that plans onto
// conv_wino3_kernel, gn_finalize of the skip half + an un-split conv_wino3_kernel launch of it into a partial tensor P, on
// the side lane and planned for HOLO_SIDE_LANE_CUS CUs, so that they run beside the latency-bound 8^3 / 4^3 stretch.  The
// ResBlock later launches the h half alone with P as its residual (resblock).  Parts are emitted in consumption order.
// WHERE the sum is split is numerics (one fp32 addition per output element changes its place), so a batch-invariant plan
// splits exactly where the batch-1 plan does; which stream runs a part is free.
bool Planner::split_eligible(const Block& b, const Act& x1, int n_for) {
  const int C0 = b.cin - x1.C, cpg = b.cin / 32;
  if (x1.R < knobs.side_lane_min_r || C0 <= 0 || (b.cin % 32) || (C0 % 32) || (C0 % cpg)) return false;
  const std::string saved = err;  // (trial launches: their refusals are answers, not errors)
  const int saved_N = N;
  N = n_for;
  const Act x0 = view(x1.off, C0, x1.R), out = view(x1.off, b.cout, x1.R);
  const std::string layer = b.prefix + ".in_layers.2";
  bool ok = true;
  for (int form = 0; form < 3 && ok; ++form) {  // the whole launch, the h half, the skip half
    ConvDesc d = conv_of(layer, form == 2 ? x1 : x0, out);
    d.x1 = form == 0 ? &x1 : nullptr;
    d.coef = x1.off;  // (any non-null address: conv_plan asks only whether there are coefficients)
    d.act = 1;
    d.w_slice = form != 0;
    d.w_cin0 = form == 2 ? C0 : 0;
    d.cus = form == 2 ? (int)knobs.side_lane_cus : 0;
    if (form == 1) d.residual = ptr<float>(x1.off);
    if (form == 2) d.bias = nullptr;
    ConvParams p;
    memset(&p, 0, sizeof p);
    plan_conv(d, p);
    // (the skip half is a DIRECT launch: no split-K scratch and no reduce launch on the side lane)
    ok = err.empty() && p.kernel == ConvKernel::Wino3 && !p.wino3_up && (form != 2 || p.nsplit == 1);
    err = saved;
  }
  N = saved_N;
  return ok;
}
void Planner::plan_side_lane(const std::vector<Act>& hs) {
  if (tape || u->compute_mode != 0 || knobs.side_lane_cus <= 0) return;
  // A free plan of a batch keeps the whole launches (its numerics owe nothing to batch 1, and the deep levels of a batch leave
  // less of the chip idle); a batch-invariant one must split where batch 1 does.
  if (N > 1 && !u->batch_invariant) return;
  const size_t fork_at = ops.size(), n_in = u->inputs.size();
  int n_parts = 0;
  for (size_t i = 0; i < u->outputs.size(); ++i) {
    const size_t j = n_in - 1 - i;  // build(): output block i pops hs[j]
    const Block& b = u->outputs[i][0];
    if (j >= hs.size() || b.kind != B_RES) continue;  // (a skip tensor the descent has yet to produce)
    const Act& x1 = hs[j];
    const bool ok = split_eligible(b, x1, N);
    if (plan_n() != N && ok != split_eligible(b, x1, 1) && err.empty())
      err = "batch-invariant plan: at batch " + std::to_string(N) + " the concat convolution of " + b.prefix +
            " cannot be split where the batch-1 plan splits it";
    if (!ok) continue;
    const int C0 = b.cin - x1.C, cpg = b.cin / 32;
    SidePart part;
    part.id = n_parts++;
    part.P = new_act(b.cout, x1.R);
    const size_t coef = emit_finalize_half(x1, C0, cpg, b.prefix + ".in_layers.0");
    ops.back().side = side_stream_used();
    ConvDesc d = conv_of(b.prefix + ".in_layers.2", x1, part.P);
    d.bias = nullptr;
    d.coef = coef;
    d.act = 1;
    d.w_slice = true;
    d.w_cin0 = C0;
    d.cus = (int)knobs.side_lane_cus;
    emit_conv(d);
    if (ops.back().conv.nsplit != 1 && err.empty()) err = "internal: the skip half of " + b.prefix + " is no direct launch";
    if (side_stream_used()) {
      ops.back().side = 1;
      ops.back().join = (short)(part.join = plan.n_joins++);
      side_live.push_back({part.P.off, part.P.bytes, part.id});
      side_live.push_back({x1.off, x1.bytes, part.id});
      if (x1.stats_bytes) side_live.push_back({x1.stats_off, x1.stats_bytes, part.id});
    }
    if (knobs.debug_plan)
      fprintf(stderr, "[plan] side lane: %s %d + %d -> %d @%d^3 split, skip half on %s, grid_x %d, join %d\n", b.prefix.c_str(), C0, x1.C,
              b.cout, x1.R, side_stream_used() ? "the side stream" : "the caller's stream", ops.back().conv.grid_x, part.join);
    side_parts[b.prefix] = part;
  }
  if (plan.n_joins) ops[fork_at].fork = 1;
}

Act Planner::resblock(const Block& b, Act& x0, Act* x1) {
  const std::string& p = b.prefix;
  const int R = x0.R;
  const auto sp = x1 ? side_parts.find(p) : side_parts.end();
  const bool split = sp != side_parts.end();
  // (split: the skip half of the sum is the partial tensor P of plan_side_lane; this launch adds the h half, the bias and P)
  size_t coefA = split ? emit_finalize_half(x0, 0, b.cin / 32, p + ".in_layers.0") : emit_finalize(x0, x1, p + ".in_layers.0");
  const size_t momA = last_mom;
  Act h1 = new_act(b.cout, R);
  ConvDesc c1 = conv_of(p + ".in_layers.2", x0, h1);
  c1.x1 = split ? nullptr : x1;
  c1.coef = coefA;
  c1.act = 1;
  c1.stats_of = &h1;
  if (split) {
    SidePart& part = sp->second;
    c1.w_slice = true;
    c1.residual = ptr<float>(part.P.off);
    const size_t at = ops.size();
    emit_conv(c1);
    ops[at].join = (short)part.join;  // (-1 where the side part ran on the caller's stream)
    // the join is behind us in stream order: P and the skip tensor are ordinary main-lane memory again
    side_live.erase(std::remove_if(side_live.begin(), side_live.end(), [&](const SideRange& r) { return r.join == part.id; }),
                    side_live.end());
    release(part.P);
    part.consumed = true;
  } else {
    emit_conv(c1);
  }
  const float* film = ptr<float>(eml_off) + u->emb_row_off.at(p);
  size_t coefB = emit_finalize(h1, nullptr, p + ".out_layers.0", film, b.cout);
  const size_t momB = last_mom;
  const bool has_skip = b.cin != b.cout;
  // the 1x1x1 skip conv rides inside the second 3x3x3 conv (halo kernel) wherever that kernel applies
  // (the bf16x3 kernel has no fused-skip variant: its skip connection runs as a separate fp32 1x1x1 conv)
  // (below 8^3 the convolution runs on the row-tile kernel, which takes the skip's channels as extra K chunks: exact-fp32
  //  mode; four launches + four reduces less at the 4^3 level of the north-star net)
  bool fuse_skip = has_skip && ((R % 8) == 0 || (u->compute_mode == 0 && R < 8)) && b.cout >= 64 && u->compute_mode != 2 &&
                   !knobs.no_skip_fusion;
  // From 64^3 on (exact-fp32 mode) the skip runs as its own streaming 1x1x1 launch (conv1x1_stream_kernel) whose output is the
  // second convolution's residual: measured on the north-star net, fused 305 us per launch against 208 (plain) + ~45.
  // HOLO_SKIP_FUSION_BELOW_R=<R>: development knob for the threshold (A/B of the two forms)
  if (fuse_skip && u->compute_mode == 0 && R >= knobs.skip_fusion_below_r && (b.cin % 32) == 0 && b.cin <= 256 && (b.cout % 64) == 0)
    fuse_skip = false;
  Act s;
  if (has_skip && !fuse_skip) {
    s = new_act(b.cout, R);
    ConvDesc cs = conv_of(p + ".skip_connection", x0, s);
    cs.x1 = x1;
    cs.ksz = 1;
    emit_conv(cs);
  }
  Act out = new_act(b.cout, R);
  ConvDesc c2 = conv_of(p + ".out_layers.3", h1, out);
  c2.coef = coefB;
  c2.act = 1;
  c2.stats_of = &out;
  if (fuse_skip) {
    c2.skip.x0 = &x0;
    c2.skip.x1 = x1;
    c2.skip.w = W(u, p + ".skip_connection.weight");
    c2.skip.bias = P(u, p + ".skip_connection.bias");
  } else {
    c2.residual = ptr<float>(has_skip ? s.off : x0.off);
  }
  emit_conv(c2);
  release(h1);
  if (has_skip && !fuse_skip) release(s);
  if (tape) {
    Tape& t = record(b, x0, out);
    t.has_x1 = x1 != nullptr;
    if (x1) t.x1 = *x1;
    t.h1 = h1;
    t.coefA = coefA;
    t.coefB = coefB;
    t.momA = momA;
    t.momB = momB;
    t.film = film;
    t.has_skip = has_skip;
  }
  return out;
}

Act Planner::attention(const Block& b, Act& x) {
  const std::string& p = b.prefix;
  const int C = x.C, R = x.R, H = u->cfg.num_heads, ch = C / H;
  const int64_t T = vox(R);
  const AttnDims dims{N, H, C, T};
  size_t coef = emit_finalize(x, nullptr, p + ".norm");
  const size_t momX = last_mom;
  const size_t qkv_bytes = (size_t)N * T * 3 * C * sizeof(float);
  const size_t s_bytes = (size_t)N * H * T * T * sizeof(float);
  const size_t a_bytes = (size_t)N * T * C * sizeof(float);
  size_t qkv = scratch_alloc(qkv_bytes);
  size_t a = scratch_alloc(a_bytes);
  size_t v2_work = 0, v2_bytes = 0;
  bool a_is_bf16 = false;
  const bool flash = flash_attn_supported((int)T, ch) && !knobs.no_flash_attn;
  Op fop = make_op(OP_FLASH);
  Flash& fl = fop.flash;
  fl.attn.qkv = ptr<float>(qkv);
  fl.attn.out = ptr<float>(a);
  fl.attn.N = N;
  fl.attn.T = (int)T;
  fl.attn.C = C;
  fl.attn.H = H;
  fl.attn.scale2 = dims.scale2();
  fl.attn.nsplit = 1;
  size_t split_work = 0, split_bytes = 0;
  // bf16 mode, sequences of 1 024 tokens and more: the packed-operand bf16 kernel (it splits the key range to fill
  // the chip, so it also serves the shorter of them; below that the exact-fp32 kernel is as fast).
  // HOLO_BF16_FLASH_MIN_T lowers the threshold (tests).  (A first, shared-tile form of the bf16 kernel was removed in
  // round 3: no shape reached it any more, and forced on by the tests it showed a rare dependence on stale memory.)
  ConvParams qp;
  memset(&qp, 0, sizeof qp);
  bool offer_pack = false;
  if (flash) {
    if (u->compute_mode == 1 && T >= knobs.bf16_flash_min_t && flash_attn_bf16v2_supported((int)T, ch)) {
      // packed bf16 operands (V transposed) in scratch, bf16 attention output
      fl.form = 2;
      fl.ksplit = flash_attn_bf16v2_ksplit(fl.attn, u->num_cus, knobs);
      fl.lazy = knobs.attn_exact ? 0 : 1;  // (HOLO_ATTN_EXACT: the exact loop alone)
      v2_bytes = flash_attn_bf16v2_workspace_bytes(fl.attn, fl.ksplit);
      v2_work = scratch_alloc(v2_bytes);
      fl.packed = ptr<float>(v2_work);
      fl.out_bf16 = 1;
      a_is_bf16 = true;
      if (!tape && bfs()) {  // the qkv convolution may write the packed operands itself (the backward's tape keeps fp32 qkv)
        flash_attn_bf16v2_operands(fl.attn, fl.packed, &qp.qkv_q, &qp.qkv_k, &qp.qkv_vt, &qp.qkv_scale);
        qp.qkv_T = (int)T, qp.qkv_CH = ch, qp.qkv_H = H;
        offer_pack = true;
      }
    } else {
      // exact fp32: the key range split across workgroups where one per query tile leaves CUs empty
      fl.attn.nsplit = flash_attn_splits(plan_n(), (int)T, H, u->num_cus, knobs);
      split_bytes = flash_attn_workspace_bytes(fl.attn);
      if (split_bytes) {
        split_work = scratch_alloc(split_bytes);
        fl.attn.part = ptr<float>(split_work);
        fl.attn.part_ml = fl.attn.part + (size_t)fl.attn.nsplit * N * T * C;
      }
    }
  }
  // (the attention internals - qkv and the attention output - stay fp32 in every mode)
  ConvDesc cq = conv_of(p + ".qkv", x, view(qkv, 3 * C, R));
  cq.ksz = 1;
  cq.coef = coef;
  cq.out_f32 = true;
  if (offer_pack) cq.qkv_pack = &qp;
  emit_conv(cq);
  if (flash) {
    fl.operands_packed = ops.back().conv.kernel == ConvKernel::Qkv ? 1 : 0;
    if (knobs.debug_plan)
      fprintf(stderr, "[plan] attention %s: T=%lld C=%d heads=%d -> %s flash kernel, %d key splits\n", p.c_str(),
              (long long)T, C, H, fl.form == 2 ? "bf16" : "fp32", fl.form == 2 ? 1 : fl.attn.nsplit);
    ops.push_back(fop);
  } else {  // S = scale2 q k^T; softmax over its rows; a = S v
    size_t S = scratch_alloc(s_bytes);
    float* qkvp = ptr<float>(qkv);
    Op op = make_op(OP_GEMM);
    op.gemm = attn_gemm(dims, dims.qkv(qkvp, 0), dims.qkv(qkvp, 1), false, dims.scores(ptr<float>(S)), dims.scale2());
    ops.push_back(op);
    Op sm = make_op(OP_SOFTMAX);
    sm.softmax.S = ptr<float>(S);
    sm.softmax.rows = (int64_t)N * H * T;
    sm.softmax.cols = (int)T;
    ops.push_back(sm);
    op.gemm = attn_gemm(dims, dims.scores(ptr<float>(S)), dims.qkv(qkvp, 2), true, dims.heads(ptr<float>(a)), 1.0f);
    ops.push_back(op);
    scratch_free(S, s_bytes);
  }
  Act out = new_act(C, R);
  const Act av = view(a, C, R);  // `a` as an activation for the 1x1 conv
  ConvDesc cp = conv_of(p + ".proj_out", av, out);
  cp.ksz = 1;
  cp.residual = ptr<float>(x.off);
  cp.stats_of = &out;
  cp.in_f32 = !a_is_bf16;
  emit_conv(cp);
  if (v2_bytes) scratch_free(v2_work, v2_bytes);
  if (split_bytes) scratch_free(split_work, split_bytes);
  scratch_free(qkv, qkv_bytes);
  scratch_free(a, a_bytes);
  if (tape) {
    Tape& t = record(b, x, out);
    t.coefA = coef;
    t.momA = momX;
    t.qkv = qkv;
    t.a = a;
  }
  return out;
}

// runs a TimestepEmbedSequential; consumes (releases) the input activation(s)
Act Planner::run_layers(const std::vector<Block>& layers, Act h, Act* skip, bool release_h) {
  bool first = true;
  for (const Block& b : layers) {
    Act out;
    if (b.kind == B_RES) {
      out = resblock(b, h, first ? skip : nullptr);
    } else if (b.kind == B_ATTN) {
      out = attention(b, h);
    } else {  // a bare convolution: input conv, Downsample (stride 2), Upsample (nearest x2 on load)
      out = new_act(b.cout, b.kind == B_DOWN ? h.R / 2 : b.kind == B_UP ? h.R * 2 : h.R);
      ConvDesc d = conv_of(b.prefix + (b.kind == B_DOWN ? ".op" : b.kind == B_UP ? ".conv" : ""), h, out);
      if (b.kind == B_DOWN) d.out_R = out.R, d.stride = 2;
      if (b.kind == B_UP) d.in_R = out.R, d.ups = 1;
      d.stats_of = &out;
      emit_conv(d);
      if (tape) record(b, h, out);
    }
    if (!first || release_h) release(h);
    if (first && skip) release(*skip);
    h = out;
    first = false;
  }
  return h;
}

void Planner::build() {
  const HoloUnetCfg& c = u->cfg;
  const int R = c.image_size;
  plan.invalidate();
  plan.sizing = sizing;
  // time embedding
  size_t emb = small_alloc((size_t)N * u->ted * 4);
  size_t embs = small_alloc((size_t)N * u->ted * 4);
  eml_off = small_alloc((size_t)N * u->emb_rows * 4);
  embs_off = embs;
  {
    Op op = make_op(OP_TEMB);
    op.temb.w1 = P(u, "time_embed.0.weight");
    op.temb.b1 = P(u, "time_embed.0.bias");
    op.temb.w2 = P(u, "time_embed.2.weight");
    op.temb.b2 = P(u, "time_embed.2.bias");
    op.temb.emb = ptr<float>(emb);
    op.temb.emb_silu = ptr<float>(embs);
    op.temb.load_kind = (int)knobs.debug_timestep_load;
    ops.push_back(op);
  }
  {
    Op op = make_op(OP_EMBLIN);
    op.emblin.emb_silu = ptr<float>(embs);
    op.emblin.w = u->emb_w;
    op.emblin.b = u->emb_b;
    op.emblin.out = ptr<float>(eml_off);
    ops.push_back(op);
  }
  Act x = new_act(c.in_channels, R);
  x_in = x;
  {
    Op op = make_op(OP_IN);
    op.in.dst = ptr<float>(x.off);
    op.in.C = c.in_channels;
    op.in.V = vox(R);
    op.in.dst_bf16 = bfs() ? 1 : 0;
    ops.push_back(op);
  }
  std::vector<Act> hs;
  Act h = x;
  char tag[64];
  bool forked = false;
  for (size_t i = 0; i < u->inputs.size(); ++i) {
    // the side lane starts in front of the first level whose edge is at most HOLO_SIDE_LANE_FORK_R (else in front of the middle)
    if (!forked && (u->inputs[i][0].kind == B_DOWN ? h.R / 2 : h.R) <= knobs.side_lane_fork_r) {
      plan_side_lane(hs);
      forked = true;
    }
    // h is also referenced by hs (except the raw input x): do not release it when consumed
    h = run_layers(u->inputs[i], h, nullptr, /*release_h=*/i == 0);
    hs.push_back(h);
    snprintf(tag, sizeof tag, "input_blocks.%d", (int)i);
    plan.block_outputs[tag] = h;
  }
  if (!forked) plan_side_lane(hs);
  // middle: h == hs.back(); keep it alive for the skip connection
  h = run_layers(u->middle, h, nullptr, false);
  plan.block_outputs["middle_block"] = h;
  for (size_t i = 0; i < u->outputs.size(); ++i) {
    Act skip = hs.back();
    hs.pop_back();
    h = run_layers(u->outputs[i], h, &skip, true);
    snprintf(tag, sizeof tag, "output_blocks.%d", (int)i);
    plan.block_outputs[tag] = h;
  }
  for (const auto& kv : side_parts)
    if (!kv.second.consumed && err.empty()) err = "internal: the side part of " + kv.first + " has no consumer";
  size_t coef = emit_finalize(h, nullptr, "out.0");
  Act y = new_act(c.out_channels, R, /*f32=*/true);  // the network output stays fp32
  if (tape) {
    Tape& t = record(Block{B_HEAD, "out", u->final_ch, c.out_channels}, h, y);
    t.coefA = coef;
    t.momA = last_mom;
  }
  ConvDesc head = conv_of("out.2", h, y);
  head.coef = coef;
  head.act = 1;
  head.out_f32 = true;
  emit_conv(head);
  y_out = y;
  release(h);
  {
    Op op = make_op(OP_OUT);
    op.out.src = ptr<float>(y.off);
    op.out.C = c.out_channels;
    op.out.V = vox(R);
    ops.push_back(op);
  }
  release(y);
  if (knobs.debug_plan) {  // development: what the plan launches
    int n_fin = 0, n_conv = 0, n_split = 0;
    for (const Op& o : ops) {
      n_fin += o.kind == OP_FINAL;
      if (o.kind != OP_CONV) continue;
      ++n_conv;
      n_split += o.conv.nsplit > 1;
    }
    fprintf(stderr, "[plan] batch %d: %zu ops | %d convs, %d of them split-K (+ a reduce launch) | %d gn_finalize launches\n", N, ops.size(),
            n_conv, n_split, n_fin);
  }
  find_cl_ends();
  plan.batch = N;
  plan.ws = ptr<void>(0);
  plan.bytes = arena_base + arena.peak;
}
// holo_unet_forward_cl points every convolution that reads the plan's input buffer or writes its output buffer at the
// caller's channels-last tensors instead (by POSITION in the op list, not by address: the arena hands the input
// buffer's memory to later activations).  Which two those are, and whether they can, is a property of the plan.
void Planner::find_cl_ends() {
  const float* in_buf = nullptr;
  const float* out_buf = nullptr;
  int first = -1, last = -1;
  for (size_t i = 0; i < ops.size(); ++i) {
    const Op& op = ops[i];
    if (op.kind == OP_IN) in_buf = op.in.dst;
    if (op.kind == OP_OUT) out_buf = op.out.src;
    if (op.kind == OP_CONV) {
      if (first < 0 && in_buf) first = (int)i;
      last = (int)i;
    }
  }
  plan.first_conv = first;
  plan.last_conv = last;
  // (a split-K launch at either end is fine: its kernel reads src0 like an un-split one, and the reduce launch behind it
  // writes `out` - the small and the non-tileable grids, whose 16- or 32-channel end convolutions are split to fill the chip)
  if (first < 0 || !in_buf || !out_buf || ops[first].conv.src0 != in_buf || ops[first].conv.src1 ||
      ops[last].conv.out != out_buf || first == last) {
    plan.cl_refusal = "holo_unet_forward_cl: this plan's first / last convolution cannot take the caller's tensors";
  } else if (bfs() && (ops[last].conv.out_bf16 || !ops[first].conv.in_bf16)) {
    plan.cl_refusal = "holo_unet_forward_cl: unexpected storage types at the ends of the bf16 plan";
  }
}


const char* preact_refusal(const PreactShape& s) {
  // the finalize block walks its group in 4-channel quads, each from one source of the virtual concat
  if (s.cpg % 4 != 0) return "a group is no whole number of 4-channel quads";
  if (s.C0 % 4 != 0) return "a quad would straddle the seam of the concat";
  // one block per (group, sample) writes V x cpg elements behind its reduction: beyond the deepest level that is a serial
  // pass of its own in front of the convolution
  if (s.V > PREACT_MAX_VOX) return "the tensor is too large for the finalize launch";
  // the extra write and read of the tensor must replace many activations per element
  if (s.redundancy < PREACT_MIN_REDUNDANCY) return "the convolution repeats too little of the activation";
  return nullptr;
}

Preact preactivate_rowtile(Plan& plan, const Knobs& knobs) {
  Preact r;
  std::vector<Op>& ops = plan.ops;
  const int N = plan.batch;
  const uintptr_t base = reinterpret_cast<uintptr_t>(plan.ws);
  r.scratch_off = Arena::al(plan.bytes);
  float* const scratch = reinterpret_cast<float*>(base + r.scratch_off);
  for (size_t i = 0; knobs.rowtile_preact && i < ops.size(); ++i) {
    if (ops[i].kind != OP_FINAL || ops[i].side || ops[i].fin.act) continue;
    GnFinalize& f = ops[i].fin;
    int readers = 0;
    for (const Op& o : ops) readers += o.kind == OP_CONV && o.conv.coef == f.coef;
    size_t j = i + 1;
    while (j < ops.size() && (ops[j].side || ops[j].kind != OP_CONV)) ++j;  // the next convolution of the caller's stream
    if (readers != 1 || j == ops.size() || ops[j].conv.coef != f.coef) continue;
    ConvParams& p = ops[j].conv;
    const int Cin = p.C0 + p.C1;
    const int64_t V = (int64_t)p.ID * p.IH * p.IW;
    if (p.kernel != ConvKernel::RowTile || p.bf16 != 0 || p.in_bf16 != 0 || p.ups || p.N != N || f.moments) continue;
    if (Cin != f.C0 + f.C1 || V != f.V || f.groups < 1 || Cin % f.groups) continue;  // (the finalize of this very input)
    const PreactShape shape{Cin / f.groups, p.C0, V, p.ksz * p.ksz * p.ksz * ((p.Cout + 63) / 64)};
    if (preact_refusal(shape)) continue;
    ConvParams q = p;
    q.src0 = scratch, q.C0 = Cin, q.src1 = nullptr, q.C1 = 0, q.coef = nullptr;
    if (!conv_can_launch(q)) continue;
    f.x0 = p.src0, f.x1 = p.src1, f.act = scratch, f.act_silu = p.act;
    q.act = 0;  // (only with coef)
    p = q;
    const size_t bytes = (size_t)N * (size_t)V * Cin * sizeof(float);
    if (bytes > r.scratch_bytes) r.scratch_bytes = bytes;
    ++r.pairs;
  }
  if (r.pairs) plan.bytes = r.scratch_off + Arena::al(r.scratch_bytes);
  if (knobs.debug_plan)
    fprintf(stderr, "[plan] batch %d: %d finalize + row-tile convolution pairs pre-activated (%zu bytes of scratch behind the plan)\n",
            N, r.pairs, r.pairs ? Arena::al(r.scratch_bytes) : (size_t)0);
  return r;
}

}  // namespace unetplan
}  // namespace holo
