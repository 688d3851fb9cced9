// unet_train_plan.cpp — the training planner of the denoiser (unet_train_plan.h): host-only arithmetic, no HIP header.
#include "unet_train_plan.h"

namespace holo {
namespace unetplan {

TrainPlanner::TrainPlanner(const UnetDesc* u_, const DgradTable& dgrad_, int N_, void* ws, TrainPlan& tp_)
    : u(u_), dgrad(dgrad_), N(N_), tp(tp_), pl(u_, N_, ws, tp_.fwd), bops(tp_.bops) {
  pl.arena.keep = true;
  pl.tape = &tape;
}

size_t TrainPlanner::grad_of(const Act& a, int* acc) {
  auto it = grads.find(a.off);
  if (it == grads.end()) {
    const size_t off = alloc((size_t)N * vox(a.R) * a.C * sizeof(float));
    grads[a.off] = std::make_pair(off, true);
    *acc = 0;
    return off;
  }
  *acc = 1;
  return it->second.first;
}
size_t TrainPlanner::grad_ready(const Act& a) {
  auto it = grads.find(a.off);
  if (it == grads.end()) {
    err = "internal: a layer output has no gradient";
    return NONE;
  }
  return it->second.first;
}
float* TrainPlanner::pgrad(const std::string& name) {
  auto it = u->pindex.find(name);
  return it == u->pindex.end() ? nullptr : ptr<float>(tp.grad_off[it->second]);
}
// The transposed weights under `name`, or null.  A sizing pass (Plan::sizing) launches nothing and must not fail
// on weights that were not supplied yet, so there every convolution weight counts as present, and so does the stride-1
// form "<name>#s1" of a Downsample weight whose two leading dims are multiples of 4 (the one holo_unet_set_dgrad_weight
// creates); they count as plain fp32 copies, without Winograd forms.
std::optional<ConvWeights> TrainPlanner::find_dgw(const std::string& name) {
  auto it = dgrad.find(name);
  if (it != dgrad.end()) return it->second;
  if (!tp.fwd.sizing) return std::nullopt;
  const bool s1 = name.size() > 3 && name.compare(name.size() - 3, 3, "#s1") == 0;
  auto pi = u->pindex.find(s1 ? name.substr(0, name.size() - 3) : name);
  if (pi == u->pindex.end()) return std::nullopt;
  const ParamSlot& s = u->params[pi->second];
  if (!s.is_conv()) return std::nullopt;
  if (s1 && (!is_downsample_weight(s.name) || (s.shape[0] & 3) || (s.shape[1] & 3))) return std::nullopt;
  static float never_read;
  ConvWeights assumed;
  assumed.f32 = &never_read;
  assumed.layout = s.layout(true);
  return assumed;
}
std::optional<ConvWeights> TrainPlanner::dgw(const std::string& name) {
  const std::optional<ConvWeights> w = find_dgw(name);
  if (!w) err = "holo_unet_backward: call holo_unet_set_dgrad_weight for '" + name + "' first";
  return w;
}

// dgrad of a stride-1 conv (3x3x3 pad 1 or 1x1x1): out[M][cin] = conv(gy[M][cout], flipped weights)
void TrainPlanner::emit_dgrad(size_t gy_off, int cout, int R, const std::string& wname, int cin, int ksz, size_t out_off,
                              bool accumulate) {
  const std::optional<ConvWeights> w = dgw(wname);
  if (!w) return;
  const Act g = view(gy_off, cout, R);
  ConvDesc d;
  d.x0 = &g;
  d.ksz = ksz;
  d.w = *w;
  d.residual = accumulate ? ptr<float>(out_off) : nullptr;
  d.out = ptr<float>(out_off);
  d.Cout = cin;
  BwdOp op = make_bwd_op(BOP_CONV);
  op.conv = pl.place_conv(d);
  bops.push_back(op);
}
// wgrad of the forward convolution `f` (sources, geometry, coefficients on load, Cout) into the gradients of
// `layer`.weight / .bias
void TrainPlanner::emit_wgrad(size_t gy_off, const ConvDesc& f, const std::string& layer) {
  const float* gy = ptr<float>(gy_off);
  const int cout = f.Cout;
  BwdOp op = make_bwd_op(BOP_WGRAD);
  WgradParams& w = op.wgrad.p;
  w.gy = gy;
  w.src0 = ptr<float>(f.x0->off);
  w.src1 = f.x1 ? ptr<float>(f.x1->off) : nullptr;
  w.C0 = f.x0->C;
  w.C1 = f.x1 ? f.x1->C : 0;
  w.N = N;
  w.ID = w.IH = w.IW = f.in_size();
  w.ups = f.ups;
  w.OD = w.OH = w.OW = f.out_size();
  w.stride = f.stride;
  w.pad = f.ksz == 3 ? 1 : 0;
  w.ksz = f.ksz;
  w.ntaps = f.ksz == 3 ? 27 : 1;
  w.Cout = cout;
  w.coef = f.coef ? ptr<float>(*f.coef) : nullptr;
  w.act = f.act;
  op.wgrad.plan = wgrad_plan(w, u->num_cus, pl.knobs);
  w.partial = ptr<float>(alloc(wgrad_partial_bytes(w, op.wgrad.plan)));
  op.wgrad.dw = pgrad(layer + ".weight");
  bops.push_back(op);
  BwdOp cs = make_bwd_op(BOP_COLSUM);
  cs.colsum.g = gy;
  cs.colsum.M = (int64_t)N * vox(f.out_size());
  cs.colsum.C = cout;
  cs.colsum.out = pgrad(layer + ".bias");
  cs.colsum.scratch = ptr<double>(alloc(colsum_scratch_bytes(cout)));
  bops.push_back(cs);
}
void TrainPlanner::emit_add(float* dst, const float* src, int64_t n, int acc) {
  BwdOp op = make_bwd_op(BOP_ADD);
  op.add = AddGrad{dst, src, n, acc};
  bops.push_back(op);
}
// the forward convolution of `cout` channels out of [x0 | x1], as emit_wgrad wants it
static ConvDesc fwd_conv(const Act& x0, const Act* x1, int cout) {
  ConvDesc f;
  f.x0 = &x0;
  f.x1 = x1;
  f.Cout = cout;
  return f;
}
// Backward of the stride-1 convolution `layer` = f(act(norm([x0 | x1]))) from the gradient of its output at gy_off:
// dgrad into a scratch ga [M][Cin], wgrad, then GroupNorm `norm` (+FiLM) (+SiLU) backward: ga -> gradients of x0 / x1
void TrainPlanner::bwd_norm_conv(size_t gy_off, const ConvDesc& f, const std::string& layer, const std::string& norm, size_t mom,
                                 const FilmGrad* film) {
  const Act &x0 = *f.x0, *x1 = f.x1;
  const int Cin = x0.C + (x1 ? x1->C : 0);
  const size_t ga = alloc((size_t)N * vox(x0.R) * Cin * sizeof(float));
  emit_dgrad(gy_off, f.Cout, x0.R, layer + ".weight", Cin, f.ksz, ga);
  emit_wgrad(gy_off, f, layer);
  BwdOp op = make_bwd_op(BOP_GN_BWD);
  GnBwdParams& g = op.gn;
  g.x0 = ptr<float>(x0.off);
  g.x1 = x1 ? ptr<float>(x1->off) : nullptr;
  g.C0 = x0.C;
  g.C1 = x1 ? x1->C : 0;
  g.N = N;
  g.V = vox(x0.R);
  g.ga = ptr<float>(ga);
  g.coef = ptr<float>(*f.coef);
  g.mom = ptr<float>(mom);
  g.gamma = P(u, norm + ".weight");
  g.beta = P(u, norm + ".bias");
  g.film = film ? film->film : nullptr;
  g.film_stride = u->emb_rows;
  g.film_cout = film ? film->cout : 0;
  g.act = f.act;
  g.part = ptr<double>(alloc(gn_bwd_scratch_bytes(g)));
  g.grp = ptr<float>(alloc((size_t)N * Cin * 2 * sizeof(float)));
  g.dgamma = pgrad(norm + ".weight");
  g.dbeta = pgrad(norm + ".bias");
  g.dfilm = film ? film->dfilm : nullptr;
  g.gx0 = ptr<float>(grad_of(x0, &g.acc0));
  if (x1) g.gx1 = ptr<float>(grad_of(*x1, &g.acc1));
  bops.push_back(op);
}

void TrainPlanner::bwd_res(const Tape& t, float* dfilm_base) {
  const std::string& p = t.b.prefix;
  const int R = t.x0.R, cin = t.b.cin, cout = t.b.cout;
  const int64_t M = (int64_t)N * vox(R);
  const size_t gout = grad_ready(t.out);
  if (gout == NONE) return;
  const Act* x1 = t.has_x1 ? &t.x1 : nullptr;
  // second conv: out = skip(x) + conv2(silu(film(gn2(h1))))
  ConvDesc c2 = fwd_conv(t.h1, nullptr, cout);
  c2.coef = t.coefB;
  c2.act = 1;
  const FilmGrad fg{t.film, cout, dfilm_base + u->emb_row_off.at(p)};
  bwd_norm_conv(gout, c2, p + ".out_layers.3", p + ".out_layers.0", t.momB, &fg);
  const size_t gh1 = grad_ready(t.h1);
  if (gh1 == NONE) return;
  // first conv: h1 = conv1(silu(gn1([x0 | x1])))
  ConvDesc c1 = fwd_conv(t.x0, x1, cout);
  c1.coef = t.coefA;
  c1.act = 1;
  bwd_norm_conv(gh1, c1, p + ".in_layers.2", p + ".in_layers.0", t.momA);
  // skip connection: identity, or a 1x1x1 conv of the raw input
  int a0 = 0, a1 = 0;
  float* gx0 = ptr<float>(grad_of(t.x0, &a0));
  float* gx1 = x1 ? ptr<float>(grad_of(*x1, &a1)) : nullptr;
  const float* goutp = ptr<float>(gout);
  if (!t.has_skip) {
    emit_add(gx0, goutp, M * cin, a0);
  } else {
    const size_t gso = alloc((size_t)M * cin * sizeof(float));
    const float* gs = ptr<float>(gso);
    emit_dgrad(gout, cout, R, p + ".skip_connection.weight", cin, 1, gso);
    ConvDesc cs = fwd_conv(t.x0, x1, cout);
    cs.ksz = 1;
    emit_wgrad(gout, cs, p + ".skip_connection");
    if (x1) {
      BwdOp op = make_bwd_op(BOP_SPLIT_CAT);
      op.split = SplitCat{gs, gx0, gx1, M, t.x0.C, t.x1.C, a0, a1};
      bops.push_back(op);
    } else {
      emit_add(gx0, gs, M * cin, a0);
    }
  }
}

void TrainPlanner::bwd_attn(const Tape& t) {
  const std::string& p = t.b.prefix;
  const int C = t.x0.C, R = t.x0.R, H = u->cfg.num_heads;
  const int64_t T = vox(R), M = (int64_t)N * T;
  const AttnDims dims{N, H, C, T};
  const size_t gout = grad_ready(t.out);
  if (gout == NONE) return;
  int ax = 0;
  float* gx = ptr<float>(grad_of(t.x0, &ax));
  emit_add(gx, ptr<float>(gout), M * C, ax);  // identity branch
  // proj_out (1x1 over the attention output a)
  const Act av = view(t.a, C, R);
  const size_t ga_off = alloc((size_t)M * C * sizeof(float));
  float* ga = ptr<float>(ga_off);
  emit_dgrad(gout, C, R, p + ".proj_out.weight", C, 1, ga_off);
  ConvDesc cp = fwd_conv(av, nullptr, C);
  cp.ksz = 1;
  emit_wgrad(gout, cp, p + ".proj_out");
  // attention core: P = softmax(s2 q k^T); dP = ga v^T; dS = P (dP - rowsum(dP P)); dv = P^T ga; dq = s2 dS k; dk = s2 dS^T q
  const size_t sb = (size_t)N * H * T * T * sizeof(float);
  float* Pm = ptr<float>(alloc(sb));
  float* dS = ptr<float>(alloc(sb));
  float* Tm = ptr<float>(alloc(sb));
  const size_t gqkv_off = alloc((size_t)M * 3 * C * sizeof(float));
  float* gqkv = ptr<float>(gqkv_off);
  float* qkv = ptr<float>(t.qkv);
  const float s2 = dims.scale2();
  auto gemm = [&](AttnMat A, AttnMat B, bool b_kmajor, AttnMat Cc, float alpha) {
    BwdOp op = make_bwd_op(BOP_GEMM);
    op.gemm = attn_gemm(dims, A, B, b_kmajor, Cc, alpha);
    bops.push_back(op);
  };
  auto transpose = [&](const float* in, float* out) {
    BwdOp op = make_bwd_op(BOP_TRANSPOSE);
    op.tr = Transpose{in, out, N * H, (int)T};
    bops.push_back(op);
  };
  const int64_t rows = (int64_t)N * H * T;
  BwdOp sm = make_bwd_op(BOP_SOFTMAX), ds = make_bwd_op(BOP_ATTN_DS);
  sm.softmax = Softmax{Pm, rows, (int)T};
  ds.ds = AttnDs{Pm, dS, rows, (int)T};
  gemm(dims.qkv(qkv, 0), dims.qkv(qkv, 1), false, dims.scores(Pm), s2);
  bops.push_back(sm);
  gemm(dims.heads(ga), dims.qkv(qkv, 2), false, dims.scores(dS), 1.0f);
  bops.push_back(ds);
  transpose(Pm, Tm);
  gemm(dims.scores(Tm), dims.heads(ga), true, dims.qkv(gqkv, 2), 1.0f);  // dv
  gemm(dims.scores(dS), dims.qkv(qkv, 1), true, dims.qkv(gqkv, 0), s2);    // dq
  transpose(dS, Tm);
  gemm(dims.scores(Tm), dims.qkv(qkv, 0), true, dims.qkv(gqkv, 1), s2);  // dk
  // qkv conv (1x1, C -> 3C, GroupNorm applied on load, no activation)
  ConvDesc cq = fwd_conv(t.x0, nullptr, 3 * C);
  cq.ksz = 1;
  cq.coef = t.coefA;
  bwd_norm_conv(gqkv_off, cq, p + ".qkv", p + ".norm", t.momA);
}

void TrainPlanner::bwd_conv(const Tape& t) {
  const BlockKind kind = t.b.kind;
  const int cin = t.b.cin, cout = t.b.cout, Ri = t.x0.R, Ro = t.out.R;
  const size_t gout = grad_ready(t.out);
  if (gout == NONE) return;
  ConvDesc f = fwd_conv(t.x0, nullptr, cout);
  if (kind == B_HEAD) {  // y = conv(silu(gn(h)))
    f.coef = t.coefA;
    f.act = 1;
    bwd_norm_conv(gout, f, "out.2", "out.0", t.momA);
    return;
  }
  int ax = 0;
  const size_t gx_off = grad_of(t.x0, &ax);
  float* gx = ptr<float>(gx_off);
  const float* goutp = ptr<float>(gout);
  const std::string layer = t.b.prefix + (kind == B_DOWN ? ".op" : kind == B_UP ? ".conv" : "");
  const std::string wn = layer + ".weight";
  if (kind == B_CONV) {
    if (ax) {
      err = "internal: the input conv's source already has a gradient";
      return;
    }
    emit_dgrad(gout, cout, Ri, wn, cin, 3, gx_off);
  } else if (kind == B_DOWN) {
    const std::optional<ConvWeights> wt = dgw(wn);
    if (!wt) return;
    // (HOLO_DGRAD_S2_DIRECT=1, development / test knob: conv_dgrad_s2_kernel everywhere)
    if (!pl.knobs.dgrad_s2_direct && find_dgw(wn + "#s1") && Ri == 2 * Ro && (Ri % 8) == 0) {
      // zero insertion + the stride-1 transposed convolution on the forward's conv kernels (8x the multiply-adds, on the
      // Winograd kernels: 0.24 instead of 1.35 ms at 64^3 <- 32^3)
      const size_t gz_off = alloc((size_t)N * vox(Ri) * cout * sizeof(float));
      BwdOp op = make_bwd_op(BOP_ZERO_INSERT2);
      op.zins = ZeroInsert2{goutp, ptr<float>(gz_off), N, Ro, cout};
      bops.push_back(op);
      emit_dgrad(gz_off, cout, Ri, wn + "#s1", cin, 3, gx_off, ax != 0);
    } else {
      BwdOp op = make_bwd_op(BOP_DGRAD_S2);
      op.s2 = DgradS2{goutp, wt->f32, gx, N, Ri, Ro, cin, cout, ax};
      bops.push_back(op);
    }
    f.out_R = Ro;
    f.stride = 2;
  } else {  // B_UP: conv at the fine size of the nearest-upsampled input
    const int64_t Mf = (int64_t)N * vox(Ro);
    const size_t gup_off = alloc((size_t)Mf * cin * sizeof(float));
    emit_dgrad(gout, cout, Ro, wn, cin, 3, gup_off);
    BwdOp op = make_bwd_op(BOP_SUMPOOL2);
    op.pool = SumPool2{ptr<float>(gup_off), gx, N, Ri, cin, ax};
    bops.push_back(op);
    f.in_R = Ro;
    f.ups = 1;
  }
  emit_wgrad(gout, f, layer);
}

void TrainPlanner::build() {
  const HoloUnetCfg& c = u->cfg;
  tp.invalidate();
  pl.build();
  // parameter gradients: one region in the reference's layouts; emb_layers rows alias the concatenated matrix
  tp.grad_off.assign(u->params.size(), 0);
  const size_t gembw = alloc((size_t)u->emb_rows * u->ted * sizeof(float));
  const size_t gembb = alloc((size_t)u->emb_rows * sizeof(float));
  for (size_t i = 0; i < u->params.size(); ++i) {
    const ParamSlot& s = u->params[i];
    if (s.kind == P_EMB_W || s.kind == P_EMB_B) {
      const int row = u->emb_row_off.at(s.name.substr(0, s.name.rfind(".emb_layers")));
      tp.grad_off[i] = s.kind == P_EMB_W ? gembw + (size_t)row * u->ted * sizeof(float) : gembb + (size_t)row * sizeof(float);
    } else {
      tp.grad_off[i] = alloc((size_t)s.numel * sizeof(float));
    }
  }
  // the gradient of the output arrives NCDHW and is laid out channels-last as the gradient of y
  const int R = c.image_size;
  const int64_t V = vox(R);
  const size_t gy = alloc((size_t)N * V * c.out_channels * sizeof(float));
  grads[pl.y_out.off] = std::make_pair(gy, true);
  tp.gy_off = gy;
  const size_t dfilm = alloc((size_t)N * u->emb_rows * sizeof(float));
  float* dfilm_base = ptr<float>(dfilm);
  for (int i = (int)tape.size() - 1; i >= 0 && err.empty(); --i) {
    const Tape& t = tape[i];
    if (t.b.kind == B_RES)
      bwd_res(t, dfilm_base);
    else if (t.b.kind == B_ATTN)
      bwd_attn(t);
    else
      bwd_conv(t);
  }
  if (err.empty()) err = pl.err;  // (place_conv's refusals)
  if (!err.empty()) return;
  // embedding path
  {
    float* gembs = ptr<float>(alloc((size_t)N * u->ted * sizeof(float)));
    BwdOp fb = make_bwd_op(BOP_FILM_BWD);
    fb.film = FilmBwd{dfilm_base, ptr<float>(pl.embs_off), u->emb_w, ptr<float>(gembw), ptr<float>(gembb), gembs, N, u->emb_rows, u->ted};
    bops.push_back(fb);
    BwdOp te = make_bwd_op(BOP_TEMB_BWD);
    te.temb = TimeEmbedBwd{N, c.model_channels, u->ted,
                           P(u, "time_embed.0.weight"), P(u, "time_embed.0.bias"), P(u, "time_embed.2.weight"), P(u, "time_embed.2.bias"), gembs,
                           pgrad("time_embed.0.weight"), pgrad("time_embed.0.bias"), pgrad("time_embed.2.weight"), pgrad("time_embed.2.bias")};
    bops.push_back(te);
  }
  auto gi = grads.find(pl.x_in.off);
  if (gi == grads.end()) {
    err = "internal: the network input has no gradient";
    return;
  }
  tp.gx_off = gi->second.first;
  tp.bytes = tp.fwd.bytes = pl.arena_base + pl.arena.peak;  // (the backward's buffers grew the arena after pl.build())
}

}  // namespace unetplan
}  // namespace holo
