// fold_check.cpp — stand-alone check of holo_diffusion_amd/csrc/mlp_folds.h (built and run by tests/test_mlp_folds_cpu.py
// under ASan + UBSan; no GPU, no HIP header).  From a fixed seed, for the density net, the radiance layer and the MLPMean
// pooler:
//   1. fold == layers: the folded affine map against the layer-by-layer product, both in float64, on 32 random inputs; the
//      difference is held to 1e-10 of the largest |output| (chains of <= 256-term double sums sit near 1e-13);
//   2. un-fold == adjoint of the fold: with random cotangents (G, g) and L = <G, folded weights> + <g, folded biases>, L is
//      linear in every raw parameter P separately, so for a random step d' = fl(P + d) - P (exact in float64)
//          |L(P + d') - L(P) - <grad_P, d'>| <= 1e-5 * sum |grad_P . d'|
//      (the gradients are rounded to float, 6e-8 per term);
//   3. the packed images against the float64 folds, element by element (layout, padding, transposes).
// Exit status 0 and "fold_check: OK" when everything holds; every violated check prints a line and the status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "mlp_folds.h"

using namespace holo;

static int g_failures = 0;
static void expect(bool ok, const char* what, double got, double bound) {
  if (ok) return;
  ++g_failures;
  printf("FAILED %s: %.3e (bound %.3e)\n", what, got, bound);
}

struct Rng {  // splitmix64
  uint64_t s;
  double uniform() {  // [-1, 1)
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  }
  FVec vec(size_t n, double scale) {
    FVec v(n);
    for (float& x : v) x = (float)(scale * uniform());
    return v;
  }
};

// y (+)= W x, W [rows][cols] row-major with row stride ld, columns col0 .. col0 + cols - 1
static void matvec(const FVec& W, int rows, int cols, int ld, int col0, const DVec& x, DVec& y) {
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) y[i] += (double)W[(size_t)i * ld + col0 + j] * x[j];
}
static DVec bias(const FVec& b) { return DVec(b.begin(), b.end()); }
static double max_abs(const DVec& v) {
  double m = 0;
  for (double x : v) m = std::fmax(m, std::fabs(x));
  return m;
}
static void expect_close(const DVec& got, const DVec& want, const char* what) {
  double d = 0;
  for (size_t i = 0; i < want.size(); ++i) d = std::fmax(d, std::fabs(got[i] - want[i]));
  const double bound = 1e-10 * max_abs(want);
  expect(got.size() == want.size() && d <= bound, what, d, bound);
}
static void expect_same(float got, double want, const char* what) { expect(got == (float)want, what, got, want); }

// check 2 for one raw parameter: L() evaluates the functional from the CURRENT parameter values, L0 is its value before the step
template <class Functional>
static void expect_adjoint(const char* what, FVec& P, const FVec& grad, Rng& rng, const Functional& L, double L0) {
  if (grad.size() != P.size()) return expect(false, what, (double)grad.size(), (double)P.size());
  const FVec saved = P;
  double lin = 0, mag = 0, scale = 0;
  for (float x : P) scale = std::fmax(scale, std::fabs(x));
  for (size_t i = 0; i < P.size(); ++i) {
    P[i] = saved[i] + (float)(scale * rng.uniform());
    const double step = (double)P[i] - (double)saved[i];
    lin += grad[i] * step;
    mag += std::fabs(grad[i] * step);
  }
  const double L1 = L();
  P = saved;
  expect(std::fabs(L1 - L0 - lin) <= 1e-5 * mag && mag > 0, what, std::fabs(L1 - L0 - lin), 1e-5 * mag);
}
static double dot(const FVec& g, const DVec& v, size_t n) {
  double s = 0;
  for (size_t i = 0; i < n; ++i) s += (double)g[i] * v[i];
  return s;
}

static void check_render_mlp(int C, int Hd, int De, Rng& rng) {
  const int H1 = Hd + 1, L2 = Hd + C, Hp = (H1 + 3) & ~3;
  FVec W0 = rng.vec((size_t)Hd * C, 1 / std::sqrt(C)), b0 = rng.vec(Hd, 0.5);
  FVec W1 = rng.vec((size_t)Hd * Hd, 1 / std::sqrt(Hd)), b1 = rng.vec(Hd, 0.5);
  FVec W2 = rng.vec((size_t)Hd * L2, 1 / std::sqrt(L2)), b2 = rng.vec(Hd, 0.5);
  FVec W3 = rng.vec((size_t)H1 * Hd, 1 / std::sqrt(Hd)), b3 = rng.vec(H1, 0.5);
  FVec Wr = rng.vec((size_t)3 * (Hd + De), 1 / std::sqrt(Hd + De)), br = rng.vec(3, 0.5);
  auto fold = [&] { return fold_density_net(W0, b0, W1, b1, W2, b2, W3, b3, C, Hd); };
  const DensityFold f = fold();
  // 1. fold == layers
  for (int t = 0; t < 32; ++t) {
    const DVec x = bias(rng.vec(C, 1.0));
    DVec y0 = bias(b0), y1 = bias(b1), y2 = bias(b2), o = bias(b3), folded(f.be);
    matvec(W0, Hd, C, C, 0, x, y0);
    matvec(W1, Hd, Hd, Hd, 0, y0, y1);
    matvec(W2, Hd, Hd, L2, 0, y1, y2);
    matvec(W2, Hd, C, L2, Hd, x, y2);
    matvec(W3, H1, Hd, Hd, 0, y2, o);
    for (int i = 0; i < H1; ++i)
      for (int j = 0; j < C; ++j) folded[i] += f.We[(size_t)i * C + j] * x[j];
    expect_close(folded, o, "density net: We f + be against the four layers");
  }
  // 2. un-fold == adjoint.  The cotangents have exactly Hd + 1 rows: a read of a padding row is an ASan report.
  const FVec G = rng.vec((size_t)H1 * C, 1.0), g = rng.vec(H1, 1.0);
  const DensityGrads d = unfold_density_grads(f, W0, b0, W1, W2, W3, G, g, C, Hd);
  const auto L = [&] {
    const DensityFold q = fold();
    return dot(G, q.We, G.size()) + dot(g, q.be, g.size());
  };
  const double L0 = L();
  expect_adjoint("density net: dW0", W0, d.dW0, rng, L, L0), expect_adjoint("density net: db0", b0, d.db0, rng, L, L0);
  expect_adjoint("density net: dW1", W1, d.dW1, rng, L, L0), expect_adjoint("density net: db1", b1, d.db1, rng, L, L0);
  expect_adjoint("density net: dW2", W2, d.dW2, rng, L, L0), expect_adjoint("density net: db2", b2, d.db2, rng, L, L0);
  expect_adjoint("density net: dW3", W3, d.dW3, rng, L, L0), expect_adjoint("density net: db3", b3, d.db3, rng, L, L0);
  // radiance layer: the forward image holds w_rad [3][Hd] | w_dir [3][De] behind w_feat | b_feat | w_dens, b_rad travels apart
  const FVec dWrh = rng.vec((size_t)Hd * 4, 1.0), ddir = rng.vec((size_t)3 * (De + 1), 1.0);
  const RadianceGrads rad = unfold_radiance_grads(dWrh, ddir, Hd, De);
  const auto Lr = [&] {
    const RenderMlpPack p = pack_render_mlp(f, Wr, br, C, Hd, De);
    const float* w_rad = p.image.data() + (size_t)Hd * C + Hd + C;
    const float* w_dir = w_rad + 3 * Hd;
    double s = 0;
    for (int j = 0; j < 3; ++j) {
      for (int h = 0; h < Hd; ++h) s += (double)dWrh[(size_t)h * 4 + j] * w_rad[j * Hd + h];
      for (int e = 0; e < De; ++e) s += (double)ddir[j * (De + 1) + e] * w_dir[j * De + e];
      s += (double)ddir[j * (De + 1) + De] * p.b_rad[j];
    }
    return s;
  };
  const double Lr0 = Lr();
  expect_adjoint("radiance layer: dWr", Wr, rad.dWr, rng, Lr, Lr0), expect_adjoint("radiance layer: dbr", br, rad.dbr, rng, Lr, Lr0);
  // 3. the images: the head of the forward's, the backward's GEMM operands
  const RenderMlpPack p = pack_render_mlp(f, Wr, br, C, Hd, De);
  expect(p.image.size() == (size_t)Hd * C + Hd + C + 3 * Hd + 3 * De + 3 * C, "forward image: size", p.image.size(), 0);
  const FVec ops = pack_density_gemm_operands(f, C, Hd, Hp);
  expect(ops.size() == (size_t)2 * Hp * C + Hp, "GEMM operands: size", ops.size(), 0);
  for (int i = 0; i < Hp; ++i) {
    const bool real = i < H1;
    for (int j = 0; j < C; ++j) {
      const double w = real ? f.We[(size_t)i * C + j] : 0.0;
      if (i < Hd) expect_same(p.image[(size_t)i * C + j], w, "forward image: w_feat");
      if (i == Hd) expect_same(p.image[(size_t)Hd * C + Hd + j], w, "forward image: w_dens");
      expect_same(ops[(size_t)i * C + j], w, "GEMM operands: WeP");
      expect_same(ops[(size_t)Hp * C + (size_t)j * Hp + i], w, "GEMM operands: WeT");
    }
    if (i < Hd) expect_same(p.image[(size_t)Hd * C + i], f.be[i], "forward image: b_feat");
    expect_same(ops[(size_t)2 * Hp * C + i], real ? f.be[i] : 0.0, "GEMM operands: be");
  }
  expect_same(p.b_dens, f.be[Hd], "forward image: b_dens");
}

static void check_mlp_mean(Rng& rng) {
  // feature maps of 3 and 4 channels (one quad each), 4 harmonic functions: E = 27, D = 34, padded to dp = 48
  MlpMeanShape s;
  s.nh = 128, s.D = 34, s.dp = 48, s.F = 4, s.dout = 5;
  for (int j = 0; j < 3; ++j) s.col.push_back(j);
  for (int j = 0; j < 4; ++j) s.col.push_back(4 + j);
  for (int j = 0; j < 27; ++j) s.col.push_back(8 + j);
  const int nh = s.nh, D = s.D, dp = s.dp, F = s.F, dout = s.dout, FW = (F + 1 + 3) / 4 * 4;
  FVec Ws = rng.vec((size_t)nh * D, 1 / std::sqrt(D)), bs = rng.vec(nh, 0.5), Wm = rng.vec((size_t)nh * D, 1 / std::sqrt(D));
  FVec bm = rng.vec(nh, 0.5), W1 = rng.vec((size_t)nh * nh, 1 / std::sqrt(nh)), b1 = rng.vec(nh, 0.5);
  FVec Wl = rng.vec((size_t)dout * nh, 1 / std::sqrt(nh)), bl = rng.vec(dout, 0.5), M = rng.vec((size_t)F * dout, 0.5);
  FVec mb = rng.vec(F, 0.5);
  auto fold = [&] { return fold_mlp_mean_f64(s, Ws, bs, Wm, bm, W1, b1, Wl, bl, M, mb); };
  const MlpMeanFold64 f = fold();
  // 1. fold == layers, on both sides of the LeakyReLU
  for (int t = 0; t < 32; ++t) {
    const DVec x = bias(rng.vec(D, 1.0)), mean = bias(rng.vec(D, 1.0)), hid = bias(rng.vec(nh, 1.0));
    DVec first = bias(bs), pre = bias(b1), folded(f.cb), last = bias(bl), out = bias(mb), folded_out(f.g0);
    for (int k = 0; k < nh; ++k) first[k] += bm[k];
    matvec(Ws, nh, D, D, 0, x, first);
    matvec(Wm, nh, D, D, 0, mean, first);
    matvec(W1, nh, nh, nh, 0, first, pre);
    for (int i = 0; i < nh; ++i)
      for (int j = 0; j < D; ++j) folded[i] += f.A[(size_t)i * D + j] * x[j] + f.Am[(size_t)i * D + j] * mean[j];
    expect_close(folded, pre, "pooler: A x + Am mean + cb against _first_sampled / _first_mean / _mlp");
    matvec(Wl, dout, nh, nh, 0, hid, last);
    matvec(M, F, dout, dout, 0, last, out);
    for (int i = 0; i < F; ++i)
      for (int k = 0; k < nh; ++k) folded_out[i] += f.G[(size_t)i * nh + k] * hid[k];
    expect_close(folded_out, out, "pooler: G h + g0 against _last / pooled_feature_mapper");
  }
  // 2. un-fold == adjoint.  Random cotangents everywhere, the padding columns and rows included: the un-fold must not read them.
  const FVec ct = rng.vec((size_t)2 * nh * dp + nh + (size_t)FW * nh + FW, 1.0);
  const float *hA = ct.data(), *hAm = hA + (size_t)nh * dp, *hcb = hAm + (size_t)nh * dp, *hG = hcb + nh, *hgl = hG + (size_t)FW * nh;
  const MlpMeanGrads d = unfold_mlp_mean_grads(s, FW, Ws, bs, Wm, bm, W1, Wl, bl, M, ct);
  const auto L = [&] {
    const MlpMeanFold64 q = fold();
    double v = 0;
    for (int i = 0; i < nh; ++i) {
      for (int j = 0; j < D; ++j)
        v += (double)hA[(size_t)i * dp + s.col[j]] * q.A[(size_t)i * D + j] + (double)hAm[(size_t)i * dp + s.col[j]] * q.Am[(size_t)i * D + j];
      v += (double)hcb[i] * q.cb[i];
      v += (double)hG[(size_t)F * nh + i] * Wl[i];  // the tied row 0 of _last: l
    }
    for (int i = 0; i < F; ++i) {
      for (int k = 0; k < nh; ++k) v += (double)hG[(size_t)i * nh + k] * q.G[(size_t)i * nh + k];
      v += (double)hgl[i] * q.g0[i];
    }
    return v + (double)hgl[F] * bl[0];  // l0
  };
  const double L0 = L();
  expect_adjoint("pooler: d _first_sampled.weight", Ws, d.dWs, rng, L, L0), expect_adjoint("pooler: d _first_sampled.bias", bs, d.dbsm, rng, L, L0);
  expect_adjoint("pooler: d _first_mean.weight", Wm, d.dWm, rng, L, L0), expect_adjoint("pooler: d _first_mean.bias", bm, d.dbsm, rng, L, L0);
  expect_adjoint("pooler: d _mlp.mlp.0.0.weight", W1, d.dW1, rng, L, L0), expect_adjoint("pooler: d _mlp.mlp.0.0.bias", b1, d.db1, rng, L, L0);
  expect_adjoint("pooler: d _last.weight", Wl, d.dWl, rng, L, L0), expect_adjoint("pooler: d _last.bias", bl, d.dbl, rng, L, L0);
  expect_adjoint("pooler: d pooled_feature_mapper.weight", M, d.dM, rng, L, L0);
  expect_adjoint("pooler: d pooled_feature_mapper.bias", mb, d.dmb, rng, L, L0);
  // 3. the kernels' image: a | am | cb | g | g0 | l, reference columns at s.col, zero padding
  const MlpMeanFold p = fold_mlp_mean(s, Ws, bs, Wm, bm, W1, b1, Wl, bl, M, mb);
  expect(p.image.size() == s.image_floats(), "pooler image: size", p.image.size(), s.image_floats());
  const float *a = p.image.data(), *am = a + (size_t)nh * dp, *cb = am + (size_t)nh * dp, *g = cb + nh, *g0 = g + (size_t)F * nh, *l = g0 + F;
  for (int i = 0; i < nh; ++i) {
    DVec ra(dp, 0.0), rm(dp, 0.0);
    for (int j = 0; j < D; ++j) ra[s.col[j]] = f.A[(size_t)i * D + j], rm[s.col[j]] = f.Am[(size_t)i * D + j];
    for (int c = 0; c < dp; ++c) expect_same(a[(size_t)i * dp + c], ra[c], "pooler image: a"), expect_same(am[(size_t)i * dp + c], rm[c], "pooler image: am");
    expect_same(cb[i], f.cb[i], "pooler image: cb"), expect_same(l[i], Wl[i], "pooler image: l");
    for (int k = 0; k < F; ++k) expect_same(g[(size_t)k * nh + i], f.G[(size_t)k * nh + i], "pooler image: g");
  }
  for (int k = 0; k < F; ++k) expect_same(g0[k], f.g0[k], "pooler image: g0");
  expect_same(p.l0, bl[0], "pooler image: l0");
}

int main() {
  Rng rng{20240607};
  check_render_mlp(4, 5, 9, rng);      // Hd + 1 = 6, Hp = 8; C, Hd, Hd + C all distinct
  check_render_mlp(16, 256, 27, rng);  // the released width
  check_mlp_mean(rng);
  if (g_failures) return printf("fold_check: %d checks FAILED\n", g_failures), 1;
  printf("fold_check: OK\n");
  return 0;
}
