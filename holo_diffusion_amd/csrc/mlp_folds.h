// mlp_folds.h — the float64 folds of the activation-free stretches of the renderer's and the view pooler's MLPs, and
// their chain rules (the un-folds).  Pure host arithmetic on std::vector: no HIP header, no handle, so that
// tests/cpu/fold_check.cpp can check every un-fold against its fold.  The order of every accumulation is part of the
// results (render_exec.cpp and viewpool_exec.cpp publish them bit for bit): do not reassociate.
#pragma once
#include <stddef.h>

#include <vector>

namespace holo {

typedef std::vector<float> FVec;
typedef std::vector<double> DVec;

// ---- density net of the RenderMLP:  y0=W0 f+b0; y1=W1 y0+b1; y2=W2 [y1;f]+b2; o=W3 y2+b3  (no activation in between:
// custom_modules.py:108-112)  ==  o = We f + be
struct DensityFold {
  DVec A1, c1;  // y1 = A1 f + c1 (Hd x C)
  DVec A2, c2;  // y2 = A2 f + c2 (Hd x C)
  DVec We, be;  // o = We f + be ((Hd+1) x C)
};
inline DensityFold fold_density_net(const FVec& W0, const FVec& b0, const FVec& W1, const FVec& b1, const FVec& W2,
                                    const FVec& b2, const FVec& W3, const FVec& b3, int C, int Hd) {
  DensityFold f;
  // A1 = W1 W0 (Hd x C), c1 = W1 b0 + b1
  f.A1.assign((size_t)Hd * C, 0.0), f.c1.assign(Hd, 0.0);
  for (int i = 0; i < Hd; ++i) {
    double cb = b1[i];
    for (int k = 0; k < Hd; ++k) {
      const double w = W1[(size_t)i * Hd + k];
      cb += w * b0[k];
      for (int j = 0; j < C; ++j) f.A1[(size_t)i * C + j] += w * W0[(size_t)k * C + j];
    }
    f.c1[i] = cb;
  }
  // A2 = W2a A1 + W2b (Hd x C), c2 = W2a c1 + b2 ; W2 = [W2a (Hd x Hd) | W2b (Hd x C)]
  f.A2.assign((size_t)Hd * C, 0.0), f.c2.assign(Hd, 0.0);
  const int L2 = Hd + C;
  for (int i = 0; i < Hd; ++i) {
    double cb = b2[i];
    for (int j = 0; j < C; ++j) f.A2[(size_t)i * C + j] = W2[(size_t)i * L2 + Hd + j];
    for (int k = 0; k < Hd; ++k) {
      const double w = W2[(size_t)i * L2 + k];
      cb += w * f.c1[k];
      for (int j = 0; j < C; ++j) f.A2[(size_t)i * C + j] += w * f.A1[(size_t)k * C + j];
    }
    f.c2[i] = cb;
  }
  // We = W3 A2 ((Hd+1) x C), be = W3 c2 + b3
  f.We.assign((size_t)(Hd + 1) * C, 0.0), f.be.assign(Hd + 1, 0.0);
  for (int i = 0; i < Hd + 1; ++i) {
    double cb = b3[i];
    for (int k = 0; k < Hd; ++k) {
      const double w = W3[(size_t)i * Hd + k];
      cb += w * f.c2[k];
      for (int j = 0; j < C; ++j) f.We[(size_t)i * C + j] += w * f.A2[(size_t)k * C + j];
    }
    f.be[i] = cb;
  }
  return f;
}

// the forward kernels' image of the RenderMLP (MlpParams, holo_kernels.h) and the scalars that travel in the launch parameters
struct RenderMlpPack {
  FVec image;  // w_feat [Hd][C] | b_feat [Hd] | w_dens [C] | w_rad [3][Hd] | w_dir [3][De] | u_rad [3][C]
  float k_rad[3], b_dens, b_rad[3];
};
inline RenderMlpPack pack_render_mlp(const DensityFold& f, const FVec& Wr, const FVec& br, int C, int Hd, int De) {
  RenderMlpPack p;
  FVec& pk = p.image;
  pk.resize((size_t)Hd * C + Hd + C + 3 * Hd + 3 * De + 3 * C);
  size_t o = 0;
  for (int i = 0; i < Hd * C; ++i) pk[o++] = (float)f.We[i];
  for (int i = 0; i < Hd; ++i) pk[o++] = (float)f.be[i];
  for (int j = 0; j < C; ++j) pk[o++] = (float)f.We[(size_t)Hd * C + j];
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < Hd; ++i) pk[o++] = Wr[(size_t)c * (Hd + De) + i];
  for (int c = 0; c < 3; ++c)
    for (int j = 0; j < De; ++j) pk[o++] = Wr[(size_t)c * (Hd + De) + Hd + j];
  // LeakyReLU_0.2(h) = 0.6 h + 0.4 |h|: fold the linear part of sum_rows w_rad[c][row] * leaky(h[row]) into
  // u_rad[c] = 0.6 * W_eff[:Hd]^T w_rad[c] (a C-vector) and k_rad[c] = 0.6 * w_rad[c] . b_eff[:Hd]
  for (int c = 0; c < 3; ++c) {
    double kc = 0.0;
    DVec uc(C, 0.0);
    for (int i = 0; i < Hd; ++i) {
      const double w = Wr[(size_t)c * (Hd + De) + i];
      kc += w * f.be[i];
      for (int j = 0; j < C; ++j) uc[j] += w * f.We[(size_t)i * C + j];
    }
    for (int j = 0; j < C; ++j) pk[o++] = (float)(0.6 * uc[j]);
    p.k_rad[c] = (float)(0.6 * kc);
  }
  p.b_dens = (float)f.be[Hd];
  for (int c = 0; c < 3; ++c) p.b_rad[c] = br[c];
  return p;
}
// the backward's GEMM operands: WeP [Hp][C] | WeT [C][Hp] | be [Hp]  (rows Hd+1 .. Hp-1 zero)
inline FVec pack_density_gemm_operands(const DensityFold& f, int C, int Hd, int Hp) {
  FVec pk((size_t)2 * Hp * C + Hp, 0.f);
  for (int i = 0; i <= Hd; ++i)
    for (int j = 0; j < C; ++j) {
      pk[(size_t)i * C + j] = (float)f.We[(size_t)i * C + j];
      pk[(size_t)Hp * C + (size_t)j * Hp + i] = (float)f.We[(size_t)i * C + j];
    }
  for (int i = 0; i <= Hd; ++i) pk[(size_t)2 * Hp * C + i] = (float)f.be[i];
  return pk;
}

// (dWe [>= Hd+1][C], dbe [>= Hd+1]) -> the gradients of the four Linear layers
struct DensityGrads {
  FVec dW0, db0, dW1, db1, dW2, db2, dW3, db3;
};
inline DensityGrads unfold_density_grads(const DensityFold& f, const FVec& W0, const FVec& b0, const FVec& W1, const FVec& W2,
                                         const FVec& W3, const FVec& dWe, const FVec& dbe, int C, int Hd) {
  const int H1 = Hd + 1, L2 = Hd + C;
  DensityGrads o;
  DVec G((size_t)H1 * C), gv(H1);
  for (int i = 0; i < H1; ++i) {
    gv[i] = dbe[i];
    for (int j = 0; j < C; ++j) G[(size_t)i * C + j] = dWe[(size_t)i * C + j];
  }
  // layer 3: y3 = A2 f + c2
  o.dW3.assign((size_t)H1 * Hd, 0.f), o.db3.assign(H1, 0.f);
  for (int i = 0; i < H1; ++i) {
    o.db3[i] = (float)gv[i];
    for (int k = 0; k < Hd; ++k) {
      double s = gv[i] * f.c2[k];
      for (int j = 0; j < C; ++j) s += G[(size_t)i * C + j] * f.A2[(size_t)k * C + j];
      o.dW3[(size_t)i * Hd + k] = (float)s;
    }
  }
  DVec G3((size_t)Hd * C, 0.0), g3(Hd, 0.0);  // W3^T G, W3^T g
  for (int i = 0; i < H1; ++i)
    for (int k = 0; k < Hd; ++k) {
      const double w = W3[(size_t)i * Hd + k];
      g3[k] += w * gv[i];
      for (int j = 0; j < C; ++j) G3[(size_t)k * C + j] += w * G[(size_t)i * C + j];
    }
  // layer 2: input [y2 = A1 f + c1 ; f]
  o.dW2.assign((size_t)Hd * L2, 0.f), o.db2.assign(Hd, 0.f);
  for (int i = 0; i < Hd; ++i) {
    o.db2[i] = (float)g3[i];
    for (int k = 0; k < Hd; ++k) {
      double s = g3[i] * f.c1[k];
      for (int j = 0; j < C; ++j) s += G3[(size_t)i * C + j] * f.A1[(size_t)k * C + j];
      o.dW2[(size_t)i * L2 + k] = (float)s;
    }
    for (int j = 0; j < C; ++j) o.dW2[(size_t)i * L2 + Hd + j] = (float)G3[(size_t)i * C + j];
  }
  DVec G2((size_t)Hd * C, 0.0), g2(Hd, 0.0);  // W2a^T G3, W2a^T g3
  for (int i = 0; i < Hd; ++i)
    for (int k = 0; k < Hd; ++k) {
      const double w = W2[(size_t)i * L2 + k];
      g2[k] += w * g3[i];
      for (int j = 0; j < C; ++j) G2[(size_t)k * C + j] += w * G3[(size_t)i * C + j];
    }
  // layer 1: input y1 = W0 f + b0
  o.dW1.assign((size_t)Hd * Hd, 0.f), o.db1.assign(Hd, 0.f);
  for (int i = 0; i < Hd; ++i) {
    o.db1[i] = (float)g2[i];
    for (int k = 0; k < Hd; ++k) {
      double s = g2[i] * b0[k];
      for (int j = 0; j < C; ++j) s += G2[(size_t)i * C + j] * W0[(size_t)k * C + j];
      o.dW1[(size_t)i * Hd + k] = (float)s;
    }
  }
  // layer 0
  o.dW0.assign((size_t)Hd * C, 0.f), o.db0.assign(Hd, 0.f);
  DVec G1((size_t)Hd * C, 0.0), g1(Hd, 0.0);
  for (int i = 0; i < Hd; ++i)
    for (int k = 0; k < Hd; ++k) {
      const double w = W1[(size_t)i * Hd + k];
      g1[k] += w * g2[i];
      for (int j = 0; j < C; ++j) G1[(size_t)k * C + j] += w * G2[(size_t)i * C + j];
    }
  for (int k = 0; k < Hd; ++k) {
    o.db0[k] = (float)g1[k];
    for (int j = 0; j < C; ++j) o.dW0[(size_t)k * C + j] = (float)G1[(size_t)k * C + j];
  }
  return o;
}

// radiance layer [hidden | direction embedding]: dWrh [Hd][4] (column j = colour j) and ddir [3][De + 1] (the embedding's
// columns, then the bias) -> dWr [3][Hd + De], dbr [3]
struct RadianceGrads {
  FVec dWr, dbr;
};
inline RadianceGrads unfold_radiance_grads(const FVec& dWrh, const FVec& ddir, int Hd, int De) {
  RadianceGrads o;
  o.dWr.assign((size_t)3 * (Hd + De), 0.f), o.dbr.assign(3, 0.f);
  for (int j = 0; j < 3; ++j) {
    for (int h = 0; h < Hd; ++h) o.dWr[(size_t)j * (Hd + De) + h] = dWrh[(size_t)h * 4 + j];
    for (int e = 0; e < De; ++e) o.dWr[(size_t)j * (Hd + De) + Hd + e] = ddir[j * (De + 1) + e];
    o.dbr[j] = ddir[j * (De + 1) + De];
  }
  return o;
}

// ---- MLPMeanFeatureAggregator (custom_modules.py:162-334):  A = W1 Ws, Am = W1 Wm, cb = W1 (bs + bm) + b1 in front of the
// LeakyReLU;  G = M Wl, g0 = M bl + mb behind it;  l / l0 = row 0 of _last (the weight logit), passed through
struct MlpMeanShape {
  int nh = 0, D = 0, dp = 0, F = 0, dout = 0;
  std::vector<int> col;  // column of reference channel c (torch.cat order: maps in dict order, then the embedding) of the dp padded ones
  size_t image_floats() const { return (size_t)2 * nh * dp + nh + (size_t)F * nh + F + nh; }
};
struct MlpMeanFold64 {  // in the reference's column order
  DVec A, Am, cb, G, g0;
};
inline MlpMeanFold64 fold_mlp_mean_f64(const MlpMeanShape& s, const FVec& Ws, const FVec& bs, const FVec& Wm, const FVec& bm,
                                       const FVec& W1, const FVec& b1, const FVec& Wl, const FVec& bl, const FVec& M,
                                       const FVec& mb) {
  const int nh = s.nh, D = s.D;
  MlpMeanFold64 f;
  f.A.assign((size_t)nh * D, 0.0), f.Am.assign((size_t)nh * D, 0.0), f.cb.assign(nh, 0.0);
  for (int i = 0; i < nh; ++i) {
    double* ra = &f.A[(size_t)i * D];
    double* rm = &f.Am[(size_t)i * D];
    double c = b1[i];
    for (int k = 0; k < nh; ++k) {
      const double w = W1[(size_t)i * nh + k];
      c += w * ((double)bs[k] + (double)bm[k]);
      for (int j = 0; j < D; ++j) {
        ra[j] += w * Ws[(size_t)k * D + j];
        rm[j] += w * Wm[(size_t)k * D + j];
      }
    }
    f.cb[i] = c;
  }
  f.G.assign((size_t)s.F * nh, 0.0), f.g0.assign(s.F, 0.0);
  for (int fo = 0; fo < s.F; ++fo) {
    double c = mb[fo];
    double* rg = &f.G[(size_t)fo * nh];
    for (int o = 0; o < s.dout; ++o) {
      const double w = M[(size_t)fo * s.dout + o];
      c += w * bl[o];
      for (int k = 0; k < nh; ++k) rg[k] += w * Wl[(size_t)o * nh + k];
    }
    f.g0[fo] = c;
  }
  return f;
}
// the kernels' image:  a [nh][dp] | am [nh][dp] | cb [nh] | g [F][nh] | g0 [F] | l [nh]  (padding columns zero), and l0
struct MlpMeanFold {
  FVec image;
  float l0;
};
inline MlpMeanFold fold_mlp_mean(const MlpMeanShape& s, const FVec& Ws, const FVec& bs, const FVec& Wm, const FVec& bm,
                                 const FVec& W1, const FVec& b1, const FVec& Wl, const FVec& bl, const FVec& M, const FVec& mb) {
  const MlpMeanFold64 f = fold_mlp_mean_f64(s, Ws, bs, Wm, bm, W1, b1, Wl, bl, M, mb);
  const int nh = s.nh, D = s.D, dp = s.dp, F = s.F;
  MlpMeanFold out;
  out.image.assign(s.image_floats(), 0.f);
  float* a = out.image.data();
  float* am = a + (size_t)nh * dp;
  float* cb = am + (size_t)nh * dp;
  float* g = cb + nh;
  float* g0 = g + (size_t)F * nh;
  float* l = g0 + F;
  for (int i = 0; i < nh; ++i) {
    for (int j = 0; j < D; ++j) {
      a[(size_t)i * dp + s.col[j]] = (float)f.A[(size_t)i * D + j];
      am[(size_t)i * dp + s.col[j]] = (float)f.Am[(size_t)i * D + j];
    }
    cb[i] = (float)f.cb[i];
    l[i] = Wl[i];  // row 0 of _last
  }
  for (size_t i = 0; i < f.G.size(); ++i) g[i] = (float)f.G[i];
  for (int fo = 0; fo < F; ++fo) g0[fo] = (float)f.g0[fo];
  out.l0 = bl[0];
  return out;
}

// folded gradients  dA [nh][dp] | dAm [nh][dp] | dcb [nh] | dGext [FW][nh] (rows 0..F-1: dG, row F: dl) | dg0 [F], dl0
// (FW = F + 1 rounded up to 4) -> the gradients of the reference parameters; _first_sampled.bias and _first_mean.bias enter
// the fold as their sum and share dbsm
struct MlpMeanGrads {
  FVec dWs, dWm, dbsm, dW1, db1, dWl, dbl, dM, dmb;
};
inline MlpMeanGrads unfold_mlp_mean_grads(const MlpMeanShape& s, int FW, const FVec& Ws, const FVec& bs, const FVec& Wm,
                                          const FVec& bm, const FVec& W1, const FVec& Wl, const FVec& bl, const FVec& M,
                                          const FVec& folded) {
  const int nh = s.nh, D = s.D, dp = s.dp, F = s.F, dout = s.dout;
  const std::vector<int>& col = s.col;
  const float *hA = folded.data(), *hAm = hA + (size_t)nh * dp, *hcb = hAm + (size_t)nh * dp, *hG = hcb + nh,
              *hgl = hG + (size_t)FW * nh;
  DVec gW1((size_t)nh * nh, 0.0), gWs((size_t)nh * D, 0.0), gWm((size_t)nh * D, 0.0), gbsm(nh, 0.0), gb1(nh, 0.0);
  for (int i = 0; i < nh; ++i) {  // A = W1 Ws, Am = W1 Wm, b' = W1 (bs + bm) + b1
    gb1[i] = hcb[i];
    for (int k = 0; k < nh; ++k) {
      double acc = (double)hcb[i] * ((double)bs[k] + (double)bm[k]);
      const double w = W1[(size_t)i * nh + k];
      for (int j = 0; j < D; ++j) {
        const double da = hA[(size_t)i * dp + col[j]], dam = hAm[(size_t)i * dp + col[j]];
        acc += da * Ws[(size_t)k * D + j] + dam * Wm[(size_t)k * D + j];
        gWs[(size_t)k * D + j] += w * da;
        gWm[(size_t)k * D + j] += w * dam;
      }
      gW1[(size_t)i * nh + k] = acc;
      gbsm[k] += w * hcb[i];
    }
  }
  DVec gM((size_t)F * dout, 0.0), gWl((size_t)dout * nh, 0.0), gbl(dout, 0.0), gmb(F, 0.0);
  for (int f = 0; f < F; ++f) {  // G = M Wl, g0 = M bl + mapper bias
    gmb[f] = hgl[f];
    for (int o = 0; o < dout; ++o) {
      double acc = (double)hgl[f] * bl[o];
      const double w = M[(size_t)f * dout + o];
      for (int k = 0; k < nh; ++k) {
        const double dg = hG[(size_t)f * nh + k];
        acc += dg * Wl[(size_t)o * nh + k];
        gWl[(size_t)o * nh + k] += w * dg;
      }
      gM[(size_t)f * dout + o] = acc;
      gbl[o] += w * hgl[f];
    }
  }
  for (int k = 0; k < nh; ++k) gWl[k] += hG[(size_t)F * nh + k];  // l = Wl[0]
  gbl[0] += hgl[F];                                               // l0 = bl[0]
  auto f32 = [](const DVec& v) { return FVec(v.begin(), v.end()); };
  return {f32(gWs), f32(gWm), f32(gbsm), f32(gW1), f32(gb1), f32(gWl), f32(gbl), f32(gM), f32(gmb)};
}

}  // namespace holo
