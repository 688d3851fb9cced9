// unet_plan.h — the denoiser's static launch plan as a value: the network structure and its parameter table, the
// first-fit arena, the ops of a plan, and the Planner that builds the plan of UNetModel.forward for one (description, batch,
// workspace base).  Host-only arithmetic (definitions in unet_plan.cpp): no HIP header, so a plain C++ program builds plans
// and checks them on the CPU (tests/cpu/unet_plan_check.cpp).  The training plan (TrainPlan: that forward with every
// intermediate kept + the backward's launches as BwdOp values) is built on top of Planner by TrainPlanner
// (unet_train_plan.h).  unet_exec.cpp replays both on streams.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/holo_abi.h"
#include "attn_plan.h"
#include "bwd_plan.h"
#include "conv_plan.h"
#include "conv_weights.h"
#include "holo_knobs.h"

namespace holo {
namespace unetplan {  // (short names - W, P, view - that were file-local before: keep them out of holo itself)

// ---------------------------------------------------------------------------------------------
// structure description
// ---------------------------------------------------------------------------------------------
// (B_HEAD, the output head GroupNorm + SiLU + conv, is not a block of the structure: only the training tape records it)
enum BlockKind { B_CONV, B_RES, B_ATTN, B_DOWN, B_UP, B_HEAD };
struct Block {
  BlockKind kind;
  std::string prefix;
  int cin, cout;
};

enum ParamKind { P_PLAIN, P_CONV3, P_CONV1, P_EMB_W, P_EMB_B };

struct ParamSlot {
  std::string name;
  std::vector<int64_t> shape;
  int64_t numel;
  ParamKind kind;
  ConvWeights w;  // private device copies: f32 (repacked for a conv weight) of every parameter, the rest of conv weights only
  bool set;
  bool is_conv() const { return kind == P_CONV3 || kind == P_CONV1; }
  // layout of a conv weight's copies; `transposed`: of the backward's transposed convolution (Cout' = Cin, Cin' = Cout)
  ConvWeightLayout layout(bool transposed = false) const {
    return conv_weight_layout((int)shape[transposed ? 1 : 0], (int)shape[transposed ? 0 : 1], kind == P_CONV3 ? 27 : 1);
  }
};

struct Arena {
  size_t top = 0, peak = 0;
  bool keep = false;
  std::vector<std::pair<size_t, size_t>> fl;  // free list (off, size), sorted by off
  static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
  size_t alloc(size_t bytes) {
    bytes = al(bytes);
    for (size_t i = 0; i < fl.size(); ++i) {
      if (fl[i].second >= bytes) {
        size_t off = fl[i].first;
        if (fl[i].second == bytes)
          fl.erase(fl.begin() + i);
        else {
          fl[i].first += bytes;
          fl[i].second -= bytes;
        }
        return off;
      }
    }
    size_t off = top;
    top += bytes;
    if (top > peak) peak = top;
    return off;
  }
  void free(size_t off, size_t bytes) {
    if (keep) return;
    bytes = al(bytes);
    size_t i = 0;
    while (i < fl.size() && fl[i].first < off) ++i;
    fl.insert(fl.begin() + i, std::make_pair(off, bytes));
    // coalesce
    if (i + 1 < fl.size() && fl[i].first + fl[i].second == fl[i + 1].first) {
      fl[i].second += fl[i + 1].second;
      fl.erase(fl.begin() + i + 1);
    }
    if (i > 0 && fl[i - 1].first + fl[i - 1].second == fl[i].first) {
      fl[i - 1].second += fl[i].second;
      fl.erase(fl.begin() + i);
    }
    if (!fl.empty() && fl.back().first + fl.back().second == top) {
      top = fl.back().first;
      fl.pop_back();
    }
  }
};

struct Act {  // channels-last activation [N][R][R][R][C]
  size_t off = 0, bytes = 0;
  size_t stats_off = 0, stats_bytes = 0;  // GroupNorm partial sums [N][stats_B][C][2] doubles
  int stats_B = 0;
  int C = 0, R = 0;
  int refs = 0;
};

struct Tape {  // one layer of the training forward (what its backward needs); b.kind tells which
  Block b;
  Act x0, x1, h1, out;
  bool has_x1 = false;
  size_t coefA = 0, coefB = 0, momA = 0, momB = 0;
  const float* film = nullptr;
  size_t qkv = 0, a = 0;
  bool has_skip = false;
};

// One launch of the forward.  The numbers are public (HoloOpTiming.op, SimpleUnet3D.OP_NAMES); 0 was a memset and stays reserved.
enum OpKind { OP_IN = 1, OP_TEMB, OP_EMBLIN, OP_STATS, OP_FINAL, OP_CONV, OP_GEMM, OP_SOFTMAX, OP_FLASH, OP_OUT };
// caller's NCDHW x -> the plan's channels-last input buffer, and that of the output -> caller's NCDHW y
struct LayoutIn { float* dst; int C; int64_t V; int dst_bf16; };
struct LayoutOut { const float* src; int C; int64_t V; };
struct TimeEmbed {
  const float *w1, *b1, *w2, *b2;
  float *emb, *emb_silu;
  int load_kind;  // HOLO_DEBUG_TIMESTEP_LOAD of the plan (0 in production)
};
struct EmbLinears {  // every ResBlock's emb_layers as one [emb_rows][ted] product
  const float *emb_silu, *w, *b;
  float* out;
};
struct GnStats {  // GroupNorm partial sums by a pass of their own (where the producing conv cannot write them)
  const float* x;
  double* part;
  int C, x_bf16;
  int64_t V;
};
struct GnFinalize {  // partial sums of the (virtual concat) input -> per-(sample, channel) affine, GroupNorm folded with FiLM
  const double *part0, *part1;  // [N][B0][C0][2], [N][B1][C1][2] (part1 may be null)
  int C0, B0, C1, B1;
  int64_t V;
  const float *gamma, *beta, *film;
  int film_stride, film_cout;
  float *coef, *moments;  // moments: (mean, rstd) kept for the backward in a training plan, else null
  int groups;             // 32, or fewer where one half of a split concat is normalised alone (Planner::plan_side_lane)
  // preactivate_rowtile: the launch also writes act[N][V][C0 + C1] = a*x + b (act_silu: SiLU of it) of the raw sources x0 / x1
  // (channels-last fp32, C0 / C1 channels), which its one consumer reads as raw input.  All null / 0: coefficients only.
  const float *x0, *x1;
  float* act;
  int act_silu;
};
struct Softmax { float* S; int64_t rows; int cols; };  // in place
struct Flash {
  AttnParams attn;
  int form;             // 0: exact-fp32 kernel; 2: packed-operand bf16 kernel
  float* packed;        // form 2: scratch of the packed operands and split partials
  int out_bf16;         // form 2: attn.out is bf16
  int operands_packed;  // form 2: the qkv convolution wrote the packed operands itself
  int ksplit, lazy;     // form 2: key splits (`packed` is sized and laid out for them); the LAZY pass runs before the exact kernel
};
struct Op {  // trivially copyable: holo_unet_forward_cl patches copies of two of them
  OpKind kind;
  union {
    LayoutIn in;
    TimeEmbed temb;
    EmbLinears emblin;
    GnStats stats;
    GnFinalize fin;
    ConvParams conv;
    GemmParams gemm;
    Softmax softmax;
    Flash flash;
    LayoutOut out;
  };
  // The lane of the op (run_lanes): the caller's stream, or the handle's side stream.  `fork`: the side stream starts in front
  // of this op (it waits for everything the caller's stream was given before).  `join`: on a side op, the event recorded
  // behind it; on a main op, the event the caller's stream waits for in front of it (-1: none).
  unsigned char side, fork;
  short join;
};
inline Op make_op(OpKind kind) {
  Op op;
  memset(&op, 0, sizeof op);
  op.kind = kind;
  op.join = -1;
  return op;
}

// A built forward plan.  Planner fills one; nothing else of it lives on the net.
struct Plan {
  int batch = -1;
  void* ws = nullptr;   // workspace base it was built for (null in a sizing pass)
  bool sizing = false;  // a sizing pass: built on no workspace, nothing of it can be launched, only `bytes` is of use
  std::vector<Op> ops;
  size_t bytes = 0;  // workspace it needs
  std::map<std::string, Act> block_outputs;  // holo_unet_fetch_block
  // holo_unet_forward_cl: the convolutions that read the plan's input buffer / write its output buffer, and why the
  // entry cannot use this plan (null: it can)
  int first_conv = -1, last_conv = -1;
  const char* cl_refusal = nullptr;
  int n_joins = 0;  // join events of the side lane (0: every op runs on the caller's stream)
  bool built_for(int b, const void* w) const { return !sizing && batch == b && ws == w && !ops.empty(); }
  void invalidate() { *this = Plan(); }
};

// One launch of the backward (kernels_bwd.hip, and the forward's conv / GEMM / softmax launchers on gradients).  A kind of
// its own: the forward's OpKind numbers are public and stay what they are.  Every accumulate flag (`acc*`, a conv whose
// residual is its out) says that an earlier op of the list wrote the destination and this one adds to it.
enum BwdOpKind {
  BOP_CONV = 1, BOP_WGRAD, BOP_COLSUM, BOP_GN_BWD, BOP_ADD, BOP_SPLIT_CAT, BOP_SUMPOOL2, BOP_ZERO_INSERT2, BOP_DGRAD_S2, BOP_GEMM,
  BOP_SOFTMAX, BOP_ATTN_DS, BOP_TRANSPOSE, BOP_FILM_BWD, BOP_TEMB_BWD
};
struct Wgrad { WgradParams p; WgradPlan plan; float* dw; };                             // dw: OIDHW, overwritten
struct Colsum { const float* g; int64_t M; int C; double* scratch; float* out; };       // bias gradient: column sums of g [M][C]
struct AddGrad { float* dst; const float* src; int64_t n; int acc; };                   // dst (+)= src
struct SplitCat { const float* g; float *g0, *g1; int64_t M; int C0, C1, acc0, acc1; };  // g [M][C0 + C1] -> g0 [M][C0], g1 [M][C1]
struct SumPool2 { const float* gup; float* gin; int N, R, C, acc; };                    // gup (2R)^3 -> gin R^3
struct ZeroInsert2 { const float* gy; float* out; int N, Rs, C; };                      // gy Rs^3 -> out (2 Rs)^3
struct DgradS2 { const float *gy, *wt; float* gx; int N, RI, RO, Ci, Co, acc; };
struct AttnDs { const float* P; float* dP; int64_t rows; int cols; };  // dP in place: dS = P (dP - rowsum(dP P))
struct Transpose { const float* in; float* out; int batch, T; };
struct FilmBwd { const float *dfilm, *embs, *w; float *dw, *db, *gembs; int N, rows, K; };
struct TimeEmbedBwd {  // (the timesteps are an argument of the run, like the forward's)
  int N, mc, ted;
  const float *w1, *b1, *w2, *b2, *gembs;
  float *dw1, *db1, *dw2, *db2;
};
struct BwdOp {  // trivially copyable
  BwdOpKind kind;
  union {
    ConvParams conv;  // dgrad of a stride-1 convolution: the forward's kernels on the transposed weights
    Wgrad wgrad;
    Colsum colsum;
    GnBwdParams gn;
    AddGrad add;
    SplitCat split;
    SumPool2 pool;
    ZeroInsert2 zins;
    DgradS2 s2;
    GemmParams gemm;
    Softmax softmax;
    AttnDs ds;
    Transpose tr;
    FilmBwd film;
    TimeEmbedBwd temb;
  };
};
inline BwdOp make_bwd_op(BwdOpKind kind) {
  BwdOp op;
  memset(&op, 0, sizeof op);
  op.kind = kind;
  return op;
}

// The training plan: the forward with every intermediate kept + the backward launches in execution order.
struct TrainPlan {
  Plan fwd;
  std::vector<BwdOp> bops;
  std::vector<size_t> grad_off;  // per parameter: byte offset of its gradient in the workspace
  size_t gy_off = 0, gx_off = 0;  // gradient of the output (laid out channels-last) / of the input
  size_t bytes = 0;
  bool built_for(int b, const void* w) const { return fwd.built_for(b, w); }
  void invalidate() { *this = TrainPlan(); }
};

// Everything a plan depends on, as plain data: what HoloUnet (unet_exec.cpp) holds by value next to its device stores,
// caches, streams and events.  Planner reads nothing else.
struct UnetDesc {
  HoloUnetCfg cfg;
  std::vector<std::vector<Block>> inputs, outputs;
  std::vector<Block> middle;
  int final_ch = 0;
  int ted = 0;
  std::vector<ParamSlot> params;
  std::map<std::string, int> pindex;
  // holo_unet_set_compute_dtype: 0 exact fp32 MFMA; 1 bf16: activations stored as bf16 in HBM, bf16 products with fp32
  // accumulation in the 3x3x3 convolutions and the long-sequence attention, fp32 GroupNorm statistics; 2 bf16x3 split
  // (fp32 storage, fp32-accurate)
  int compute_mode = 0;
  // holo_unet_set_batch_invariant: the forward plan makes every geometry choice for ONE sample and launches it over the
  // batch, so row b of a batched forward is bit-identical to the batch-1 forward of that row (exact-fp32 mode only)
  bool batch_invariant = false;
  // concatenated emb_layers
  int emb_rows = 0;
  std::map<std::string, int> emb_row_off;  // resblock prefix -> first row
  float* emb_w = nullptr;                  // [emb_rows][ted]
  float* emb_b = nullptr;                  // [emb_rows]
  Knobs knobs;      // snapshot of holo_unet_create (holo_knobs.h): which weight copies exist, whether plans release activations
  int num_cus = 0;  // the context's: what launches are planned for
};

void build_structure(UnetDesc* u);
void enumerate_params(UnetDesc* u);
// Hands every parameter its private copies out of the three stores - f32, bf16 planes, Winograd packs - and returns the
// element count of each.  holo_unet_create runs it twice, like a planner: on null bases to size the stores (the pointers it
// leaves are null), then on the allocations.  All arithmetic is in offsets.
struct StoreSizes {
  int64_t f32 = 0, bf = 0, wino = 0;
};
StoreSizes carve_params(UnetDesc* u, float* f32, uint16_t* bf, float* wino);
// the private copies of parameter `name`: P its fp32 copy, W the whole set of a convolution weight
ConvWeights W(const UnetDesc* u, const std::string& name);
inline bool is_downsample_weight(const std::string& name) {  // Downsample: the stride-2 convolution
  return name.size() > 10 && name.compare(name.size() - 10, 10, ".op.weight") == 0;
}
inline const float* P(const UnetDesc* u, const std::string& name) { return W(u, name).f32; }

// ---------------------------------------------------------------------------------------------
// plan builder
// ---------------------------------------------------------------------------------------------
// One convolution as its call site describes it: only what differs from a plain 3x3x3 stride-1 conv of x0 is set, by name.
struct ConvDesc {
  const Act* x0 = nullptr;
  const Act* x1 = nullptr;  // second source of the virtual channel concat
  int in_R = 0;             // logical input size (AFTER the upsampling when ups); 0: x0's
  int ups = 0;
  int out_R = 0;  // 0: the logical input size
  int stride = 1, ksz = 3;
  ConvWeights w;
  const float* bias = nullptr;
  std::optional<size_t> coef;  // workspace offset of the GroupNorm (+ FiLM) coefficients applied on load
  int act = 0;                 // 1: SiLU after them
  const float* residual = nullptr;
  float* out = nullptr;
  int Cout = 0;
  Act* stats_of = nullptr;  // the output activation, when its GroupNorm statistics are wanted
  struct {                  // 1x1x1 skip connection fused as extra K chunks (w.f32 null: none)
    const Act* x0 = nullptr;
    const Act* x1 = nullptr;
    ConvWeights w;
    const float* bias = nullptr;
  } skip;
  bool in_f32 = false, out_f32 = false;  // bf16 storage mode: this operand stays fp32
  const ConvParams* qkv_pack = nullptr;  // an attention block's qkv convolution: where it may write the packed operands
  // One half of a split concat convolution (Planner::plan_side_lane): the launch sums the input channels [w_cin0, w_cin0 + x0->C)
  // of `w` only.  conv_wino3_kernel's pack is chunk-major, so the half is the same pack entered at its first chunk.
  bool w_slice = false;
  int w_cin0 = 0;
  int cus = 0;  // CUs the launch is planned for (0: the context's)
  int in_size() const { return in_R ? in_R : x0->R; }
  int out_size() const { return out_R ? out_R : in_size(); }
};

// a workspace range seen as an activation (attention internals, gradients)
inline Act view(size_t off, int C, int R) {
  Act a;
  a.off = off;
  a.C = C;
  a.R = R;
  return a;
}

// One operand of the attention GEMMs, batched over (sample, head), and the three layouts they come in
struct AttnMat {
  float* p;
  int ld;
  int64_t s0, s1;  // leading dimension; strides over samples / heads
};
struct AttnDims {
  int N, H, C;
  int64_t T;
  int ch() const { return C / H; }
  float scale2() const {
    const double sc = 1.0 / sqrt(sqrt((double)ch()));
    return (float)(sc * sc);
  }
  AttnMat qkv(float* base, int part) const { return AttnMat{base + part * ch(), 3 * C, T * 3 * C, 3 * ch()}; }  // q, k or v of [N][T][3C]
  AttnMat scores(float* S) const { return AttnMat{S, (int)T, (int64_t)H * T * T, T * T}; }                     // [N][H][T][T]
  AttnMat heads(float* a) const { return AttnMat{a, C, T * C, ch()}; }                                          // [N][T][C]
};
// C = alpha A B^T ([T][T] out of two [T][ch] operands), or with b_kmajor C = alpha A B ([T][ch] out of [T][T] and [T][ch])
GemmParams attn_gemm(const AttnDims& d, AttnMat A, AttnMat B, bool b_kmajor, AttnMat C, float alpha);

struct Planner {
  const UnetDesc* u;  // read only: everything a build produces goes into `plan`
  int N;
  uintptr_t base;  // workspace base as an integer: addresses are formed, never dereferenced, and a sizing pass has none
  const bool sizing;  // no workspace: the plan is built for its size alone (build() hands it to Plan::sizing)
  Plan& plan;
  const Knobs knobs = Knobs::from_env();  // THE snapshot of this build: nothing below or behind it reads the environment
  std::vector<Op>& ops;       // plan.ops
  Arena arena;                // big activations, after the small region
  size_t small_top = 0;       // coef / emb buffers
  size_t small_cap, arena_base;
  std::vector<Tape>* tape = nullptr;  // training forward: every layer is recorded, nothing is released
  size_t last_mom = 0;                // moments buffer of the last emit_finalize (training)
  std::string err;                    // a batch-invariant plan that cannot be kept (ensure_plan reports it)
  size_t eml_off = 0, embs_off = 0;
  Act x_in, y_out;
  struct SideRange {
    size_t off, bytes;
    int join;
  };
  std::vector<SideRange> side_live;  // what the side ops in flight touch (LIFETIMES, unet_plan.cpp)
  struct SidePart {
    Act P;
    int id = 0, join = -1;  // join: the event behind the side launch (-1: it ran on the caller's stream)
    bool consumed = false;
  };
  std::map<std::string, SidePart> side_parts;  // up-path ResBlock prefix -> the skip half of its first convolution

  Planner(const UnetDesc* u_, int N_, void* ws, Plan& plan_);
  void build();
  bool regions_ok() const { return small_top <= small_cap; }

  template <class T>
  T* ptr(size_t off) const {
    return reinterpret_cast<T*>(base + off);
  }
  int64_t vox(int R) const { return (int64_t)R * R * R; }
  bool bfs() const { return u->compute_mode == 1; }  // bf16 storage of the activations
  // the sample count the geometry choices are made for: one in a batch-invariant forward (the training plan keeps its own)
  int plan_n() const { return u->batch_invariant && !tape ? 1 : N; }

  Act new_act(int C, int R, bool f32 = false);
  void alloc_stats(Act& a, int slabs);
  void release(Act& a);
  size_t small_alloc(size_t bytes);
  size_t scratch_alloc(size_t bytes) { return guarded(arena_base + arena.alloc(bytes), bytes); }
  void scratch_free(size_t off, size_t bytes) { arena.free(off - arena_base, bytes); }
  size_t guarded(size_t off, size_t bytes);

  void emit_stats(Act& a);
  size_t emit_finalize(const Act& x0, const Act* x1, const std::string& norm, const float* film = nullptr, int film_cout = 0);
  size_t emit_finalize_half(const Act& x, int c_first, int cpg, const std::string& norm);
  Tape& record(const Block& b, const Act& x0, const Act& out);
  ConvDesc conv_of(const std::string& layer, const Act& x, const Act& out);
  void hand_over(const ConvWeights& cw, ConvParams& p, bool skip, int cin0 = -1);
  size_t plan_conv(const ConvDesc& d, ConvParams& p);
  ConvParams place_conv(const ConvDesc& d, int* stats_slabs = nullptr);  // plan_conv + the launch's scratch and statistics placed
  void emit_conv(const ConvDesc& d);                                     // ... appended to the plan as an op

  // (both lanes on ONE stream cost 12 % of the B = 4 chain rate, DESIGN.md section 8: the parts always take the side stream)
  bool side_stream_used() const { return true; }
  bool split_eligible(const Block& b, const Act& x1, int n_for);
  void plan_side_lane(const std::vector<Act>& hs);

  Act resblock(const Block& b, Act& x0, Act* x1);
  Act attention(const Block& b, Act& x);
  Act run_layers(const std::vector<Block>& layers, Act h, Act* skip, bool release_h);
  void find_cl_ends();
};

// ---------------------------------------------------------------------------------------------
// rewrite pass: deep levels apply GroupNorm (+ SiLU) once per tensor
// ---------------------------------------------------------------------------------------------
// The row-tile convolution applies (a, b) and SiLU while it stages, once per (tap, Cout tile) workgroup: at 4^3 every input
// element of a 512 -> 512 3x3x3 convolution is activated 216 times.  Where that redundancy is high and the tensor small, the
// finalize launch in front - one block per (group, sample), which has just computed the group's (a, b) - writes the
// activated tensor once, and the convolution reads it as raw input (its ACTM = 0 instance).  Same arithmetic, same bits.
struct PreactShape {
  int cpg, C0;     // channels per GroupNorm group; channels of the first source
  int64_t V;       // voxels per sample
  int redundancy;  // taps x 64-channel Cout tiles: how often the convolution would activate an element
};
// Voxels per sample up to which a pair is rewritten, and the redundancy from which (DESIGN.md section 4f'': the shapes
// measured as a pair, finalize + convolution, against the pair they replace)
constexpr int64_t PREACT_MAX_VOX = 64;
constexpr int PREACT_MIN_REDUNDANCY = 16;
// null: the shape is rewritten; else why not
const char* preact_refusal(const PreactShape& s);
struct Preact {
  int pairs = 0;
  size_t scratch_off = 0, scratch_bytes = 0;  // the activated tensor of every pair (they are serial on the caller's stream)
};
// Rewrites a plan Planner::build() made (not a training plan: the tape keeps coefficients and raw inputs).  For every
// main-lane OP_FINAL whose coefficients have exactly one reader, that reader being the next main-lane OP_CONV, on
// ConvKernel::RowTile, exact fp32 on fp32 storage, of a shape preact_refusal admits: the finalize gets the convolution's
// sources and the scratch, the convolution the scratch as its one raw source.  The scratch lies behind the plan's workspace:
// plan.bytes grows by it, in a sizing pass as in a placed one.  knobs.rowtile_preact == 0: nothing is rewritten.
Preact preactivate_rowtile(Plan& plan, const Knobs& knobs);

}  // namespace unetplan
}  // namespace holo
