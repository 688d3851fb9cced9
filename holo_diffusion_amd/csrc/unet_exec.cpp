// unet_exec.cpp — native runtime of the denoiser: builds the static launch plan of
// UNetModel.forward (holo_diffusion/guided_diffusion/unet.py:800-837, block construction :645-798 as
// configured by SimpleUnet3D, holo_diffusion/utils/diffusion_utils.py:56-75) and replays it on a stream.
//
// Everything is static for a given (config, batch): tensor shapes, workspace offsets, split-K factors,
// kernel parameters.  The plan is a flat vector of ops; forward() only patches the three caller pointers
// (x, timesteps, y) and launches.  No allocation, no host synchronisation inside forward().
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <map>
#include <optional>
#include <string>
#include <vector>

#include "../../include/holo_abi.h"
#include "conv_weights.h"
#include "holo_common.h"
#include "holo_kernels.h"

namespace holo {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

}  // namespace holo

using namespace holo;

int holo::pack_conv_weights(const float* src, const ConvWeights& dst, void* stream) {
  const ConvWeightLayout& l = dst.layout;
  int rc = repack_conv_weight_launch(src, dst.f32, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  if (!rc && dst.bf) rc = repack_conv_weight_bf16_launch(src, dst.bf, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  if (!rc && dst.wino2) rc = repack_conv_weight_wino2_launch(src, dst.wino2, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  if (!rc && dst.wino3) rc = repack_conv_weight_wino3_launch(src, dst.wino3, l.Cout, l.Cin, l.taps, l.CoutP, l.CinP, stream);
  return rc;
}

// struct HoloCtx { device, num_cus }: holo_kernels.h (shared with render_exec.cpp)

// ---------------------------------------------------------------------------------------------
// structure description
// ---------------------------------------------------------------------------------------------
namespace {

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
static bool is_downsample_weight(const std::string& name) {  // Downsample: the stride-2 convolution
  return name.size() > 10 && name.compare(name.size() - 10, 10, ".op.weight") == 0;
}

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
static Op make_op(OpKind kind) {
  Op op;
  memset(&op, 0, sizeof op);
  op.kind = kind;
  op.join = -1;
  return op;
}

// A built forward plan.  Planner fills one; nothing else of it lives on the net.
struct Plan {
  int batch = -1;
  void* ws = nullptr;  // workspace base it was built for (null: a sizing pass)
  std::vector<Op> ops;
  size_t bytes = 0;  // workspace it needs
  std::map<std::string, Act> block_outputs;  // holo_unet_fetch_block
  // holo_unet_forward_cl: the convolutions that read the plan's input buffer / write its output buffer, and why the
  // entry cannot use this plan (null: it can)
  int first_conv = -1, last_conv = -1;
  const char* cl_refusal = nullptr;
  int n_joins = 0;  // join events of the side lane (0: every op runs on the caller's stream)
  bool built_for(int b, const void* w) const { return batch == b && ws == w && !ops.empty(); }
  void invalidate() { *this = Plan(); }
};
// The training plan: the forward with every intermediate kept + the backward launches in execution order.
struct TrainPlan {
  Plan fwd;
  std::vector<std::function<int(void*)>> bops;
  std::vector<size_t> grad_off;  // per parameter: byte offset of its gradient in the workspace
  size_t gy_off = 0, gx_off = 0;  // gradient of the output (laid out channels-last) / of the input
  size_t bytes = 0;
  bool built_for(int b, const void* w) const { return fwd.built_for(b, w); }
  void invalidate() { *this = TrainPlan(); }
};

}  // namespace

struct HoloUnet {
  HoloCtx* ctx;
  HoloUnetCfg cfg;
  std::vector<std::vector<Block>> inputs, outputs;
  std::vector<Block> middle;
  int final_ch;
  int ted;
  std::vector<ParamSlot> params;
  std::map<std::string, int> pindex;
  float* pstore = nullptr;       // one allocation for all private parameter copies
  uint16_t* pstore_bf = nullptr;  // bf16 copies of the conv weights
  float* pstore_wino = nullptr;  // Winograd copies of the conv weights
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
  Knobs knobs;  // snapshot of holo_unet_create (holo_knobs.h): which weight copies exist, whether plans release activations
  Plan plan;                                        // inference (holo_unet_forward, _forward_cl, _fetch_block, _time_*)
  std::map<std::pair<int, bool>, size_t> ws_cache;  // (batch, batch_invariant) -> workspace bytes
  // ---- training (holo_unet_backward): weights of the transposed convolutions, packed like the forward ones
  // ([Cin][Cout] flipped taps for the stride-1 convs; [tap][Cout][Cin] for the stride-2 Downsample convs, whose stride-1
  // form lives under "<name>#s1"), supplied by holo_unet_set_dgrad_weight; this table owns every buffer it points to
  std::map<std::string, ConvWeights> dgrad;
  std::vector<float*> adam_copies;  // holo_unet_adam_step: per parameter, its plain private copy (null for a conv weight)
  float* dgrad_tmp = nullptr;  // the flipped / transposed OIDHW weight on its way into the packs: the largest conv weight's numel
  TrainPlan tplan;
  const int64_t* t_dev = nullptr;  // timesteps of the running call (time_embed backward)
  bool tape_valid = false;         // holo_unet_forward_train ran and nothing has consumed its tape
  std::map<int, size_t> tws_cache;
  // ---- the side lane of an inference plan (Planner::plan_side_lane, run_lanes): one non-blocking stream, the fork event, one
  // join event per consumer and the event of the error path; created by the first forward whose plan has a side lane
  void* side_stream = nullptr;
  void *fork_event = nullptr, *tail_event = nullptr;
  std::vector<void*> join_events;
};

namespace {

void build_structure(HoloUnet* u) {
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

void add_param(HoloUnet* u, const std::string& name, std::vector<int64_t> shape, ParamKind kind) {
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

void enumerate_params(HoloUnet* u) {
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

// Hands every parameter its private copies out of the three stores - f32 (HoloUnet::pstore), bf16 planes (pstore_bf),
// Winograd packs (pstore_wino) - and returns the element count of each.  holo_unet_create runs it twice, like a planner: on
// null bases to size the stores (the pointers it leaves are null), then on the allocations.  All arithmetic is in offsets.
struct StoreSizes {
  int64_t f32 = 0, bf = 0, wino = 0;
};
StoreSizes carve_params(HoloUnet* u, float* f32, uint16_t* bf, float* wino) {
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

// the private copies of parameter `name`: P its fp32 copy, W the whole set of a convolution weight
ConvWeights W(const HoloUnet* u, const std::string& name) {
  auto it = u->pindex.find(name);
  return it == u->pindex.end() ? ConvWeights() : u->params[it->second].w;
}
const float* P(const HoloUnet* u, const std::string& name) { return W(u, name).f32; }

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
static Act view(size_t off, int C, int R) {
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
static GemmParams attn_gemm(const AttnDims& d, AttnMat A, AttnMat B, bool b_kmajor, AttnMat C, float alpha) {
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

struct Planner {
  const HoloUnet* u;  // read only: everything a build produces goes into `plan`
  int N;
  char* base;  // workspace base (may be null for a sizing pass)
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

  Planner(const HoloUnet* u_, int N_, void* ws, Plan& plan_) : u(u_), N(N_), base((char*)ws), plan(plan_), ops(plan_.ops) {
    // a generous fixed region for the small buffers
    small_cap = Arena::al((size_t)N * 8 * 1024 * 256 * 2 + (size_t)N * (u->emb_rows + 4 * u->ted) * 4 * 2 + 65536);
    arena_base = small_cap;
    arena.keep = u->knobs.keep_intermediates;
  }
  template <class T>
  T* ptr(size_t off) {
    return reinterpret_cast<T*>(base + off);
  }
  int64_t vox(int R) const { return (int64_t)R * R * R; }
  bool bfs() const { return u->compute_mode == 1; }  // bf16 storage of the activations
  // the sample count the geometry choices are made for: one in a batch-invariant forward (the training plan keeps its own)
  int plan_n() const { return u->batch_invariant && !tape ? 1 : N; }

  Act new_act(int C, int R, bool f32 = false) {
    Act a;
    a.C = C;
    a.R = R;
    a.bytes = (size_t)N * vox(R) * C * ((bfs() && !f32) ? 2 : sizeof(float));
    a.off = guarded(arena_base + arena.alloc(a.bytes), a.bytes);
    return a;
  }
  // GroupNorm partial-sum buffer [N][slabs][C][2] doubles; the slab count depends on the producing kernel
  void alloc_stats(Act& a, int slabs) {
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
  void release(Act& a) {
    arena.free(a.off - arena_base, a.bytes);
    if (a.stats_bytes) arena.free(a.stats_off - arena_base, a.stats_bytes);
  }
  size_t small_alloc(size_t bytes) {
    size_t off = small_top;
    small_top += Arena::al(bytes);
    return off;
  }
  size_t scratch_alloc(size_t bytes) { return guarded(arena_base + arena.alloc(bytes), bytes); }
  struct SideRange {
    size_t off, bytes;
    int join;
  };
  std::vector<SideRange> side_live;
  size_t guarded(size_t off, size_t bytes) {
    for (const SideRange& r : side_live)
      if (off < r.off + r.bytes && r.off < off + bytes && err.empty())
        err = "internal: an allocation between the side lane's fork and join " + std::to_string(r.join) + " overlaps a buffer of that side op";
    return off;
  }
  void scratch_free(size_t off, size_t bytes) { arena.free(off - arena_base, bytes); }

  void emit_stats(Act& a) {
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
  size_t emit_finalize(const Act& x0, const Act* x1, const std::string& norm, const float* film = nullptr, int film_cout = 0) {
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
  size_t emit_finalize_half(const Act& x, int c_first, int cpg, const std::string& norm) {
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
  Tape& record(const Block& b, const Act& x0, const Act& out) {  // training: a layer onto the tape
    tape->emplace_back();
    Tape& t = tape->back();
    t.b = b;
    t.x0 = x0;
    t.out = out;
    return t;
  }
  // the convolution `layer` (its .weight / .bias) of x into the activation `out`
  ConvDesc conv_of(const std::string& layer, const Act& x, const Act& out) {
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
  void hand_over(const ConvWeights& cw, ConvParams& p, bool skip, int cin0 = -1) {
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
  size_t plan_conv(const ConvDesc& d, ConvParams& p) {
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
    const int cus = d.cus > 0 ? d.cus : u->ctx->num_cus;
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
  void emit_conv(const ConvDesc& d) {
    Op op = make_op(OP_CONV);
    ConvParams& p = op.conv;
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
  struct SidePart {
    Act P;
    int id = 0, join = -1;  // join: the event behind the side launch (-1: it ran on the caller's stream)
    bool consumed = false;
  };
  std::map<std::string, SidePart> side_parts;  // up-path ResBlock prefix -> the skip half of its first convolution
  // (both lanes on ONE stream cost 12 % of the B = 4 chain rate, DESIGN.md section 8: the parts always take the side stream)
  bool side_stream_used() const { return true; }
  bool split_eligible(const Block& b, const Act& x1, int n_for) {
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
  void plan_side_lane(const std::vector<Act>& hs) {
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

  Act resblock(const Block& b, Act& x0, Act* x1) {
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

  Act attention(const Block& b, Act& x) {
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
        fl.ksplit = flash_attn_bf16v2_ksplit(fl.attn, u->ctx->num_cus, knobs);
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
        fl.attn.nsplit = flash_attn_splits(plan_n(), (int)T, H, u->ctx->num_cus, knobs);
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
  Act run_layers(const std::vector<Block>& layers, Act h, Act* skip, bool release_h) {
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

  void build() {
    const HoloUnetCfg& c = u->cfg;
    const int R = c.image_size;
    plan.invalidate();
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
    plan.ws = base;
    plan.bytes = arena_base + arena.peak;
  }
  // holo_unet_forward_cl points every convolution that reads the plan's input buffer or writes its output buffer at the
  // caller's channels-last tensors instead (by POSITION in the op list, not by address: the arena hands the input
  // buffer's memory to later activations).  Which two those are, and whether they can, is a property of the plan.
  void find_cl_ends() {
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
  bool regions_ok() const { return small_top <= small_cap; }
};

// ---------------------------------------------------------------------------------------------
// training plan (second half): the forward with every intermediate kept and every layer recorded,
// then the backward as a list of launches in reverse layer order.  fp32 mode only.
//   * dgrad of a stride-1 convolution = the forward conv kernels on the flipped / transposed weights
//     (holo_unet_set_dgrad_weight);  Downsample: conv_dgrad_s2_kernel;  Upsample: dgrad at the fine size + sumpool2
//   * wgrad: conv_wgrad_kernel re-applies GroupNorm . FiLM . SiLU to the raw input like the forward's staging does
//   * GroupNorm (+ FiLM + SiLU): gn_bwd_launch;  attention: batched fp32 MFMA GEMMs around the softmax rows
// Gradients of activations are allocated on first use and ACCUMULATED by later consumers (skip connections, the
// identity branches of ResBlock / AttentionBlock).  Parameter gradients live in the workspace in the reference's layouts.
// ---------------------------------------------------------------------------------------------
struct TrainPlanner {
  const HoloUnet* u;  // read only: everything a build produces goes into `tp`
  int N;
  TrainPlan& tp;
  Planner pl;
  std::vector<Tape> tape;
  std::vector<std::function<int(void*)>>& bops;      // tp.bops
  std::map<size_t, std::pair<size_t, bool>> grads;  // activation offset -> (gradient offset, already written)
  std::string err;

  TrainPlanner(const HoloUnet* u_, int N_, void* ws, TrainPlan& tp_) : u(u_), N(N_), tp(tp_), pl(u_, N_, ws, tp_.fwd), bops(tp_.bops) {
    pl.arena.keep = true;
    pl.tape = &tape;
  }
  template <class T>
  T* ptr(size_t off) {
    return pl.ptr<T>(off);
  }
  size_t alloc(size_t bytes) { return pl.scratch_alloc(bytes); }
  int64_t vox(int R) const { return (int64_t)R * R * R; }
  // gradient buffer of an activation; `acc` tells the caller whether to accumulate (a consumer wrote it before)
  // (all bookkeeping is in workspace OFFSETS: the sizing pass runs with a null base, and pointer differences against a
  // null base are undefined behaviour that an optimising compiler does exploit)
  static constexpr size_t NONE = ~(size_t)0;
  size_t grad_of(const Act& a, int* acc) {
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
  size_t grad_ready(const Act& a) {  // gradient of a layer OUTPUT: must have been written by its consumers
    auto it = grads.find(a.off);
    if (it == grads.end()) {
      err = "internal: a layer output has no gradient";
      return NONE;
    }
    return it->second.first;
  }
  float* pgrad(const std::string& name) {
    auto it = u->pindex.find(name);
    return it == u->pindex.end() ? nullptr : reinterpret_cast<float*>(pl.base + tp.grad_off[it->second]);
  }
  // The transposed weights under `name`, or null.  A sizing pass (no workspace base) launches nothing and must not fail
  // on weights that were not supplied yet, so there every convolution weight counts as present, and so does the stride-1
  // form "<name>#s1" of a Downsample weight whose two leading dims are multiples of 4 (the one holo_unet_set_dgrad_weight
  // creates); they count as plain fp32 copies, without Winograd forms.
  std::optional<ConvWeights> find_dgw(const std::string& name) {
    auto it = u->dgrad.find(name);
    if (it != u->dgrad.end()) return it->second;
    if (pl.base) return std::nullopt;
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
  std::optional<ConvWeights> dgw(const std::string& name) {
    const std::optional<ConvWeights> w = find_dgw(name);
    if (!w) err = "holo_unet_backward: call holo_unet_set_dgrad_weight for '" + name + "' first";
    return w;
  }

  // dgrad of a stride-1 conv (3x3x3 pad 1 or 1x1x1): out[M][cin] = conv(gy[M][cout], flipped weights)
  void emit_dgrad(size_t gy_off, int cout, int R, const std::string& wname, int cin, int ksz, size_t out_off,
                  bool accumulate = false) {
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
    pl.emit_conv(d);
    const ConvParams cp = pl.ops.back().conv;
    pl.ops.pop_back();
    bops.push_back([cp](void* st) { return conv_launch(cp, st); });
  }
  // wgrad of the forward convolution `f` (sources, geometry, coefficients on load, Cout) into the gradients of
  // `layer`.weight / .bias
  void emit_wgrad(size_t gy_off, const ConvDesc& f, const std::string& layer) {
    const float* gy = ptr<float>(gy_off);
    const int cout = f.Cout;
    WgradParams w;
    memset(&w, 0, sizeof w);
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
    const WgradPlan wg = wgrad_plan(w, u->ctx->num_cus, pl.knobs);
    w.partial = ptr<float>(alloc(wgrad_partial_bytes(w, wg)));
    float* dw = pgrad(layer + ".weight");
    float* db = pgrad(layer + ".bias");
    double* cs = ptr<double>(alloc(colsum_scratch_bytes(cout)));
    const int64_t M = (int64_t)N * vox(f.out_size());
    bops.push_back([w, wg, dw](void* st) { return conv_wgrad_launch(w, wg, dw, 0, st); });
    bops.push_back([gy, M, cout, cs, db](void* st) { return colsum_launch(gy, M, cout, cs, db, 0, st); });
  }
  // the forward convolution of `cout` channels out of [x0 | x1], as emit_wgrad wants it
  static ConvDesc fwd_conv(const Act& x0, const Act* x1, int cout) {
    ConvDesc f;
    f.x0 = &x0;
    f.x1 = x1;
    f.Cout = cout;
    return f;
  }
  struct FilmGrad {  // a FiLM-modulated GroupNorm: the rows it was modulated with, and where their gradient goes
    const float* film;
    int cout;
    float* dfilm;
  };
  // Backward of the stride-1 convolution `layer` = f(act(norm([x0 | x1]))) from the gradient of its output at gy_off:
  // dgrad into a scratch ga [M][Cin], wgrad, then GroupNorm `norm` (+FiLM) (+SiLU) backward: ga -> gradients of x0 / x1
  void bwd_norm_conv(size_t gy_off, const ConvDesc& f, const std::string& layer, const std::string& norm, size_t mom,
                     const FilmGrad* film = nullptr) {
    const Act &x0 = *f.x0, *x1 = f.x1;
    const int Cin = x0.C + (x1 ? x1->C : 0);
    const size_t ga = alloc((size_t)N * vox(x0.R) * Cin * sizeof(float));
    emit_dgrad(gy_off, f.Cout, x0.R, layer + ".weight", Cin, f.ksz, ga);
    emit_wgrad(gy_off, f, layer);
    GnBwdParams g;
    memset(&g, 0, sizeof g);
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
    bops.push_back([g](void* st) { return gn_bwd_launch(g, st); });
  }

  void bwd_res(const Tape& t, float* dfilm_base) {
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
      const int64_t n = M * cin;
      bops.push_back([gx0, goutp, n, a0](void* st) { return add_launch(gx0, goutp, n, a0, st); });
    } else {
      const size_t gso = alloc((size_t)M * cin * sizeof(float));
      const float* gs = ptr<float>(gso);
      emit_dgrad(gout, cout, R, p + ".skip_connection.weight", cin, 1, gso);
      ConvDesc cs = fwd_conv(t.x0, x1, cout);
      cs.ksz = 1;
      emit_wgrad(gout, cs, p + ".skip_connection");
      if (x1) {
        const int C0 = t.x0.C, C1 = t.x1.C;
        bops.push_back([gs, gx0, gx1, M, C0, C1, a0, a1](void* st) { return split_cat_launch(gs, gx0, gx1, M, C0, C1, a0, a1, st); });
      } else {
        const int64_t n = M * cin;
        bops.push_back([gx0, gs, n, a0](void* st) { return add_launch(gx0, gs, n, a0, st); });
      }
    }
  }

  void bwd_attn(const Tape& t) {
    const std::string& p = t.b.prefix;
    const int C = t.x0.C, R = t.x0.R, H = u->cfg.num_heads;
    const int64_t T = vox(R), M = (int64_t)N * T;
    const AttnDims dims{N, H, C, T};
    const size_t gout = grad_ready(t.out);
    if (gout == NONE) return;
    int ax = 0;
    float* gx = ptr<float>(grad_of(t.x0, &ax));
    {  // identity branch
      const int64_t n = M * C;
      const float* goutp = ptr<float>(gout);
      bops.push_back([gx, goutp, n, ax](void* st) { return add_launch(gx, goutp, n, ax, st); });
    }
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
      const GemmParams g = attn_gemm(dims, A, B, b_kmajor, Cc, alpha);
      bops.push_back([g](void* st) { return gemm_launch(g, st); });
    };
    const int Ti = (int)T, NH = N * H;
    const int64_t rows = (int64_t)NH * T;
    gemm(dims.qkv(qkv, 0), dims.qkv(qkv, 1), false, dims.scores(Pm), s2);
    bops.push_back([Pm, rows, Ti](void* st) { return softmax_rows_launch(Pm, rows, Ti, st); });
    gemm(dims.heads(ga), dims.qkv(qkv, 2), false, dims.scores(dS), 1.0f);
    bops.push_back([Pm, dS, rows, Ti](void* st) { return attn_ds_launch(Pm, dS, rows, Ti, st); });
    bops.push_back([Pm, Tm, NH, Ti](void* st) { return transpose_launch(Pm, Tm, NH, Ti, st); });
    gemm(dims.scores(Tm), dims.heads(ga), true, dims.qkv(gqkv, 2), 1.0f);  // dv
    gemm(dims.scores(dS), dims.qkv(qkv, 1), true, dims.qkv(gqkv, 0), s2);    // dq
    bops.push_back([dS, Tm, NH, Ti](void* st) { return transpose_launch(dS, Tm, NH, Ti, st); });
    gemm(dims.scores(Tm), dims.qkv(qkv, 0), true, dims.qkv(gqkv, 1), s2);  // dk
    // qkv conv (1x1, C -> 3C, GroupNorm applied on load, no activation)
    ConvDesc cq = fwd_conv(t.x0, nullptr, 3 * C);
    cq.ksz = 1;
    cq.coef = t.coefA;
    bwd_norm_conv(gqkv_off, cq, p + ".qkv", p + ".norm", t.momA);
  }

  void bwd_conv(const Tape& t) {  // input conv / Downsample / Upsample / output head
    const BlockKind kind = t.b.kind;
    const int cin = t.b.cin, cout = t.b.cout, Ri = t.x0.R, Ro = t.out.R, Nn = N;
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
        float* gz = ptr<float>(gz_off);
        bops.push_back([goutp, gz, Nn, Ro, cout](void* st) { return zero_insert2_launch(goutp, gz, Nn, Ro, cout, st); });
        emit_dgrad(gz_off, cout, Ri, wn + "#s1", cin, 3, gx_off, ax != 0);
      } else {
        const float* wtp = wt->f32;
        bops.push_back([goutp, wtp, gx, Nn, Ri, Ro, cin, cout, ax](void* st) {
          return conv_dgrad_s2_launch(goutp, wtp, gx, Nn, Ri, Ro, cin, cout, ax, st);
        });
      }
      f.out_R = Ro;
      f.stride = 2;
    } else {  // B_UP: conv at the fine size of the nearest-upsampled input
      const int64_t Mf = (int64_t)N * vox(Ro);
      const size_t gup_off = alloc((size_t)Mf * cin * sizeof(float));
      float* gup = ptr<float>(gup_off);
      emit_dgrad(gout, cout, Ro, wn, cin, 3, gup_off);
      bops.push_back([gup, gx, Nn, Ri, cin, ax](void* st) { return sumpool2_launch(gup, gx, Nn, Ri, cin, ax, st); });
      f.in_R = Ro;
      f.ups = 1;
    }
    emit_wgrad(gout, f, layer);
  }

  int build() {
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
    if (err.empty()) err = pl.err;  // (emit_conv's refusals)
    if (!err.empty()) {
      set_error("%s", err.c_str());
      return HOLO_E_STATE;
    }
    // embedding path
    {
      const float* embs = ptr<float>(pl.embs_off);
      float* gembs = ptr<float>(alloc((size_t)N * u->ted * sizeof(float)));
      float* dw = ptr<float>(gembw);
      float* db = ptr<float>(gembb);
      const float* w = u->emb_w;
      const int rows = u->emb_rows, K = u->ted, Nn = N;
      bops.push_back([dfilm_base, embs, w, dw, db, gembs, Nn, rows, K](void* st) {
        return film_bwd_launch(dfilm_base, embs, w, dw, db, gembs, Nn, rows, K, st);
      });
      const HoloUnet* uu = u;  // (t_dev is the running call's)
      const int mc = c.model_channels;
      const float *w1 = P(u, "time_embed.0.weight"), *b1 = P(u, "time_embed.0.bias"), *w2 = P(u, "time_embed.2.weight"),
                  *b2 = P(u, "time_embed.2.bias");
      float *dw1 = pgrad("time_embed.0.weight"), *db1 = pgrad("time_embed.0.bias"), *dw2 = pgrad("time_embed.2.weight"),
            *db2 = pgrad("time_embed.2.bias");
      bops.push_back([uu, Nn, mc, K, w1, b1, w2, b2, gembs, dw1, db1, dw2, db2](void* st) {
        return time_embed_bwd_launch(uu->t_dev, Nn, mc, K, w1, b1, w2, b2, gembs, dw1, db1, dw2, db2, st);
      });
    }
    auto gi = grads.find(pl.x_in.off);
    if (gi == grads.end()) {
      set_error("internal: the network input has no gradient");
      return HOLO_E_STATE;
    }
    tp.gx_off = gi->second.first;
    tp.bytes = tp.fwd.bytes = pl.arena_base + pl.arena.peak;  // (the backward's buffers grew the arena after pl.build())
    return 0;
  }
};

bool params_set(const HoloUnet* u, const char* entry) {
  for (auto& s : u->params)
    if (!s.set) {
      set_error("%s: parameter '%s' has not been set", entry, s.name.c_str());
      return false;
    }
  return true;
}

// the training plan of (batch, ws), rebuilt when either changed; `entry` names the caller in the workspace message
int ensure_train_plan(HoloUnet* u, const char* entry, int batch, void* ws, size_t ws_bytes) {
  if (!u->tplan.built_for(batch, ws)) {
    if (u->compute_mode != 0) {
      set_error("holo_unet_backward: the backward pass runs in the fp32 mode only");
      return HOLO_E_UNSUPPORTED;
    }
    if (!params_set(u, "holo_unet_backward")) return HOLO_E_STATE;
    TrainPlanner tp(u, batch, ws, u->tplan);
    int rc = tp.build();
    if (!rc && !tp.pl.regions_ok()) {
      set_error("internal: small-buffer regions overflow");
      rc = HOLO_E_INVALID;
    }
    if (rc) {
      u->tplan.invalidate();
      return rc;
    }
  }
  if (ws_bytes < u->tplan.bytes) {
    set_error("%s: workspace too small (%zu < %zu)", entry, ws_bytes, u->tplan.bytes);
    u->tplan.invalidate();
    return HOLO_E_WORKSPACE;
  }
  return 0;
}

int ensure_plan(HoloUnet* u, int batch, void* ws) {
  if (u->plan.built_for(batch, ws)) return 0;
  if (!params_set(u, "holo_unet_forward")) return HOLO_E_STATE;
  if (u->batch_invariant && u->compute_mode != 0) {  // (both setters refuse this; a guard for the plan itself)
    set_error("holo_unet_forward: the batch-invariant plan is exact-fp32 only");
    return HOLO_E_UNSUPPORTED;
  }
  Planner pl(u, batch, ws, u->plan);
  pl.build();
  int rc = 0;
  if (!pl.err.empty()) {
    set_error("holo_unet_forward: %s", pl.err.c_str());
    rc = HOLO_E_UNSUPPORTED;
  } else if (!pl.regions_ok()) {
    set_error("internal: small-buffer regions overflow");
    rc = HOLO_E_INVALID;
  }
  if (rc) u->plan.invalidate();
  return rc;
}

int run_op(const HoloUnet* u, const Op& op, int N, const float* x, const int64_t* t, float* y, void* stream) {
  switch (op.kind) {
    case OP_IN:
      return ncdhw_to_ndhwc_launch(x, op.in.dst, N, op.in.C, op.in.V, 0, stream, op.in.dst_bf16);
    case OP_TEMB:
      return time_embed_launch(t, N, u->cfg.model_channels, u->ted, op.temb.w1, op.temb.b1, op.temb.w2, op.temb.b2,
                               op.temb.emb, op.temb.emb_silu, op.temb.load_kind, stream);
    case OP_EMBLIN:
      return rows_linear_launch(op.emblin.emb_silu, op.emblin.w, op.emblin.b, op.emblin.out, N, u->emb_rows, u->ted, stream);
    case OP_STATS:
      return gn_stats_launch(op.stats.x, op.stats.part, N, op.stats.C, op.stats.V, stream, op.stats.x_bf16);
    case OP_FINAL: {
      const GnFinalize& f = op.fin;
      return gn_finalize_launch(f.part0, f.C0, f.B0, f.part1, f.C1, f.B1, N, f.V, f.groups, 1e-5f, f.gamma, f.beta, f.film,
                                f.film_stride, f.film_cout, f.coef, stream, f.moments);
    }
    case OP_CONV:
      return conv_launch(op.conv, stream);
    case OP_GEMM:
      return gemm_launch(op.gemm, stream);
    case OP_SOFTMAX:
      return softmax_rows_launch(op.softmax.S, op.softmax.rows, op.softmax.cols, stream);
    case OP_FLASH: {
      const Flash& f = op.flash;
      if (f.form == 2) return flash_attn_bf16v2_launch(f.attn, f.packed, f.out_bf16, f.ksplit, f.lazy, stream, f.operands_packed);
      return flash_attn_launch(f.attn, stream);
    }
    case OP_OUT:
      return ndhwc_to_ncdhw_launch(op.out.src, y, N, op.out.C, op.out.V, stream);
  }
  return 0;
}

// The side lane's stream and events (the handle owns them; holo_unet_destroy).  The emulation build has one stream: its
// side lane is the caller's stream, fork and join are nothing (run_lanes).
int ensure_lanes(HoloUnet* u, int n_joins) {
#ifndef HOLO_EMU
  if (!u->side_stream) HIP_TRY(hipStreamCreateWithFlags((hipStream_t*)&u->side_stream, hipStreamNonBlocking));
  for (void** e : {&u->fork_event, &u->tail_event})
    if (!*e) HIP_TRY(hipEventCreateWithFlags((hipEvent_t*)e, hipEventDisableTiming));
  while ((int)u->join_events.size() < n_joins) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    u->join_events.push_back(e);
  }
#endif
  (void)u, (void)n_joins;
  return 0;
}

// Issues the ops of a plan in plan order from the host, each on its lane: `run(i, op, stream)` launches op i (or skips it)
// and returns its code.  Plan order is a valid serial order, and a side op stands in front of its consumer in it, so every
// event is recorded before anything waits for it - host order alone guarantees that.  The side stream starts behind everything
// the caller's stream holds at the fork, so the side ops of one call cannot overtake the previous call either.  Whatever
// happens after the fork, the caller's stream is left waiting for the side stream: on success through the consumers' joins
// (the last of them stands behind every side op, the side stream runs in order), on an error through the tail event.
template <class Run>
int run_lanes(HoloUnet* u, const Plan& plan, void* stream, Run run) {
  int rc = 0;
#ifdef HOLO_EMU
  for (size_t i = 0; i < plan.ops.size() && !rc; ++i) rc = run((int)i, plan.ops[i], stream);
#else
  if (!plan.n_joins) {
    for (size_t i = 0; i < plan.ops.size() && !rc; ++i) rc = run((int)i, plan.ops[i], stream);
    return rc ? (rc < 0 ? rc : HOLO_E_INVALID) : 0;
  }
  if ((rc = ensure_lanes(u, plan.n_joins))) return rc;
  const hipStream_t main = (hipStream_t)stream, side = (hipStream_t)u->side_stream;
  bool forked = false;
  hipError_t he = hipSuccess;
  for (size_t i = 0; i < plan.ops.size() && !rc && he == hipSuccess; ++i) {
    const Op& op = plan.ops[i];
    if (op.fork) {
      if ((he = hipEventRecord((hipEvent_t)u->fork_event, main)) != hipSuccess) break;
      if ((he = hipStreamWaitEvent(side, (hipEvent_t)u->fork_event, 0)) != hipSuccess) break;
      forked = true;
    }
    if (op.side) {
      rc = run((int)i, op, side);
      if (!rc && op.join >= 0) he = hipEventRecord((hipEvent_t)u->join_events[op.join], side);
    } else {
      if (op.join >= 0 && (he = hipStreamWaitEvent(main, (hipEvent_t)u->join_events[op.join], 0)) != hipSuccess) break;
      rc = run((int)i, op, main);
    }
  }
  if (he != hipSuccess) {
    set_error("the side lane of the forward failed: %s", hipGetErrorString(he));
    rc = HOLO_E_HIP;
  }
  if (rc && forked) {  // (best effort: the caller's stream still ends behind the side stream)
    if (hipEventRecord((hipEvent_t)u->tail_event, side) == hipSuccess) (void)hipStreamWaitEvent(main, (hipEvent_t)u->tail_event, 0);
  }
#endif
  return rc ? (rc < 0 ? rc : HOLO_E_INVALID) : 0;
}

// the forward of a plan (inference or training) on the caller's tensors; y may be null where the caller does not want it
int run_plan(HoloUnet* u, const Plan& plan, const float* x, const int64_t* t, float* y, void* stream) {
  return run_lanes(u, plan, stream, [&](int, const Op& op, void* st) {
    return op.kind == OP_OUT && !y ? 0 : run_op(u, op, plan.batch, x, t, y, st);
  });
}
// the backward launches of a training plan whose taped forward has run on `workspace`
int run_backward(const HoloUnet* u, const TrainPlan& tp, const float* grad_out, float* grad_x, void* workspace, void* stream) {
  const HoloUnetCfg& c = u->cfg;
  const int batch = tp.fwd.batch;
  const int64_t V = (int64_t)c.image_size * c.image_size * c.image_size;
  if (ncdhw_to_ndhwc_launch(grad_out, (float*)((char*)workspace + tp.gy_off), batch, c.out_channels, V, 0, stream))
    return HOLO_E_INVALID;
  for (auto& f : tp.bops) {
    const int rc = f(stream);
    if (rc) return rc < 0 ? rc : HOLO_E_INVALID;
  }
  if (grad_x && ndhwc_to_ncdhw_launch((const float*)((char*)workspace + tp.gx_off), grad_x, batch, c.in_channels, V, stream))
    return HOLO_E_INVALID;
  return 0;
}

// The sampler step entries (holo_*_step*, include/holo_abi.h): each names the pointers it needs, then its launcher checks the shapes
template <class Launch>
int step_entry(const char* entry, bool args_ok, Launch launch) {
  if (!args_ok) {
    set_error("%s: null/invalid argument", entry);
    return HOLO_E_INVALID;
  }
  return launch() ? HOLO_E_INVALID : 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int holo_abi_version(void) { return HOLO_ABI_VERSION; }
const char* holo_last_error(void) { return get_error(); }

int holo_ctx_create(int device_id, HoloCtx** out) {
  if (!out) {
    set_error("holo_ctx_create: null out");
    return HOLO_E_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  HoloCtx* c = new HoloCtx;
  c->device = device_id;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // (HOLO_NUM_CUS, test knob: planners size grids / split-K for this many CUs - the one knob read here, holo_knobs.h)
  if (const int64_t v = Knobs::from_env().num_cus) c->num_cus = (int)v;
  *out = c;
  return 0;
}
int holo_ctx_destroy(HoloCtx* ctx) {
  delete ctx;
  return 0;
}
int holo_ctx_set_deterministic(HoloCtx* ctx, int on) {
  if (!ctx) {
    set_error("holo_ctx_set_deterministic: null context");
    return HOLO_E_INVALID;
  }
  ctx->deterministic = on ? 1 : 0;
  return 0;
}
int holo_ctx_get_deterministic(const HoloCtx* ctx) { return ctx ? ctx->deterministic : 0; }

int holo_unet_create(HoloCtx* ctx, const HoloUnetCfg* cfg, HoloUnet** out) {
  if (!ctx || !cfg || !out) {
    set_error("holo_unet_create: null argument");
    return HOLO_E_INVALID;
  }
  if (!cfg->homogeneous_resample) {
    set_error("holo_unet_create: only homogeneous_resample=True is supported");
    return HOLO_E_UNSUPPORTED;
  }
  if (cfg->n_channel_mult < 1 || cfg->n_channel_mult > 8 || cfg->n_attention_resolutions > 8 ||
      cfg->model_channels % 32 || cfg->in_channels % 4 || cfg->out_channels % 4 || cfg->model_channels > 256 ||
      cfg->image_size % (1 << (cfg->n_channel_mult - 1))) {
    set_error("holo_unet_create: unsupported configuration");
    return HOLO_E_UNSUPPORTED;
  }
  HoloUnet* u = new HoloUnet;
  u->ctx = ctx;
  u->cfg = *cfg;
  build_structure(u);
  enumerate_params(u);
  u->knobs = Knobs::from_env();
  // private parameter storage
  const StoreSizes n = carve_params(u, nullptr, nullptr, nullptr);
  if (hipMalloc((void**)&u->pstore, (size_t)n.f32 * sizeof(float)) != hipSuccess ||
      (n.bf && hipMalloc((void**)&u->pstore_bf, (size_t)n.bf * sizeof(uint16_t)) != hipSuccess) ||
      (n.wino && hipMalloc((void**)&u->pstore_wino, (size_t)n.wino * sizeof(float)) != hipSuccess)) {
    set_error("holo_unet_create: hipMalloc of the parameter stores (%lld floats, %lld bf16 weights, %lld Winograd floats) failed",
              (long long)n.f32, (long long)n.bf, (long long)n.wino);
    holo_unet_destroy(u);
    return HOLO_E_HIP;
  }
  carve_params(u, u->pstore, u->pstore_bf, u->pstore_wino);
  *out = u;
  return 0;
}

int holo_unet_destroy(HoloUnet* net) {
  if (!net) return 0;
  if (net->pstore) (void)hipFree(net->pstore);
  if (net->pstore_bf) (void)hipFree(net->pstore_bf);
  if (net->pstore_wino) (void)hipFree(net->pstore_wino);
  for (auto& kv : net->dgrad)
    for (float* buf : {kv.second.f32, kv.second.wino2, kv.second.wino3})
      if (buf) (void)hipFree(buf);
  if (net->dgrad_tmp) (void)hipFree(net->dgrad_tmp);
#ifndef HOLO_EMU
  if (net->side_stream) {  // (every forward left the caller's stream waiting for it; drain it before its events go)
    (void)hipStreamSynchronize((hipStream_t)net->side_stream);
    (void)hipStreamDestroy((hipStream_t)net->side_stream);
  }
  for (void* e : {net->fork_event, net->tail_event})
    if (e) (void)hipEventDestroy((hipEvent_t)e);
  for (void* e : net->join_events) (void)hipEventDestroy((hipEvent_t)e);
#endif
  delete net;
  return 0;
}

int holo_unet_num_params(const HoloUnet* net) { return net ? (int)net->params.size() : 0; }

int holo_unet_param_info(const HoloUnet* net, int index, char* name, int name_cap, int64_t shape[8], int* ndim) {
  if (!net || index < 0 || index >= (int)net->params.size()) {
    set_error("holo_unet_param_info: bad index");
    return HOLO_E_INVALID;
  }
  const ParamSlot& s = net->params[index];
  if (name && name_cap > 0) {
    strncpy(name, s.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ndim) *ndim = (int)s.shape.size();
  if (shape)
    for (size_t i = 0; i < s.shape.size() && i < 8; ++i) shape[i] = s.shape[i];
  return 0;
}

int holo_unet_set_param(HoloUnet* net, const char* name, const void* dev_ptr, int dtype, int ndim,
                        const int64_t* shape, void* stream) {
  if (!net || !name || !dev_ptr) {
    set_error("holo_unet_set_param: null argument");
    return HOLO_E_INVALID;
  }
  if (dtype != HOLO_DTYPE_F32) {
    set_error("holo_unet_set_param: only fp32 parameters are supported");
    return HOLO_E_UNSUPPORTED;
  }
  auto it = net->pindex.find(name);
  if (it == net->pindex.end()) {
    set_error("holo_unet_set_param: unknown parameter '%s'", name);
    return HOLO_E_INVALID;
  }
  ParamSlot& s = net->params[it->second];
  bool ok = ndim == (int)s.shape.size();
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == s.shape[i];
  if (!ok) {
    set_error("holo_unet_set_param: shape mismatch for '%s'", name);
    return HOLO_E_INVALID;
  }
  if (s.is_conv()) {
    if (const int rc = pack_conv_weights((const float*)dev_ptr, s.w, stream)) return rc;
  } else {  // biases, GroupNorm parameters, Linear layers: a copy kernel with system-scope loads (holo_ld_sys) - like the
            // weight repack kernels, every ingestion of a caller-provided tensor reads it past the L2
    if (copy_sys_launch((const float*)dev_ptr, s.w.f32, s.numel, stream)) return HOLO_E_INVALID;
  }
  s.set = true;
  return 0;
}

int holo_unet_set_compute_dtype(HoloUnet* net, int dtype) {
  if (!net || (dtype != HOLO_DTYPE_F32 && dtype != HOLO_DTYPE_BF16 && dtype != HOLO_DTYPE_F32_BF16X3)) {
    set_error("holo_unet_set_compute_dtype: HOLO_DTYPE_F32, HOLO_DTYPE_BF16 or HOLO_DTYPE_F32_BF16X3");
    return HOLO_E_INVALID;
  }
  const int mode = dtype == HOLO_DTYPE_BF16 ? 1 : dtype == HOLO_DTYPE_F32_BF16X3 ? 2 : 0;
  if (mode != 0 && net->batch_invariant) {
    set_error("holo_unet_set_compute_dtype: the batch-invariant plan is exact-fp32 only; turn it off first "
              "(holo_unet_set_batch_invariant(net, 0))");
    return HOLO_E_UNSUPPORTED;
  }
  if (mode != net->compute_mode) {
    net->compute_mode = mode;
    net->plan.invalidate();  // re-plan: the conv ops carry the choice
    net->ws_cache.clear();   // ... and the plan's workspace differs between modes (fused skips, statistics slabs)
  }
  return 0;
}

int holo_unet_set_batch_invariant(HoloUnet* net, int on) {
  if (!net) {
    set_error("holo_unet_set_batch_invariant: null net");
    return HOLO_E_INVALID;
  }
  // Exact fp32 only.  The bf16 modes are refused rather than half supported: their plans pick kernels (the persistent
  // bf16 convolution, the streaming bf16 1x1x1 GEMMs, the packed bf16 attention) whose geometry helpers size their
  // work per launch, and no test pins the rows of those modes.
  if (on && net->compute_mode != 0) {
    set_error("holo_unet_set_batch_invariant: batch-invariant plans are exact-fp32 only (compute dtype HOLO_DTYPE_F32); "
              "the bf16 and bf16x3 modes are not supported");
    return HOLO_E_UNSUPPORTED;
  }
  if ((on != 0) != net->batch_invariant) {
    net->batch_invariant = on != 0;
    net->plan.invalidate();  // re-plan: the conv ops carry the choices (ws_cache is keyed on the flag)
  }
  return 0;
}

size_t holo_unet_workspace_bytes(HoloUnet* net, int batch) {
  if (!net || batch < 1) return 0;
  const std::pair<int, bool> key(batch, net->batch_invariant);
  auto it = net->ws_cache.find(key);
  if (it != net->ws_cache.end()) return it->second;
  Plan sizing;  // built on a null base and dropped
  Planner(net, batch, nullptr, sizing).build();
  net->ws_cache[key] = sizing.bytes;
  return sizing.bytes;
}

int holo_unet_forward(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, float* y, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!net || !x || !timesteps || !y || !workspace || batch < 1) {
    set_error("holo_unet_forward: null/invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  if (workspace_bytes < net->plan.bytes) {
    set_error("holo_unet_forward: workspace too small (%zu < %zu)", workspace_bytes, net->plan.bytes);
    return HOLO_E_WORKSPACE;
  }
  return run_plan(net, net->plan, x, timesteps, y, stream);
}

int holo_unet_forward_cl(HoloUnet* net, int batch, const float* x_cl, const int64_t* timesteps, float* y_cl, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!net || !x_cl || !timesteps || !y_cl || !workspace || batch < 1) {
    set_error("holo_unet_forward_cl: null/invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  const Plan& plan = net->plan;
  if (workspace_bytes < plan.bytes) {
    set_error("holo_unet_forward_cl: workspace too small (%zu < %zu)", workspace_bytes, plan.bytes);
    return HOLO_E_WORKSPACE;
  }
  if (plan.cl_refusal) {
    set_error("%s", plan.cl_refusal);
    return HOLO_E_UNSUPPORTED;
  }
  // the first / last convolution (Planner::find_cl_ends) run on the caller's channels-last tensors instead of the plan's
  // own input / output buffers, and the two layout passes are skipped
  const bool bf16_storage = net->compute_mode == 1;  // the plan's input buffer is bf16: a cast replaces the layout pass
  return run_lanes(net, plan, stream, [&](int i, const Op& op, void* st) {
    if (op.kind == OP_IN && bf16_storage)  // fp32 channels-last -> the plan's bf16 channels-last input buffer
      return f32_to_bf16_launch(x_cl, op.in.dst, (int64_t)batch * op.in.C * op.in.V, st) ? (int)HOLO_E_INVALID : 0;
    if (op.kind == OP_IN || op.kind == OP_OUT) return 0;
    if (i == plan.first_conv || i == plan.last_conv) {
      Op o2 = op;
      if (i == plan.first_conv && !bf16_storage) o2.conv.src0 = x_cl;
      if (i == plan.last_conv) o2.conv.out = y_cl;
      return run_op(net, o2, batch, x_cl, timesteps, y_cl, st);
    }
    return run_op(net, op, batch, x_cl, timesteps, y_cl, st);
  });
}

int holo_unet_fetch_block(HoloUnet* net, const char* tag, float* dst, int64_t dst_capacity, int64_t* numel,
                          void* workspace, void* stream) {
  if (!net || !tag || !dst || !workspace) {
    set_error("holo_unet_fetch_block: null argument");
    return HOLO_E_INVALID;
  }
  if (!net->knobs.keep_intermediates) {
    set_error("holo_unet_fetch_block: create the net with HOLO_KEEP_INTERMEDIATES=1");
    return HOLO_E_STATE;
  }
  const Plan& plan = net->plan;
  if (plan.ws != workspace || plan.ops.empty()) {
    set_error("holo_unet_fetch_block: no forward has run on this workspace");
    return HOLO_E_STATE;
  }
  auto it = plan.block_outputs.find(tag);
  if (it == plan.block_outputs.end()) {
    set_error("holo_unet_fetch_block: unknown tag '%s'", tag);
    return HOLO_E_INVALID;
  }
  const Act& a = it->second;
  const int64_t V = (int64_t)a.R * a.R * a.R;
  const int64_t n = (int64_t)plan.batch * V * a.C;
  if (numel) *numel = n;
  if (dst_capacity < n) {
    set_error("holo_unet_fetch_block: destination too small");
    return HOLO_E_INVALID;
  }
  return ndhwc_to_ncdhw_launch((const float*)((char*)workspace + a.off), dst, plan.batch, a.C, V, stream,
                               net->compute_mode == 1 ? 1 : 0);
}

int holo_unet_time_convs(HoloUnet* net, int batch, void* workspace, size_t workspace_bytes, int iters, void* stream,
                         float* total_ms, double* total_flops, int* n_launches) {
  if (!net || !workspace || iters < 1) {
    set_error("holo_unet_time_convs: invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  if (workspace_bytes < net->plan.bytes) {
    set_error("holo_unet_time_convs: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  double flops = 0.0;
  int launches = 0;
  for (const Op& op : net->plan.ops)
    if (op.kind == OP_CONV && op.conv.ksz == 3) {
      flops += conv_flops(op.conv);
      ++launches;
    }
  HIP_TRY(hipEventRecord(e0, (hipStream_t)stream));
  for (int it = 0; it < iters; ++it)
    for (const Op& op : net->plan.ops)
      if (op.kind == OP_CONV && op.conv.ksz == 3) {
        rc = conv_launch(op.conv, stream);
        if (rc) return HOLO_E_INVALID;
      }
  HIP_TRY(hipEventRecord(e1, (hipStream_t)stream));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (total_ms) *total_ms = ms / iters;
  if (total_flops) *total_flops = flops;
  if (n_launches) *n_launches = launches;
  return 0;
}

int holo_unet_time_ops(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, float* y, void* workspace,
                       size_t workspace_bytes, int iters, void* stream, HoloOpTiming* out, int cap, int* n_ops) {
  if (!net || !workspace || !x || !timesteps || !y || iters < 1 || !n_ops || (cap > 0 && !out)) {
    set_error("holo_unet_time_ops: invalid argument");
    return HOLO_E_INVALID;
  }
  int rc = ensure_plan(net, batch, workspace);
  if (rc) return rc;
  if (workspace_bytes < net->plan.bytes) {
    set_error("holo_unet_time_ops: workspace too small");
    return HOLO_E_WORKSPACE;
  }
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  int n = 0;
  for (const Op& op : net->plan.ops) {
    rc = run_op(net, op, batch, x, timesteps, y, stream);  // untimed first touch (also keeps the data flow valid)
    if (rc) return HOLO_E_INVALID;
    if (n < cap) {
      HIP_TRY(hipEventRecord(e0, (hipStream_t)stream));
      for (int it = 0; it < iters; ++it) run_op(net, op, batch, x, timesteps, y, stream);
      HIP_TRY(hipEventRecord(e1, (hipStream_t)stream));
      HIP_TRY(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
      HoloOpTiming& t = out[n];
      memset(&t, 0, sizeof(t));
      t.op = (int)op.kind;
      t.ms = ms / iters;
      if (op.kind == OP_CONV) {
        const ConvParams& c = op.conv;
        t.kernel = (int)c.kernel;
        t.tile_depth = c.tz;  // (0 off the halo forms)
        t.fused_skip = c.skip_w ? 1 : 0;
        t.nsplit = c.nsplit;
        t.cin = c.C0 + c.C1;
        t.cout = c.Cout;
        t.out_dim = c.OD;
        t.stride = c.stride;
        t.upsample = c.ups;
        t.ksz = c.ksz;
        t.flops = conv_flops(c);
        t.flops_executed = conv_exec_flops(c);
      } else if (op.kind == OP_FLASH) {
        const AttnParams& at = op.flash.attn;
        t.cin = t.cout = at.C;
        t.out_dim = at.T;
        t.flops = 4.0 * at.N * (double)at.T * at.T * at.C;
      } else if (op.kind == OP_GEMM) {
        t.cin = op.gemm.K;
        t.cout = op.gemm.Nn;
        t.out_dim = op.gemm.M;
        t.flops = 2.0 * op.gemm.nb0 * op.gemm.nb1 * (double)op.gemm.M * op.gemm.Nn * op.gemm.K;
      }
    }
    ++n;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *n_ops = n;
  return 0;
}

// ---- training: backward of the denoiser -----------------------------------------------------------------------------
// The transposed-convolution copies of convolution weight `s` from the caller's OIDHW tensor: holo_unet_set_dgrad_weight, and
// the refresh of holo_unet_adam_step (which meets every buffer already allocated).
static int prepare_dgrad_weight(HoloUnet* net, const ParamSlot& s, const void* dev_ptr, void* stream) {
  const int Co = (int)s.shape[0], Ci = (int)s.shape[1], T = s.kind == P_CONV3 ? 27 : 1;
  const std::string& nm = s.name;
  const bool down = is_downsample_weight(nm);
  if (down) {  // [tap][co][ci] for conv_dgrad_s2_kernel (the fallback), then the stride-1 form below under "<name>#s1":
               // the transposed stride-2 convolution runs as zero insertion + the stride-1 transposed convolution
    float*& d2 = net->dgrad[nm].f32;
    if (!d2) HIP_TRY(hipMalloc((void**)&d2, (size_t)T * Co * Ci * sizeof(float)));
    if (weight_tco_ci_launch((const float*)dev_ptr, d2, Co, Ci, T, stream)) return HOLO_E_INVALID;
    if ((Co & 3) || (Ci & 3)) return 0;
  }
  // The transposed convolution (Cout' = Ci, Cin' = Co), packed like a forward weight.  Its buffers are created at the first
  // call for this weight (an inference-only user pays nothing): the fp32 pack, and the Winograd packs of dgrad_copies - the
  // dgrad of a wide-level 3x3x3 conv runs on conv_wino2_kernel / conv_wino3_kernel like the forward conv.
  ConvWeights& dw = net->dgrad[down ? nm + "#s1" : nm];
  const ConvWeightLayout l = dw.layout = s.layout(true);
  const ConvCopies c = dgrad_copies(l, net->compute_mode, net->knobs);
  if (!dw.f32) HIP_TRY(hipMalloc((void**)&dw.f32, (size_t)l.f32_floats() * sizeof(float)));
  if ((c.wino2 && !dw.wino2) || (c.wino3 && !dw.wino3)) {  // a plan sized before these copies existed chose other kernels
    net->tws_cache.clear();                                 // (and scratch sizes)
    net->tplan.invalidate();
    if (!dw.wino2) HIP_TRY(hipMalloc((void**)&dw.wino2, (size_t)l.wino2_floats() * sizeof(float)));
    if (c.wino3 && !dw.wino3) HIP_TRY(hipMalloc((void**)&dw.wino3, (size_t)l.wino3_floats() * sizeof(float)));
  }
  if (!net->dgrad_tmp) {
    int64_t largest = 0;
    for (const ParamSlot& q : net->params)
      if (q.is_conv() && q.numel > largest) largest = q.numel;
    HIP_TRY(hipMalloc((void**)&net->dgrad_tmp, (size_t)largest * sizeof(float)));
  }
  if (flip_transpose_weight_launch((const float*)dev_ptr, net->dgrad_tmp, Co, Ci, T, stream)) return HOLO_E_INVALID;
  if (pack_conv_weights(net->dgrad_tmp, dw, stream)) return HOLO_E_INVALID;
  return 0;
}

int holo_unet_set_dgrad_weight(HoloUnet* net, const char* name, const void* dev_ptr, void* stream) {
  if (!net || !name || !dev_ptr) {
    set_error("holo_unet_set_dgrad_weight: null argument");
    return HOLO_E_INVALID;
  }
  auto it = net->pindex.find(name);
  if (it == net->pindex.end() || !net->params[it->second].is_conv()) {
    set_error("holo_unet_set_dgrad_weight: '%s' is not a convolution weight", name);
    return HOLO_E_INVALID;
  }
  return prepare_dgrad_weight(net, net->params[it->second], dev_ptr, stream);
}

size_t holo_unet_backward_workspace_bytes(HoloUnet* net, int batch) {
  if (!net || batch < 1) return 0;
  auto it = net->tws_cache.find(batch);
  if (it != net->tws_cache.end()) return it->second;
  TrainPlan sizing;  // built on a null base (TrainPlanner::find_dgw: no transposed weight is missed there) and dropped
  if (TrainPlanner(net, batch, nullptr, sizing).build()) return 0;  // the message is in holo_last_error()
  net->tws_cache[batch] = sizing.bytes;
  return sizing.bytes;
}

// The two halves of holo_unet_backward as entries of their own (ABI 4): a caller whose cotangent depends on the output - the
// clamp of pred_xstart in HoloDiffusionModel.training_backward - runs the taped forward, forms grad_out from y, then the backward,
// instead of paying a plain forward first.
int holo_unet_forward_train(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, float* y, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!net || !x || !timesteps || !workspace || batch < 1) {
    set_error("holo_unet_forward_train: null/invalid argument");
    return HOLO_E_INVALID;
  }
  net->tape_valid = false;
  int rc = ensure_train_plan(net, "holo_unet_forward_train", batch, workspace, workspace_bytes);
  if (rc) return rc;
  net->t_dev = timesteps;
  rc = run_plan(net, net->tplan.fwd, x, timesteps, y, stream);
  net->tape_valid = rc == 0;
  return rc;
}

int holo_unet_backward_taped(HoloUnet* net, int batch, const float* grad_out, float* grad_x, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (!net || !grad_out || !workspace || batch < 1) {
    set_error("holo_unet_backward_taped: null/invalid argument");
    return HOLO_E_INVALID;
  }
  if (!net->tape_valid || !net->tplan.built_for(batch, workspace) || workspace_bytes < net->tplan.bytes) {
    set_error("holo_unet_backward_taped: no taped forward of this batch on this workspace (holo_unet_forward_train first)");
    return HOLO_E_STATE;
  }
  net->tape_valid = false;  // the backward consumes the tape (gradient buffers share its workspace)
  return run_backward(net, net->tplan, grad_out, grad_x, workspace, stream);
}

int holo_unet_backward(HoloUnet* net, int batch, const float* x, const int64_t* timesteps, const float* grad_out, float* y,
                       float* grad_x, void* workspace, size_t workspace_bytes, void* stream) {
  if (!net || !x || !timesteps || !grad_out || !workspace || batch < 1) {
    set_error("holo_unet_backward: null/invalid argument");
    return HOLO_E_INVALID;
  }
  net->tape_valid = false;
  int rc = ensure_train_plan(net, "holo_unet_backward", batch, workspace, workspace_bytes);
  if (rc) return rc;
  net->t_dev = timesteps;
  rc = run_plan(net, net->tplan.fwd, x, timesteps, y, stream);
  return rc ? rc : run_backward(net, net->tplan, grad_out, grad_x, workspace, stream);
}

int holo_unet_get_grad(HoloUnet* net, const char* name, float* dst, int64_t numel, const void* workspace, void* stream) {
  if (!net || !name || !dst || !workspace) {
    set_error("holo_unet_get_grad: null argument");
    return HOLO_E_INVALID;
  }
  auto it = net->pindex.find(name);
  if (it == net->pindex.end()) {
    set_error("holo_unet_get_grad: unknown parameter '%s'", name);
    return HOLO_E_INVALID;
  }
  if (net->tplan.fwd.ws != workspace || net->tplan.grad_off.size() != net->params.size()) {
    set_error("holo_unet_get_grad: no backward pass has run on this workspace");
    return HOLO_E_STATE;
  }
  const ParamSlot& s = net->params[it->second];
  if (numel != s.numel) {
    set_error("holo_unet_get_grad: '%s' has %lld elements, not %lld", name, (long long)s.numel, (long long)numel);
    return HOLO_E_INVALID;
  }
  HIP_TRY(hipMemcpyAsync(dst, (const char*)workspace + net->tplan.grad_off[it->second], (size_t)numel * sizeof(float),
                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// ---- parameter update (kernels_optim.hip) ----------------------------------------------------------------------------
// A float of the configuration as the double the caller wrote: the shortest decimal that rounds to it (0.9f -> 0.9).  torch
// forms 1 - beta2 and the bias corrections from the DOUBLE hyper-parameters; (double)0.999f would put 1.3e-5 of relative
// error into 1 - beta2.
static double widen_decimal(float f) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof(buf), "%.*g", prec, (double)f);
    if (strtof(buf, nullptr) == f) break;
  }
  return strtod(buf, nullptr);
}

static int adam_scalars(const char* who, const HoloAdamCfg* cfg, AdamScalars* s, double* dbg) {
  if (cfg->step < 1 || !(cfg->lr >= 0.f) || !(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) || !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f) ||
      !(cfg->eps >= 0.f) || !(cfg->weight_decay >= 0.f)) {
    set_error("%s: step >= 1, lr >= 0, betas in [0, 1), eps >= 0 and weight_decay >= 0 are required", who);
    return HOLO_E_INVALID;
  }
  const double lr = widen_decimal(cfg->lr), b1 = widen_decimal(cfg->beta1), b2 = widen_decimal(cfg->beta2);
  const double wd = widen_decimal(cfg->weight_decay);
  const double bc1 = 1.0 - pow(b1, (double)cfg->step), bc2 = 1.0 - pow(b2, (double)cfg->step);
  const double step_size = lr / bc1, bc2_sqrt = sqrt(bc2);
  if (s) {
    s->w1 = (float)(1.0 - b1);
    s->beta2 = (float)b2;
    s->w2 = (float)(1.0 - b2);
    s->eps = cfg->eps;
    s->neg_step_size = (float)-step_size;
    s->bc2_sqrt = (float)bc2_sqrt;
    s->weight_decay = (float)wd;
    s->decay = (float)(1.0 - lr * wd);
    s->adamw = cfg->adamw != 0;
  }
  if (dbg) {
    const double v[6] = {bc1, bc2, step_size, bc2_sqrt, 1.0 - b1, 1.0 - b2};
    memcpy(dbg, v, sizeof(v));
  }
  return 0;
}

int holo_adam_scalars(const HoloAdamCfg* cfg, double* out) {
  if (!cfg || !out) {
    set_error("holo_adam_scalars: null argument");
    return HOLO_E_INVALID;
  }
  return adam_scalars("holo_adam_scalars", cfg, nullptr, out);
}

int holo_adam_step(HoloCtx* ctx, const HoloAdamTensor* tensors, int n, const HoloAdamCfg* cfg, const float* clip_coef_dev,
                   void* stream) {
  if (!tensors || !cfg || n < 0) {
    set_error("holo_adam_step: null/invalid argument");
    return HOLO_E_INVALID;
  }
  (void)ctx;
  AdamScalars s;
  if (const int rc = adam_scalars("holo_adam_step", cfg, &s, nullptr)) return rc;
  return adam_step_launch(tensors, nullptr, n, s, clip_coef_dev, stream) ? HOLO_E_INVALID : 0;
}

size_t holo_grad_norm_workspace_bytes(const HoloAdamTensor* tensors, int n) {
  if (!tensors || n < 0) return 0;
  return (size_t)grad_norm_partials(tensors, n) * sizeof(double);
}

int holo_grad_norm(HoloCtx* ctx, const HoloAdamTensor* tensors, int n, float max_norm, void* workspace, size_t ws_bytes,
                   float* total_norm_dev, float* clip_coef_dev, void* stream) {
  if (!tensors || n < 0 || !total_norm_dev || !clip_coef_dev) {
    set_error("holo_grad_norm: null/invalid argument");
    return HOLO_E_INVALID;
  }
  (void)ctx;
  const size_t need = holo_grad_norm_workspace_bytes(tensors, n);
  if (need && (!workspace || ws_bytes < need || ((uintptr_t)workspace & 7))) {
    set_error("holo_grad_norm: workspace of %zu bytes (8-byte aligned) needed, got %zu", need, ws_bytes);
    return HOLO_E_WORKSPACE;
  }
  return grad_norm_launch(tensors, n, max_norm, (double*)workspace, total_norm_dev, clip_coef_dev, stream) ? HOLO_E_INVALID : 0;
}

int holo_unet_adam_step(HoloUnet* net, const HoloAdamTensor* tensors, int n, const HoloAdamCfg* cfg, const float* clip_coef_dev,
                        void* stream) {
  if (!net || !tensors || !cfg) {
    set_error("holo_unet_adam_step: null argument");
    return HOLO_E_INVALID;
  }
  if (n != (int)net->params.size()) {
    set_error("holo_unet_adam_step: %d tensors for %d parameters (holo_unet_param_info order)", n, (int)net->params.size());
    return HOLO_E_INVALID;
  }
  AdamScalars sc;
  if (const int rc = adam_scalars("holo_unet_adam_step", cfg, &sc, nullptr)) return rc;
  for (int i = 0; i < n; ++i) {
    const ParamSlot& s = net->params[i];
    if (!s.set) {
      set_error("holo_unet_adam_step: parameter '%s' was never bound (holo_unet_set_param)", s.name.c_str());
      return HOLO_E_STATE;
    }
    if (tensors[i].numel != s.numel || !tensors[i].param) {
      set_error("holo_unet_adam_step: tensor %d must be '%s' with %lld elements", i, s.name.c_str(), (long long)s.numel);
      return HOLO_E_INVALID;
    }
  }
  // (a) the update; a parameter the library keeps as a plain copy is written there by the same kernel
  if (net->adam_copies.size() != net->params.size()) {
    net->adam_copies.clear();
    for (const ParamSlot& s : net->params) net->adam_copies.push_back(s.is_conv() ? nullptr : s.w.f32);
  }
  net->tape_valid = false;  // (d) the taped activations belong to the old weights
  if (adam_step_launch(tensors, net->adam_copies.data(), n, sc, clip_coef_dev, stream)) return HOLO_E_INVALID;
  for (int i = 0; i < n; ++i) {
    const ParamSlot& s = net->params[i];
    if (!s.is_conv()) continue;
    // (b) the forward packs, (c) the transposed-convolution packs that exist (a Downsample weight: "<name>" and "<name>#s1")
    if (const int rc = pack_conv_weights(tensors[i].param, s.w, stream)) return rc;
    if (net->dgrad.count(s.name) || net->dgrad.count(s.name + "#s1"))
      if (const int rc = prepare_dgrad_weight(net, s, tensors[i].param, stream)) return rc;
  }
  return 0;
}

int holo_ddpm_step(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, int batch,
                   int64_t elems_per_sample, const float* x_t, const float* model_out, const float* noise,
                   int clip_denoised, float* sample, float* pred_xstart, void* stream) {
  return step_entry("holo_ddpm_step",
                    tables && timesteps && x_t && model_out && noise && sample && pred_xstart && batch >= 1, [&] {
    return ddpm_step_launch(tables, num_timesteps, timesteps, batch, elems_per_sample, x_t, model_out, noise, clip_denoised,
                            sample, pred_xstart, stream);
  });
}

int holo_ddpm_step_philox(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, int batch,
                          int64_t elems_per_sample, const float* x_t, const float* model_out, uint64_t seed,
                          uint64_t stream_offset, int clip_denoised, float* sample, float* pred_xstart, float* noise_out,
                          int ncdhw_channels, void* stream) {
  return step_entry("holo_ddpm_step_philox", tables && timesteps && x_t && model_out && sample && batch >= 1, [&] {
    return ddpm_step_philox_launch(tables, num_timesteps, timesteps, batch, elems_per_sample, x_t, model_out, seed, nullptr,
                                   stream_offset, clip_denoised, sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

int holo_ddpm_step_philox_rows(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, int batch,
                               int64_t elems_per_sample, const float* x_t, const float* model_out, uint64_t seed,
                               const uint32_t* row_streams, uint32_t timestep_index, int clip_denoised, float* sample,
                               float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddpm_step_philox_rows",
                    tables && timesteps && x_t && model_out && row_streams && sample && batch >= 1, [&] {
    return ddpm_step_philox_launch(tables, num_timesteps, timesteps, batch, elems_per_sample, x_t, model_out, seed,
                                   row_streams, timestep_index, clip_denoised, sample, pred_xstart, noise_out,
                                   ncdhw_channels, stream);
  });
}

// gaussian_diffusion.py:645-727 (ddim_sample / ddim_reverse_sample, the elementwise tail)
int holo_ddim_step(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                   const float* model_out, const float* noise, int clip_denoised, float* sample, float* pred_xstart,
                   void* stream) {
  return step_entry("holo_ddim_step", coefs && x_t && model_out && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_launch(coefs, batch, elems_per_sample, x_t, model_out, noise, clip_denoised, sample, pred_xstart, stream);
  });
}

// gaussian_diffusion.py:645-693 with the noise of :685 drawn in the kernel
int holo_ddim_step_philox(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                          const float* model_out, uint64_t seed, uint64_t stream_offset, int clip_denoised, float* sample,
                          float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddim_step_philox", coefs && x_t && model_out && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_philox_launch(coefs, batch, elems_per_sample, x_t, model_out, seed, nullptr, stream_offset, clip_denoised,
                                   sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

int holo_ddim_step_philox_rows(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                               const float* model_out, uint64_t seed, const uint32_t* row_streams, uint32_t timestep_index,
                               int clip_denoised, float* sample, float* pred_xstart, float* noise_out, int ncdhw_channels,
                               void* stream) {
  return step_entry("holo_ddim_step_philox_rows",
                    coefs && x_t && model_out && row_streams && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_philox_launch(coefs, batch, elems_per_sample, x_t, model_out, seed, row_streams, timestep_index,
                                   clip_denoised, sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

// DPM-Solver++ multistep update (the elementwise tail of ImplicitronGaussianDiffusion.dpm_sample_loop*)
int holo_dpm_step(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                  const float* model_out, const float* hist1, const float* hist2, int clip_denoised, float* sample,
                  float* pred_xstart, void* stream) {
  return step_entry("holo_dpm_step", coefs && x_t && model_out && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return dpm_step_launch(coefs, batch, elems_per_sample, x_t, model_out, hist1, hist2, clip_denoised, sample, pred_xstart,
                           stream);
  });
}

// gaussian_diffusion.py:429-433 (condition_mean) inside p_sample :499-506
int holo_ddpm_step_guided(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps, const float* variances,
                          int batch, int64_t elems_per_sample, const float* x_t, const float* model_out, const float* grad,
                          const float* noise, int clip_denoised, float* sample, float* pred_xstart, void* stream) {
  return step_entry("holo_ddpm_step_guided",
                    tables && timesteps && variances && x_t && model_out && grad && noise && sample && batch >= 1, [&] {
    return ddpm_step_guided_launch(tables, num_timesteps, timesteps, variances, batch, elems_per_sample, x_t, model_out, grad,
                                   noise, clip_denoised, sample, pred_xstart, stream);
  });
}

// the same with the noise of :498 drawn in the kernel; row_streams null: the offset form, else one stream per row
int holo_ddpm_step_guided_philox(HoloCtx*, const float* tables, int num_timesteps, const int64_t* timesteps,
                                 const float* variances, int batch, int64_t elems_per_sample, const float* x_t,
                                 const float* model_out, const float* grad, uint64_t seed, uint64_t stream_offset,
                                 const uint32_t* row_streams, uint32_t timestep_index, int clip_denoised, float* sample,
                                 float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddpm_step_guided_philox",
                    tables && timesteps && variances && x_t && model_out && grad && sample && batch >= 1, [&] {
    return ddpm_step_guided_philox_launch(tables, num_timesteps, timesteps, variances, batch, elems_per_sample, x_t, model_out,
                                          grad, seed, row_streams, row_streams ? (uint64_t)timestep_index : stream_offset,
                                          clip_denoised, sample, pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

// gaussian_diffusion.py:445-453 (condition_score) followed by ddim_sample :674-693
int holo_ddim_step_guided(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                          const float* model_out, const float* grad, const float* noise, int clip_denoised, float* sample,
                          float* pred_xstart, void* stream) {
  return step_entry("holo_ddim_step_guided",
                    coefs && x_t && model_out && grad && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_guided_launch(coefs, batch, elems_per_sample, x_t, model_out, grad, noise, clip_denoised, sample,
                                   pred_xstart, stream);
  });
}

// the same with the noise of :685 drawn in the kernel; row_streams as holo_ddpm_step_guided_philox
int holo_ddim_step_guided_philox(HoloCtx*, const float* coefs, int batch, int64_t elems_per_sample, const float* x_t,
                                 const float* model_out, const float* grad, uint64_t seed, uint64_t stream_offset,
                                 const uint32_t* row_streams, uint32_t timestep_index, int clip_denoised, float* sample,
                                 float* pred_xstart, float* noise_out, int ncdhw_channels, void* stream) {
  return step_entry("holo_ddim_step_guided_philox",
                    coefs && x_t && model_out && grad && sample && batch >= 1 && elems_per_sample >= 4, [&] {
    return ddim_step_guided_philox_launch(coefs, batch, elems_per_sample, x_t, model_out, grad, seed, row_streams,
                                          row_streams ? (uint64_t)timestep_index : stream_offset, clip_denoised, sample,
                                          pred_xstart, noise_out, ncdhw_channels, stream);
  });
}

int holo_tanh(HoloCtx* ctx, const float* x, float* y, int64_t n, void* stream) {
  (void)ctx;
  return tanh_launch(x, y, n, stream);
}
int holo_clip(HoloCtx* ctx, const float* x, float* y, float lo, float hi, int64_t n, void* stream) {
  (void)ctx;
  return clip_launch(x, y, lo, hi, n, stream);
}

int holo_event_timer_create(void** timer) {
  hipEvent_t* ev = new hipEvent_t[2];
  if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
    set_error("hipEventCreate failed");
    return HOLO_E_HIP;
  }
  *timer = ev;
  return 0;
}
int holo_event_timer_start(void* timer, void* stream) {
  HIP_TRY(hipEventRecord(((hipEvent_t*)timer)[0], (hipStream_t)stream));
  return 0;
}
int holo_event_timer_stop(void* timer, void* stream, float* elapsed_ms) {
  hipEvent_t* ev = (hipEvent_t*)timer;
  HIP_TRY(hipEventRecord(ev[1], (hipStream_t)stream));
  HIP_TRY(hipEventSynchronize(ev[1]));
  HIP_TRY(hipEventElapsedTime(elapsed_ms, ev[0], ev[1]));
  return 0;
}
int holo_event_timer_destroy(void* timer) {
  hipEvent_t* ev = (hipEvent_t*)timer;
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  delete[] ev;
  return 0;
}

}  // extern "C"
