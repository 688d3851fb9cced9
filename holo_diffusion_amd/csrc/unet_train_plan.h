// unet_train_plan.h — TrainPlanner: builds the training plan (TrainPlan, unet_plan.h) of one (description, transposed-weight
// table, batch, workspace base): the forward with every intermediate kept and every layer recorded (Planner with a tape),
// then the backward as a list of BwdOp values in reverse layer order.  fp32 mode only.  Host-only arithmetic like Planner
// (definitions in unet_train_plan.cpp): tests/cpu/unet_plan_check.cpp builds training plans and checks them on the CPU.
//   * dgrad of a stride-1 convolution = the forward conv kernels on the flipped / transposed weights
//     (holo_unet_set_dgrad_weight);  Downsample: conv_dgrad_s2_kernel;  Upsample: dgrad at the fine size + sumpool2
//   * wgrad: conv_wgrad_kernel re-applies GroupNorm . FiLM . SiLU to the raw input like the forward's staging does
//   * GroupNorm (+ FiLM + SiLU): gn_bwd_launch;  attention: batched fp32 MFMA GEMMs around the softmax rows
// Gradients of activations are allocated on first use and ACCUMULATED by later consumers (skip connections, the
// identity branches of ResBlock / AttentionBlock).  Parameter gradients live in the workspace in the reference's layouts.
#pragma once
#include "unet_plan.h"

namespace holo {
namespace unetplan {

// name -> the transposed weights of a convolution, packed like the forward ones ([Cin][Cout] flipped taps for the stride-1
// convs; [tap][Cout][Cin] for the stride-2 Downsample convs, whose stride-1 form lives under "<name>#s1")
typedef std::map<std::string, ConvWeights> DgradTable;

struct TrainPlanner {
  const UnetDesc* u;        // read only: everything a build produces goes into `tp`
  const DgradTable& dgrad;  // read only; its owner (the handle) keeps the buffers it points to
  int N;
  TrainPlan& tp;
  Planner pl;
  std::vector<Tape> tape;
  std::vector<BwdOp>& bops;                         // tp.bops
  std::map<size_t, std::pair<size_t, bool>> grads;  // activation offset -> (gradient offset, already written)
  std::string err;                                  // why the plan cannot be built (ensure_train_plan reports it)

  TrainPlanner(const UnetDesc* u_, const DgradTable& dgrad_, int N_, void* ws, TrainPlan& tp_);
  void build();  // on failure `err` is set and tp is of no use

  template <class T>
  T* ptr(size_t off) {
    return pl.ptr<T>(off);
  }
  size_t alloc(size_t bytes) { return pl.scratch_alloc(bytes); }
  int64_t vox(int R) const { return (int64_t)R * R * R; }
  // gradient buffer of an activation; `acc` tells the caller whether to accumulate (a consumer wrote it before)
  // (all bookkeeping is in workspace OFFSETS: a sizing pass has no workspace, and Planner::ptr forms addresses from integers,
  // never by arithmetic on a null pointer - undefined behaviour that an optimising compiler does exploit)
  static constexpr size_t NONE = ~(size_t)0;
  size_t grad_of(const Act& a, int* acc);
  size_t grad_ready(const Act& a);  // gradient of a layer OUTPUT: must have been written by its consumers
  float* pgrad(const std::string& name);
  std::optional<ConvWeights> find_dgw(const std::string& name);
  std::optional<ConvWeights> dgw(const std::string& name);

  void emit_dgrad(size_t gy_off, int cout, int R, const std::string& wname, int cin, int ksz, size_t out_off, bool accumulate = false);
  void emit_wgrad(size_t gy_off, const ConvDesc& f, const std::string& layer);
  void emit_add(float* dst, const float* src, int64_t n, int acc);
  struct FilmGrad {  // a FiLM-modulated GroupNorm: the rows it was modulated with, and where their gradient goes
    const float* film;
    int cout;
    float* dfilm;
  };
  void bwd_norm_conv(size_t gy_off, const ConvDesc& f, const std::string& layer, const std::string& norm, size_t mom,
                     const FilmGrad* film = nullptr);
  void bwd_res(const Tape& t, float* dfilm_base);
  void bwd_attn(const Tape& t);
  void bwd_conv(const Tape& t);  // input conv / Downsample / Upsample / output head
};

}  // namespace unetplan
}  // namespace holo
