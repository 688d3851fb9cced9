// host_params.h — the host-resident parameter set of a handle whose weights are folded on the host (HoloRenderer,
// HoloMlpMeanPooler): HostParams holds the raw parameters by reference name, HostGrads the parameter gradients of the last
// backward.  `entry` is the ABI function the error texts name.
#pragma once
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "holo_common.h"
#include "holo_kernels.h"

namespace holo {

class HostParams {
 public:
  void declare(const char* name, std::vector<int64_t> shape) { expected_[name] = std::move(shape); }
  // checks the shape, copies the fp32 tensor at dev_ptr to the host and synchronises
  int set(const char* entry, const char* name, const void* dev_ptr, int ndim, const int64_t* shape, void* stream) {
    auto it = expected_.find(name);
    if (it == expected_.end()) {
      set_error("%s: unknown parameter '%s'", entry, name);
      return HOLO_E_INVALID;
    }
    bool ok = ndim == (int)it->second.size();
    int64_t numel = 1;
    for (int i = 0; ok && i < ndim; ++i) {
      ok = shape[i] == it->second[i];
      numel *= shape[i];
    }
    if (!ok) {
      set_error("%s: shape mismatch for '%s'", entry, name);
      return HOLO_E_INVALID;
    }
    std::vector<float>& h = host_[name];
    h.resize((size_t)numel);
    HIP_TRY(hipMemcpyAsync(h.data(), dev_ptr, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  }
  // the first declared parameter that has not been set, or null
  const char* first_missing() const {
    for (auto& kv : expected_)
      if (!host_.count(kv.first)) return kv.first.c_str();
    return nullptr;
  }
  const std::vector<float>& operator[](const char* name) const { return host_.at(name); }

 private:
  std::map<std::string, std::vector<float>> host_;
  std::map<std::string, std::vector<int64_t>> expected_;
};

class HostGrads {
 public:
  explicit HostGrads(const char* backward_entry) : backward_(backward_entry) {}
  void put(const char* name, std::vector<float> values) { host_[name] = std::move(values); }
  // ONE device image of all gradients per backward (64-float slots, grown on demand): fetch copies out of it on the
  // device (a per-parameter host->device copy of a 3-float bias would be the tiny-copy pattern holo_ld_sys exists for)
  int publish(void* stream) {
    size_t total = 0;
    off_.clear();
    for (auto& kv : host_) {
      off_[kv.first] = total;
      total += (kv.second.size() + 63) & ~(size_t)63;
    }
    if (total > dev_floats_) {
      release();
      HIP_TRY(hipMalloc((void**)&dev_, total * sizeof(float)));
      dev_floats_ = total;
    }
    std::vector<float> pack(total, 0.f);
    for (auto& kv : host_) memcpy(pack.data() + off_[kv.first], kv.second.data(), kv.second.size() * sizeof(float));
    HIP_TRY(hipMemcpyAsync(dev_, pack.data(), total * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  }
  int fetch(const char* entry, const char* name, float* out_dev, int64_t numel, void* stream) const {
    auto it = host_.find(name);
    if (it == host_.end()) {
      set_error("%s: no gradient for '%s' (run %s first)", entry, name, backward_);
      return HOLO_E_STATE;
    }
    if ((int64_t)it->second.size() != numel) {
      set_error("%s: '%s' has %lld elements, not %lld", entry, name, (long long)it->second.size(), (long long)numel);
      return HOLO_E_INVALID;
    }
    auto off = off_.find(name);
    if (!dev_ || off == off_.end()) {
      set_error("%s: no device image of the gradients (run %s first)", entry, backward_);
      return HOLO_E_STATE;
    }
    return copy_sys_launch(dev_ + off->second, out_dev, numel, stream) ? HOLO_E_INVALID : 0;
  }
  void clear() { host_.clear(), off_.clear(); }
  void release() {  // the device image (the handle's destroy entry)
    if (dev_) (void)hipFree(dev_);
    dev_ = nullptr;
    dev_floats_ = 0;
  }

 private:
  const char* backward_;
  std::map<std::string, std::vector<float>> host_;
  std::map<std::string, size_t> off_;
  float* dev_ = nullptr;
  size_t dev_floats_ = 0;
};

}  // namespace holo
