// wg_device.h -- the one home of per-device library state (resident tables,
// launch configuration, the timeout record): a record per HIP device, made on
// first use.  Needs no HIP: the host-only translation units use it too.  The
// device a call belongs to comes from its stream (wg_common.h call_device).
#pragma once
#include <mutex>

namespace wg {

constexpr int kMaxDevices = 64;

template <class T>
class PerDevice {
 public:
  // Device dev's record, made by init(T&) -> bool, which runs under the lock
  // and at most once per device.  A failed init leaves the slot empty (the
  // next call runs it again on the same record) and, like a dev outside
  // [0, kMaxDevices), gives nullptr.
  template <class Init>
  T* get(int dev, Init&& init) {
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    std::lock_guard<std::mutex> lock(mu_);
    if (!made_[dev]) made_[dev] = init(records_[dev]);
    return made_[dev] ? &records_[dev] : nullptr;
  }
  // fn(T&) under the same lock, for a record that changes after it is made
  // (or is made piecewise: it starts value-initialised); not run for a dev
  // out of range.
  template <class Fn>
  void update(int dev, Fn&& fn) {
    if (dev < 0 || dev >= kMaxDevices) return;
    std::lock_guard<std::mutex> lock(mu_);
    fn(records_[dev]);
  }

 private:
  std::mutex mu_;
  T records_[kMaxDevices]{};
  bool made_[kMaxDevices]{};
};

}  // namespace wg
