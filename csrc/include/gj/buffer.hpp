// Scoped ownership of memory obtained from a Device.
//
// DevBuf<T> is what Device::alloc / alloc_pinned / alloc_pinned_coherent return, owned: move-only,
// empty by default, released through the matching Device call when it goes out of scope, is reset()
// or is assigned over.  It converts to T* so that a handle stands wherever the raw pointer stood.
// Device::release and release_pinned return only once the device is idle (gj/device.hpp), so a handle
// may go while work that uses it is still enqueued -- also when an exception unwinds past it.
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>

#include "gj/device.hpp"

namespace gj {

template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  // `count` elements (bytes for T = void).  A label names the allocation in schedule-check reports.
  static DevBuf device(Device& dev, size_t count, const char* label = nullptr) {
    return DevBuf(dev, dev.alloc(bytes_of(count)), false, label);
  }
  static DevBuf pinned(Device& dev, size_t count, const char* label = nullptr) {
    return DevBuf(dev, dev.alloc_pinned(bytes_of(count)), true, label);
  }
  static DevBuf pinned_coherent(Device& dev, size_t count, const char* label = nullptr) {
    return DevBuf(dev, dev.alloc_pinned_coherent(bytes_of(count)), true, label);
  }
  DevBuf(DevBuf&& o) noexcept : dev_(o.dev_), p_(std::exchange(o.p_, nullptr)), pinned_(o.pinned_) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      dev_ = o.dev_;
      p_ = std::exchange(o.p_, nullptr);
      pinned_ = o.pinned_;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (!p_) return;
    T* p = std::exchange(p_, nullptr);
    if (pinned_)
      dev_->release_pinned(p);
    else
      dev_->release(p);
  }

 private:
  // owns p before the label call, so that nothing is lost if that call throws
  DevBuf(Device& dev, void* p, bool pinned, const char* label) : dev_(&dev), p_(static_cast<T*>(p)), pinned_(pinned) {
    if (label) dev.label(p, label);
  }
  static size_t bytes_of(size_t count) {
    if constexpr (std::is_void_v<T>)
      return count;
    else
      return count * sizeof(T);
  }
  Device* dev_ = nullptr;
  T* p_ = nullptr;
  bool pinned_ = false;
};

// Waits for the device when the scope ends, errors swallowed.  Declared after the buffers of a scope,
// it runs before they are released: the scope's enqueued work has finished, or failed quietly, first.
struct DrainOnExit {
  Device& dev;
  ~DrainOnExit() {
    try {
      dev.sync_all();
    } catch (...) {
    }
  }
};

}  // namespace gj
