// dev_owner.h — what one slot of a matcher handle made on the GPU, released in one place (elas_api.cpp, sgm.hip, bm.hip).  Product code.
//
// Every allocation, event and stream a slot makes goes through its DevOwner, which records it; release() gives everything back in reverse
// order.  A call that fails records nothing and leaves the caller's pointer null, so a slot that fails half-way is released like a whole
// one.  The caller sets the device and makes sure nothing is in flight before release() (the handles join their workers / synchronise
// their streams first).  Not an allocator, and nothing is shared: whoever made a thing releases it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <vector>

namespace jnav {

class __attribute__((visibility("hidden"))) DevOwner {   // (hidden: the library exports its C ABI, not this)
 public:
  template <typename T>
  hipError_t alloc(T** p, size_t count) { return alloc_bytes(reinterpret_cast<void**>(p), count * sizeof(T)); }
  hipError_t alloc_bytes(void** p, size_t bytes) { return keep(hipMalloc(p, bytes), DEVICE, p); }
  template <typename T>
  hipError_t pinned(T** p, size_t count) {
    return keep(hipHostMalloc(reinterpret_cast<void**>(p), count * sizeof(T), hipHostMallocDefault), PINNED, reinterpret_cast<void**>(p));
  }
  // signal memory: a word that hipStreamWaitValue32 can wait on and the host writes
  hipError_t signal(uint32_t** p, size_t bytes) {
    return keep(hipExtMallocWithFlags(reinterpret_cast<void**>(p), bytes, hipMallocSignalMemory), DEVICE, reinterpret_cast<void**>(p));
  }
  hipError_t event(hipEvent_t* e, unsigned flags = hipEventDefault) { return keep(hipEventCreateWithFlags(e, flags), EVENT, reinterpret_cast<void**>(e)); }
  hipError_t stream(hipStream_t* s, unsigned flags) { return keep(hipStreamCreateWithFlags(s, flags), STREAM, reinterpret_cast<void**>(s)); }
  hipError_t stream(hipStream_t* s, unsigned flags, int priority) {
    return keep(hipStreamCreateWithPriority(s, flags, priority), STREAM, reinterpret_cast<void**>(s));
  }

  void release() {
    for (size_t i = made_.size(); i-- > 0;) {
      void* p = made_[i].p;
      switch (made_[i].kind) {
        case DEVICE: (void)hipFree(p); break;
        case PINNED: (void)hipHostFree(p); break;
        case EVENT: (void)hipEventDestroy(static_cast<hipEvent_t>(p)); break;
        case STREAM: (void)hipStreamDestroy(static_cast<hipStream_t>(p)); break;
      }
    }
    made_.clear();
  }

 private:
  enum Kind { DEVICE, PINNED, EVENT, STREAM };
  struct Made { Kind kind; void* p; };
  std::vector<Made> made_;

  hipError_t keep(hipError_t e, Kind kind, void** p) {
    if (e == hipSuccess) made_.push_back(Made{kind, *p});
    else *p = nullptr;
    return e;
  }
};

}  // namespace jnav
