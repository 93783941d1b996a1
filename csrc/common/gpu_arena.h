// GpuArena: the owner of an object's HIP resources -- device and pinned memory, events, streams
// and page-locked host ranges.  Every acquisition is recorded; the destructor releases what is
// left in reverse order of acquisition and ignores errors, so a constructor that throws half-way
// leaks nothing and no destructor keeps a free list in step with its allocations by hand.
//
// The handles returned are plain HIP handles: whoever holds the arena declares it BEFORE every
// member that uses them, so that it is destroyed after them.  An arena is not synchronised: one
// thread at a time (the encoders' frame slots have one each for that reason).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hip_check.h"

namespace mx {

class GpuArena {
   public:
    GpuArena() = default;
    GpuArena(const GpuArena&) = delete;
    GpuArena& operator=(const GpuArena&) = delete;
    ~GpuArena() {
        while (!held_.empty()) {
            free_one(held_.back());
            held_.pop_back();
        }
    }

    template <class T>
    T* device(size_t count) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, sizeof(T) * count));
        return static_cast<T*>(hold(kDevice, p));
    }
    // device() + hipMemsetAsync of the whole buffer to `byte` on stream s
    template <class T>
    T* device_fill(size_t count, int byte, hipStream_t s) {
        T* p = device<T>(count);
        HIP_CHECK(hipMemsetAsync(p, byte, sizeof(T) * count, s));
        return p;
    }
    template <class T>
    T* pinned(size_t count, unsigned flags) {
        void* p = nullptr;
        HIP_CHECK(hipHostMalloc(&p, sizeof(T) * count, flags));
        return static_cast<T*>(hold(kPinned, p));
    }
    hipEvent_t event(unsigned flags) {  // flags 0: as hipEventCreate
        hipEvent_t e = nullptr;
        HIP_CHECK(hipEventCreateWithFlags(&e, flags));
        return static_cast<hipEvent_t>(hold(kEvent, e));
    }
    hipStream_t stream(unsigned flags) {
        hipStream_t s = nullptr;
        HIP_CHECK(hipStreamCreateWithFlags(&s, flags));
        return static_cast<hipStream_t>(hold(kStream, s));
    }
    hipStream_t stream(unsigned flags, int priority) {
        hipStream_t s = nullptr;
        HIP_CHECK(hipStreamCreateWithPriority(&s, flags, priority));
        return static_cast<hipStream_t>(hold(kStream, s));
    }
    // a stream confined to the compute units set in `mask` (one bit per CU, 32 per word)
    hipStream_t stream_cu_mask(const std::vector<uint32_t>& mask) {
        hipStream_t s = nullptr;
        HIP_CHECK(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
        return static_cast<hipStream_t>(hold(kStream, s));
    }
    // a host range hipHostRegister succeeded on: unregistered with the rest
    void registered(void* p) { hold(kRegistered, p); }

    // Frees one handle now (memory, event or stream) and forgets it; a handle the arena does not
    // hold is left alone.
    void release(const void* handle) {
        for (size_t i = held_.size(); i-- > 0;)
            if (held_[i].handle == handle) {
                free_one(held_[i]);
                held_.erase(held_.begin() + (std::ptrdiff_t)i);
                return;
            }
    }

    // Handles held by all arenas of the process at this moment.
    static long live() { return live_.load(); }

   private:
    enum Kind : uint8_t { kDevice, kPinned, kEvent, kStream, kRegistered };
    struct Held {
        Kind kind;
        void* handle;
    };
    void* hold(Kind k, void* h) {
        ++live_;
        try {
            held_.push_back(Held{k, h});
        } catch (...) {  // out of host memory with the handle in hand
            free_one(Held{k, h});
            throw;
        }
        return h;
    }
    static void free_one(const Held& h) {
        switch (h.kind) {
            case kDevice: (void)hipFree(h.handle); break;
            case kPinned: (void)hipHostFree(h.handle); break;
            case kEvent: (void)hipEventDestroy(static_cast<hipEvent_t>(h.handle)); break;
            case kStream: (void)hipStreamDestroy(static_cast<hipStream_t>(h.handle)); break;
            case kRegistered: (void)hipHostUnregister(h.handle); break;
        }
        --live_;
    }
    std::vector<Held> held_;
    inline static std::atomic<long> live_{0};
};

}  // namespace mx
