// The context behind the C ABI (include/neptune_hip.h) and the staging of its host-buffer calls,
// shared by capi.hip and ms_capi.hip.
//
// One nhip_ctx = one GPU, one non-blocking HIP stream, a grow-only device workspace for the
// host-buffer entry points, and an optional event timer around every kernel launch.  Calls on
// one context are serialized by a mutex (the reference calls verify() concurrently from many
// tokio tasks: neptune-core/src/protocol/proof_abstractions/verifier.rs:60-63).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/neptune_hip.h"
#include "device_scope.hpp"
#include "host_numa.hpp"
#include "stage_layout.hpp"

struct nhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    void* ws = nullptr;  // workspace for host-buffer calls
    size_t ws_bytes = 0;
    void* staging = nullptr;  // pinned host staging for batch uploads (grow-only, under mu)
    size_t staging_bytes = 0;
    void* verify_scratch = nullptr;  // reusable device / stream resources of nhip_verify_batch
    void (*verify_scratch_free)(void*) = nullptr;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;  // recorded, not yet read
    std::vector<hipEvent_t> free_events;
    double timed_ms = 0.0;
    uint64_t timed_launches = 0;
    nhip::HostTopo topo;       // the GPU's NUMA node and its CPUs (host_numa.cpp)
    unsigned host_threads = 0;  // staging copy threads per upload (0: the default)
};

namespace nhip {

inline int hip_fail(hipError_t e) {
    if (e == hipSuccess) return NHIP_OK;
    if (e == hipErrorOutOfMemory) return NHIP_ERR_OOM;
    return NHIP_ERR_HIP;
}

inline hipEvent_t take_event(nhip_ctx* c) {
    if (!c->free_events.empty()) {
        hipEvent_t e = c->free_events.back();
        c->free_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Launch helper: brackets the launch with events when timing is on.
template <class F>
int timed_launch(nhip_ctx* c, F&& f) {
    hipEvent_t a = nullptr, b = nullptr;
    if (c->timing) {
        a = take_event(c);
        b = take_event(c);
        if (a && b) (void)hipEventRecord(a, c->stream);
    }
    hipError_t e = f();
    if (c->timing && a && b) {
        (void)hipEventRecord(b, c->stream);
        c->pending.emplace_back(a, b);
    }
    return hip_fail(e);
}

inline int ensure_ws(nhip_ctx* c, size_t bytes) {
    if (bytes <= c->ws_bytes) return NHIP_OK;
    if (c->ws) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(c->ws);
        c->ws = nullptr;
        c->ws_bytes = 0;
    }
    size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    hipError_t e = hipMalloc(&c->ws, want);
    if (e != hipSuccess) return hip_fail(e);
    c->ws_bytes = want;
    return NHIP_OK;
}

// One host-buffer call: it holds c->mu and makes the context's device current while it lives.
// Declare every buffer once by binding the device pointer that will name it: in(dev, src, count)
// with its host source, tmp(dev, count) for scratch and outputs.  commit() lays them out
// (StageLayout), sets the bound pointers and enqueues the uploads in declaration order; then
// step() / launch() / out(), and return finish().  The first error sticks and everything after it
// is skipped; finish() drains the stream on every path once anything was enqueued (the sources may
// be the call's own temporaries).  A HIP error is NHIP_ERR_HIP or NHIP_ERR_OOM, never a verdict.
class Stage {
  public:
    explicit Stage(nhip_ctx* c) : c_(c), lock_(c->mu), device_scope_(c->device) {}

    // dev: count * per elements, uploaded from src (nothing when that is zero bytes); null until commit()
    template <class D, class T>
    void in(D*& dev, const T* src, size_t count, size_t per = 1) {
        static_assert(std::is_same<typename std::remove_const<D>::type, T>::value, "element types differ");
        tmp(dev, count, per);
        if (!lay_.overflow) slot_[lay_.n - 1].src = src;
    }
    template <class T>
    void tmp(T*& dev, size_t count, size_t per = 1) {
        dev = nullptr;
        const unsigned i = lay_.add(count, per, sizeof(T));
        if (!lay_.overflow) slot_[i] = Slot{&dev, [](void* d, char* p) { *static_cast<T**>(d) = reinterpret_cast<T*>(p); }, nullptr};
    }

    int commit() {
        if (lay_.overflow) return rc_ = NHIP_ERR_OOM;  // before the device is touched
        if ((rc_ = ensure_ws(c_, lay_.total)) != NHIP_OK) return rc_;
        char* base = static_cast<char*>(c_->ws);
        for (unsigned i = 0; i < lay_.n; ++i) slot_[i].set(slot_[i].dev, base + lay_.off[i]);
        for (unsigned i = 0; i < lay_.n; ++i)
            if (slot_[i].src) copy(base + lay_.off[i], slot_[i].src, lay_.bytes[i], hipMemcpyHostToDevice);
        return rc_;
    }

    // An upload that has to follow other work of the call (else: in())
    template <class T>
    void up(T* dev, const T* src, size_t count) {
        copy(dev, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
    // Read back count elements of dev from elem_offset on
    template <class T>
    void out(T* host_dst, const T* dev, size_t count, size_t elem_offset = 0) {
        copy(host_dst, dev + elem_offset, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    // f enqueues on the stream and returns an NHIP_* code
    template <class F>
    void step(F&& f) {
        if (rc_ != NHIP_OK) return;
        enqueued_ = true;
        rc_ = f();
    }
    // f launches a kernel and returns a hipError_t
    template <class F>
    void launch(F&& f) {
        step([&] { return timed_launch(c_, f); });
    }

    int finish() {
        const hipError_t es = enqueued_ ? hipStreamSynchronize(c_->stream) : hipSuccess;
        return rc_ != NHIP_OK ? rc_ : hip_fail(es);
    }

  private:
    struct Slot {
        void* dev;                  // the bound T*
        void (*set)(void*, char*);  // *(T**)dev = (T*)address
        const void* src;            // host source, or null
    };
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (bytes) step([&] { return hip_fail(hipMemcpyAsync(dst, src, bytes, kind, c_->stream)); });
    }

    nhip_ctx* c_;
    const std::lock_guard<std::mutex> lock_;
    const DeviceScope device_scope_;
    StageLayout lay_;
    Slot slot_[STAGE_MAX_BUFS];
    int rc_ = NHIP_OK;
    bool enqueued_ = false;
};

}  // namespace nhip
