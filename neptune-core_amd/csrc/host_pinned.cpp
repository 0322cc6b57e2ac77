// Pinned host ranges handed out by nhip_host_alloc / registered by nhip_host_register: proofs and
// wire bytes that live in one are DMA'd to the device straight from the caller's memory (no staging
// copy).  The batch fill (stark_host.cpp) asks through pinned_contains, capi.hip and chain_capi.hip
// through nhip_internal_is_pinned.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "stark_host_internal.hpp"

namespace {

struct PinnedRanges {
    std::mutex mu;
    std::vector<std::pair<uintptr_t, size_t>> r;  // (start, bytes)
    bool contains(const void* p, size_t bytes) {
        const uintptr_t a = (uintptr_t)p;
        std::lock_guard<std::mutex> g(mu);
        for (const auto& x : r)
            if (a >= x.first && a + bytes <= x.first + x.second && a + bytes >= a) return true;
        return false;
    }
};
PinnedRanges& pinned() {
    static PinnedRanges p;
    return p;
}

bool pinned_remember(void* p, size_t bytes) {
    try {
        std::lock_guard<std::mutex> g(pinned().mu);
        pinned().r.emplace_back((uintptr_t)p, bytes);
    } catch (const std::bad_alloc&) {
        return false;
    }
    return true;
}

bool pinned_forget(void* p) {
    std::lock_guard<std::mutex> g(pinned().mu);
    auto& r = pinned().r;
    for (size_t i = 0; i < r.size(); ++i)
        if (r[i].first == (uintptr_t)p) {
            r.erase(r.begin() + (ptrdiff_t)i);
            return true;
        }
    return false;
}

// The tail of both allocators: remember the new range, or free it.
int alloc_done(hipError_t e, void* p, size_t bytes, void** out) {
    if (e != hipSuccess) return NHIP_ERR_OOM;
    if (!pinned_remember(p, bytes)) {
        (void)hipHostFree(p);
        return NHIP_ERR_OOM;
    }
    *out = p;
    return NHIP_OK;
}

}  // namespace

bool nhip::pinned_contains(const void* p, size_t bytes) { return pinned().contains(p, bytes); }

extern "C" {

int nhip_host_alloc(size_t bytes, void** out) {
    if (!out) return NHIP_ERR_ARG;
    *out = nullptr;
    void* p = nullptr;
    return alloc_done(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable), p, bytes, out);
}

int nhip_host_alloc_near(nhip_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return NHIP_ERR_ARG;
    *out = nullptr;
    void* p = nullptr;
    return alloc_done(nhip::host_malloc_on(&p, bytes ? bytes : 1, nhip::ctx_topo(ctx).numa_node, hipHostMallocPortable),
                      p, bytes, out);
}

int nhip_host_free(void* p) {
    if (!p) return NHIP_OK;
    if (!pinned_forget(p)) return NHIP_ERR_ARG;
    return nhip::hipfail(hipHostFree(p));
}

int nhip_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return NHIP_ERR_ARG;
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) return nhip::hipfail(e);
    if (!pinned_remember(p, bytes)) {
        (void)hipHostUnregister(p);
        return NHIP_ERR_OOM;
    }
    return NHIP_OK;
}

int nhip_host_unregister(void* p) {
    if (!p || !pinned_forget(p)) return NHIP_ERR_ARG;
    return nhip::hipfail(hipHostUnregister(p));
}

// capi.hip (nhip_le_words_gpu), chain_capi.hip: is the range pinned host memory this library knows of?
int nhip_internal_is_pinned(const void* p, size_t bytes) { return pinned().contains(p, bytes) ? 1 : 0; }

}  // extern "C"
