// C-ABI layer of libneptune_hip.so (declarations: include/neptune_hip.h).
//
// One nhip_ctx = one GPU, one non-blocking HIP stream, a grow-only device workspace for the
// host-buffer entry points, and an optional event timer around every kernel launch.  Calls on
// one context are serialized by a mutex (the reference calls verify() concurrently from many
// tokio tasks: neptune-core/src/protocol/proof_abstractions/verifier.rs:60-63).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/neptune_hip.h"
#include "device_scope.hpp"
#include "host_numa.hpp"
#include "kernels.hpp"
#include "ms_shape.hpp"
#include "wire.hpp"

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

namespace {

int hip_fail(hipError_t e) {
    if (e == hipSuccess) return NHIP_OK;
    if (e == hipErrorOutOfMemory) return NHIP_ERR_OOM;
    return NHIP_ERR_HIP;
}

hipEvent_t take_event(nhip_ctx* c) {
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

int ensure_ws(nhip_ctx* c, size_t bytes) {
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

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// Carve a list of sizes out of the workspace.
template <size_t N>
int carve(nhip_ctx* c, const size_t (&sizes)[N], void* (&ptrs)[N]) {
    size_t total = 0;
    for (size_t i = 0; i < N; ++i) total += align_up(sizes[i] ? sizes[i] : 1);
    int rc = ensure_ws(c, total);
    if (rc) return rc;
    char* base = (char*)c->ws;
    size_t off = 0;
    for (size_t i = 0; i < N; ++i) {
        ptrs[i] = base + off;
        off += align_up(sizes[i] ? sizes[i] : 1);
    }
    return NHIP_OK;
}

// Batch verdict: any_bad |= (v[i] != 1) over n bytes; 16 B per lane per step, one atomic per wave.
__global__ void __launch_bounds__(256) k_any_bad(const uint8_t* __restrict__ v, size_t n, uint32_t* __restrict__ any_bad) {
    uint32_t bad = 0;
    const size_t n16 = (reinterpret_cast<uintptr_t>(v) & 15u) ? 0 : n / 16;  // unaligned: byte path
    const uint4* __restrict__ v16 = reinterpret_cast<const uint4*>(v);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 w = v16[i];
        bad |= (w.x ^ 0x01010101u) | (w.y ^ 0x01010101u) | (w.z ^ 0x01010101u) | (w.w ^ 0x01010101u);
    }
    for (size_t i = n16 * 16 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        bad |= (v[i] != 1) ? 1u : 0u;
    if (__any(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(any_bad, 1u);
}

int build_tree_dev(nhip_ctx* c, const uint64_t* d_leafs, size_t n, uint64_t* d_nodes) {
    // level 0: leafs -> nodes[n/2 .. n)
    int rc = timed_launch(c, [&] { return nhip::launch_mtree_level(d_leafs, d_nodes + 5 * (n / 2), n / 2, c->stream); });
    if (rc) return rc;
    for (size_t parents = n / 4; parents >= 1; parents /= 2) {
        rc = timed_launch(c, [&] {
            return nhip::launch_mtree_level(d_nodes + 5 * (2 * parents), d_nodes + 5 * parents, parents, c->stream);
        });
        if (rc) return rc;
    }
    hipError_t e = hipMemsetAsync(d_nodes, 0, 5 * sizeof(uint64_t), c->stream);
    return hip_fail(e);
}

bool is_pow2(size_t n) { return n >= 2 && (n & (n - 1)) == 0; }

}  // namespace

extern "C" {

// 2000: nhip_stark_params.input_form (the struct grew), nhip_set_fs_form, the streaming group
// 2100: nhip_stats.ms_row_hash_exec (the struct grew), the NUMA entry points (nhip_host_alloc_near,
// nhip_device_numa, nhip_numa_from_sysfs, nhip_cpulist_parse, nhip_host_page_node,
// nhip_set_host_threads)
// 2200: nhip_batch_set_launch_timing (per-dispatch timestamps off by default), nhip_batch_set_streams
// 2300: nhip_air_create_ex (compiler options instead of environment variables), nhip_set_climb_from_ops,
// the per-member proof arenas (nhip_arena_*, nhip_group_stream_submit_placed), nhip_queue_latencies,
// nhip_batch_set_graph
// 2400: the in-place feed path (nhip_span, nhip_le_words_gpu, nhip_wire_scan_*, nhip_verify_batch_wire,
// nhip_batch_prepare_wire, nhip_batch_refill_wire, nhip_group_stream_submit_wire)
// 2500: the mutator-set checks (nhip_mmr, nhip_msa, nhip_ms_chunks, NHIP_MS_*, nhip_mmr_verify_batch,
// nhip_ms_can_remove_batch, nhip_ms_verify_batch)
// 2600: batched mutator-set updates (nhip_ms_apply_in, nhip_ms_apply_out, nhip_ms_apply_batch, four NHIP_MS_*)
int nhip_abi_version(void) { return 2600; }

int nhip_set_fs_form(int form) { return nhip::set_fs_form(form) == 0 ? NHIP_OK : NHIP_ERR_ARG; }
int nhip_set_climb_from_ops(int64_t ops) { return nhip::set_climb_from_ops(ops) == 0 ? NHIP_OK : NHIP_ERR_ARG; }

const char* nhip_strerror(int code) {
    switch (code) {
        case NHIP_OK: return "ok";
        case NHIP_ERR_NO_DEVICE: return "no HIP device";
        case NHIP_ERR_HIP: return "HIP runtime error";
        case NHIP_ERR_OOM: return "out of device memory";
        case NHIP_ERR_ARG: return "invalid argument";
        case NHIP_ERR_DECODE: return "malformed encoding";
        default: return "unknown error";
    }
}

int nhip_init(uint32_t device_mask, nhip_ctx** out) {
    if (!out) return NHIP_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NHIP_ERR_NO_DEVICE;
    int dev = 0;
    if (device_mask) {
        dev = __builtin_ctz(device_mask);
        if (dev >= count) return NHIP_ERR_NO_DEVICE;
    }
    nhip_ctx* c = new (std::nothrow) nhip_ctx();
    if (!c) return NHIP_ERR_OOM;
    c->device = dev;
    // the caller's current device is left as it was (a host with its own HIP user, e.g. torch,
    // must not find another device current after creating a context)
    int prev = -1;
    (void)hipGetDevice(&prev);
    const bool ok = hipSetDevice(dev) == hipSuccess &&
                    hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    if (!ok) {
        delete c;
        return NHIP_ERR_HIP;
    }
    try {
        c->topo = nhip::device_topo(dev);
    } catch (const std::bad_alloc&) {
        c->topo = nhip::HostTopo{};
    }
    *out = c;
    return NHIP_OK;
}

void nhip_destroy(nhip_ctx* c) {
    if (!c) return;
    const DeviceScope device_scope(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->pending) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    for (auto e : c->free_events) (void)hipEventDestroy(e);
    if (c->ws) (void)hipFree(c->ws);
    if (c->staging) (void)hipHostFree(c->staging);
    if (c->verify_scratch && c->verify_scratch_free) c->verify_scratch_free(c->verify_scratch);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int nhip_device_ordinal(const nhip_ctx* c) { return c ? c->device : -1; }

// internal accessors for the other translation units (not in the public header)
hipStream_t nhip_internal_stream(nhip_ctx* c) { return c->stream; }
int nhip_internal_device(nhip_ctx* c) { return c->device; }
std::mutex* nhip_internal_mutex(nhip_ctx* c) { return &c->mu; }
// The context's nhip_verify_batch scratch (created by `make` on first use, freed by `freefn` in
// nhip_destroy).
void* nhip_internal_verify_scratch(nhip_ctx* c, void* (*make)(), void (*freefn)(void*)) {
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->verify_scratch) {
        c->verify_scratch = make();
        c->verify_scratch_free = freefn;
    }
    return c->verify_scratch;
}
// Pinned staging of at least `bytes` (caller holds c->mu); nullptr if it cannot be pinned.
void* nhip_internal_staging(nhip_ctx* c, size_t bytes) {
    if (bytes <= c->staging_bytes) return c->staging;
    const size_t have = c->staging_bytes;
    if (c->staging) (void)hipHostFree(c->staging);
    c->staging = nullptr;
    c->staging_bytes = 0;
    // headroom, at least doubling: hipHostFree waits for the device, so a context whose batches
    // vary in size should stop reallocating after a few calls
    const size_t want = std::max(bytes + bytes / 4, 2 * have);
    // on the GPU's NUMA node: the copy threads (bound there) write it and the DMA reads it locally
    if (nhip::host_malloc_on(&c->staging, want, c->topo.numa_node, hipHostMallocDefault) != hipSuccess) {
        c->staging = nullptr;
        return nullptr;
    }
    c->staging_bytes = want;
    return c->staging;
}

const void* nhip_internal_topo(nhip_ctx* c) { return &c->topo; }  // a const nhip::HostTopo*
unsigned nhip_internal_host_threads(nhip_ctx* c) { return c->host_threads; }

int nhip_device_numa(nhip_ctx* c, int* numa_node, int* cpus, size_t cpu_cap, size_t* n_cpus) {
    if (!c || !numa_node) return NHIP_ERR_ARG;
    *numa_node = c->topo.numa_node;
    if (n_cpus) *n_cpus = c->topo.cpus.size();
    if (cpus)
        for (size_t i = 0; i < std::min(cpu_cap, c->topo.cpus.size()); ++i) cpus[i] = c->topo.cpus[i];
    return NHIP_OK;
}

int nhip_set_host_threads(nhip_ctx* c, unsigned threads) {
    if (!c || threads > 256) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->host_threads = threads;
    return NHIP_OK;
}

// ------------------------------------------------------------------ device-resident form
int nhip_dev_alloc(nhip_ctx* c, size_t bytes, void** dptr) {
    if (!c || !dptr) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    return hip_fail(hipMalloc(dptr, bytes ? bytes : 1));
}

int nhip_dev_free(nhip_ctx* c, void* d) {
    if (!c) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    (void)hipStreamSynchronize(c->stream);
    return hip_fail(hipFree(d));
}

int nhip_memcpy_h2d(nhip_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

int nhip_memcpy_d2h(nhip_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

int nhip_synchronize(nhip_ctx* c) {
    if (!c) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    return hip_fail(hipStreamSynchronize(c->stream));
}

int nhip_tip5_permutation_dev(nhip_ctx* c, uint64_t* d_states, size_t n) {
    if (!c || (n && !d_states)) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    return timed_launch(c, [&] { return nhip::launch_permutation(d_states, n, c->stream); });
}

int nhip_tip5_hash_pair_dev(nhip_ctx* c, const uint64_t* l, const uint64_t* r, size_t n, uint64_t* o) {
    if (!c || (n && (!l || !r || !o))) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    return timed_launch(c, [&] { return nhip::launch_hash_pair(l, r, o, n, c->stream); });
}

int nhip_tip5_hash_varlen_dev(nhip_ctx* c, const uint64_t* d, const uint64_t* off, size_t n, uint64_t* o) {
    if (!c || (n && (!off || !o))) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    return timed_launch(c, [&] { return nhip::launch_hash_varlen(d, off, n, o, c->stream); });
}

int nhip_mtree_build_dev(nhip_ctx* c, const uint64_t* d_leafs, size_t n, uint64_t* d_nodes) {
    if (!c || !is_pow2(n) || !d_leafs || !d_nodes) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    return build_tree_dev(c, d_leafs, n, d_nodes);
}

int nhip_mtree_verify_dev(nhip_ctx* c, const uint64_t* roots, size_t n_roots, const uint64_t* idx,
                          const uint64_t* leafs, const uint64_t* paths, uint32_t depth, size_t n, uint8_t* v) {
    if (!c || (n_roots != 1 && n_roots != n)) return NHIP_ERR_ARG;
    if (n && (!roots || !idx || !leafs || !v || (depth && !paths))) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    const int per_path = (n_roots == n && n != 1) ? 1 : 0;
    return timed_launch(c, [&] {
        return nhip::launch_mtree_verify(roots, per_path, idx, leafs, paths, depth, n, v, c->stream);
    });
}

int nhip_verdicts_all_dev(nhip_ctx* c, const uint8_t* d_v, size_t n, uint8_t* all_ok) {
    if (!c || !all_ok || (n && !d_v)) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    size_t sizes[1] = {sizeof(uint32_t)};
    void* p[1];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    uint32_t* d_out = (uint32_t*)p[0];
    hipError_t e = hipMemsetAsync(d_out, 0, sizeof(uint32_t), c->stream);
    if (e != hipSuccess) return hip_fail(e);
    size_t blocks = (n / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    rc = timed_launch(c, [&] {
        hipLaunchKernelGGL(k_any_bad, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_v, n, d_out);
        return hipGetLastError();
    });
    if (rc) return rc;
    uint32_t h = 1;
    e = hipMemcpyAsync(&h, d_out, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e);
    h = h ? 0u : 1u;
    *all_ok = (uint8_t)(h ? 1 : 0);
    return NHIP_OK;
}

// ------------------------------------------------------------------ host-buffer form
int nhip_tip5_permutation(nhip_ctx* c, uint64_t* states, size_t n) {
    if (!c || (n && !states)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    const size_t bytes = n * 16 * sizeof(uint64_t);
    size_t sizes[1] = {bytes};
    void* p[1];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p[0], states, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    rc = timed_launch(c, [&] { return nhip::launch_permutation((uint64_t*)p[0], n, c->stream); });
    if (rc) return rc;
    e = hipMemcpyAsync(states, p[0], bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

int nhip_tip5_hash_pair(nhip_ctx* c, const uint64_t* l, const uint64_t* r, size_t n, uint64_t* o) {
    if (!c || (n && (!l || !r || !o))) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    const size_t db = n * 5 * sizeof(uint64_t);
    size_t sizes[3] = {db, db, db};
    void* p[3];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p[0], l, db, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p[1], r, db, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    rc = timed_launch(c, [&] {
        return nhip::launch_hash_pair((const uint64_t*)p[0], (const uint64_t*)p[1], (uint64_t*)p[2], n, c->stream);
    });
    if (rc) return rc;
    e = hipMemcpyAsync(o, p[2], db, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

int nhip_tip5_hash_varlen(nhip_ctx* c, const uint64_t* data, const uint64_t* offsets, size_t n, uint64_t* o) {
    if (!c || (n && (!offsets || !o))) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return NHIP_ERR_ARG;
    const size_t total = (size_t)offsets[n];
    if (total && !data) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    size_t sizes[3] = {total * sizeof(uint64_t), (n + 1) * sizeof(uint64_t), n * 5 * sizeof(uint64_t)};
    void* p[3];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (total) e = hipMemcpyAsync(p[0], data, sizes[0], hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p[1], offsets, sizes[1], hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    rc = timed_launch(c, [&] {
        return nhip::launch_hash_varlen((const uint64_t*)p[0], (const uint64_t*)p[1], n, (uint64_t*)p[2], c->stream);
    });
    if (rc) return rc;
    e = hipMemcpyAsync(o, p[2], sizes[2], hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

int nhip_mtree_build(nhip_ctx* c, const uint64_t* leafs, size_t n, uint64_t* nodes_out) {
    if (!c || !is_pow2(n) || !leafs || !nodes_out) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    const size_t db = n * 5 * sizeof(uint64_t);
    size_t sizes[2] = {db, db};
    void* p[2];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p[0], leafs, db, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    rc = build_tree_dev(c, (const uint64_t*)p[0], n, (uint64_t*)p[1]);
    if (rc) return rc;
    e = hipMemcpyAsync(nodes_out, p[1], db, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

int nhip_mtree_verify(nhip_ctx* c, const uint64_t* roots, size_t n_roots, const uint64_t* idx,
                      const uint64_t* leafs, const uint64_t* paths, uint32_t depth, size_t n, uint8_t* v) {
    if (!c || (n_roots != 1 && n_roots != n)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!roots || !idx || !leafs || !v || (depth && !paths)) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    size_t sizes[5] = {n_roots * 5 * sizeof(uint64_t), n * sizeof(uint64_t), n * 5 * sizeof(uint64_t),
                       n * (size_t)depth * 5 * sizeof(uint64_t), n};
    void* p[5];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p[0], roots, sizes[0], hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p[1], idx, sizes[1], hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p[2], leafs, sizes[2], hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && depth) e = hipMemcpyAsync(p[3], paths, sizes[3], hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    const int per_path = (n_roots == n && n != 1) ? 1 : 0;
    rc = timed_launch(c, [&] {
        return nhip::launch_mtree_verify((const uint64_t*)p[0], per_path, (const uint64_t*)p[1],
                                         (const uint64_t*)p[2], (const uint64_t*)p[3], depth, n, (uint8_t*)p[4],
                                         c->stream);
    });
    if (rc) return rc;
    e = hipMemcpyAsync(v, p[4], n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

// ------------------------------------------------------------------ wire bytes -> words
int nhip_internal_is_pinned(const void* p, size_t bytes);  // stark_host.cpp

// The device counterpart of nhip_le_words: the spans' raw bytes uploaded run by run (wire.hpp), gathered
// by k_wire_words into one aligned word buffer (span i at the sum of the lengths before it), read back.
int nhip_le_words_gpu(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, const nhip_span* spans, size_t n,
                      uint64_t* out) {
    if (!c || (n_bytes && !bytes) || (n && !spans) || n > 0xFFFFFFFFull) return NHIP_ERR_ARG;
    if (!nhip::wire_spans_ok(spans, n, n_bytes)) return NHIP_ERR_ARG;
    try {
        std::vector<nhip::ProofIn> in(n);
        uint64_t total = 0;
        for (size_t i = 0; i < n; ++i) {
            in[i] = nhip::ProofIn{};
            in[i].off = total;
            in[i].len = spans[i].len;
            total += spans[i].len;
        }
        if (total == 0) return NHIP_OK;
        if (!out) return NHIP_ERR_ARG;
        nhip::WirePlan plan;
        nhip::wire_plan(bytes, spans, n, plan);
        std::lock_guard<std::mutex> g(c->mu);
        const DeviceScope device_scope(c->device);
        size_t sizes[4] = {plan.raw_bytes, n * 8, n * sizeof(nhip::ProofIn), (size_t)total * 8};
        void* p[4];
        int rc = carve(c, sizes, p);
        if (rc) return rc;
        bool any_pageable = false;
        for (const nhip::WireRun& r : plan.runs)
            any_pageable |= !nhip_internal_is_pinned(bytes + r.start, (size_t)(r.end - r.start));
        std::vector<uint8_t> pageable;
        uint8_t* stage = nullptr;
        if (any_pageable) {
            stage = (uint8_t*)nhip_internal_staging(c, plan.raw_bytes);
            if (!stage) {
                pageable.resize(plan.raw_bytes);
                stage = pageable.data();
            }
        }
        hipError_t e = nhip::wire_upload(plan, bytes, (uint8_t*)p[0], stage,
                                         [](const void* q, size_t b) { return nhip_internal_is_pinned(q, b) != 0; },
                                         c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(p[1], plan.boff.data(), sizes[1], hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(p[2], in.data(), sizes[2], hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);  // the sources are this call's
            return hip_fail(e);
        }
        rc = timed_launch(c, [&] {
            return nhip::launch_wire_words((const uint8_t*)p[0], (const uint64_t*)p[1], (const nhip::ProofIn*)p[2],
                                           (uint32_t)n, total, (uint64_t*)p[3], c->stream);
        });
        if (rc == NHIP_OK) e = hipMemcpyAsync(out, p[3], sizes[3], hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (rc) return rc;
        return hip_fail(e != hipSuccess ? e : es);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// ------------------------------------------------------------------ timing
int nhip_timing_enable(nhip_ctx* c, int on) {
    if (!c) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->timing = on != 0;
    return NHIP_OK;
}

int nhip_timing_read(nhip_ctx* c, double* total_ms, uint64_t* launches, int reset) {
    if (!c) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e);
    for (auto& pr : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) c->timed_ms += ms;
        c->timed_launches += 1;
        c->free_events.push_back(pr.first);
        c->free_events.push_back(pr.second);
    }
    c->pending.clear();
    if (total_ms) *total_ms = c->timed_ms;
    if (launches) *launches = c->timed_launches;
    if (reset) {
        c->timed_ms = 0.0;
        c->timed_launches = 0;
    }
    return NHIP_OK;
}

// MastHash::mast_hash (mast_hash.rs:22-39) for n objects of `fields` field sequences each:
// field sequence (i, f) = data[offsets[i*fields+f] .. offsets[i*fields+f+1]).
int nhip_mast_hash_batch(nhip_ctx* c, const uint64_t* data, const uint64_t* offsets, uint32_t fields, size_t n,
                         uint64_t* roots_out) {
    if (!c || fields < 1 || fields > 16 || (n && (!offsets || !roots_out))) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    const size_t nl = n * fields;
    for (size_t i = 0; i < nl; ++i)
        if (offsets[i + 1] < offsets[i]) return NHIP_ERR_ARG;
    const size_t total = (size_t)offsets[nl];
    if (total && !data) return NHIP_ERR_ARG;
    uint32_t pow2 = 1;
    while (pow2 < fields) pow2 <<= 1;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    size_t sizes[4] = {total * 8, (nl + 1) * 8, nl * 40, n * 40};
    void* p[4];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (total) e = hipMemcpyAsync(p[0], data, sizes[0], hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p[1], offsets, sizes[1], hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    rc = timed_launch(c, [&] {
        return nhip::launch_hash_varlen((const uint64_t*)p[0], (const uint64_t*)p[1], nl, (uint64_t*)p[2], c->stream);
    });
    if (rc) return rc;
    rc = timed_launch(c, [&] {
        return nhip::launch_mast_roots((const uint64_t*)p[2], fields, pow2, n, (uint64_t*)p[3], c->stream);
    });
    if (rc) return rc;
    e = hipMemcpyAsync(roots_out, p[3], sizes[3], hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

// AbsoluteIndexSet::compute (absolute_index_set.rs:86-113) for n removal records.
int nhip_absolute_index_sets(nhip_ctx* c, const uint64_t* items, const uint64_t* sender_randomness,
                             const uint64_t* receiver_preimages, const uint64_t* aocl_leaf_indices, size_t n,
                             uint64_t* minimum_out, uint32_t* distances_out) {
    if (!c || (n && (!items || !sender_randomness || !receiver_preimages || !aocl_leaf_indices || !minimum_out ||
                     !distances_out)))
        return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    std::vector<uint64_t> in(15 * n);
    for (size_t i = 0; i < n; ++i)
        for (int q = 0; q < 5; ++q) {
            in[15 * i + q] = items[5 * i + q];
            in[15 * i + 5 + q] = sender_randomness[5 * i + q];
            in[15 * i + 10 + q] = receiver_preimages[5 * i + q];
        }
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    size_t sizes[4] = {15 * n * 8, n * 8, 2 * n * 8, 45 * n * 4};
    void* p[4];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(p[0], in.data(), sizes[0], hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p[1], aocl_leaf_indices, sizes[1], hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e);
    rc = timed_launch(c, [&] {
        return nhip::launch_absolute_index_sets((const uint64_t*)p[0], (const uint64_t*)p[1], n, (uint64_t*)p[2],
                                                (uint32_t*)p[3], c->stream);
    });
    if (rc) return rc;
    e = hipMemcpyAsync(minimum_out, p[2], sizes[2], hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(distances_out, p[3], sizes[3], hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return hip_fail(e);
}

// ------------------------------------------------------------------ mutator-set checks
namespace {

// Host-to-device copies of one call; the first HIP error sticks and later copies are skipped.
struct Uploader {
    hipStream_t st;
    hipError_t e = hipSuccess;
    void operator()(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    }
};

// Ends a staged call: the stream is drained on every path (the sources may be this call's own
// temporaries), and a HIP error is never a verdict.
int ms_finish(nhip_ctx* c, int rc, hipError_t e) {
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    return hip_fail(e != hipSuccess ? e : es);
}

}  // namespace

// twenty-first MmrMembershipProof::verify for n (leaf, path) items against one MMR
// (application/loops/peer_loop.rs:1235, protocol/peer.rs:824; path shape archival_mmr.rs:250-281).
int nhip_mmr_verify_batch(nhip_ctx* c, const nhip_mmr* mmr, const uint64_t* leaf_index, const uint64_t* leaves,
                          const uint64_t* path_off, const uint64_t* path, size_t n, uint8_t* verdicts) {
    if (!c || nhip::ms_mmr_ok(mmr)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!leaf_index || !leaves || !verdicts || n > SIZE_MAX / 64) return NHIP_ERR_ARG;
    uint64_t pd = 0;
    if (nhip::ms_paths_ok(path_off, path, n, &pd)) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const DeviceScope device_scope(c->device);
    size_t sizes[6] = {(size_t)mmr->n_peaks * 40, n * 8, n * 40, (n + 1) * 8, (size_t)pd * 40, n};
    void* p[6];
    int rc = carve(c, sizes, p);
    if (rc) return rc;
    Uploader up{c->stream};
    up(p[0], mmr->peaks, sizes[0]);
    up(p[1], leaf_index, sizes[1]);
    up(p[2], leaves, sizes[2]);
    up(p[3], path_off, sizes[3]);
    up(p[4], path, sizes[4]);
    if (up.e != hipSuccess) return ms_finish(c, NHIP_OK, up.e);
    const nhip::MmrDev dm{(const uint64_t*)p[0], mmr->n_peaks, mmr->num_leafs};
    rc = timed_launch(c, [&] {
        return nhip::launch_mmr_verify(dm, (const uint64_t*)p[1], (const uint64_t*)p[2], (const uint64_t*)p[3],
                                       (const uint64_t*)p[4], n, (uint8_t*)p[5], c->stream);
    });
    hipError_t e = hipSuccess;
    if (rc == NHIP_OK) e = hipMemcpyAsync(verdicts, p[5], n, hipMemcpyDeviceToHost, c->stream);
    return ms_finish(c, rc, e);
}

// RemovalRecord::validate (removal_record.rs:202-251) and MutatorSetAccumulator::can_remove
// (mutator_set_accumulator.rs:187-222) for n records (block/mod.rs:816-822, transaction_kernel.rs:129,145):
// k_ms_chunk_auth over every dictionary entry, then k_ms_records.
int nhip_ms_can_remove_batch(nhip_ctx* c, const nhip_msa* msa, const uint64_t* minimum, const uint32_t* distances,
                             const nhip_ms_chunks* chunks, size_t n, uint8_t* valid, uint8_t* can_remove,
                             uint8_t* status) {
    if (!c || nhip::ms_msa_ok(msa)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!minimum || !distances || !valid || !can_remove || !status || n > SIZE_MAX / 256) return NHIP_ERR_ARG;
    nhip::MsChunkCounts cc;
    if (nhip::ms_chunks_ok(chunks, n, &cc)) return NHIP_ERR_ARG;
    try {
        // membership is order-free: the kernel searches a sorted copy of the active window
        std::vector<uint32_t> active(msa->active, msa->active + (msa->n_active ? msa->n_active : 0));
        std::sort(active.begin(), active.end());
        const size_t E = (size_t)cc.entries;
        std::lock_guard<std::mutex> g(c->mu);
        const DeviceScope device_scope(c->device);
        size_t sizes[12] = {(size_t)msa->swbf_inactive.n_peaks * 40, active.size() * 4, n * 16, n * 45 * 4,
                            (n + 1) * 8, E * 8, (E + 1) * 8, (size_t)cc.path_digests * 40, (E + 1) * 8,
                            (size_t)cc.rel_words * 4, E, 3 * n};
        void* p[12];
        int rc = carve(c, sizes, p);
        if (rc) return rc;
        Uploader up{c->stream};
        up(p[0], msa->swbf_inactive.peaks, sizes[0]);
        up(p[1], active.data(), sizes[1]);
        up(p[2], minimum, sizes[2]);
        up(p[3], distances, sizes[3]);
        up(p[4], chunks->entry_off, sizes[4]);
        up(p[5], chunks->chunk_index, sizes[5]);
        up(p[6], chunks->path_off, sizes[6]);
        up(p[7], chunks->path, sizes[7]);
        up(p[8], chunks->rel_off, sizes[8]);
        up(p[9], chunks->rel, sizes[9]);
        if (up.e != hipSuccess) return ms_finish(c, NHIP_OK, up.e);
        const nhip::MmrDev swbf{(const uint64_t*)p[0], msa->swbf_inactive.n_peaks, msa->swbf_inactive.num_leafs};
        rc = timed_launch(c, [&] {
            return nhip::launch_ms_chunk_auth(swbf, (const uint64_t*)p[5], (const uint64_t*)p[6], (const uint64_t*)p[7],
                                              (const uint64_t*)p[8], (const uint32_t*)p[9], E, (uint8_t*)p[10],
                                              c->stream);
        });
        uint8_t* out = (uint8_t*)p[11];
        if (rc == NHIP_OK) {
            nhip::MsRecordsDev r{};
            r.minimum = (const uint64_t*)p[2];
            r.distances = (const uint32_t*)p[3];
            r.entry_off = (const uint64_t*)p[4];
            r.chunk_index = (const uint64_t*)p[5];
            r.rel_off = (const uint64_t*)p[8];
            r.rel = (const uint32_t*)p[9];
            r.auth = (const uint8_t*)p[10];
            r.aocl_member = nullptr;
            r.active = (const uint32_t*)p[1];
            r.n_active = active.size();
            r.aocl_num_leafs = msa->aocl.num_leafs;
            r.valid = out;
            r.verdict = out + n;
            r.status = out + 2 * n;
            rc = timed_launch(c, [&] { return nhip::launch_ms_records(r, n, c->stream); });
        }
        hipError_t e = hipSuccess;
        if (rc == NHIP_OK) e = hipMemcpyAsync(valid, out, n, hipMemcpyDeviceToHost, c->stream);
        if (rc == NHIP_OK && e == hipSuccess) e = hipMemcpyAsync(can_remove, out + n, n, hipMemcpyDeviceToHost, c->stream);
        if (rc == NHIP_OK && e == hipSuccess) e = hipMemcpyAsync(status, out + 2 * n, n, hipMemcpyDeviceToHost, c->stream);
        return ms_finish(c, rc, e);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// MutatorSetAccumulator::verify (mutator_set_accumulator.rs:252-339) for n (item, membership proof) pairs
// (wallet_state.rs:1796,1958; state/mod.rs:1050,1206,1341): k_ms_aocl_leaf, AbsoluteIndexSet::compute into
// device buffers (no host round trip), k_ms_chunk_auth, k_ms_records.
int nhip_ms_verify_batch(nhip_ctx* c, const nhip_msa* msa, const uint64_t* items, const uint64_t* sender_randomness,
                         const uint64_t* receiver_preimages, const uint64_t* aocl_leaf_index,
                         const uint64_t* aocl_path_off, const uint64_t* aocl_path, const nhip_ms_chunks* chunks,
                         size_t n, uint8_t* verdicts, uint8_t* status) {
    if (!c || nhip::ms_msa_ok(msa)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!items || !sender_randomness || !receiver_preimages || !aocl_leaf_index || !verdicts || !status ||
        n > SIZE_MAX / 256)
        return NHIP_ERR_ARG;
    uint64_t apd = 0;
    if (nhip::ms_paths_ok(aocl_path_off, aocl_path, n, &apd)) return NHIP_ERR_ARG;
    nhip::MsChunkCounts cc;
    if (nhip::ms_chunks_ok(chunks, n, &cc)) return NHIP_ERR_ARG;
    try {
        std::vector<uint32_t> active(msa->active, msa->active + (msa->n_active ? msa->n_active : 0));
        std::sort(active.begin(), active.end());
        std::vector<uint64_t> in(15 * n);
        for (size_t i = 0; i < n; ++i)
            for (int q = 0; q < 5; ++q) {
                in[15 * i + q] = items[5 * i + q];
                in[15 * i + 5 + q] = sender_randomness[5 * i + q];
                in[15 * i + 10 + q] = receiver_preimages[5 * i + q];
            }
        const size_t E = (size_t)cc.entries;
        std::lock_guard<std::mutex> g(c->mu);
        const DeviceScope device_scope(c->device);
        size_t sizes[18] = {(size_t)msa->aocl.n_peaks * 40, (size_t)msa->swbf_inactive.n_peaks * 40, active.size() * 4,
                            15 * n * 8, n * 8, (n + 1) * 8, (size_t)apd * 40, (n + 1) * 8, E * 8, (E + 1) * 8,
                            (size_t)cc.path_digests * 40, (E + 1) * 8, (size_t)cc.rel_words * 4,
                            n * 16, n * 45 * 4, n, E, 2 * n};
        void* p[18];
        int rc = carve(c, sizes, p);
        if (rc) return rc;
        Uploader up{c->stream};
        up(p[0], msa->aocl.peaks, sizes[0]);
        up(p[1], msa->swbf_inactive.peaks, sizes[1]);
        up(p[2], active.data(), sizes[2]);
        up(p[3], in.data(), sizes[3]);
        up(p[4], aocl_leaf_index, sizes[4]);
        up(p[5], aocl_path_off, sizes[5]);
        up(p[6], aocl_path, sizes[6]);
        up(p[7], chunks->entry_off, sizes[7]);
        up(p[8], chunks->chunk_index, sizes[8]);
        up(p[9], chunks->path_off, sizes[9]);
        up(p[10], chunks->path, sizes[10]);
        up(p[11], chunks->rel_off, sizes[11]);
        up(p[12], chunks->rel, sizes[12]);
        if (up.e != hipSuccess) return ms_finish(c, NHIP_OK, up.e);
        const nhip::MmrDev aocl{(const uint64_t*)p[0], msa->aocl.n_peaks, msa->aocl.num_leafs};
        const nhip::MmrDev swbf{(const uint64_t*)p[1], msa->swbf_inactive.n_peaks, msa->swbf_inactive.num_leafs};
        rc = timed_launch(c, [&] {
            return nhip::launch_ms_aocl_leaf(aocl, (const uint64_t*)p[3], (const uint64_t*)p[4], (const uint64_t*)p[5],
                                             (const uint64_t*)p[6], n, (uint8_t*)p[15], c->stream);
        });
        if (rc == NHIP_OK)
            rc = timed_launch(c, [&] {
                return nhip::launch_absolute_index_sets((const uint64_t*)p[3], (const uint64_t*)p[4], n,
                                                        (uint64_t*)p[13], (uint32_t*)p[14], c->stream);
            });
        if (rc == NHIP_OK)
            rc = timed_launch(c, [&] {
                return nhip::launch_ms_chunk_auth(swbf, (const uint64_t*)p[8], (const uint64_t*)p[9],
                                                  (const uint64_t*)p[10], (const uint64_t*)p[11],
                                                  (const uint32_t*)p[12], E, (uint8_t*)p[16], c->stream);
            });
        uint8_t* out = (uint8_t*)p[17];
        if (rc == NHIP_OK) {
            nhip::MsRecordsDev r{};
            r.minimum = (const uint64_t*)p[13];
            r.distances = (const uint32_t*)p[14];
            r.entry_off = (const uint64_t*)p[7];
            r.chunk_index = (const uint64_t*)p[8];
            r.rel_off = (const uint64_t*)p[11];
            r.rel = (const uint32_t*)p[12];
            r.auth = (const uint8_t*)p[16];
            r.aocl_member = (const uint8_t*)p[15];
            r.active = (const uint32_t*)p[2];
            r.n_active = active.size();
            r.aocl_num_leafs = msa->aocl.num_leafs;
            r.valid = nullptr;
            r.verdict = out;
            r.status = out + n;
            rc = timed_launch(c, [&] { return nhip::launch_ms_records(r, n, c->stream); });
        }
        hipError_t e = hipSuccess;
        if (rc == NHIP_OK) e = hipMemcpyAsync(verdicts, out, n, hipMemcpyDeviceToHost, c->stream);
        if (rc == NHIP_OK && e == hipSuccess) e = hipMemcpyAsync(status, out + n, n, hipMemcpyDeviceToHost, c->stream);
        return ms_finish(c, rc, e);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// Block::validate rules 2.b-2.e and Block::mutator_set_accumulator_after for independent jobs (DESIGN.md
// §6d): k_ms_chunk_auth_jobs, k_ms_records_jobs, k_ms_apply.  The host stages order only: sorted copies of
// the active windows, each job's index slots sorted by (index, record) and grouped by chunk index, and its
// records sorted by their index arrays.  It hashes nothing and decides nothing.
int nhip_ms_apply_batch(nhip_ctx* c, const nhip_ms_apply_in* in, nhip_ms_apply_out* out) {
    using u128 = unsigned __int128;
    nhip::MsApplyCounts cnt;
    if (!c || nhip::ms_apply_ok(in, out, &cnt)) return NHIP_ERR_ARG;
    const size_t n = in->n_jobs;
    if (n == 0) return NHIP_OK;
    try {
        const size_t R = (size_t)cnt.records, E = (size_t)cnt.chunks.entries;
        std::vector<nhip::MsApplyJob> jobs(n);
        std::vector<uint64_t> peaks;
        std::vector<uint32_t> active, exp_active, rec_job(R), entry_rec(E), idx_perm(45 * R), grp, rec_perm(R);
        std::vector<u128> vals;
        uint64_t dig_total = 0, grp_total = 0, win_total = 0;
        auto put_peaks = [&](const nhip_mmr& m) {
            const uint64_t off = peaks.size() / 5;
            if (m.n_peaks) peaks.insert(peaks.end(), m.peaks, m.peaks + 5 * (size_t)m.n_peaks);
            return off;
        };
        for (size_t j = 0; j < n; ++j) {
            const nhip_msa& b = in->msa_before[j];
            nhip::MsApplyJob& jb = jobs[j];
            jb = nhip::MsApplyJob{};
            jb.aocl_n = b.aocl.num_leafs;
            jb.swbf_n = b.swbf_inactive.num_leafs;
            jb.aocl_np = b.aocl.n_peaks;
            jb.swbf_np = b.swbf_inactive.n_peaks;
            jb.aocl_peaks = put_peaks(b.aocl);
            jb.swbf_peaks = put_peaks(b.swbf_inactive);
            jb.act_off = active.size();
            jb.n_active = b.n_active;
            if (b.n_active) active.insert(active.end(), b.active, b.active + b.n_active);
            std::sort(active.begin() + jb.act_off, active.end());
            jb.add_off = in->add_off[j];
            jb.k = in->add_off[j + 1] - in->add_off[j];
            jb.rec_off = in->rec_off[j];
            jb.m = in->rec_off[j + 1] - in->rec_off[j];
            if (in->msa_expected) {
                const nhip_msa& x = in->msa_expected[j];
                jb.exp_aocl_n = x.aocl.num_leafs;
                jb.exp_swbf_n = x.swbf_inactive.num_leafs;
                jb.exp_aocl_np = x.aocl.n_peaks;
                jb.exp_swbf_np = x.swbf_inactive.n_peaks;
                jb.exp_aocl_peaks = put_peaks(x.aocl);
                jb.exp_swbf_peaks = put_peaks(x.swbf_inactive);
                jb.exp_act_off = exp_active.size();
                jb.exp_n_active = x.n_active;
                if (x.n_active) exp_active.insert(exp_active.end(), x.active, x.active + x.n_active);
            }
            // order only: the job's index slots by (index, record), the runs of one chunk index, the records
            // by their index arrays
            const size_t m = (size_t)jb.m, r0 = (size_t)jb.rec_off;
            vals.resize(45 * m);
            for (size_t r = 0; r < m; ++r) {
                rec_job[r0 + r] = (uint32_t)j;
                const u128 mn = ((u128)in->minimum[2 * (r0 + r) + 1] << 64) | in->minimum[2 * (r0 + r)];
                for (size_t t = 0; t < 45; ++t) vals[45 * r + t] = mn + in->distances[45 * (r0 + r) + t];
                for (uint64_t e = in->chunks->entry_off[r0 + r]; e < in->chunks->entry_off[r0 + r + 1]; ++e)
                    entry_rec[e] = (uint32_t)(r0 + r);
            }
            uint32_t* perm = idx_perm.data() + 45 * r0;
            for (size_t s = 0; s < 45 * m; ++s) perm[s] = (uint32_t)s;
            std::sort(perm, perm + 45 * m, [&](uint32_t x, uint32_t y) { return vals[x] != vals[y] ? vals[x] < vals[y] : x < y; });
            jb.grp_off = grp_total;
            for (size_t s = 0; s < 45 * m; ++s)
                if (s == 0 || (vals[perm[s]] >> 12) != (vals[perm[s - 1]] >> 12)) {
                    grp.push_back((uint32_t)s);
                    ++jb.n_grp;
                }
            grp.push_back((uint32_t)(45 * m));
            grp_total += jb.n_grp;
            uint32_t* rp = rec_perm.data() + r0;
            for (size_t r = 0; r < m; ++r) rp[r] = (uint32_t)r;
            std::stable_sort(rp, rp + m, [&](uint32_t x, uint32_t y) {
                return std::lexicographical_compare(vals.begin() + 45 * x, vals.begin() + 45 * x + 45,
                                                    vals.begin() + 45 * y, vals.begin() + 45 * y + 45);
            });
            const uint64_t n1 = jb.aocl_n + jb.k;
            const uint64_t slides =
                n1 < jb.aocl_n ? 0 : (n1 ? n1 - 1 : 0) / 8 - (jb.aocl_n ? jb.aocl_n - 1 : 0) / 8;  // <= k / 8 + 1
            jb.dig_off = dig_total;
            dig_total += (jb.k + 1) + (2 * slides + 1) + 2 * jb.n_grp;
            jb.win_off = cnt.accumulators ? out->active_off[j] : win_total;
            jb.win_cap = cnt.accumulators ? out->active_off[j + 1] - out->active_off[j] : jb.n_active + 45 * jb.m;
            win_total += jb.win_cap;
        }
        if (cnt.accumulators) win_total = cnt.window_cap;
        const nhip_ms_chunks* ch = in->chunks;
        std::lock_guard<std::mutex> g(c->mu);
        const DeviceScope device_scope(c->device);
        size_t sizes[29] = {n * sizeof(nhip::MsApplyJob), peaks.size() * 8, active.size() * 4, (size_t)cnt.additions * 40,
                            R * 16, R * 45 * 4, R ? (R + 1) * 8 : 0, E * 8, R ? (E + 1) * 8 : 0,
                            (size_t)cnt.chunks.path_digests * 40, R ? (E + 1) * 8 : 0, (size_t)cnt.chunks.rel_words * 4,
                            R * 4, E * 4, R * 45 * 4, grp.size() * 4, R * 4, exp_active.size() * 4, E, 3 * R, 45 * R,
                            (size_t)dig_total * 40, (size_t)grp_total * 16, 2 * n, n * 8, 2 * n * 64 * 40, 2 * n * 4,
                            3 * n * 8, (size_t)win_total * 4};
        void* p[29];
        int rc = carve(c, sizes, p);
        if (rc) return rc;
        Uploader up{c->stream};
        up(p[0], jobs.data(), sizes[0]);
        up(p[1], peaks.data(), sizes[1]);
        up(p[2], active.data(), sizes[2]);
        up(p[3], in->additions, sizes[3]);
        up(p[4], in->minimum, sizes[4]);
        up(p[5], in->distances, sizes[5]);
        if (R) {
            up(p[6], ch->entry_off, sizes[6]);
            up(p[7], ch->chunk_index, sizes[7]);
            up(p[8], ch->path_off, sizes[8]);
            up(p[9], ch->path, sizes[9]);
            up(p[10], ch->rel_off, sizes[10]);
            up(p[11], ch->rel, sizes[11]);
        }
        up(p[12], rec_job.data(), sizes[12]);
        up(p[13], entry_rec.data(), sizes[13]);
        up(p[14], idx_perm.data(), sizes[14]);
        up(p[15], grp.data(), sizes[15]);
        up(p[16], rec_perm.data(), sizes[16]);
        up(p[17], exp_active.data(), sizes[17]);
        if (up.e != hipSuccess) return ms_finish(c, NHIP_OK, up.e);
        nhip::MsApplyDev a{};
        a.jobs = (const nhip::MsApplyJob*)p[0];
        a.peaks = (const uint64_t*)p[1];
        a.active = (const uint32_t*)p[2];
        a.additions = (const uint64_t*)p[3];
        a.rec.minimum = (const uint64_t*)p[4];
        a.rec.distances = (const uint32_t*)p[5];
        a.rec.entry_off = (const uint64_t*)p[6];
        a.rec.chunk_index = (const uint64_t*)p[7];
        a.path_off = (const uint64_t*)p[8];
        a.path = (const uint64_t*)p[9];
        a.rec.rel_off = (const uint64_t*)p[10];
        a.rec.rel = (const uint32_t*)p[11];
        a.rec_job = (const uint32_t*)p[12];
        a.entry_rec = (const uint32_t*)p[13];
        a.idx_perm = (const uint32_t*)p[14];
        a.grp = (const uint32_t*)p[15];
        a.rec_perm = (const uint32_t*)p[16];
        a.exp_active = (const uint32_t*)p[17];
        a.has_expected = in->msa_expected ? 1 : 0;
        a.rec.auth = (const uint8_t*)p[18];
        a.rec.aocl_member = nullptr;
        a.rec.valid = (uint8_t*)p[19];
        a.rec.verdict = (uint8_t*)p[19] + R;
        a.rec.status = (uint8_t*)p[19] + 2 * R;
        a.index_set = (uint8_t*)p[20];
        a.dig = (uint64_t*)p[21];
        a.aux = (uint64_t*)p[22];
        a.verdict = (uint8_t*)p[23];
        a.status = (uint8_t*)p[23] + n;
        a.bad = (uint64_t*)p[24];
        a.out_peaks = (uint64_t*)p[25];
        a.out_np = (uint32_t*)p[26];
        a.out_n = (uint64_t*)p[27];
        a.out_active = (uint32_t*)p[28];
        rc = timed_launch(c, [&] { return nhip::launch_ms_chunk_auth_jobs(a, E, c->stream); });
        if (rc == NHIP_OK) rc = timed_launch(c, [&] { return nhip::launch_ms_records_jobs(a, R, c->stream); });
        if (rc == NHIP_OK) rc = timed_launch(c, [&] { return nhip::launch_ms_apply(a, n, c->stream); });
        hipError_t e = hipSuccess;
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (rc == NHIP_OK && e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
        };
        // into temporaries first: the outputs stay untouched unless the whole call succeeds
        std::vector<uint8_t> vs(2 * n);
        std::vector<uint64_t> bad(n);
        down(vs.data(), p[23], 2 * n);
        down(bad.data(), p[24], n * 8);
        if (cnt.accumulators) {
            down(out->aocl_peaks, a.out_peaks, n * 64 * 40);
            down(out->swbf_peaks, a.out_peaks + n * 64 * 5, n * 64 * 40);
            down(out->aocl_n_peaks, a.out_np, n * 4);
            down(out->swbf_n_peaks, a.out_np + n, n * 4);
            down(out->aocl_num_leafs, a.out_n, n * 8);
            down(out->swbf_num_leafs, a.out_n + n, n * 8);
            down(out->n_active, a.out_n + 2 * n, n * 8);
            down(out->active, a.out_active, (size_t)win_total * 4);
        }
        rc = ms_finish(c, rc, e);
        if (rc == NHIP_OK) {
            std::copy(vs.begin(), vs.begin() + n, out->verdict);
            std::copy(vs.begin() + n, vs.end(), out->status);
            std::copy(bad.begin(), bad.end(), out->bad_record);
        }
        return rc;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
