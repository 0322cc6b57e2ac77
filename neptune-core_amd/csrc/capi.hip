// C-ABI layer of libneptune_hip.so (declarations: include/neptune_hip.h): the context (ctx.hpp), the
// device-resident and host-buffer hashing calls, wire bytes -> words, timing.  The mutator-set entry
// points are ms_capi.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "device_scope.hpp"
#include "kernels.hpp"
#include "ms_shape.hpp"
#include "wire.hpp"

using nhip::hip_fail;
using nhip::Stage;
using nhip::timed_launch;

namespace {

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
// 2700: block digests and the header chain (nhip_blk_header, nhip_difficulty_target, nhip_difficulty_control,
// nhip_chain_params, NHIP_LINK_*, nhip_blk_digests, nhip_blk_chain_check)
// 2800: packed removal records, block rule 2.a (nhip_ms_unpack_plan, nhip_ms_unpack_batch,
// nhip_ms_apply_batch_packed; NHIP_MS_UNPACK_*)
// 2900: witnesses across a block (nhip_ms_update_plan, nhip_ms_update_batch)
// 3000: witnesses resident on the device across blocks (nhip_ms_store_*)
// 3100: witnesses back across a block (nhip_ms_revert_plan, nhip_ms_revert_batch, nhip_ms_store_revert)
// 3200: the archival mutator set resident on the device (nhip_ms_archive_*)
// 3300: the archival mutator set back across a block (nhip_ms_archive_revert)
// 3400: restored witnesses straight into a store (nhip_ms_archive_restore_shape, nhip_ms_store_append_restored;
// DESIGN.md §6k)
int nhip_abi_version(void) { return 3400; }

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
    Stage st(c);
    uint32_t* d_out;
    st.tmp(d_out, 1);
    if (st.commit()) return st.finish();
    st.step([&] { return hip_fail(hipMemsetAsync(d_out, 0, sizeof(uint32_t), c->stream)); });
    size_t blocks = (n / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    st.launch([&] {
        hipLaunchKernelGGL(k_any_bad, dim3((unsigned)blocks), dim3(256), 0, c->stream, d_v, n, d_out);
        return hipGetLastError();
    });
    uint32_t h = 1;
    st.out(&h, d_out, 1);
    const int rc = st.finish();
    if (rc) return rc;
    *all_ok = (uint8_t)(h ? 0 : 1);
    return NHIP_OK;
}

// ------------------------------------------------------------------ host-buffer form
int nhip_tip5_permutation(nhip_ctx* c, uint64_t* states, size_t n) {
    if (!c || (n && !states)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    Stage st(c);
    uint64_t* d_states;
    st.in(d_states, states, n, 16);
    if (st.commit()) return st.finish();
    st.launch([&] { return nhip::launch_permutation(d_states, n, c->stream); });
    st.out(states, d_states, 16 * n);
    return st.finish();
}

int nhip_tip5_hash_pair(nhip_ctx* c, const uint64_t* l, const uint64_t* r, size_t n, uint64_t* o) {
    if (!c || (n && (!l || !r || !o))) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    Stage st(c);
    const uint64_t *d_l, *d_r;
    uint64_t* d_o;
    st.in(d_l, l, n, 5);
    st.in(d_r, r, n, 5);
    st.tmp(d_o, n, 5);
    if (st.commit()) return st.finish();
    st.launch([&] { return nhip::launch_hash_pair(d_l, d_r, d_o, n, c->stream); });
    st.out(o, d_o, 5 * n);
    return st.finish();
}

int nhip_tip5_hash_varlen(nhip_ctx* c, const uint64_t* data, const uint64_t* offsets, size_t n, uint64_t* o) {
    if (!c || (n && (!offsets || !o))) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return NHIP_ERR_ARG;
    const size_t total = (size_t)offsets[n];
    if (total && !data) return NHIP_ERR_ARG;
    Stage st(c);
    const uint64_t *d_data, *d_off;
    uint64_t* d_o;
    st.in(d_data, data, total);
    st.in(d_off, offsets, n + 1);
    st.tmp(d_o, n, 5);
    if (st.commit()) return st.finish();
    st.launch([&] { return nhip::launch_hash_varlen(d_data, d_off, n, d_o, c->stream); });
    st.out(o, d_o, 5 * n);
    return st.finish();
}

int nhip_mtree_build(nhip_ctx* c, const uint64_t* leafs, size_t n, uint64_t* nodes_out) {
    if (!c || !is_pow2(n) || !leafs || !nodes_out) return NHIP_ERR_ARG;
    Stage st(c);
    const uint64_t* d_leafs;
    uint64_t* d_nodes;
    st.in(d_leafs, leafs, n, 5);
    st.tmp(d_nodes, n, 5);
    if (st.commit()) return st.finish();
    st.step([&] { return build_tree_dev(c, d_leafs, n, d_nodes); });
    st.out(nodes_out, d_nodes, 5 * n);
    return st.finish();
}

int nhip_mtree_verify(nhip_ctx* c, const uint64_t* roots, size_t n_roots, const uint64_t* idx,
                      const uint64_t* leafs, const uint64_t* paths, uint32_t depth, size_t n, uint8_t* v) {
    if (!c || (n_roots != 1 && n_roots != n)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!roots || !idx || !leafs || !v || (depth && !paths)) return NHIP_ERR_ARG;
    Stage st(c);
    const uint64_t *d_roots, *d_idx, *d_leafs, *d_paths;
    uint8_t* d_v;
    st.in(d_roots, roots, n_roots, 5);
    st.in(d_idx, idx, n);
    st.in(d_leafs, leafs, n, 5);
    st.in(d_paths, paths, n, (size_t)depth * 5);
    st.tmp(d_v, n);
    if (st.commit()) return st.finish();
    const int per_path = (n_roots == n && n != 1) ? 1 : 0;
    st.launch([&] {
        return nhip::launch_mtree_verify(d_roots, per_path, d_idx, d_leafs, d_paths, depth, n, d_v, c->stream);
    });
    st.out(v, d_v, n);
    return st.finish();
}

// ------------------------------------------------------------------ wire bytes -> words
int nhip_internal_is_pinned(const void* p, size_t bytes);  // host_pinned.cpp

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
        Stage st(c);
        uint8_t* d_raw;
        uint64_t *d_boff, *d_words;
        nhip::ProofIn* d_in;
        st.tmp(d_raw, plan.raw_bytes);
        st.tmp(d_boff, n);
        st.tmp(d_in, n);
        st.tmp(d_words, (size_t)total);
        if (st.commit()) return st.finish();
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
        st.step([&] {
            return hip_fail(nhip::wire_upload(plan, bytes, d_raw, stage,
                                              [](const void* q, size_t b) { return nhip_internal_is_pinned(q, b) != 0; },
                                              c->stream));
        });
        st.up(d_boff, plan.boff.data(), n);  // after the raw runs, as the stream has always had them
        st.up(d_in, in.data(), n);
        st.launch([&] {
            return nhip::launch_wire_words(d_raw, d_boff, d_in, (uint32_t)n, total, d_words, c->stream);
        });
        st.out(out, d_words, (size_t)total);
        return st.finish();
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
    Stage st(c);
    const uint64_t *d_data, *d_off;
    uint64_t *d_leaves, *d_roots;
    st.in(d_data, data, total);
    st.in(d_off, offsets, nl + 1);
    st.tmp(d_leaves, nl, 5);
    st.tmp(d_roots, n, 5);
    if (st.commit()) return st.finish();
    st.launch([&] { return nhip::launch_hash_varlen(d_data, d_off, nl, d_leaves, c->stream); });
    st.launch([&] { return nhip::launch_mast_roots(d_leaves, fields, pow2, n, d_roots, c->stream); });
    st.out(roots_out, d_roots, 5 * n);
    return st.finish();
}

// AbsoluteIndexSet::compute (absolute_index_set.rs:86-113) for n removal records.
int nhip_absolute_index_sets(nhip_ctx* c, const uint64_t* items, const uint64_t* sender_randomness,
                             const uint64_t* receiver_preimages, const uint64_t* aocl_leaf_indices, size_t n,
                             uint64_t* minimum_out, uint32_t* distances_out) {
    if (!c || (n && (!items || !sender_randomness || !receiver_preimages || !aocl_leaf_indices || !minimum_out ||
                     !distances_out)))
        return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    try {
        const std::vector<uint64_t> in = nhip::ms_interleave15(items, sender_randomness, receiver_preimages, n);
        Stage st(c);
        const uint64_t *d_in, *d_aocl;
        uint64_t* d_min;
        uint32_t* d_dist;
        st.in(d_in, in.data(), n, 15);
        st.in(d_aocl, aocl_leaf_indices, n);
        st.tmp(d_min, n, 2);
        st.tmp(d_dist, n, 45);
        if (st.commit()) return st.finish();
        st.launch([&] { return nhip::launch_absolute_index_sets(d_in, d_aocl, n, d_min, d_dist, c->stream); });
        st.out(minimum_out, d_min, 2 * n);
        st.out(distances_out, d_dist, 45 * n);
        return st.finish();
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
