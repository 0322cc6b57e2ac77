// Host side of a STARK batch (include/neptune_hip.h: nhip_batch_*, nhip_verify_batch*): sizing a
// batch from its proof lengths and headers (stark_layout.hpp), uploading the raw proof words or
// wire bytes and the staged claim encodings, placing the device scratch, and launching, waiting
// for and reading back the phase kernels (stark_kernels.hip).  The host decodes nothing: k_decode
// walks every proof stream on the device, every run, and any structural error there gives verdict 0
// (triton_vm::verify returns false on every Err), never an infrastructure error.  The AIR object
// is air_host.cpp's, the pinned-range registry host_pinned.cpp's.
//
// A batch's memory is a BatchMem and its streams and phase events a LaunchRes: its own (a resident
// batch), or the context's VerifyScratch's (nhip_verify_batch*).  The batch holds a pointer to the
// one it uses, so only destroy tells the two apart.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/neptune_hip.h"
#include "device_scope.hpp"
#include "goldilocks.hpp"
#include "host_copy.hpp"
#include "host_numa.hpp"
#include "kernels.hpp"
#include "stark.hpp"
#include "stark_host_internal.hpp"
#include "stark_layout.hpp"
#include "wire.hpp"

using namespace nhip;

namespace {

// A batch's proofs given as spans of a wire buffer (the in-place feed path) instead of nhip_proof records.
struct WireSrc {
    const uint8_t* bytes;
    size_t n_bytes;
    const nhip_span* spans;
};

// The claim's BFieldCodec encoding (pinned layout, new_claim.rs:38-100):
// [out_n + 1, out_n, out.., in_n + 1, in_n, in.., version, digest(5)], staged in the batch's input
// form (the kernels read the claim and the proof words alike): the caller's field elements reduced
// mod p in their own form, the lengths and the version (plain integers) converted into it.
void encode_claim(const nhip_claim& claim, bool mont, uint64_t* c) {
    auto len = [&](uint64_t v) { return mont ? to_mont(v) : v; };
    *c++ = len(claim.output_len + 1);
    *c++ = len(claim.output_len);
    for (size_t i = 0; i < claim.output_len; ++i) *c++ = canon(claim.output[i]);
    *c++ = len(claim.input_len + 1);
    *c++ = len(claim.input_len);
    for (size_t i = 0; i < claim.input_len; ++i) *c++ = canon(claim.input[i]);
    *c++ = len(claim.version);
    for (int i = 0; i < 5; ++i) *c++ = canon(claim.program_digest[i]);
}

// The staging copy of a proof (pageable caller memory -> pinned staging) with non-temporal
// stores: the staging is written once and read only by the DMA engine, so ordinary stores would
// first read every destination line into the cache (a read-for-ownership) and then evict it: one
// more host-DRAM pass per proof byte.  The feed path's host bandwidth is what an 8-GPU node runs
// out of first, so the copy streams: 8-byte head to 16-byte alignment, 64-byte
// blocks of four 16-byte streaming stores, then the tail.  The caller fences (_mm_sfence) before
// the DMA of the chunk is issued.  NHIP_STAGE_NT=0: plain memcpy (A/B).
bool stage_nt() {
    static const bool on = [] {
        const char* v = nhip::ab_env("NHIP_STAGE_NT");
        return !v || std::strtol(v, nullptr, 10) != 0;
    }();
    return on;
}
// Host threads for staging copies (at most 16, the GPU box's CPU share).
unsigned host_threads(uint64_t bytes) {
    unsigned t = nhip::host_threads_env() ? nhip::host_threads_env() : std::thread::hardware_concurrency();
    t = std::max(1u, std::min(t, 16u));
    return bytes < (8ull << 20) ? 1u : t;
}

// Size of a buffer that must grow from `have` to hold `need`: exact for a one-shot batch; for
// buffers refilled again and again (streams, the queue's slots, the verify scratch) with headroom
// and at least doubling, so that batches of varying size stop reallocating after a few calls (a
// hipFree / hipHostFree waits for the device, which stalls the other batches in flight).
inline size_t grown(size_t need, size_t have, bool refilled) {
    if (!refilled) return need;
    return std::max(need + need / 4, have ? 2 * have : 0);
}

// A grow-only allocation, device or pinned host memory.  Its contents are never kept across a
// growth: every user writes the whole buffer anew.
struct GrowBuf {
    enum Kind { DEVICE, PINNED };
    const Kind kind;
    void* p = nullptr;
    size_t bytes = 0;
    explicit GrowBuf(Kind k) : kind(k) {}
    // Room for `need` bytes: nothing to do when they fit; otherwise the buffer is freed and one of
    // grown(need, have, refilled) bytes, at least `at_least`, allocated.  On failure it is empty.
    hipError_t reserve(size_t need, bool refilled, size_t at_least = 0) {
        if (bytes >= need) return hipSuccess;
        const size_t want = std::max(grown(need, bytes, refilled), at_least);
        release();
        const hipError_t e = kind == DEVICE ? hipMalloc(&p, want) : hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        else bytes = want;
        return e;
    }
    void release() {
        if (p) (void)(kind == DEVICE ? hipFree(p) : hipHostFree(p));
        p = nullptr;
        bytes = 0;
    }
};

// The allocations of a batch.
struct BatchMem {
    GrowBuf words{GrowBuf::DEVICE};     // proof words, then the staged claim encodings
    GrowBuf raw{GrowBuf::DEVICE};       // raw wire bytes of an in-place fill (k_wire_words gathers them into words)
    GrowBuf scratch{GrowBuf::DEVICE};   // ScratchLayout
    GrowBuf readback{GrowBuf::PINNED};  // Readback: [device counters | plan counters | verdicts (n B)]
    void release() {
        readback.release();
        scratch.release();
        words.release();
        raw.release();
    }
};

// The streams and phase events of a batch's launches (made by launch_resources).
struct LaunchRes {
    hipStream_t main = nullptr;  // hashing chain (rows -> Merkle levels -> roots -> verdicts)
    hipStream_t aux = nullptr;   // latency-bound chain (Fiat-Shamir -> plan -> OOD -> FRI -> DEEP)
    hipEvent_t ev[STARK_EVENTS] = {};
    bool made = false;
    void destroy() {
        if (made)
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (aux && aux != main) (void)hipStreamDestroy(aux);
        if (main) (void)hipStreamDestroy(main);
        *this = LaunchRes{};
    }
};

// Device memory, streams, events and pinned readback of nhip_verify_batch, kept in the context
// and reused call after call: a one-proof call is otherwise dominated by hipMalloc / stream /
// event / pinned-buffer setup and teardown (~10 ms against ~2 ms of device work).  `mu` holds
// the scratch for a whole call, so concurrent callers are serialized.
struct VerifyScratch {
    std::mutex mu;
    BatchMem mem;
    LaunchRes res;
};

void free_verify_scratch(void* p) {
    auto* sc = (VerifyScratch*)p;
    if (sc->res.made) {
        (void)hipStreamSynchronize(sc->res.main);
        (void)hipStreamSynchronize(sc->res.aux);
    }
    sc->res.destroy();
    sc->mem.release();
    delete sc;
}

}  // namespace

struct nhip_batch {
    HostBatch H;
    const nhip_air* air = nullptr;
    int device = 0;
    // memory, streams and events: the batch's own, or a verify scratch's (nhip_verify_batch*)
    BatchMem own_mem;
    BatchMem* mem = &own_mem;
    LaunchRes own_res;
    LaunchRes* res = &own_res;
    bool borrowed() const { return mem != &own_mem; }
    Readback rb;  // the readback region of the current contents
    StarkBatchDev dev{};
    StarkPhaseTimer tm{};
    bool timed = false, in_flight = false;
    struct {
        double decode, fs, rows, plan, hash, roots, ood, fri, deep, total;
    } ph{};
    double stage_ms = 0, upload_ms = 0;
    // The batch's launch sequence captured into a HIP graph (nhip_batch_set_graph): replayed by every
    // untimed launch while the contents and streams are unchanged, captured again at the next launch
    // after a refill or a stream change.  The capture records its own fork / join events (gev): an
    // event once captured into a graph cannot be recorded on a stream again.
    hipGraphExec_t gexec = nullptr;
    bool graph_on = false;
    bool last_graph = false;  // the last launch replayed the graph (no phase timestamps)
    hipEvent_t gev[STARK_EVENTS] = {};
    double mp_hash_exec_ms = 0;  // summed dispatch durations of the hash launches
    double row_hash_exec_ms = 0;  // the row-hashing launch's dispatch duration
    uint64_t merkle_perms = 0;
    std::vector<uint64_t> mp_cap;  // multiproof op capacity per level
};

namespace {

// The argument checks of a fill: they need no device and no lock.
int check_fill_args(nhip_ctx* ctx, const nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                    const nhip_proof* proofs, const WireSrc* wire, size_t n, nhip_batch** out, const nhip_batch* reuse,
                    Dims& D) {
    // the wire source's own argument checks come first
    if (wire) {
        if (proofs || !sp || sp->input_form != NHIP_INPUT_CANONICAL) return NHIP_ERR_ARG;
        if ((wire->n_bytes && !wire->bytes) || (n && !wire->spans)) return NHIP_ERR_ARG;
        if (!wire_spans_ok(wire->spans, n, wire->n_bytes)) return NHIP_ERR_ARG;
    }
    if (!ctx || !out || (n && (!claims || (!proofs && !wire)))) return NHIP_ERR_ARG;
    if (reuse && (reuse->in_flight || reuse->borrowed())) return NHIP_ERR_ARG;
    if (!reuse) *out = nullptr;
    if (!dims_from(sp, air, D)) return NHIP_ERR_ARG;
    if (n > 0xFFFFFFFFull) return NHIP_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if ((!wire && proofs[i].len && !proofs[i].words) || (claims[i].input_len && !claims[i].input) ||
            (claims[i].output_len && !claims[i].output) || claims[i].input_len > 0xFFFFFFFFull ||
            claims[i].output_len > 0xFFFFFFFFull)
            return NHIP_ERR_ARG;
    return NHIP_OK;
}

// Upload of the records source.  Proofs in pinned caller memory (nhip_host_alloc /
// nhip_host_register) are DMA'd as they lie, adjacent ones as one copy; the others are copied into
// the context's pinned staging (same layout as the device buffer) by host threads, ~64 MB chunks in
// proof order, each chunk's DMA issued as soon as its copies are done.  The claim encodings go
// through the staging too.
hipError_t upload_records(nhip_ctx* ctx, const HostBatch& H, const std::vector<ProofIn>& pin, const nhip_claim* claims,
                          const nhip_proof* proofs, uint64_t* d_words, hipStream_t st) {
    const size_t n = pin.size();
    hipError_t e = hipSuccess;
    auto dma = [&](uint64_t dst_word, const uint64_t* src, uint64_t nw) {
        if (e == hipSuccess && nw) e = hipMemcpyAsync(d_words + dst_word, src, nw * 8, hipMemcpyHostToDevice, st);
    };
    std::vector<uint8_t> direct(n, 0);
    for (size_t i = 0; i < n; ++i)
        direct[i] = proofs[i].len && pinned_contains(proofs[i].words, proofs[i].len * 8) ? 1 : 0;
    for (size_t i = 0; i < n;) {  // direct segments first: the DMA engine starts right away
        if (!direct[i]) {
            ++i;
            continue;
        }
        size_t j = i + 1;
        while (j < n && direct[j] && proofs[j].words == proofs[j - 1].words + proofs[j - 1].len) ++j;
        dma(pin[i].off, proofs[i].words, pin[j - 1].off + pin[j - 1].len - pin[i].off);
        i = j;
    }
    std::vector<uint64_t> pageable;
    uint64_t* stage = (uint64_t*)nhip_internal_staging(ctx, H.words_total * 8 + 8);
    if (!stage) {
        pageable.resize(H.words_total + 1);
        stage = pageable.data();
    }
    for (size_t i = 0; i < n; ++i) encode_claim(claims[i], H.D.mont_words != 0, stage + pin[i].claim_off);
    std::vector<size_t> todo;  // staged proofs, in order
    uint64_t staged_bytes = 0;
    for (size_t i = 0; i < n; ++i)
        if (!direct[i] && proofs[i].len) todo.push_back(i), staged_bytes += proofs[i].len * 8;
    constexpr uint64_t CHUNK_WORDS = 8ull << 20;  // 64 MB
    std::vector<size_t> cut{0};                   // chunk c = todo[cut[c] .. cut[c + 1])
    for (size_t q = 1; q < todo.size(); ++q)
        if (pin[todo[q]].off - pin[todo[cut.back()]].off >= CHUNK_WORDS) cut.push_back(q);
    cut.push_back(todo.size());
    const size_t nc = todo.empty() ? 0 : cut.size() - 1;
    std::unique_ptr<std::atomic<size_t>[]> left(new std::atomic<size_t>[nc + 1]);
    std::vector<size_t> chunk_of(todo.size());
    for (size_t c = 0; c < nc; ++c) {
        left[c].store(cut[c + 1] - cut[c]);
        for (size_t q = cut[c]; q < cut[c + 1]; ++q) chunk_of[q] = c;
    }
    std::atomic<size_t> next{0};
    const bool nt = stage_nt() && stage != pageable.data();
    auto work = [&]() {
        for (size_t q; (q = next.fetch_add(1)) < todo.size();) {
            const size_t i = todo[q];
            if (nt) {
                copy_words_nt(stage + pin[i].off, proofs[i].words, proofs[i].len);
                _mm_sfence();  // the streaming stores are globally visible before the chunk is released
            } else {
                std::memcpy(stage + pin[i].off, proofs[i].words, proofs[i].len * 8);
            }
            left[chunk_of[q]].fetch_sub(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    // copy threads on the CPUs of the GPU's NUMA node, where the staging lives (host_numa.cpp):
    // at most that node's CPUs, or the count set by nhip_set_host_threads (a group divides a
    // node's CPUs among the members on it)
    const nhip::HostTopo& topo = ctx_topo(ctx);
    unsigned threads = host_threads(staged_bytes);
    if (const unsigned set = nhip_internal_host_threads(ctx); set && threads > 1 && !nhip::host_threads_env())
        threads = set;
    if (!topo.cpus.empty() && nhip::numa_enabled()) threads = std::min<unsigned>(threads, (unsigned)topo.cpus.size());
    if (threads > 1 && stage != pageable.data()) {
        pool.reserve(threads);
        for (unsigned t = 0; t < threads; ++t) {
            try {
                pool.emplace_back([&]() {
                    (void)nhip::bind_thread(topo.cpus);
                    work();
                });
            } catch (const std::system_error&) {
                break;  // fewer threads: the running ones (and this one, below) take the rest
            }
        }
    }
    if (pool.empty()) work();
    // DMA each chunk once copied: its staged proofs, adjacent ones as one copy
    for (size_t c = 0; c < nc; ++c) {
        while (left[c].load(std::memory_order_acquire) != 0) {
            if (pool.empty()) break;
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        for (size_t q = cut[c]; q < cut[c + 1];) {
            size_t r = q + 1;
            while (r < cut[c + 1] && todo[r] == todo[r - 1] + 1) ++r;
            const size_t i0 = todo[q], i1 = todo[r - 1];
            dma(pin[i0].off, stage + pin[i0].off, pin[i1].off + pin[i1].len - pin[i0].off);
            q = r;
        }
    }
    for (auto& th : pool) th.join();
    dma(H.proof_words, stage + H.proof_words, H.words_total - H.proof_words);
    if (stage == pageable.data() && e == hipSuccess) e = hipStreamSynchronize(st);  // pageable source
    return e;
}

// Upload of the wire source (the in-place path of DESIGN.md §6b): the spans' raw bytes, run by run
// (wire.hpp), into the batch's device raw buffer; k_wire_words turns them into the proof region of
// the word buffer once the ProofIn records are up (place_scratch).  The claim encodings are staged
// as for the other source, the raw bytes of a pageable buffer after them.
hipError_t upload_wire(nhip_ctx* ctx, const HostBatch& H, const std::vector<ProofIn>& pin, const nhip_claim* claims,
                       const WireSrc& wire, const WirePlan& plan, uint8_t* d_raw, uint64_t* d_words, hipStream_t st) {
    const uint64_t cw = H.words_total - H.proof_words;  // claim words
    const size_t raw_at = (size_t)((cw * 8 + 8 + 63) & ~(uint64_t)63);
    bool any_pageable = false;
    for (const WireRun& r : plan.runs) any_pageable |= !pinned_contains(wire.bytes + r.start, (size_t)(r.end - r.start));
    const size_t sbytes = raw_at + (any_pageable ? plan.raw_bytes : 0);
    std::vector<uint64_t> pageable;
    uint8_t* stage = (uint8_t*)nhip_internal_staging(ctx, sbytes);
    if (!stage) {
        pageable.resize(sbytes / 8 + 1);
        stage = (uint8_t*)pageable.data();
    }
    hipError_t e = wire_upload(plan, wire.bytes, d_raw, stage + raw_at,
                               [](const void* p, size_t bytes) { return pinned_contains(p, bytes); }, st);
    uint64_t* cstage = (uint64_t*)stage;
    for (size_t i = 0; i < pin.size(); ++i) encode_claim(claims[i], false, cstage + (pin[i].claim_off - H.proof_words));
    if (e == hipSuccess && cw)
        e = hipMemcpyAsync(d_words + H.proof_words, cstage, cw * 8, hipMemcpyHostToDevice, st);
    if (stage == (uint8_t*)pageable.data() && e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

// stark_set_kernel_attributes, once per device.
bool kernel_attributes_set(int device) {
    static std::mutex mu;
    static uint64_t done = 0;  // devices whose kernel attributes are set
    std::lock_guard<std::mutex> lock(mu);
    if (device >= 64 || !((done >> device) & 1u)) {
        if (stark_set_kernel_attributes() != hipSuccess) return false;
        if (device < 64) done |= 1ull << device;
    }
    return true;
}

// Bind the kernels' view of the batch: its sizes, the word buffer, the scratch buffers by name, and
// the compiled AIR program `pk` on this GPU.
void bind_dev(nhip_batch* b, const ScratchLayout& S, const nhip_air::Dev& adev, int pk) {
    const HostBatch& H = b->H;
    const OodProgram& pg = b->air->progs[pk];
    char* base = (char*)b->mem->scratch.p;
    const auto at = [base](const ScratchLayout::Buf& f) { return (void*)(base + f.off); };
    StarkBatchDev& dv = b->dev;
    dv.n_proofs = H.n;
    dv.max_R = H.max_R;
    dv.dims = H.D.d;
    dv.D = H.D;
    dv.fs_stride = H.fs_stride;
    dv.xs_stride = H.xs_stride;
    dv.words = (const uint64_t*)b->mem->words.p;
    dv.desc = (ProofDesc*)at(S.desc);
    dv.ops = (FsOp*)at(S.fs_ops);
    dv.xs = (uint64_t*)at(S.xs);
    dv.idx = (uint32_t*)at(S.idx);
    dv.dig = (uint64_t*)at(S.dig);
    dv.ood = (uint64_t*)at(S.ood);
    dv.fail = (uint32_t*)at(S.fail);
    dv.in = (const ProofIn*)at(S.proof_in);
    dv.counters = (unsigned long long*)at(S.readback);
    dv.mp.counter = (uint32_t*)((char*)at(S.readback) + b->rb.plan_counters_off);
    dv.verdicts = (uint8_t*)at(S.readback) + b->rb.verdicts_off;
    dv.mp.ops = (uint64_t*)at(S.mp_ops);
    dv.mp.arena = (uint64_t*)at(S.mp_arena);
    dv.mp.shard_base = (const uint64_t*)at(S.mp_shard_base);
    dv.mp.shard_cap = (const uint64_t*)at(S.mp_shard_cap);
    dv.mp.roots = (MpRoot*)at(S.mp_roots);
    dv.mp.dups = (uint32_t*)at(S.mp_dups);
    dv.mp.ndup = (uint32_t*)at(S.mp_ndup);
    dv.mp.levels = H.levels;
    dv.mp.lvl_g0 = (uint64_t*)at(S.mp_lvl_g0);
    dv.mp.lvl_cnt = (uint32_t*)at(S.mp_lvl_cnt);
    dv.mp.lvl_n = (uint32_t*)at(S.mp_lvl_n);
    dv.xdom = (uint64_t*)at(S.xdom);
    dv.lcw = (uint64_t*)at(S.lcw);
    dv.max_lcw = H.max_last_cw;
    dv.mp_cap_host = b->mp_cap.data();
    dv.air_prog = adev.d_prog[pk];
    dv.air_prog_off = adev.d_prog_off[pk];
    dv.air_n_levels = (uint32_t)pg.prog_off.size() - 1;
    dv.air_consts = adev.d_consts[pk];
    dv.air_cons_off = b->air->cons_off;
    dv.air_lds_slots = air_lds_slots(pg.slots, b->air->lds_cap);
    dv.air_gslot_n = pg.slots - dv.air_lds_slots;
    dv.air_gslots = (Xfe*)at(S.air_gslots);
    dv.air_lds_bytes = AIR_LDS_HEADER + (size_t)dv.air_lds_slots * 24;
    // 256 threads per proof: 1,024-thread workgroups for a triton-air-sized circuit (one workgroup
    // per CU either way, the slot area fills its LDS) ran the 256-proof evaluation 0.248 -> 0.213 ms
    // alone but took the wave slots the concurrent hashing needs (config 4: 354k -> 305k proofs/s)
    dv.air_block = 256u;
}

// Size the multiproof plan and the scratch, grow the scratch, and send the small tables: the
// ProofIn records, the shard tables and, for the wire source, the proofs' byte offsets followed by
// the gather (k_wire_words) of the raw bytes into the word buffer.  Then wait for the context
// stream: every source of this fill is a host vector or the staging.
int place_scratch(nhip_batch* b, const std::vector<ProofIn>& pin, const std::vector<ProofShape>& shp,
                  const std::vector<uint64_t>* wire_boff, uint32_t air_gslot_n, bool refilled, hipStream_t st,
                  ScratchLayout& S) {
    const HostBatch& H = b->H;
    MpCaps caps;
    mp_capacities(H, pin, shp, caps);
    b->mp_cap.swap(caps.cap);
    b->rb = Readback::of(H.levels, H.n);
    S = ScratchLayout::of(H, b->rb, wire_boff != nullptr, caps.total, air_gslot_n);
    if (S.overflow) return NHIP_ERR_OOM;
    GrowBuf& scratch = b->mem->scratch;
    if (scratch.bytes < S.total) (void)hipStreamSynchronize(st);  // the uploads, before the free waits for the device
    hipError_t e = scratch.reserve(S.total, refilled);
    if (e != hipSuccess) return hipfail(e);
    char* base = (char*)scratch.p;
    const size_t n = pin.size();
    if (n) e = hipMemcpyAsync(base + S.proof_in.off, pin.data(), n * sizeof(ProofIn), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && H.levels)
        e = hipMemcpyAsync(base + S.mp_shard_base.off, caps.sbase.data(), caps.sbase.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && H.levels)
        e = hipMemcpyAsync(base + S.mp_shard_cap.off, caps.scap.data(), caps.scap.size() * 8, hipMemcpyHostToDevice, st);
    if (wire_boff && n) {
        // the gather: after the raw uploads and the ProofIn records on this stream, before anything
        // reads the proof words (the launch streams start after the synchronize below)
        if (e == hipSuccess)
            e = hipMemcpyAsync(base + S.wire_boff.off, wire_boff->data(), n * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = launch_wire_words((const uint8_t*)b->mem->raw.p, (const uint64_t*)(base + S.wire_boff.off),
                                  (const ProofIn*)(base + S.proof_in.off), (uint32_t)n, H.proof_words,
                                  (uint64_t*)b->mem->words.p, st);
    }
    const hipError_t es = hipStreamSynchronize(st);
    return hipfail(e == hipSuccess ? es : e);
}

// Stage + upload the batch's contents into b->mem: proof words (raw; k_decode walks them on the
// device every run) and the staged claim encodings into the word buffer, the per-proof ProofIn
// records, and the scratch sized from the padded height each proof header declares.  The proofs
// come from one of two sources: nhip_proof records (word pointers, `proofs`), or spans of a wire
// buffer (`wire`: the spans' raw bytes are uploaded as they lie; canonical input form only).
// refilled: the buffers will be filled again (a resident batch being refilled, the verify scratch).
int fill_batch(nhip_ctx* ctx, nhip_batch* b, nhip_air* air, const Dims& D, const nhip_claim* claims,
               const nhip_proof* proofs, const WireSrc* wire, size_t n, bool refilled) {
    BatchMem& m = *b->mem;
    hipStream_t st = nhip_internal_stream(ctx);
    b->air = air;
    b->device = nhip_internal_device(ctx);
    b->H = HostBatch{};
    HostBatch& H = b->H;
    H.D = D;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<ProofIn> pin(n);
    std::vector<ProofShape> shp;
    for (size_t i = 0; i < n; ++i) {
        pin[i].len = wire ? wire->spans[i].len : (uint64_t)proofs[i].len;
        pin[i].claim_in_n = (uint32_t)claims[i].input_len;
        pin[i].claim_out_n = (uint32_t)claims[i].output_len;
    }
    // the five header words by an unaligned-safe load: the wire pointer is never a uint64_t*
    size_batch(H, pin, shp, [&](size_t i, uint64_t* h5) {
        std::memcpy(h5, wire ? (const void*)(wire->bytes + wire->spans[i].offset) : (const void*)proofs[i].words, 40);
    });
    hipError_t e = m.words.reserve(H.words_total * 8 + 8, refilled);
    if (e != hipSuccess) return hipfail(e);
    WirePlan plan;
    if (wire) {
        wire_plan(wire->bytes, wire->spans, n, plan);
        e = m.raw.reserve(plan.raw_bytes, refilled);
        if (e != hipSuccess) return hipfail(e);
        e = upload_wire(ctx, H, pin, claims, *wire, plan, (uint8_t*)m.raw.p, (uint64_t*)m.words.p, st);
    } else {
        e = upload_records(ctx, H, pin, claims, proofs, (uint64_t*)m.words.p, st);
    }
    const auto t1 = std::chrono::steady_clock::now();
    b->stage_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (e != hipSuccess) return hipfail(e);
    nhip_air::Dev adev{};
    if (int rc = air_upload(ctx, air, &adev)) return rc;
    if (!kernel_attributes_set(b->device)) return NHIP_ERR_HIP;
    const int pk = ood_program_for((uint32_t)n);
    const uint32_t slots = air->progs[pk].slots;
    ScratchLayout S;
    const int rc = place_scratch(b, pin, shp, wire ? &plan.boff : nullptr, slots - air_lds_slots(slots, air->lds_cap),
                                 refilled, st, S);
    b->upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (rc) return rc;
    bind_dev(b, S, adev, pk);
    return NHIP_OK;
}

// A batch with the given contents.  reuse == nullptr: a new batch (*out), on `scr`'s memory and
// streams if given (nhip_verify_batch*), else on its own; otherwise `reuse` is refilled in place
// (same streams and events; its device memory reused when large enough).  On failure a new batch is
// deleted; a refilled one is left empty (n = 0) but usable.
int batch_prepare(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                  const nhip_proof* proofs, const WireSrc* wire, size_t n, nhip_batch** out, VerifyScratch* scr,
                  nhip_batch* reuse = nullptr) {
    Dims D{};
    if (int rc = check_fill_args(ctx, air, sp, claims, proofs, wire, n, out, reuse, D)) return rc;
    std::lock_guard<std::mutex> g(*nhip_internal_mutex(ctx));
    const DeviceScope device_scope(nhip_internal_device(ctx));
    nhip_batch* b = reuse ? reuse : new (std::nothrow) nhip_batch();
    if (!b) return NHIP_ERR_OOM;
    if (scr) b->mem = &scr->mem, b->res = &scr->res;
    int rc;
    try {
        rc = fill_batch(ctx, b, air, D, claims, proofs, wire, n, reuse || scr);
    } catch (const std::bad_alloc&) {  // a host allocation (the upload threads are joined before anything can throw)
        rc = NHIP_ERR_OOM;
    }
    if (rc == NHIP_OK) {
        *out = b;
        return NHIP_OK;
    }
    (void)hipStreamSynchronize(nhip_internal_stream(ctx));  // nothing of this fill is still in flight
    if (reuse) {
        b->H = HostBatch{};
        b->dev.n_proofs = 0;
        b->rb = Readback::of(b->dev.mp.levels, 0);
    } else {
        b->own_mem.release();
        delete b;
    }
    return rc;
}

void drop_graph(nhip_batch* b) {
    if (b->gexec) (void)hipGraphExecDestroy(b->gexec);
    b->gexec = nullptr;
}

// The batch's launch resources: its two streams and timing events (or a verify scratch's) and the
// pinned readback.  Made when the batch is prepared (and on the first launch of one prepared
// before): creating streams, events and pinned memory waits on the device, so doing it at a
// batch's first launch stalled the other batches in flight (a run whose resident batches first
// launch inside a timed region: config 4 at 512 proofs and 10 in flight, 5 warm-up steps, ran at a
// quarter of its rate).
int launch_resources(nhip_batch* b) {
    LaunchRes& r = *b->res;
    const bool own = !b->borrowed();
    if (!b->timed) {
        const char* pm = nhip::ab_env("NHIP_PHASE_MARKS");  // A/B: 0 = the phase events off
        b->tm.phase_marks = !(pm && pm[0] == '0');
        if (!r.made) {
            for (int i = 0; i < STARK_EVENTS; ++i)
                if (hipEventCreate(&r.ev[i]) != hipSuccess) return NHIP_ERR_HIP;
            // a resident batch's per-launch events (the verify scratch's launches have none)
            for (uint32_t i = 0; own && i < 2 * MAX_HASH_LAUNCHES; ++i)  // per hash launch
                if (hipEventCreate(&b->tm.lev[i]) != hipSuccess) {
                    for (uint32_t j = 0; j < i; ++j) (void)hipEventDestroy(b->tm.lev[j]);
                    for (uint32_t j = 0; j < 2 * MAX_HASH_LAUNCHES; ++j) b->tm.lev[j] = nullptr;
                    break;  // untimed hash launches: a fault of the timing only
                }
            if (own) {
                hipEvent_t r0 = nullptr, r1 = nullptr;
                if (hipEventCreate(&r0) == hipSuccess && hipEventCreate(&r1) == hipSuccess) {
                    b->tm.rev[0] = r0;
                    b->tm.rev[1] = r1;
                } else if (r0) {
                    (void)hipEventDestroy(r0);  // an untimed row launch: a fault of the timing only
                }
            }
            if (hipStreamCreateWithFlags(&r.main, hipStreamNonBlocking) != hipSuccess) return NHIP_ERR_HIP;
            if (hipStreamCreateWithFlags(&r.aux, hipStreamNonBlocking) != hipSuccess) return NHIP_ERR_HIP;
            r.made = true;
        }
        for (int i = 0; i < STARK_EVENTS; ++i) b->tm.ev[i] = r.ev[i];
        b->timed = true;
    }
    // pinned readback, grown when a refill needs more: the scratch's to twice the need, a batch's own
    // by the growth rule and to 64 KB at least
    const size_t need = b->rb.host_bytes;
    if (b->mem->readback.reserve(need, true, own ? (size_t)64 << 10 : 2 * need) != hipSuccess) return NHIP_ERR_OOM;
    return NHIP_OK;
}

// Every device phase of the batch, its counter resets and its readback, on the batch's streams.
hipError_t enqueue_batch(nhip_batch* b) {
    hipStream_t st = b->res->main;
    hipError_t e = hipMemsetAsync(b->dev.counters, 0, b->rb.verdicts_off, st);
    if (e == hipSuccess) e = launch_stark_phases(b->dev, st, b->res->aux, &b->tm);
    if (e == hipSuccess)
        e = hipMemcpyAsync(b->mem->readback.p, b->dev.counters, b->rb.copy_bytes, hipMemcpyDeviceToHost, st);
    return e;
}

// A resident batch: prepared, and its launch resources made now rather than at its first launch (a
// failure there is left to the launch to report)
int prepare_resident(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                     const nhip_proof* proofs, const WireSrc* wire, size_t n, nhip_batch** out, nhip_batch* reuse) {
    if (reuse && !reuse->in_flight) {  // new contents: the captured launch sequence is stale
        const DeviceScope device_scope(reuse->device);
        drop_graph(reuse);
    }
    const int rc = batch_prepare(ctx, air, sp, claims, proofs, wire, n, out, nullptr, reuse);
    if (rc != NHIP_OK || !*out) return rc;
    std::lock_guard<std::mutex> g(*nhip_internal_mutex(ctx));
    const DeviceScope device_scope((*out)->device);
    (void)launch_resources(*out);
    return NHIP_OK;
}

// The graph bakes in the launch-order wave priority, which applies from 2,048 proofs on: larger
// batches always launch directly.
constexpr uint32_t GRAPH_MAX_PROOFS = 1024;
bool graphs_enabled() {  // NHIP_GRAPHS=0 (A/B builds only): every launch direct
    static const bool on = [] {
        const char* e = nhip::ab_env("NHIP_GRAPHS");
        return !e || e[0] != '0';
    }();
    return on;
}

// Capture the batch's launch sequence (its two streams joined, as enqueue_batch leaves them) into an
// executable graph, with the capture's own events; false (and no graph) if the runtime cannot
// capture it: the direct launch is used then.
bool capture_graph(nhip_batch* b) {
    if (!b->gev[0])
        for (int i = 0; i < STARK_EVENTS; ++i)
            if (hipEventCreateWithFlags(&b->gev[i], hipEventDisableTiming) != hipSuccess) return false;
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(b->res->main, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    StarkPhaseTimer saved = b->tm;
    for (int i = 0; i < STARK_EVENTS; ++i) b->tm.ev[i] = b->gev[i];
    b->tm.phase_marks = false;
    const hipError_t e = enqueue_batch(b);
    const uint32_t launches = b->tm.mp_hash_launches;  // the captured sequence's hash launches
    b->tm = saved;
    b->tm.mp_hash_launches = launches;
    const hipError_t ee = hipStreamEndCapture(b->res->main, &graph);
    if (e != hipSuccess || ee != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        return false;
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess || !exec) {
        (void)hipGetLastError();
        return false;
    }
    b->gexec = exec;
    return true;
}

}  // namespace

// host allocations failing inside an entry point become an error code, never an exception
// crossing the C ABI
#define NHIP_GUARD(expr)                                    \
    try {                                                   \
        return (expr);                                      \
    } catch (const std::bad_alloc&) {                       \
        return NHIP_ERR_OOM;                                \
    } catch (...) {                                         \
        return NHIP_ERR_HIP;                                \
    }

extern "C" {

int nhip_batch_prepare(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                       const nhip_proof* proofs, size_t n, nhip_batch** out) {
    NHIP_GUARD(prepare_resident(ctx, air, sp, claims, proofs, nullptr, n, out, nullptr))
}

int nhip_batch_prepare_wire(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                            const uint8_t* bytes, size_t n_bytes, const nhip_span* spans, size_t n, nhip_batch** out) {
    const WireSrc wire{bytes, n_bytes, spans};
    NHIP_GUARD(prepare_resident(ctx, air, sp, claims, nullptr, &wire, n, out, nullptr))
}

int nhip_batch_refill(nhip_ctx* ctx, nhip_batch* b, nhip_air* air, const nhip_stark_params* sp,
                      const nhip_claim* claims, const nhip_proof* proofs, size_t n) {
    if (!b) return NHIP_ERR_ARG;
    nhip_batch* out = b;
    NHIP_GUARD(prepare_resident(ctx, air, sp, claims, proofs, nullptr, n, &out, b))
}

int nhip_batch_refill_wire(nhip_ctx* ctx, nhip_batch* b, nhip_air* air, const nhip_stark_params* sp,
                           const nhip_claim* claims, const uint8_t* bytes, size_t n_bytes, const nhip_span* spans,
                           size_t n) {
    if (!b) return NHIP_ERR_ARG;
    nhip_batch* out = b;
    const WireSrc wire{bytes, n_bytes, spans};
    NHIP_GUARD(prepare_resident(ctx, air, sp, claims, nullptr, &wire, n, &out, b))
}

// Enqueue every device phase of the batch on the batch's own two streams (no host wait).  Batches
// launched back to back run concurrently on the device.
int nhip_batch_launch(nhip_ctx* ctx, nhip_batch* b) {
    if (!ctx || !b) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(*nhip_internal_mutex(ctx));
    const DeviceScope device_scope(b->device);
    if (b->in_flight) return NHIP_ERR_ARG;
    if (int rc = launch_resources(b)) return rc;
    hipError_t e = hipSuccess;
    const bool graphable = b->graph_on && !b->tm.launch_events && b->dev.n_proofs <= GRAPH_MAX_PROOFS;
    if (graphable && !b->gexec) (void)capture_graph(b);  // after a refill or a stream change
    b->last_graph = graphable && b->gexec;
    if (b->last_graph) e = hipGraphLaunch(b->gexec, b->res->main);
    else e = enqueue_batch(b);
    if (e != hipSuccess) return hipfail(e);
    b->in_flight = true;
    return NHIP_OK;
}

// Replay the batch's launch sequence from a captured HIP graph (on != 0): one submission per launch
// instead of ~25 runtime calls, for resident batches of at most 1,024 proofs relaunched many times
// (a pipeline enqueueing R batches back to back delays the device's start of the last one by R host
// enqueues, ~0.2 ms each at 512 proofs).  A launch with launch timing on is always direct; a replayed
// launch reports no phase split (nhip_stats phase fields 0).  NHIP_ERR_ARG while in flight or for a
// batch past 1,024 proofs; a runtime that cannot capture leaves the direct launch (NHIP_OK).
int nhip_batch_set_graph(nhip_batch* b, int on) {
    if (!b || b->in_flight || b->borrowed()) return NHIP_ERR_ARG;
    if (on && b->dev.n_proofs > GRAPH_MAX_PROOFS) return NHIP_ERR_ARG;
    if (on && !graphs_enabled()) return NHIP_OK;  // an A/B build with graphs off: direct launches
    const DeviceScope device_scope(b->device);
    b->graph_on = on != 0;
    if (!b->graph_on) {
        drop_graph(b);
        return NHIP_OK;
    }
    if (int rc = launch_resources(b)) return rc;
    if (!b->gexec) (void)capture_graph(b);  // now, before the batch's first replay
    return NHIP_OK;
}

// Dispatch begin / end timestamps on the batch's Merkle hash launches and its row launch (the
// bench's kernel timing: nhip_stats.ms_mp_hash_exec / ms_row_hash_exec); off by default, since
// they cost a small batch ~2% of its rate and the product paths do not read them.
int nhip_batch_set_launch_timing(nhip_batch* b, int on) {
    if (!b || b->in_flight) return NHIP_ERR_ARG;
    b->tm.launch_events = on != 0;  // a timed launch is never the graph (its events are per launch)
    return NHIP_OK;
}

// One stream or two for a resident batch.  Two (the default): the latency-bound chain (decode,
// Fiat-Shamir replay, plan, OOD / FRI / DEEP) and the VALU-bound hashing overlap within the batch.
// One: every phase in order on the main stream, one hardware queue per batch, so a caller can keep
// twice as many batches in flight — the better trade for tiny batches run many at a time
// (BASELINE config 5's 8-64 proofs per GPU: +12-18% at twice the depth), the worse one from a few
// hundred proofs on (config 4 at 512-4,096 proofs: -10 to -23%).
int nhip_batch_set_streams(nhip_batch* b, int streams) {
    if (!b || b->in_flight || b->borrowed() || (streams != 1 && streams != 2)) return NHIP_ERR_ARG;
    const DeviceScope device_scope(b->device);
    if (int rc = launch_resources(b)) return rc;
    LaunchRes& r = *b->res;
    const bool had_graph = b->gexec != nullptr;
    if (streams == 1 && r.aux != r.main) {
        drop_graph(b);
        (void)hipStreamSynchronize(r.aux);
        (void)hipStreamDestroy(r.aux);
        r.aux = r.main;
    } else if (streams == 2 && r.aux == r.main) {
        drop_graph(b);
        hipStream_t s2 = nullptr;
        if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) return NHIP_ERR_HIP;
        r.aux = s2;
    }
    if (had_graph && b->graph_on && !b->gexec) (void)capture_graph(b);  // the new stream layout, now
    return NHIP_OK;
}

// Internal (queue.cpp): has every phase of a launched batch completed?  Its last packets (the verdict
// copy) are on the main stream, which joins the aux chain before them.
bool nhip_internal_batch_done(nhip_batch* b) {
    if (!b || !b->in_flight) return true;
    const DeviceScope device_scope(b->device);
    return hipStreamQuery(b->res->main) != hipErrorNotReady;
}

// Wait for a launched batch; verdicts (n bytes, nullable) and the batch AND (nullable).
int nhip_batch_wait(nhip_ctx* ctx, nhip_batch* b, uint8_t* verdicts, uint8_t* all_ok) {
    if (!ctx || !b) return NHIP_ERR_ARG;
    if (!b->in_flight) return NHIP_ERR_ARG;
    const DeviceScope device_scope(b->device);
    hipError_t e = hipStreamSynchronize(b->res->main);
    b->in_flight = false;
    if (e != hipSuccess) return hipfail(e);
    const uint32_t n = b->dev.n_proofs;
    const uint8_t* h_out = (const uint8_t*)b->mem->readback.p;
    // Merkle permutations: multiproof ops reserved by the plan (per level and shard) minus the ops of
    // trees whose authentication structure failed, plus the last-codeword trees; the sponge + row
    // permutations of the proofs k_decode accepted
    uint64_t cnt[CNT_N], reserved = 0;
    std::memcpy(cnt, h_out, sizeof(cnt));
    for (size_t at = b->rb.plan_counters_off; at < b->rb.verdicts_off; at += 4) {
        uint32_t c;
        std::memcpy(&c, h_out + at, 4);
        reserved += c;
    }
    {  // the hash launches' own durations (dispatch begin / end timestamps; launch timing on)
        double exec = 0;
        const bool ev = b->tm.launch_events;
        const uint32_t nl = ev ? std::min<uint32_t>(b->tm.mp_hash_launches, MAX_HASH_LAUNCHES) : 0u;
        for (uint32_t i = 0; i < nl && b->tm.lev[0]; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, b->tm.lev[2 * i], b->tm.lev[2 * i + 1]) == hipSuccess) exec += ms;
        }
        b->mp_hash_exec_ms = exec;
        float rms = 0.f;
        b->row_hash_exec_ms =
            ev && b->tm.rev[0] && hipEventElapsedTime(&rms, b->tm.rev[0], b->tm.rev[1]) == hipSuccess ? rms : 0.0;
    }
    b->H.perms_static = cnt[CNT_PERMS_STATIC];
    b->H.perms_lcw = cnt[CNT_PERMS_LCW];
    b->merkle_perms = reserved - cnt[CNT_MP_SKIPPED] + b->H.perms_lcw;
    // each phase between the events the launch's plan brackets it with
    auto el = [&](PhaseSpan s) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, b->tm.ev[s.from], b->tm.ev[s.to]);
        return (double)ms;
    };
    if (b->last_graph || !b->tm.phase_marks) {
        b->ph = {};  // a replayed launch (its events are the graph's own, untimed) or one without marks
    } else if (n) {
        const PhaseBrackets& sp = b->tm.spans;
        b->ph.decode = el(sp.decode);
        b->ph.fs = el(sp.fs);
        b->ph.rows = el(sp.rows);
        b->ph.plan = el(sp.plan);
        b->ph.hash = std::min(el(sp.hash[0]), el(sp.hash[1]));
        b->ph.roots = el(sp.roots);
        b->ph.ood = el(sp.ood);
        b->ph.fri = el(sp.fri);
        b->ph.deep = el(sp.deep);
        b->ph.total = el(sp.total);
    }
    const uint8_t* v = h_out + b->rb.verdicts_off;
    if (verdicts && n) std::memcpy(verdicts, v, n);
    if (all_ok) {
        uint8_t a = 1;
        for (uint32_t i = 0; i < n; ++i) a &= v[i];
        *all_ok = a;
    }
    return NHIP_OK;
}

int nhip_batch_run(nhip_ctx* ctx, nhip_batch* b, uint8_t* verdicts, uint8_t* all_ok) {
    const int rc = nhip_batch_launch(ctx, b);
    if (rc) return rc;
    return nhip_batch_wait(ctx, b, verdicts, all_ok);
}

int nhip_batch_stats(const nhip_batch* b, nhip_stats* s) {
    if (!b || !s) return NHIP_ERR_ARG;
    std::memset(s, 0, sizeof(*s));
    s->num_proofs = b->dev.n_proofs;
    s->proof_words = b->H.proof_words;
    s->ms_decode = b->stage_ms;
    s->ms_upload = b->upload_ms;
    s->ms_fiat_shamir = b->ph.fs;
    s->ms_row_hash = b->ph.rows;
    s->ms_merkle = b->ph.plan + b->ph.hash + b->ph.roots;
    s->ms_merkle_hash = b->ph.hash;
    s->merkle_hash_launches = b->tm.mp_hash_launches;
    s->ms_ood_air = b->ph.ood;
    s->ms_fri = b->ph.fri;
    s->ms_deep = b->ph.deep;
    s->ms_device_total = b->ph.total;
    s->ms_device_decode = b->ph.decode;
    s->ms_mp_hash_exec = b->mp_hash_exec_ms;
    s->ms_row_hash_exec = b->row_hash_exec_ms;
    s->tip5_perms_static = b->H.perms_static;
    s->tip5_perms_merkle = b->merkle_perms;
    // every Merkle hash launch (k_mp_hash + the 16-lane-row k_mp_hash_wide): back to back on the
    // batch's main stream, so the phase span is their summed duration
    s->ms_mp_hash_kernel = b->ph.hash;
    s->mp_hash_kernel_launches = b->tm.mp_hash_launches;
    s->mp_hash_kernel_perms = b->merkle_perms;
    return NHIP_OK;
}

int nhip_batch_transcript(nhip_ctx* ctx, const nhip_batch* b, size_t proof, uint64_t* xfe_out, size_t xfe_cap,
                          uint32_t* idx_out, size_t idx_cap, uint32_t* fail_out, size_t* n_xfe) {
    if (!ctx || !b || proof >= b->dev.n_proofs || b->in_flight) return NHIP_ERR_ARG;
    std::lock_guard<std::mutex> g(*nhip_internal_mutex(ctx));
    const DeviceScope device_scope(b->device);
    hipStream_t st = nhip_internal_stream(ctx);
    ProofDesc pd{};
    hipError_t e = hipMemcpyAsync(&pd, b->dev.desc + proof, sizeof(pd), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hipfail(e);
    const size_t nx = pd.n_xs;
    if (n_xfe) *n_xfe = nx;
    std::vector<uint64_t> raw(nx * 3);
    if (nx) e = hipMemcpyAsync(raw.data(), b->dev.xs + pd.xs_off * 3, nx * 24, hipMemcpyDeviceToHost, st);
    std::vector<uint32_t> ix(b->dev.dims.num_checks);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ix.data(), b->dev.idx + pd.idx_off, ix.size() * 4, hipMemcpyDeviceToHost, st);
    uint32_t f = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&f, b->dev.fail + proof, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hipfail(e);
    if (xfe_out)
        for (size_t i = 0; i < std::min(nx * 3, xfe_cap * 3); ++i) xfe_out[i] = from_mont(raw[i]);
    if (idx_out) std::memcpy(idx_out, ix.data(), std::min(ix.size(), idx_cap) * 4);
    if (fail_out) *fail_out = f;
    return NHIP_OK;
}

// Releases what the batch owns: the graph and its events always, the per-launch events, streams and
// memory of a resident batch (a verify scratch's stay with the context).
void nhip_batch_destroy(nhip_batch* b) {
    if (!b) return;
    const DeviceScope device_scope(b->device);
    if (b->in_flight && b->res->main) (void)hipStreamSynchronize(b->res->main);
    drop_graph(b);
    for (hipEvent_t e : b->gev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->tm.lev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->tm.rev)
        if (e) (void)hipEventDestroy(e);
    b->own_res.destroy();
    b->own_mem.release();
    delete b;
}

static int verify_batch_from(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                             const nhip_proof* proofs, const WireSrc* wire, size_t n, uint8_t* verdicts,
                             nhip_stats* stats) {
    if (!verdicts && n) return NHIP_ERR_ARG;
    if (!ctx) return NHIP_ERR_ARG;
    auto* scr = (VerifyScratch*)nhip_internal_verify_scratch(
        ctx, []() -> void* { return new (std::nothrow) VerifyScratch(); }, &free_verify_scratch);
    if (!scr) return NHIP_ERR_OOM;
    std::lock_guard<std::mutex> g(scr->mu);
    nhip_batch* b = nullptr;
    int rc;
    try {
        rc = batch_prepare(ctx, air, sp, claims, proofs, wire, n, &b, scr);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
    if (rc) return rc;
    rc = nhip_batch_run(ctx, b, verdicts, nullptr);
    if (!rc && stats) nhip_batch_stats(b, stats);
    nhip_batch_destroy(b);
    return rc;
}

int nhip_verify_batch(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                      const nhip_proof* proofs, size_t n, uint8_t* verdicts, nhip_stats* stats) {
    return verify_batch_from(ctx, air, sp, claims, proofs, nullptr, n, verdicts, stats);
}

int nhip_verify_batch_wire(nhip_ctx* ctx, nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claims,
                           const uint8_t* bytes, size_t n_bytes, const nhip_span* spans, size_t n, uint8_t* verdicts,
                           nhip_stats* stats) {
    const WireSrc wire{bytes, n_bytes, spans};
    return verify_batch_from(ctx, air, sp, claims, nullptr, &wire, n, verdicts, stats);
}

}  // extern "C"
