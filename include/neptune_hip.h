/*
 * neptune_hip.h — C ABI of libneptune_hip.so, the MI355X (gfx950) batched verifier
 * library for neptune-core's proof-validation hot path.
 *
 * Conventions (mirroring the reference's Rust types; see INTEGRATION.md for bindings):
 *   - Field elements are passed as canonical u64 (BFieldElement::value()).  Inputs >= p are
 *     reduced mod p, i.e. BFieldElement::new semantics.  The STARK entry points also take them as
 *     they lie in a `Vec<BFieldElement>` (nhip_stark_params.input_form = NHIP_INPUT_MONTGOMERY:
 *     twenty-first's raw word x * 2^64 mod p), so a `Proof` is handed over without a copy.
 *   - A Digest is 5 consecutive u64 (Digest::values()), 40 bytes.
 *   - The caller owns every buffer; buffers are borrowed for the duration of the call.
 *   - Return value: 0 (NHIP_OK) or an infrastructure error code (no device, HIP failure,
 *     out of memory, bad argument).  A verification *failure* is never an error: it is a
 *     verdict byte 0.  Callers must treat a non-zero return as "unknown", never as "accept"
 *     (SURVEY.md §8b).
 *   - Thread safety: a context may be shared by threads; calls on one context are serialized
 *     onto that context's HIP stream.
 *   - Every entry point leaves the calling thread's current HIP device as it found it (a host
 *     with its own HIP user, e.g. torch, is not disturbed).
 *   - One context drives one GPU.  Every GPU of a node is driven from the one neptune-core
 *     process by a group (nhip_group_*: one context per member device, batches LPT-sharded at
 *     proof granularity, verdicts merged on the host; nhip_group_stream_* for batch after batch).
 *     The multi-process form (one rank per GPU, one RCCL verdict all-gather per step) is the
 *     Python host's neptune_hip.shard / bench.py.
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   nhip_tip5_hash_pair     <- twenty-first 1.0.0 Tip5::hash_pair, as called by
 *                              neptune-core/src/protocol/consensus/block/pow.rs:112,130,171-175
 *   nhip_tip5_hash_varlen   <- Tip5::hash_varlen, as called by
 *                              neptune-core/src/protocol/proof_abstractions/mast_hash.rs:26,
 *                              neptune-core/src/state/wallet/wallet_entropy.rs:76-82 and the
 *                              STARK row hashing inside triton_vm::verify
 *   nhip_tip5_permutation   <- Tip5::permutation (twenty-first, the sponge core)
 *   nhip_mtree_build        <- MTree::build_inplace, neptune-core/src/protocol/consensus/block/pow.rs:73-119
 *   nhip_mtree_verify       <- MTree::verify,        neptune-core/src/protocol/consensus/block/pow.rs:162-180
 *   nhip_sponge_*           <- Tip5 Sponge (pad_and_absorb_all / squeeze / sample_indices /
 *                              sample_scalars) as driven by triton_vm's ProofStream Fiat-Shamir
 *                              (SURVEY.md §8a a13); single call site of the verifier:
 *                              neptune-core/src/protocol/proof_abstractions/verifier.rs:60-63
 */
#ifndef NEPTUNE_HIP_H
#define NEPTUNE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nhip_ctx nhip_ctx;

enum {
    NHIP_OK = 0,
    NHIP_ERR_NO_DEVICE = 1,
    NHIP_ERR_HIP = 2,
    NHIP_ERR_OOM = 3,
    NHIP_ERR_ARG = 4,
    NHIP_ERR_DECODE = 5  /* malformed bincode input (block files, peer transactions) */
};

/* ---- context --------------------------------------------------------------------------- */
/* Hardware queues per process the verifier's pipeline wants: two batches in flight, each with a
 * hashing and a latency stream, plus the context stream (streams that share a queue serialize; HIP's
 * default is 4).  HIP reads GPU_MAX_HW_QUEUES once, at its initialisation.  The library never
 * changes the environment: the operator, or the host binary's main() before it starts any thread,
 * sets GPU_MAX_HW_QUEUES (e.g. to this value) when it wants more than the default. */
#define NHIP_HW_QUEUES_RECOMMENDED 8
/* Bind to the lowest HIP device whose bit is set in device_mask (0 = device 0). */
int nhip_init(uint32_t device_mask, nhip_ctx **out);
void nhip_destroy(nhip_ctx *ctx);
const char *nhip_strerror(int code);
int nhip_device_ordinal(const nhip_ctx *ctx);
/* ABI version: major * 1000 + minor */
int nhip_abi_version(void);

/* ---- Tip5 primitives (host buffers) ----------------------------------------------------- */
/* states: n x 16 u64, permuted in place. */
int nhip_tip5_permutation(nhip_ctx *ctx, uint64_t *states, size_t n);
/* out[i] = Tip5::hash_pair(left[i], right[i]); left/right/out: n digests. */
int nhip_tip5_hash_pair(nhip_ctx *ctx, const uint64_t *left, const uint64_t *right, size_t n, uint64_t *out);
/* Ragged rows: row i = data[offsets[i] .. offsets[i+1]); offsets has n+1 entries.
 * out[i] = Tip5::hash_varlen(row i). */
int nhip_tip5_hash_varlen(nhip_ctx *ctx, const uint64_t *data, const uint64_t *offsets, size_t n, uint64_t *out);

/* ---- MTree (pow.rs) (host buffers) ------------------------------------------------------ */
/* n_leafs a power of two >= 2.  nodes_out: n_leafs digests; nodes_out[1] is the root,
 * node i = hash_pair(node 2i, node 2i+1), leaf k acts as node n_leafs + k; nodes_out[0] = 0. */
int nhip_mtree_build(nhip_ctx *ctx, const uint64_t *leafs, size_t n_leafs, uint64_t *nodes_out);
/* verdicts[i] = MTree::verify(root_i, indices[i], path_i, leafs[i]).
 * roots: n_roots digests with n_roots == 1 (shared root) or n_roots == n.
 * paths: n x depth digests (sibling of the leaf first).  verdicts: n bytes, 1 = accept. */
int nhip_mtree_verify(nhip_ctx *ctx, const uint64_t *roots, size_t n_roots, const uint64_t *indices,
                      const uint64_t *leafs, const uint64_t *paths, uint32_t depth, size_t n, uint8_t *verdicts);

/* ---- device-resident form (pointers from nhip_dev_alloc; asynchronous on the ctx stream) -- */
int nhip_dev_alloc(nhip_ctx *ctx, size_t bytes, void **dptr);
int nhip_dev_free(nhip_ctx *ctx, void *dptr);
int nhip_memcpy_h2d(nhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int nhip_memcpy_d2h(nhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int nhip_synchronize(nhip_ctx *ctx);
int nhip_tip5_permutation_dev(nhip_ctx *ctx, uint64_t *d_states, size_t n);
int nhip_tip5_hash_pair_dev(nhip_ctx *ctx, const uint64_t *d_left, const uint64_t *d_right, size_t n,
                            uint64_t *d_out);
int nhip_tip5_hash_varlen_dev(nhip_ctx *ctx, const uint64_t *d_data, const uint64_t *d_offsets, size_t n,
                              uint64_t *d_out);
int nhip_mtree_build_dev(nhip_ctx *ctx, const uint64_t *d_leafs, size_t n_leafs, uint64_t *d_nodes);
int nhip_mtree_verify_dev(nhip_ctx *ctx, const uint64_t *d_roots, size_t n_roots, const uint64_t *d_indices,
                          const uint64_t *d_leafs, const uint64_t *d_paths, uint32_t depth, size_t n,
                          uint8_t *d_verdicts);
/* *all_ok = AND of n verdict bytes (device buffer), the per-batch / per-block verdict. */
int nhip_verdicts_all_dev(nhip_ctx *ctx, const uint8_t *d_verdicts, size_t n, uint8_t *all_ok);

/* ---- batched STARK verification ---------------------------------------------------------
 * Replaces triton_vm::verify(Stark::default(), &claim, &proof) -> bool at its single production
 * call site neptune-core/src/protocol/proof_abstractions/verifier.rs:60-63, batched
 * (verify_batch) for the sequential callers proof_collection.rs:342-388, block_program.rs:51-65
 * and state/mod.rs:2226-2272.  Semantics: verdict 1 = accept, 0 = reject (any decode or
 * verification error, incl. empty / short / garbage proofs, as in the reference's reject tests).
 * The AIR is data (nhip_air_create; format in DESIGN.md §9): triton-air's generated constraints
 * are not vendored in the reference, so the AIR is supplied by the caller. */
/* How the field elements of the claims and proofs handed to the STARK entry points are given: */
enum {
    NHIP_INPUT_CANONICAL = 0,  /* canonical values (BFieldElement::value()), any u64 read mod p */
    NHIP_INPUT_MONTGOMERY = 1  /* twenty-first's in-memory words (x * 2^64 mod p, BFieldElement's
                                  repr(transparent) u64): Proof.0.as_ptr(), Digest / input /
                                  output slices as they lie, no conversion; any u64 read mod p */
};
typedef struct {
    uint32_t security_level;          /* Stark::default: 160 */
    uint32_t log2_fri_expansion;      /* 2 (expansion factor 4) */
    uint32_t num_collinearity_checks; /* security_level / log2_fri_expansion = 80; <= 256 */
    uint32_t num_main;                /* main table columns (triton-vm: 379) */
    uint32_t num_aux;                 /* auxiliary table columns (triton-vm: 88) */
    uint32_t num_quotient_segments;   /* 4 */
    uint32_t input_form;              /* NHIP_INPUT_CANONICAL (default) or NHIP_INPUT_MONTGOMERY */
} nhip_stark_params;

/* triton_vm::proof::Claim { program_digest, version, input, output } (field elements in the
 * params' input_form; version is a plain integer) */
typedef struct {
    uint64_t program_digest[5];
    uint32_t version;
    const uint64_t *input;
    size_t input_len;
    const uint64_t *output;
    size_t output_len;
} nhip_claim;

/* triton_vm::proof::Proof(Vec<BFieldElement>) */
typedef struct {
    const uint64_t *words;
    size_t len;
} nhip_proof;

typedef struct {
    uint64_t num_proofs, proof_words;
    uint64_t tip5_perms_static;  /* Fiat-Shamir + row hashing (from the proof shapes) */
    uint64_t tip5_perms_merkle;  /* authentication-structure hash_pairs performed (device-counted) + last-codeword trees */
    double ms_decode, ms_upload;  /* host: layout + staging copy (+ DMA issue), then the wait for the uploads */
    double ms_fiat_shamir, ms_row_hash, ms_merkle, ms_ood_air, ms_fri, ms_deep, ms_device_total; /* device */
    double ms_merkle_hash;          /* the per-level hash_pair launches inside ms_merkle */
    uint64_t merkle_hash_launches;  /* number of those launches (one per tree level) */
    /* the lane-per-op k_mp_hash launches only (HIP events around each launch; the small levels
     * run k_mp_hash_wide): summed kernel time, launch count, permutations they performed */
    double ms_mp_hash_kernel;
    uint64_t mp_hash_kernel_launches, mp_hash_kernel_perms;
    double ms_device_decode;        /* k_decode: the proof-stream walk on the device (every run) */
    /* the same hash launches' own durations (dispatch begin / end timestamps of each launch, as the
     * rocprofv3 kernel trace reports them), summed: ms_mp_hash_kernel minus the gaps between them */
    double ms_mp_hash_exec;
    /* the row-hashing launch's own duration (k_hash_rows: every revealed main / aux / quotient row's
     * hash_varlen; dispatch begin / end timestamps) */
    double ms_row_hash_exec;
} nhip_stats;

typedef struct nhip_air nhip_air;
typedef struct nhip_batch nhip_batch;

void nhip_stark_params_default(nhip_stark_params *out);
int nhip_air_create(const uint64_t *words, size_t n_words, nhip_air **out);
/* The OOD program compiler's options (0 = the default for each): LDS-held value slots (fewer puts the
 * rest in the per-proof global area), instructions per program step, working-slot budget.  Tests of
 * the compiler and of k_ood_air's global-slot path; nhip_air_create(w, n, out) = _ex(w, n, NULL, out). */
typedef struct {
    uint32_t lds_slots;
    uint32_t step_width;   /* 16 .. 65536 */
    uint32_t slot_budget;  /* >= 64 */
} nhip_air_options;
int nhip_air_create_ex(const uint64_t *words, size_t n_words, const nhip_air_options *options, nhip_air **out);
void nhip_air_destroy(nhip_air *air);
int nhip_air_info(const nhip_air *air, uint32_t *num_nodes, uint32_t *num_levels, uint32_t *num_constraints);
/* The OOD evaluator's value slots (liveness-allocated): those in LDS, and those past the LDS budget
 * (~6K XFEs), which live in a per-proof global area (an AIR of triton-air's size class). */
int nhip_air_slots(const nhip_air *air, uint32_t *lds_slots, uint32_t *global_slots);
/* The compiled OOD program (host only, for tools and tests of the compiler): steps + 1 step offsets
 * and 4 u32 per instruction (op, a, b, dst; stark.hpp OodIns).  NULL arrays (or too
 * small capacities) just report the sizes; NHIP_ERR_ARG when a given array is too small. */
int nhip_air_program(const nhip_air *air, uint32_t *step_off, size_t step_cap, uint32_t *ins, size_t ins_cap,
                     size_t *n_steps, size_t *n_ins);
/* The per-kind segments of that program's steps (host only): 3 bounds per step, of its copies (LOAD /
 * ACC), its products and its sums and differences, then the end of the program: 3 * steps + 1 offsets,
 * seg_off[3 s] == step_off[s].  k_ood_air runs a step segment by segment, each from its thread 0, so
 * a wave runs one kind of operation.  A NULL array just reports the count. */
int nhip_air_segments(const nhip_air *air, uint32_t *seg_off, size_t seg_cap, size_t *n_bounds);
/* Host-only structural decode (no GPU needed): 1 = decodes, 0 = malformed, < 0 = bad argument. */
int nhip_proof_decodes(const nhip_air *air, const nhip_stark_params *params, const nhip_claim *claim,
                       const nhip_proof *proof);
/* Pinned host memory for proofs: proofs whose words lie in a range from nhip_host_alloc or
 * nhip_host_register are DMA'd straight from it (no staging copy); adjacent proofs of one range
 * go as one copy.  Any other host memory works too, through the context's pinned staging. */
int nhip_host_alloc(size_t bytes, void **out);
int nhip_host_free(void *p);
int nhip_host_register(void *p, size_t bytes);
int nhip_host_unregister(void *p);
/* ---- host topology of the feed path (NUMA) -------------------------------------------------
 * The receive path of a node feeding GPU ctx: pinned memory whose pages lie on the NUMA node of
 * ctx's GPU (the socket its PCIe link ends at).  A proof deserialized into it is DMA'd as it lies
 * (no staging copy, no inter-socket traffic); free with nhip_host_free.  Falls back to unplaced
 * pinned memory when the platform reports no node.  Replaces the `Vec<BFieldElement>` a peer
 * message is decoded into (peer_loop.rs:315-323, state/mod.rs:2226-2272). */
int nhip_host_alloc_near(nhip_ctx *ctx, size_t bytes, void **out);
/* The NUMA node of ctx's GPU (-1: none reported) and that node's CPUs this process may use, read
 * from sysfs through the device's PCI bus id.  The context's pinned staging is placed on that node
 * and its staging copy threads are bound to those CPUs (NHIP_NUMA=0 disables both).  cpus may be
 * NULL (count query). */
int nhip_device_numa(nhip_ctx *ctx, int *numa_node, int *cpus, size_t cpu_cap, size_t *n_cpus);
/* The same lookup under another sysfs root (host-only, no GPU: tests use fixture trees) for a PCI
 * bus id "dddd:bb:dd.f": <root>/bus/pci/devices/<id>/numa_node, then
 * <root>/devices/system/node/node<N>/cpulist. */
int nhip_numa_from_sysfs(const char *sysfs_root, const char *pci_bus_id, int *numa_node, int *cpus, size_t cpu_cap,
                         size_t *n_cpus);
/* Parse a kernel cpulist ("0-3,8,10-15:2") into sorted CPU ids (host-only). */
int nhip_cpulist_parse(const char *list, int *cpus, size_t cpu_cap, size_t *n_cpus);
/* The NUMA node holding the page at ptr (-1 if unknown; host-only). */
int nhip_host_page_node(const void *ptr);
/* Staging copy threads per upload for this context (0 = default: up to 16, at most its NUMA
 * node's CPUs).  A group sets each member's share of its node's CPUs. */
int nhip_set_host_threads(nhip_ctx *ctx, unsigned threads);
/* One-shot: upload, decode (on the device), verify, verdicts[n]. */
int nhip_verify_batch(nhip_ctx *ctx, nhip_air *air, const nhip_stark_params *params, const nhip_claim *claims,
                      const nhip_proof *proofs, size_t n, uint8_t *verdicts, nhip_stats *stats);
/* Device-resident form: prepare (stage + one upload of the raw proof words), run (every device
 * phase, starting with the proof-stream decode) any number of times, read stats / the
 * Fiat-Shamir transcript of one proof, destroy. */
int nhip_batch_prepare(nhip_ctx *ctx, nhip_air *air, const nhip_stark_params *params, const nhip_claim *claims,
                       const nhip_proof *proofs, size_t n, nhip_batch **out);
/* Refill an idle batch in place with new proofs (same semantics as prepare; its streams,
 * events and device memory are reused when large enough).  Streaming from host memory:
 * launch(A); refill(B, next); wait(A); launch(B); refill(A, next); ... overlaps each host decode
 * + upload with the other batch's device run.  On failure the batch is left empty (n = 0). */
int nhip_batch_refill(nhip_ctx *ctx, nhip_batch *batch, nhip_air *air, const nhip_stark_params *params,
                      const nhip_claim *claims, const nhip_proof *proofs, size_t n);
int nhip_batch_run(nhip_ctx *ctx, nhip_batch *batch, uint8_t *verdicts, uint8_t *all_ok);
/* Asynchronous form of nhip_batch_run: launch enqueues every phase on the batch's own streams and
 * returns; wait blocks until that batch is done.  Batches launched back to back run concurrently
 * (e.g. two half-batches overlap each other's latency-bound tails). */
int nhip_batch_launch(nhip_ctx *ctx, nhip_batch *batch);
int nhip_batch_wait(nhip_ctx *ctx, nhip_batch *batch, uint8_t *verdicts, uint8_t *all_ok);
int nhip_batch_stats(const nhip_batch *batch, nhip_stats *stats);
/* Per-dispatch begin / end timestamps on the batch's Merkle hash launches and its row-hashing
 * launch, read back as nhip_stats.ms_mp_hash_exec / ms_row_hash_exec (0 when off).  Off by
 * default; a benchmark's kernel timing turns it on.  NHIP_ERR_ARG while the batch is in flight. */
int nhip_batch_set_launch_timing(nhip_batch *batch, int on);
/* 2 (default): the batch's latency-bound chain and its hashing run on two streams and overlap; 1:
 * every phase in order on one stream (one hardware queue), so twice as many batches fit in flight —
 * for many tiny batches at once (e.g. 8-64 proofs each).  NHIP_ERR_ARG while in flight. */
int nhip_batch_set_streams(nhip_batch *batch, int streams);
/* on != 0: every later untimed launch replays the batch's launch sequence from a captured HIP graph
 * (one submission instead of ~25 runtime calls), captured now and again after a refill or a stream
 * change — for resident batches of at most 1,024 proofs relaunched many times (a pipeline enqueueing
 * batches back to back otherwise delays each batch's device start by the host enqueues before it).
 * A replayed launch reports no phase split (nhip_stats phase fields 0; launch timing on = direct).
 * NHIP_ERR_ARG while in flight or past 1,024 proofs. */
int nhip_batch_set_graph(nhip_batch *batch, int on);
/* Fiat-Shamir replay form of later launches, process-wide (tests and A/B runs): -1 = chosen by the
 * batch size (default), 0 = 16-lane row, 1 = two-row pair, 2 = quad.  NHIP_ERR_ARG otherwise. */
int nhip_set_fs_form(int form);
/* Merkle climb-from threshold of later launches, process-wide (tests): -1 = the default (trees of
 * at least 24 hash levels hand their remaining levels to one per-tree climb launch at the first level
 * with at most 4,096 hash ops), 0 = never, k > 0 = at k ops for every depth. */
int nhip_set_climb_from_ops(int64_t ops);
/* Samples squeezed for proof `proof` in squeeze order (challenges, quotient weights, z, linear-
 * combination weights, FRI folding challenges, last-round indeterminate) as canonical XFE
 * triples, the FRI indices, and the proof's failure bits (0 = accepted). */
int nhip_batch_transcript(nhip_ctx *ctx, const nhip_batch *batch, size_t proof, uint64_t *xfe_out, size_t xfe_cap,
                          uint32_t *idx_out, size_t idx_cap, uint32_t *fail_bits, size_t *n_xfe);
void nhip_batch_destroy(nhip_batch *batch);

/* ---- coalescing queue for concurrent single-proof callers ---------------------------------
 * The reference calls triton_vm::verify once per proof from many tokio tasks at once
 * (verifier.rs:60-63; e.g. peer_loop.rs:1342 per peer transaction).  nhip_queue_verify is that
 * call: blocking, thread-safe, nhip_verify_batch semantics for its own proofs; a worker thread
 * gathers the proofs of every caller waiting at the time (up to max_batch proofs, at most
 * max_wait_us after the oldest arrival) into one device batch, with the next batch collected while
 * the current one runs.  Each caller copies its proofs into the queue's pinned arena itself (in
 * parallel with the other callers), so the worker only DMAs them; a request the arena cannot hold
 * at the time goes through the context's staging instead.  max_batch 0 = 4096.
 * Pinned footprint: the arena is min(256 MB, max(16 MB, 4 MB x max_batch)) of pinned host memory
 * per queue; the environment variable NHIP_QUEUE_ARENA_MB (read at create) sets it instead, 0 for
 * none. */
typedef struct nhip_queue nhip_queue;
int nhip_queue_create(nhip_ctx *ctx, nhip_air *air, const nhip_stark_params *params, uint32_t max_batch,
                      uint32_t max_wait_us, nhip_queue **out);
int nhip_queue_verify(nhip_queue *queue, const nhip_claim *claims, const nhip_proof *proofs, size_t n,
                      uint8_t *verdicts);
/* batches launched and proofs verified so far */
int nhip_queue_stats(const nhip_queue *queue, uint64_t *batches, uint64_t *proofs);
/* Where a queue's time goes, summed over its batches since creation (or the last reset). */
typedef struct {
    uint64_t batches, proofs;
    uint64_t size_hist[8];   /* batches of 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64-127, >= 128 proofs */
    double ms_window;        /* oldest request's arrival -> its batch's staging starts (coalescing wait) */
    double ms_stage;         /* host: layout + staging copy + DMA issue of the batch's proofs */
    double ms_upload;        /* host: the wait for those uploads */
    double ms_launch;        /* host: enqueueing the batch's device phases */
    double ms_device;        /* device: first phase start -> verdicts (k_decode to the verdict copy) */
    double ms_wait;          /* worker blocked in nhip_batch_wait on the batch (not overlapped) */
    double ms_turnaround;    /* oldest request's arrival -> its verdicts delivered */
    uint64_t pinned_proofs;  /* proofs their caller's thread copied into the queue's pinned arena (DMA'd
                                from there without a staging copy on the worker) */
} nhip_queue_profile;
int nhip_queue_profile_read(const nhip_queue *queue, nhip_queue_profile *out, int reset);
/* Per-request latency in microseconds (a caller's arrival in nhip_queue_verify -> its verdicts
 * delivered), the last 65,536 requests oldest first: *n = how many are held; up to cap written.
 * reset != 0 forgets them. */
int nhip_queue_latencies(const nhip_queue *queue, float *us_out, size_t cap, size_t *n, int reset);
/* Drains the pending requests, then stops the worker. */
void nhip_queue_destroy(nhip_queue *queue);

/* ---- several GPUs from one process --------------------------------------
 * neptune-core is one process; its batch callers (proof_collection.rs:342-388,
 * state/mod.rs:2226-2272, peer_loop.rs:315-323) end in n calls of triton_vm::verify at
 * verifier.rs:60-63.  A group owns one context per member device (duplicates allowed: several
 * contexts on one GPU).  nhip_group_verify_batch shards the proofs over the members (LPT on the
 * proof length, nhip_group_shard), verifies every shard concurrently on its member (one host
 * thread each, nhip_verify_batch semantics) and writes the verdicts in the caller's order;
 * *all_ok (nullable) = AND of the verdicts.  A non-zero return (any member's infrastructure
 * fault) leaves the verdicts unknown: never "accept". */
typedef struct nhip_group nhip_group;
int nhip_group_create(const int *devices, size_t n_devices, nhip_group **out);
/* One member per set bit of device_mask (0 = every visible device). */
int nhip_group_init(uint32_t device_mask, nhip_group **out);
void nhip_group_destroy(nhip_group *group);
size_t nhip_group_size(const nhip_group *group);
/* Borrowed member context (NULL when i is out of range). */
nhip_ctx *nhip_group_member(nhip_group *group, size_t i);
/* member_of[i] = the member proof i goes to: longest proofs first, each to the least-loaded
 * member (host only, deterministic). */
int nhip_group_shard(const nhip_proof *proofs, size_t n, size_t n_members, uint32_t *member_of);
int nhip_group_verify_batch(nhip_group *group, nhip_air *air, const nhip_stark_params *params,
                            const nhip_claim *claims, const nhip_proof *proofs, size_t n, uint8_t *verdicts,
                            uint8_t *all_ok);
/* Streaming form for callers that verify batch after batch (bootstrap import state/mod.rs:2226-2272,
 * block batches peer_loop.rs:315-323): every member keeps two device batches, so each member's share
 * of the next batch is staged and uploaded while the member's share of the current one still runs.
 * nhip_group_stream_submit shards the batch over the members (nhip_group_shard), refills each
 * member's idle device batch with its share and launches it, then waits for the PREVIOUS submitted
 * batch and writes its verdicts / AND into the buffers given with that batch.  When it returns, the
 * claims / proofs of this batch may be reused (they are on the devices); its `verdicts` (n bytes)
 * and `all_ok` (nullable) stay borrowed until the next submit or nhip_group_stream_finish writes
 * them.  A non-zero return is an infrastructure fault: the batches in flight are drained and their
 * verdicts are unknown (never "accept"); the stream stays usable. */
typedef struct nhip_group_stream nhip_group_stream;
int nhip_group_stream_create(nhip_group *group, nhip_air *air, const nhip_stark_params *params,
                             nhip_group_stream **out);
int nhip_group_stream_submit(nhip_group_stream *stream, const nhip_claim *claims, const nhip_proof *proofs,
                             size_t n, uint8_t *verdicts, uint8_t *all_ok);
/* nhip_group_stream_submit with the caller's placement: proof i goes to member member_of[i] (< the
 * group's size) instead of nhip_group_shard's.  For proofs decoded into a member's arena
 * (nhip_arena_ingest_*, which return that placement): each member's share then lies adjacent in
 * pinned memory on its GPU's node and is DMA'd as it lies. */
int nhip_group_stream_submit_placed(nhip_group_stream *stream, const nhip_claim *claims, const nhip_proof *proofs,
                                    const uint32_t *member_of, size_t n, uint8_t *verdicts, uint8_t *all_ok);
/* Waits for the last submitted batch and writes its verdicts. */
int nhip_group_stream_finish(nhip_group_stream *stream);
/* Host / device milliseconds of the stream's batches so far (summed over members: stage = host
 * staging copy + DMA issue, upload = the wait for it, device = the members' device time). */
int nhip_group_stream_stats(const nhip_group_stream *stream, uint64_t *batches, uint64_t *proofs, double *ms_stage,
                            double *ms_upload, double *ms_device);
void nhip_group_stream_destroy(nhip_group_stream *stream);

/* ---- ingestion formats -------------------------------------------
 * Proof files of neptune-core/src/protocol/proof_abstractions/tasm/program.rs:374-390: 8-byte
 * big-endian chunks, each BFieldElement::new (reduced mod p); n_bytes not a multiple of 8 ->
 * NHIP_ERR_ARG (the reference returns None).  words == NULL: size query (*n_words). */
int nhip_proof_from_be_bytes(const uint8_t *bytes, size_t n_bytes, uint64_t *words, size_t cap, size_t *n_words);
/* Writer side (program.rs:565-572): value().to_be_bytes() per element; out: 8 * n bytes. */
int nhip_proof_to_be_bytes(const uint64_t *words, size_t n, uint8_t *out);
/* Tip5::hash(claim) = hash_varlen(claim.encode()) (program.rs:355-358, proof file name). */
int nhip_claim_hash(nhip_ctx *ctx, const nhip_claim *claim, uint64_t digest_out[5]);

/* ---- block files and peer transactions ----------------------------
 * bincode 1.x as neptune-core writes them; host-only, no GPU.  Field lists, BFieldCodec rules and
 * their pin status: neptune-core_amd/csrc/bincode.cpp and DESIGN.md §8f.
 *
 * Block files replace `blocks_from_file_without_record`
 * (state/archival_state/import_blocks_from_files.rs:100-115): blocks back to back, each
 * `bincode::deserialize::<Block>` then advance by its serialized size; a malformed block fails the
 * whole file (NHIP_ERR_DECODE; *n_blocks = the blocks before it).  pow_tree_height is BlockPow's
 * MERKLE_TREE_HEIGHT (pow.rs:33-37: 29, 10 in the reference's test builds). */
enum { NHIP_BLOCK_PROOF_GENESIS = 0, NHIP_BLOCK_PROOF_INVALID = 1, NHIP_BLOCK_PROOF_SINGLE = 2 };
typedef struct {
    uint64_t offset, size;          /* the block's bytes in the buffer */
    uint64_t height, timestamp;     /* BlockHeader::height, ::timestamp (canonical) */
    uint64_t prev_block_digest[5];
    uint32_t proof_kind;            /* BlockProof variant (block/mod.rs:114-119) */
    uint32_t n_claims;              /* BlockAppendix claims */
    uint64_t proof_offset;          /* SingleProof: byte offset of Proof.0's first word */
    uint64_t proof_len;             /* SingleProof: words */
    uint64_t kernel_offset;         /* byte offset of body.transaction_kernel */
    uint64_t appendix_offset;       /* byte offset of the appendix claims */
    uint64_t claim_words;           /* input + output words of all appendix claims */
    uint64_t seq_words;             /* words of nhip_blk_sequences' output (0 on a count-only scan) */
} nhip_blk_block;
/* blocks == NULL: count only.  Otherwise cap >= the block count. */
int nhip_blk_scan(const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height, nhip_blk_block *blocks,
                  size_t cap, size_t *n_blocks);
/* BFieldCodec MAST sequences: the transaction kernel's 8 (transaction_kernel.rs:246-277), then the
 * body's sequences 2-4 (block_body.rs:175-182: mutator set accumulator, lock-free MMR, block MMR;
 * sequence 1 is the kernel's MAST hash).  Sequence i = words[offsets[i] .. offsets[i+1]);
 * words == NULL: offsets only (offsets[11] = total words). */
int nhip_blk_sequences(const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block *block,
                       uint64_t *words, size_t cap, uint64_t offsets[12]);
/* The appendix claims: claims[n_claims] whose input / output point into words[claim_words]. */
int nhip_blk_claims(const uint8_t *bytes, size_t n_bytes, const nhip_blk_block *block, uint64_t *words,
                    nhip_claim *claims);
/* n little-endian u64 words at byte `offset` (any alignment), reduced mod p: proof words straight
 * into a (pinned) staging buffer. */
int nhip_le_words(const uint8_t *bytes, size_t n_bytes, uint64_t offset, size_t n, uint64_t *out);
/* A run of field words inside a byte buffer: byte offset of the first word (any alignment), words. */
typedef struct {
    uint64_t offset, len;
} nhip_span;
/* The device counterpart of nhip_le_words: out (host, the sum of the spans' len words, spans back to
 * back in order) = the spans' words gathered and reduced on the GPU (k_wire_words), bit-exact with
 * nhip_le_words for each span.  bytes is DMA'd as it lies when it is pinned (nhip_host_alloc*,
 * nhip_host_register), else it goes through the context's pinned staging.  Spans may overlap or
 * repeat; one that leaves the buffer is NHIP_ERR_ARG. */
int nhip_le_words_gpu(nhip_ctx *ctx, const uint8_t *bytes, size_t n_bytes, const nhip_span *spans, size_t n,
                      uint64_t *out);

/* Peer transactions: `TransferTransaction { kernel, proof }` (protocol/peer/transfer_transaction.rs:31-47). */
enum { NHIP_TX_PROOF_COLLECTION = 0, NHIP_TX_SINGLE_PROOF = 1 };
typedef struct {
    uint64_t size;                  /* bytes consumed */
    uint32_t kind;                  /* TransferTransactionProof variant */
    uint32_t n_proofs;              /* 1, or ProofCollection::num_proofs() */
    uint32_t n_lock_scripts, n_type_scripts;    /* lock_scripts_halt / type_scripts_halt lengths */
    uint32_t n_lock_hashes, n_type_hashes, n_merge_path;
    uint32_t n_digests;             /* n_lock_hashes + n_type_hashes + 3 + n_merge_path (ProofCollection) */
    uint64_t seq_words;             /* words of the kernel's 8 MAST sequences */
} nhip_tx;
int nhip_tx_scan(const uint8_t *bytes, size_t n_bytes, nhip_tx *tx);
/* seq_words[tx->seq_words] + seq_offsets[9]: the kernel's MAST sequences; proof_spans[2 * n_proofs]:
 * (byte offset, word count) per proof in ProofCollection field order (removal_records_integrity,
 * collect_lock_scripts, lock_scripts_halt.., kernel_to_outputs, collect_type_scripts,
 * type_scripts_halt..; proof_collection.rs:36-49); digests[5 * n_digests]: lock_script_hashes,
 * type_script_hashes, kernel_mast_hash, salted_inputs_hash, salted_outputs_hash, merge_bit_mast_path. */
int nhip_tx_parts(const uint8_t *bytes, size_t n_bytes, const nhip_tx *tx, uint64_t *seq_words,
                  uint64_t seq_offsets[9], uint64_t *proof_spans, uint64_t *digests);

/* ---- per-member proof arenas: wire bytes decoded straight into pinned memory per GPU (§8f row 2)
 * The receive side of the feed path.  An arena set holds, for every member of a group, bytes_per_member
 * of pinned host memory on that member GPU's NUMA node (nhip_host_alloc_near).  The ingest functions
 * scan bincode bytes (blk files: import_blocks_from_files.rs:100-115; peer TransferTransactions:
 * transfer_transaction.rs:31-47), give each proof to the least-loaded member with room (by words) and
 * decode its words (8-byte little-endian, reduced mod p: nhip_le_words, i.e. canonical values ->
 * nhip_stark_params.input_form NHIP_INPUT_CANONICAL) straight into that member's arena, on copy
 * threads bound to the member's node (NHIP_HOST_THREADS, else the group's share per member).  They
 * return nhip_proof records pointing into the arenas and each proof's member, ready for
 * nhip_group_stream_submit_placed.  The arena's proofs stay valid until nhip_arena_reset; reset only
 * after the submit of the batch holding them has returned (its words are then on the devices).
 * Double-buffer with two arena sets to decode batch k + 1 while batch k uploads. */
typedef struct nhip_arena nhip_arena;
int nhip_arena_create(nhip_group *group, size_t bytes_per_member, nhip_arena **out);
void nhip_arena_destroy(nhip_arena *arena);
int nhip_arena_reset(nhip_arena *arena);
/* words placed since the last reset, capacity in words, and the NUMA node of the member's pages
 * (-1: unknown); each output nullable */
int nhip_arena_member_info(const nhip_arena *arena, size_t member, uint64_t *used_words, uint64_t *cap_words,
                           int *page_node);
/* Proofs given as n (byte offset, word count) pairs `spans` of bytes[n_bytes].  NHIP_ERR_OOM when an
 * arena cannot take a proof (the ones before it are placed and decoded). */
int nhip_arena_ingest_spans(nhip_arena *arena, const uint8_t *bytes, size_t n_bytes, const uint64_t *spans, size_t n,
                            nhip_proof *proofs, uint32_t *member_of);
/* Back-to-back TransferTransactions: up to max_txs of them, every proof (a SingleProof's one, a
 * ProofCollection's in field order) in stream order.  Stops early with NHIP_OK, before the
 * transaction that does not fit, when proof_cap or the arenas are full (*consumed < n_bytes: submit,
 * reset, continue from there); NHIP_ERR_DECODE at a malformed transaction (those before it are placed
 * and counted).  *n_txs, *n_proofs, *consumed nullable. */
int nhip_arena_ingest_txs(nhip_arena *arena, const uint8_t *bytes, size_t n_bytes, size_t max_txs, nhip_proof *proofs,
                          uint32_t *member_of, size_t proof_cap, size_t *n_txs, size_t *n_proofs, size_t *consumed);
/* A blk file's bytes: the SingleProof block proof of every block (block_of[i] = its block's index;
 * nullable).  A malformed block fails the whole file (NHIP_ERR_DECODE, nothing placed); NHIP_ERR_ARG
 * when proof_cap is short of the file's SingleProof blocks, NHIP_ERR_OOM when the arenas are. */
int nhip_arena_ingest_blocks(nhip_arena *arena, const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height,
                             nhip_proof *proofs, uint32_t *member_of, uint64_t *block_of, size_t proof_cap,
                             size_t *n_proofs, size_t *n_blocks);

/* ---- in-place submission: proofs verified from the wire bytes as they lie -----
 * The arena path above reads the receive buffer once and writes the pinned arena once before the DMA
 * reads it: with the receive itself, four host-DRAM passes per proof byte.  Here the receive buffer IS
 * the pinned memory (nhip_host_alloc_near): the scanners below only find the proofs (no word copied),
 * the spans' bytes are DMA'd as they lie, and the device gathers them into the batch's aligned word
 * buffer (two passes).  bincode's Vec<BFieldElement> is already canonical 8-byte little-endian words,
 * so params->input_form must be NHIP_INPUT_CANONICAL (else NHIP_ERR_ARG); every word is reduced mod p
 * on the device (BFieldElement::new), so the batch holds the bits the arena path would.
 *
 * Scanners (host only, no GPU).  Back-to-back TransferTransactions (transfer_transaction.rs:31-47,
 * as received in peer_loop.rs:315-323): up to max_txs of them, every proof (a SingleProof's one, a
 * ProofCollection's in field order) in stream order.  Stops early with NHIP_OK, before the transaction
 * that does not fit, when span_cap is reached (*consumed < n_bytes: submit, continue from there);
 * NHIP_ERR_DECODE at a malformed transaction (those before it are counted); NHIP_ERR_ARG when the
 * first transaction alone needs more than span_cap spans (never NHIP_OK with *consumed == 0 on a
 * non-empty stream).  *n_txs, *n_proofs, *consumed nullable. */
int nhip_wire_scan_txs(const uint8_t *bytes, size_t n_bytes, size_t max_txs, nhip_span *spans, size_t span_cap,
                       size_t *n_txs, size_t *n_proofs, size_t *consumed);
/* A blk file's bytes (import_blocks_from_files.rs:100-115): the SingleProof block proof of every
 * block (block_of[i] = its block's index; nullable).  A malformed block fails the whole file
 * (NHIP_ERR_DECODE, no span returned); NHIP_ERR_ARG when span_cap is short of the file's SingleProof
 * blocks. */
int nhip_wire_scan_blocks(const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height, nhip_span *spans,
                          uint64_t *block_of, size_t span_cap, size_t *n_proofs, size_t *n_blocks);
/* nhip_verify_batch / nhip_batch_prepare / nhip_batch_refill with proof i = spans[i] of bytes[n_bytes]
 * (a span that leaves the buffer: NHIP_ERR_ARG).  The spans are sorted by offset and neighbours at
 * most 64 KB apart go as one copy, gap included; pinned bytes are DMA'd straight from the caller's
 * buffer, other memory is copied byte for byte through the context's pinned staging.  When the call
 * returns the bytes may be reused (they are on the device). */
int nhip_verify_batch_wire(nhip_ctx *ctx, nhip_air *air, const nhip_stark_params *params, const nhip_claim *claims,
                           const uint8_t *bytes, size_t n_bytes, const nhip_span *spans, size_t n, uint8_t *verdicts,
                           nhip_stats *stats);
int nhip_batch_prepare_wire(nhip_ctx *ctx, nhip_air *air, const nhip_stark_params *params, const nhip_claim *claims,
                            const uint8_t *bytes, size_t n_bytes, const nhip_span *spans, size_t n,
                            nhip_batch **out);
int nhip_batch_refill_wire(nhip_ctx *ctx, nhip_batch *batch, nhip_air *air, const nhip_stark_params *params,
                           const nhip_claim *claims, const uint8_t *bytes, size_t n_bytes, const nhip_span *spans,
                           size_t n);
/* nhip_group_stream_submit from wire bytes: proof i = spans[i] of bytes[n_bytes], placed on member
 * member_of[i], or by nhip_group_shard's rule (LPT on the span length) when member_of is NULL.  Each
 * member uploads its own share's runs.  One receive buffer per socket, allocated with
 * nhip_host_alloc_near on a member of that socket, keeps the DMA reads node-local; which buffer a
 * message is received into is the caller's choice.  The stream's params must be NHIP_INPUT_CANONICAL. */
int nhip_group_stream_submit_wire(nhip_group_stream *stream, const nhip_claim *claims, const uint8_t *bytes,
                                  size_t n_bytes, const nhip_span *spans, const uint32_t *member_of, size_t n,
                                  uint8_t *verdicts, uint8_t *all_ok);

/* ---- proof of work (neptune-core/src/protocol/consensus/block/pow.rs) ---
 * PowMastPaths (pow.rs:202-207): MAST authentication paths of the pow field (BlockHeader, 3),
 * the header (BlockKernel, 2) and the kernel (Block, 1); canonical digests. */
typedef struct {
    uint64_t pow[3][5];
    uint64_t header[2][5];
    uint64_t kernel[1][5];
} nhip_pow_mast_paths;
typedef struct nhip_pow_buffer nhip_pow_buffer;
/* PowMastPaths::commit (pow.rs:209-217) */
int nhip_pow_mast_commit(nhip_ctx *ctx, const nhip_pow_mast_paths *mast, uint64_t out[5]);
/* Pow::preprocess (pow.rs:365-469): the guesser buffer of 2^height leaves (buds, 5 bud layers, the
 * HardforkAlpha bit-reversal swap unless reboot_rules, MTree::build_inplace), resident on the
 * device (2 x 2^height x 40 B).  reboot_rules: ConsensusRuleSet::Reboot (bud prefix = mast
 * commit); else HardforkAlpha (bud prefix = prev_block_digest). */
int nhip_pow_preprocess(nhip_ctx *ctx, uint32_t height, const nhip_pow_mast_paths *mast, int reboot_rules,
                        const uint64_t prev_block_digest[5], nhip_pow_buffer **out);
void nhip_pow_buffer_destroy(nhip_pow_buffer *buffer);
/* MTree::root / leafs[index] / MTree::path (pow.rs:147-160) of the buffer's tree */
int nhip_pow_buffer_root(nhip_ctx *ctx, const nhip_pow_buffer *buffer, uint64_t out[5]);
int nhip_pow_buffer_leaf(nhip_ctx *ctx, const nhip_pow_buffer *buffer, uint64_t index, uint64_t out[5]);
int nhip_pow_buffer_path(nhip_ctx *ctx, const nhip_pow_buffer *buffer, uint64_t index, uint64_t *out /* height x 5 */);
/* Pow::guess (pow.rs:471-507) for n nonces: pow digests (fast_mast_hash), the two opened indices,
 * and success = (digest <= target) under twenty-first's Digest ordering (unpinned: canonical
 * values compared from the last element down).  digests_out / indices_out nullable. */
int nhip_pow_guess_batch(nhip_ctx *ctx, const nhip_pow_buffer *buffer, const nhip_pow_mast_paths *mast,
                         const uint64_t index_picker_preimage[5], const uint64_t *nonces, size_t n,
                         const uint64_t target[5], uint64_t *digests_out, uint64_t *indices_out, uint8_t *success_out);
/* Pow::validate (pow.rs:509-557) for n blocks: verdicts[i] = 1 iff both paths verify against the
 * root and the pow digest meets the target.  paths: n x height x 5; reboot_rules: n bytes. */
int nhip_pow_validate_batch(nhip_ctx *ctx, uint32_t height, const uint64_t *roots, const uint64_t *paths_a,
                            const uint64_t *paths_b, const uint64_t *nonces, const nhip_pow_mast_paths *masts,
                            const uint64_t *targets, const uint64_t *parents, const uint8_t *reboot_rules, size_t n,
                            uint8_t *verdicts);

/* ---- block digests and the header chain ----------------------------------
 * What `Block::validate` rules 0.a-0.g (block/mod.rs:726-782) and `Block::has_proof_of_work`
 * (:920-942) read, and `Block::hash` (:189-195,317) for a batch of scanned blocks.
 *
 * nhip_blk_header (host only): one scanned block's header fields (canonical), the byte offsets of the
 * pow's two authentication paths (pow_tree_height digests each), the block MMR accumulator of its body
 * (mmr_n_peaks is the serialized peak count saturated at 65; at most 64 are stored) and, through
 * `words`, the appendix's BFieldCodec encoding (appendix_words) followed by the words of the proof's
 * BFieldCodec encoding that precede Proof.0's items (prefix_words: the BlockProof discriminant alone for
 * Genesis and Invalid).  words == NULL: sizes only; else cap >= appendix_words + prefix_words. */
typedef struct {
    uint64_t version, height, timestamp;
    uint64_t prev_block_digest[5];
    uint64_t pow_root[5], pow_nonce[5];
    uint64_t path_a_offset, path_b_offset;
    uint32_t cumulative_proof_of_work[6];
    uint32_t difficulty[5];
    uint32_t mmr_n_peaks;
    uint64_t receiver_digest[5], lock_script_hash[5];
    uint64_t mmr_num_leafs;
    uint64_t mmr_peaks[64][5];
    uint64_t appendix_words, prefix_words;
    uint64_t proof_offset, proof_len; /* SingleProof: Proof.0's first byte and its words, as this walk found them */
} nhip_blk_header_out;
int nhip_blk_header(const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block *block,
                    nhip_blk_header_out *out, uint64_t *words, size_t cap);
/* Difficulty::target (difficulty_control.rs:69-76): (p^5 - 1) / difficulty as a digest, element 0 the
 * lowest base-p digit (host only).  A zero difficulty (the reference panics) is NHIP_ERR_ARG. */
int nhip_difficulty_target(const uint32_t difficulty[5], uint64_t target_out[5]);
/* difficulty_control (difficulty_control.rs:441-486); timestamps and the interval in milliseconds, reduced
 * mod p as Timestamp::millis does (host only).  A zero interval after a non-genesis parent (the reference
 * panics) is NHIP_ERR_ARG. */
int nhip_difficulty_control(uint64_t new_timestamp, uint64_t old_timestamp, const uint32_t old_difficulty[5],
                            uint64_t target_block_interval, uint64_t previous_block_height,
                            uint32_t difficulty_out[5]);

/* Network parameters of the chain rules (application/config/network.rs:66-130,
 * consensus_rule_set.rs:50-70) and the validator's clock. */
typedef struct {
    uint64_t minimum_block_time_ms, target_block_interval_ms;
    uint64_t difficulty_reset_interval_ms;      /* 0: none */
    uint32_t genesis_difficulty[5];
    uint64_t hardfork_alpha_height;             /* first height under HardforkAlpha; 0: always */
    uint64_t now_ms;
    uint32_t pow_tree_height;
    uint32_t allows_mock_pow;
} nhip_chain_params;
/* block_validation_error.rs:12-31, in rule order; the first rule that fails is the status */
enum {
    NHIP_LINK_OK = 0,
    NHIP_LINK_SKIPPED = 1,             /* parent_of[i] == -1: nothing checked */
    NHIP_LINK_BLOCK_HEIGHT = 2,        /* 0.a */
    NHIP_LINK_PREV_BLOCK_DIGEST = 3,   /* 0.b */
    NHIP_LINK_BLOCK_MMR_UPDATE = 4,    /* 0.c; also a parent accumulator whose peak count is not
                                          popcount(num_leafs) or whose num_leafs is 2^64 - 1 (divergence:
                                          the reference carries the former through `append`) */
    NHIP_LINK_MINIMUM_BLOCK_TIME = 5,  /* 0.d */
    NHIP_LINK_DIFFICULTY = 6,          /* 0.e */
    NHIP_LINK_CUMULATIVE_POW = 7,      /* 0.f */
    NHIP_LINK_FUTURE_DATING = 8        /* 0.g */
};
/* Block::hash of n scanned blocks (blocks[i] from nhip_blk_scan of the same bytes with the same
 * pow_tree_height <= 32; each is parsed again, a malformed one is NHIP_ERR_DECODE): the body MAST hashes
 * as nhip_mast_hash_batch gives them, the proof encodings absorbed from the raw bytes on the device
 * (k_block_proof_leaf), the header / kernel / block MASTs (k_block_masts).  mast_out (nullable): the
 * PowMastPaths of each block (block/mod.rs:946-962), with which fast_mast_hash (pow.rs:219-241)
 * reproduces digests_out.  bytes is DMA'd as it lies when pinned, else staged (as nhip_le_words_gpu). */
int nhip_blk_digests(nhip_ctx *ctx, const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height,
                     const nhip_blk_block *blocks, size_t n, uint64_t *digests_out, nhip_pow_mast_paths *mast_out);
/* Rules 0.a-0.g for every (blocks[parent_of[i]], blocks[i]) pair, then has_proof_of_work of blocks[i]
 * against that parent's header into pow_ok (1 / 0; 0 for a skipped pair), whatever link_status is.
 * The rule set of Pow::validate is Reboot below params->hardfork_alpha_height (the height after the
 * parent's, as mod.rs:939-940) and HardforkAlpha from it on.  A parent index outside -1..n-1 is
 * NHIP_ERR_ARG; a HIP error is NHIP_ERR_HIP / NHIP_ERR_OOM, never a status byte. */
int nhip_blk_chain_check(nhip_ctx *ctx, const uint8_t *bytes, size_t n_bytes, const nhip_chain_params *params,
                         const nhip_blk_block *blocks, size_t n, const int64_t *parent_of, uint8_t *link_status,
                         uint8_t *pow_ok, uint64_t *digests_out);

/* ---- MAST and mutator-set hashing ----------------------------------
 * MastHash::mast_hash (neptune-core/src/protocol/proof_abstractions/mast_hash.rs:22-39) of n
 * objects with `fields` (1..16) field sequences each (TransactionKernel: 8): sequence (i, f) =
 * data[offsets[i*fields+f] .. offsets[i*fields+f+1]); roots_out: n digests. */
int nhip_mast_hash_batch(nhip_ctx *ctx, const uint64_t *data, const uint64_t *offsets, uint32_t fields, size_t n,
                         uint64_t *roots_out);
/* AbsoluteIndexSet::compute (util_types/mutator_set/removal_record/absolute_index_set.rs:86-113)
 * for n removal records: minimum_out n x 2 u64 (u128, little-endian), distances_out n x 45 u32. */
int nhip_absolute_index_sets(nhip_ctx *ctx, const uint64_t *items, const uint64_t *sender_randomness,
                             const uint64_t *receiver_preimages, const uint64_t *aocl_leaf_indices, size_t n,
                             uint64_t *minimum_out, uint32_t *distances_out);

/* ---- mutator-set checks (neptune-core/src/util_types/mutator_set/) ---------
 * The step after "the proof verifies": can the inputs be removed from the mutator set.  Digests are
 * canonical u64 x 5.  Variable-length data is CSR-shaped: an off[n + 1] array (off[0] = 0,
 * non-decreasing) in units of digests (paths) or of u32 indices (chunks).  The device computes
 * every verdict; the host checks shapes only (NHIP_ERR_ARG: a null pointer with a non-zero count,
 * offsets that do not start at 0 or decrease) and a HIP error is NHIP_ERR_HIP, never a verdict.
 *
 * Fail closed where the reference would panic or truncate: `(index / CHUNK_SIZE) as u64`
 * (mutator_set/shared.rs:24) truncates for indices >= 2^76, and ActiveWindow::contains
 * (active_window.rs:153-159) asserts index < WINDOW_SIZE, which an index in chunk
 * batch_index + 256 (accepted by split_by_activity, absolute_index_set.rs:140-160) violates.  Here a
 * record with any index whose untruncated chunk index exceeds batch_index + 255, or whose
 * minimum + distance saturates u128, is rejected with NHIP_MS_OUT_OF_RANGE. */
typedef struct {
    const uint64_t *peaks; /* n_peaks digests, tallest peak first */
    uint32_t n_peaks;
    uint64_t num_leafs;
} nhip_mmr;
/* MutatorSetAccumulator (mutator_set_accumulator.rs:32-36): the AOCL, the inactive part of the
 * sliding-window Bloom filter, and the active window's index list (ActiveWindow::sbf, any order) */
typedef struct {
    nhip_mmr aocl, swbf_inactive;
    const uint32_t *active;
    uint64_t n_active;
} nhip_msa;
/* The chunk dictionaries (removal_record/chunk_dictionary.rs:27-33) of n records, flattened: record
 * i owns the entries entry_off[i] .. entry_off[i + 1], in dictionary order. */
typedef struct {
    const uint64_t *entry_off;   /* n + 1 */
    const uint64_t *chunk_index; /* per entry */
    const uint64_t *path_off;    /* entries + 1, in digests */
    const uint64_t *path;        /* MMR authentication paths, leaf sibling first */
    const uint64_t *rel_off;     /* entries + 1, in u32 */
    const uint32_t *rel;         /* Chunk::relative_indices */
} nhip_ms_chunks;
/* status byte of a record; of several failures the first in this order is reported:
 * NOT_IN_AOCL, OUT_OF_RANGE, ABSENT_CHUNK, BAD_MMR_PATH, ALREADY_REMOVED */
enum {
    NHIP_MS_OK = 0,
    NHIP_MS_ABSENT_CHUNK = 1,    /* RemovalRecordValidityError::AbsentAuthenticatedChunk */
    NHIP_MS_BAD_MMR_PATH = 2,    /* RemovalRecordValidityError::InvalidSwbfiMmrMp */
    NHIP_MS_ALREADY_REMOVED = 3, /* every index is set: no absent index */
    NHIP_MS_OUT_OF_RANGE = 4,    /* a future index (AbsoluteRemovalIndexIsFutureIndex), or see above */
    NHIP_MS_NOT_IN_AOCL = 5,     /* verify only: leaf index or AOCL membership */
    /* nhip_ms_apply_batch only (a job's status) */
    NHIP_MS_INCONSISTENT = 6,      /* msa_before: popcount(num_leafs) != n_peaks, swbf_inactive.num_leafs != batch
                                      index, or num_leafs + additions wraps */
    NHIP_MS_DUPLICATE_RECORD = 7,  /* Block::validate 2.c: two records with equal index arrays */
    NHIP_MS_UPDATE_IMPOSSIBLE = 8, /* 2.d: a record whose indices are all set once the earlier ones are applied */
    NHIP_MS_UPDATE_MISMATCH = 9,   /* 2.e: the accumulator after is not the expected one */
    /* packed removal records (rule 2.a, below): RemovalRecordList::try_unpack's errors, in the reference's order */
    NHIP_MS_UNPACK_PAYLOAD_TOO_BIG = 10,          /* ChunkUnpackError::PayloadTooBig */
    NHIP_MS_UNPACK_INCONSISTENT_LENGTH = 11,      /* ChunkUnpackError::InconsistentLength */
    NHIP_MS_UNPACK_NONZERO_TRAILING_PADDING = 12, /* ChunkUnpackError::NonzeroTrailingPadding */
    NHIP_MS_UNPACK_ILLEGAL_TREE_HEIGHT = 13,      /* RemovalRecordListUnpackError::IllegalTreeHeight */
    NHIP_MS_UNPACK_DUPLICATE_TREE_HEIGHTS = 14,   /* ...::DuplicateTreeHeights */
    NHIP_MS_UNPACK_INDEX_TOO_BIG = 15,            /* ...::AbsoluteIndexTooBig */
    NHIP_MS_UNPACK_INCONSISTENT_CHUNKS = 16,      /* RemovalRecordListInconsistency::Chunks */
    NHIP_MS_UNPACK_STRUCTURE_COUNT = 17,          /* ...::AuthenticationStructureCount */
    NHIP_MS_UNPACK_STRUCTURE_LENGTH = 18,         /* ...::AuthenticationStructureLength */
    NHIP_MS_UNPACK_PANIC = 19,                    /* the reference panics on this list: fail closed */
    /* nhip_ms_update_batch only (a witness's status) */
    NHIP_MS_JOB_REJECTED = 20,   /* the witness's job did not end NHIP_MS_OK: nothing of it is brought up to date */
    NHIP_MS_UPDATE_INTERNAL = 21 /* a digest the witness needs was found nowhere it can come from: never a guess */
};
/* twenty-first MmrMembershipProof::verify(leaf_index, leaf, peaks, num_leafs) for n (leaf, path)
 * items against one MMR, as called bare in application/loops/peer_loop.rs:1235 and
 * protocol/peer.rs:824.  Path shape: util_types/archival_mmr.rs:250-281.  path_off: n + 1. */
int nhip_mmr_verify_batch(nhip_ctx *ctx, const nhip_mmr *mmr, const uint64_t *leaf_index, const uint64_t *leaves,
                          const uint64_t *path_off, const uint64_t *path, size_t n, uint8_t *verdicts);
/* RemovalRecord::validate (removal_record.rs:202-251) and MutatorSetAccumulator::can_remove
 * (mutator_set_accumulator.rs:187-222) for n removal records, as in Block::validate
 * (protocol/consensus/block/mod.rs:816-822) and the mempool's per-tip check
 * (protocol/consensus/transaction/transaction_kernel.rs:129,145).  minimum: n x 2 u64 (u128,
 * little-endian) and distances: n x 45 u32, the AbsoluteIndexSet layout the index-set entry point
 * above writes.  valid / can_remove / status: n bytes each. */
int nhip_ms_can_remove_batch(nhip_ctx *ctx, const nhip_msa *msa, const uint64_t *minimum, const uint32_t *distances,
                             const nhip_ms_chunks *chunks, size_t n, uint8_t *valid, uint8_t *can_remove,
                             uint8_t *status);
/* MutatorSetAccumulator::verify (mutator_set_accumulator.rs:252-339) for n (item, membership
 * proof) pairs, as the wallet runs it for every monitored UTXO on every block
 * (state/wallet/wallet_state.rs:1796,1958; state/mod.rs:1050,1206,1341).  The index sets are
 * derived on the device (AbsoluteIndexSet::compute).  aocl_path_off: n + 1, in digests. */
int nhip_ms_verify_batch(nhip_ctx *ctx, const nhip_msa *msa, const uint64_t *items, const uint64_t *sender_randomness,
                         const uint64_t *receiver_preimages, const uint64_t *aocl_leaf_index,
                         const uint64_t *aocl_path_off, const uint64_t *aocl_path, const nhip_ms_chunks *chunks,
                         size_t n, uint8_t *verdicts, uint8_t *status);

/* ---- batched mutator-set updates --------------------------------------------
 * Block::validate rules 2.b-2.e (protocol/consensus/block/mod.rs:816-849) and
 * Block::mutator_set_accumulator_after (mod.rs:369-378) for n_jobs independent jobs: job j is
 * (msa_before[j], the addition records add_off[j] .. add_off[j + 1], the removal records
 * rec_off[j] .. rec_off[j + 1] in block order, optionally msa_expected[j]).  The end state is computed
 * directly (MutatorSetUpdate::apply_to_accumulator, block/mutator_set_update.rs:107-153, without its
 * record-by-record proof maintenance).  Per job, in this order, the first failure is the status:
 *   1. NHIP_MS_INCONSISTENT (see the enum);
 *   2. 2.b: every record as nhip_ms_can_remove_batch decides it against msa_before[j]: the first failing
 *      record's status, bad_record = its index in the job;
 *   3. 2.c: NHIP_MS_DUPLICATE_RECORD, bad_record = the first record equal to an earlier one;
 *   4. 2.d: NHIP_MS_UPDATE_IMPOSSIBLE, bad_record = the first record all of whose indices are set in
 *      msa_before[j] or occur in an earlier record of the job;
 *   5. the accumulator after; with msa_expected, 2.e: NHIP_MS_UPDATE_MISMATCH unless both num_leafs, both
 *      peak lists, the window's length and its words in the given order are equal.
 * Divergences from the reference, both failing closed: (a) an inconsistent msa_before is a status, where
 * the reference asserts (removal_record.rs:66-70); (b) the window after is sorted ascending
 * (ActiveWindow::insert, active_window.rs:115-124), so an unsorted expected window never matches, although
 * the reference would carry an unsorted window through a block that inserts nothing (no operation of the
 * reference produces one).  Inactive chunks are taken as sorted, as Chunk::insert (chunk.rs:55-64) leaves them.
 * The accumulators after are written for jobs whose status is NHIP_MS_OK or NHIP_MS_UPDATE_MISMATCH; for the
 * others the counts are 0.  With no expected accumulator and no removal records the call is
 * Block::mutator_set_accumulator_after.  Shape errors (NHIP_ERR_ARG, outputs untouched): a null pointer with
 * a non-zero count, offsets that do not start at 0 or decrease, a window capacity below
 * n_active + 45 records of its job. */
typedef struct {
    size_t n_jobs;
    const nhip_msa *msa_before;   /* n_jobs */
    const uint64_t *add_off;      /* n_jobs + 1, in addition records */
    const uint64_t *additions;    /* AdditionRecord::canonical_commitment, 5 words each */
    const uint64_t *rec_off;      /* n_jobs + 1, in removal records */
    const uint64_t *minimum;      /* records x 2 u64 (u128, little-endian) */
    const uint32_t *distances;    /* records x 45 */
    const nhip_ms_chunks *chunks; /* the dictionaries of all records */
    const nhip_msa *msa_expected; /* n_jobs, or NULL */
} nhip_ms_apply_in;
typedef struct {
    uint8_t *verdict;             /* n_jobs: 1 = every step passed */
    uint8_t *status;              /* n_jobs: NHIP_MS_* */
    uint64_t *bad_record;         /* n_jobs: index in the job, UINT64_MAX = none */
    /* the accumulators after: all NULL, or all present */
    uint64_t *aocl_peaks;         /* n_jobs x 64 digests */
    uint32_t *aocl_n_peaks;       /* n_jobs */
    uint64_t *aocl_num_leafs;     /* n_jobs */
    uint64_t *swbf_peaks;         /* n_jobs x 64 digests */
    uint32_t *swbf_n_peaks;       /* n_jobs */
    uint64_t *swbf_num_leafs;     /* n_jobs */
    const uint64_t *active_off;   /* n_jobs + 1: job j's window goes to active[active_off[j] ..], capacity
                                     active_off[j + 1] - active_off[j] >= n_active + 45 records */
    uint32_t *active;
    uint64_t *n_active;           /* n_jobs */
} nhip_ms_apply_out;
int nhip_ms_apply_batch(nhip_ctx *ctx, const nhip_ms_apply_in *in, nhip_ms_apply_out *out);

/* ---- packed removal records: Block::validate rule 2.a --------------------------
 * RemovalRecordList::try_unpack (util_types/mutator_set/removal_record/removal_record_list.rs:653-658,
 * block/mod.rs:811-813) for n_jobs independent packed lists.  A packed list is a Vec<RemovalRecord>, so the input
 * has the shapes above: job j is the records rec_off[j] .. rec_off[j + 1] (minimum, distances), and in `packed`
 * chunk_index holds an entry's key (a tree height, a tree height + 64, or UINT64_MAX), path its authentication
 * structure and rel its chunk's packed words (chunk.rs:148-194).  The output is the unpacked dictionaries of all
 * records, a valid nhip_ms_chunks for the calls above; the records of a job that fails own no entry.  Per job the
 * status is the first failure in the reference's own order, NHIP_MS_OK otherwise; every status is an integer
 * decision of the host plan, and the path digests are computed on the device.  Divergence, failing closed:
 * where the reference panics (heights not ascending in dictionary order, an estimate 8 s + 1 past u64, a
 * structure that does not fit its own tree, a sibling missing while a path is read) the status is
 * NHIP_MS_UNPACK_PANIC.
 * Two-call sizing, as nhip_blk_scan: with every array pointer but status and num_leafs_aocl NULL only the totals
 * (and those two when present) are written; otherwise all arrays are present with their capacities, and
 * NHIP_ERR_ARG if one is too small. */
typedef struct {
    uint8_t *status;          /* n_jobs: NHIP_MS_* */
    uint64_t *num_leafs_aocl; /* n_jobs, or NULL: the estimated AOCL leaf count, 0 for a failed job */
    uint64_t *entry_off;      /* records + 1 */
    uint64_t *chunk_index;    /* entries_cap */
    uint64_t *path_off;       /* entries_cap + 1, in digests */
    uint64_t *path;           /* path_cap digests; nhip_ms_unpack_plan leaves it alone (it may be NULL there) */
    uint64_t *rel_off;        /* entries_cap + 1, in u32 */
    uint32_t *rel;            /* rel_cap: the unpacked relative indices */
    size_t entries_cap, path_cap, rel_cap;
    size_t entries, path_digests, rel_words; /* out: the totals */
} nhip_ms_unpacked;
/* The codec side (no context, host only, hashes nothing): statuses and the unpacked shape without `path`. */
int nhip_ms_unpack_plan(const uint64_t *rec_off, size_t n_jobs, const uint64_t *minimum, const uint32_t *distances,
                        const nhip_ms_chunks *packed, nhip_ms_unpacked *out);
/* try_unpack: the plan's output plus `path`, computed on the device (one Tip5::hash per distinct chunk, one
 * hash_pair per completed family). */
int nhip_ms_unpack_batch(nhip_ctx *ctx, const uint64_t *rec_off, size_t n_jobs, const uint64_t *minimum,
                         const uint32_t *distances, const nhip_ms_chunks *packed, nhip_ms_unpacked *out);
/* Rules 2.a-2.e in one call: nhip_ms_apply_batch with in->chunks read as packed.  A job that fails 2.a gets
 * verdict 0, its unpack status, bad_record = UINT64_MAX and zero accumulator counts; the others run exactly as in
 * nhip_ms_apply_batch.  The unpacked paths are produced on the device and never cross to the host. */
int nhip_ms_apply_batch_packed(nhip_ctx *ctx, const nhip_ms_apply_in *in, nhip_ms_apply_out *out);

/* ---- membership proofs and removal records across a block ----------------------
 * MsMembershipProof::batch_update_from_addition / batch_update_from_remove (ms_membership_proof.rs:76-270,
 * 417-468) and RemovalRecord::batch_update_from_addition / batch_update_from_remove (removal_record.rs:49-200)
 * over a whole block, computed as the end state: a job is a job of nhip_ms_apply_batch plus the witnesses
 * wit_off[j] .. wit_off[j + 1] to bring up to the accumulator after it.  A witness is an index set, a chunk
 * dictionary and, for a membership proof, an AOCL part (leaf index, leaf = the addition record's canonical
 * commitment, authentication path); a removal record has aocl_leaf_index == UINT64_MAX.  With n0 / n1 the
 * AOCL leaf counts before / after and b0 / b1 the batch indices before / after:
 *   job:       steps 1-5 of nhip_ms_apply_batch; unless the job ends NHIP_MS_OK every witness of it gets
 *              NHIP_MS_JOB_REJECTED.
 *   admission: per witness, the first failure of
 *              NHIP_MS_NOT_IN_AOCL   (AOCL part only) l >= n1; l < n0 and the path does not authenticate the leaf
 *                                    against msa_before.aocl; n0 <= l < n1 and the leaf is not additions[l - n0]
 *                                    or the path is not empty;
 *              NHIP_MS_OUT_OF_RANGE  minimum + distance saturates u128, or a chunk index exceeds b1 + 255;
 *              NHIP_MS_ABSENT_CHUNK  the dictionary's keys are not, strictly ascending, exactly the witness's
 *                                    chunk indices below b0;
 *              NHIP_MS_BAD_MMR_PATH  an entry does not authenticate against msa_before.swbf_inactive.
 *              Whether the item is already removed plays no part.
 *   after:     the AOCL path has ilog2(l ^ n1) digests; the dictionary's keys are the witness's chunk indices
 *              below b1, ascending, each with the chunk after the block (the old entry's chunk, or the slid part
 *              of the old window, merged with the block's indices in that chunk, repeats kept) and its path of
 *              ilog2(key ^ b1) digests in swbf_inactive after the block.
 * Every output length is an integer function of the inputs, laid out by nhip_ms_update_plan as if every job and
 * witness were accepted; the slots of a witness whose status is not NHIP_MS_OK keep their planned offsets and
 * are zero-filled (chunk_index included).  Two-call sizing as nhip_ms_unpack_plan: with every array pointer but
 * status NULL only the totals are written (and nothing runs on the device). */
typedef struct {
    const uint64_t *wit_off;         /* n_jobs + 1, in witnesses */
    const uint64_t *minimum;         /* witnesses x 2 u64 (u128, little-endian) */
    const uint32_t *distances;       /* witnesses x 45 */
    const uint64_t *aocl_leaf_index; /* witnesses; UINT64_MAX: no AOCL part */
    const uint64_t *aocl_leaf;       /* witnesses x 5 (ignored without an AOCL part) */
    const uint64_t *aocl_path_off;   /* witnesses + 1, in digests */
    const uint64_t *aocl_path;
    const nhip_ms_chunks *chunks;    /* the dictionaries of all witnesses */
} nhip_ms_update_in;
typedef struct {
    uint8_t *status;         /* witnesses: NHIP_MS_*; nhip_ms_update_plan leaves it alone */
    uint64_t *aocl_path_off; /* witnesses + 1, in digests */
    uint64_t *aocl_path;     /* aocl_cap digests; the plan leaves it alone */
    uint64_t *entry_off;     /* witnesses + 1 */
    uint64_t *chunk_index;   /* entries_cap */
    uint64_t *path_off;      /* entries_cap + 1, in digests */
    uint64_t *path;          /* path_cap digests; the plan leaves it alone */
    uint64_t *rel_off;       /* entries_cap + 1, in u32 */
    uint32_t *rel;           /* rel_cap; the plan leaves it alone */
    size_t aocl_cap, entries_cap, path_cap, rel_cap;
    size_t aocl_digests, entries, path_digests, rel_words; /* out: the totals */
} nhip_ms_updated;
/* The shape alone (no context, host only, hashes nothing): the four offset arrays and the keys. */
int nhip_ms_update_plan(const nhip_ms_apply_in *block, const nhip_ms_update_in *wit, nhip_ms_updated *out);
/* block_out is filled as nhip_ms_apply_batch fills it.  Shape errors are NHIP_ERR_ARG with the outputs untouched. */
int nhip_ms_update_batch(nhip_ctx *ctx, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out,
                         const nhip_ms_update_in *wit, nhip_ms_updated *out);

/* ---- membership proofs and removal records back across a block -----------------
 * MsMembershipProof::revert_update_from_remove / revert_update_from_batch_addition
 * (ms_membership_proof.rs:380-413, 517-557; shared.rs:154-224) over a whole block, as a reorganisation walks the
 * abandoned blocks backwards (state/mod.rs:1392-1497), computed as the end state.  A job is a job of
 * nhip_ms_apply_batch: msa_before, the block's addition records and its removal records as the block carries them
 * (valid against msa_before), optionally msa_expected, the accumulator the witnesses stand at.  The witnesses (the
 * structs of nhip_ms_update_batch) stand at the accumulator *after* the job and are taken to msa_before.  With
 * n0 / n1 the AOCL leaf counts before / after and b0 / b1 the batch indices before / after:
 *   job:       steps 1-5 of nhip_ms_apply_batch; unless the job ends NHIP_MS_OK every witness of it gets
 *              NHIP_MS_JOB_REJECTED.  With msa_expected rule 2.e checks that this block led to that accumulator.
 *   admission: per witness as it stands after the block, integer and word comparisons only, the first failure of
 *              NHIP_MS_NOT_IN_AOCL   (AOCL part only) l >= n0 (born in this block or later: the reference asserts,
 *                                    ms_membership_proof.rs:386-389), or the path has not ilog2(l ^ n1) digests;
 *              NHIP_MS_OUT_OF_RANGE  minimum + distance saturates u128, or a chunk index exceeds b1 + 255;
 *              NHIP_MS_ABSENT_CHUNK  the dictionary's keys are not, strictly ascending, exactly the witness's
 *                                    chunk indices below b1;
 *              NHIP_MS_BAD_MMR_PATH  an entry's path has not ilog2(key ^ b1) digests, or (decided on the device) a
 *                                    kept entry's chunk holds fewer copies of a block index than the block inserted.
 *   before:    the AOCL path keeps its first ilog2(l ^ n0) digests; the dictionary keeps the entries with key < b0,
 *              in order (the chunks b0 .. b1 - 1 were still in the window); a kept chunk loses one copy of each of
 *              the block's indices in it per occurrence (Chunk::remove_once); a kept path keeps its first
 *              ilog2(key ^ b0) digests, and digest t becomes the old value of node (t, (key >> t) ^ 1) where that
 *              node is a chunk a block record touches or an ancestor of one, else stays.  The old values come from
 *              the block's records alone: a record's entry holds the chunk and its path before the block.
 *   verified:  every reverted witness is authenticated against msa_before where it was written, the only
 *              cryptographic check and a complete one (the reference's assert after each reverted block): its leaf
 *              under msa_before.aocl, else NHIP_MS_NOT_IN_AOCL; every entry under msa_before.swbf_inactive, else
 *              NHIP_MS_BAD_MMR_PATH.  Whatever a revert returns NHIP_MS_OK is valid against msa_before, stale or
 *              forged input included.
 * NHIP_MS_UPDATE_INTERNAL keeps its meaning.  Output lengths are integers of the inputs (a kept chunk: its length
 * less the block's indices in that chunk, floored at 0), laid out by nhip_ms_revert_plan as if every job and witness
 * were accepted; a failed witness keeps its planned slots zero-filled, keys included.  Two-call sizing as
 * nhip_ms_update_plan.
 * One divergence fails open only by construction of the input: a removal record has no leaf index, so one whose
 * item was born in the reverted block cannot be recognised as such.  It is reverted by shape and passes or fails the
 * verification like any other; the caller drops the mempool transactions of the abandoned fork. */
int nhip_ms_revert_plan(const nhip_ms_apply_in *block, const nhip_ms_update_in *wit, nhip_ms_updated *out);
/* block_out is filled as nhip_ms_apply_batch fills it.  Shape errors are NHIP_ERR_ARG with the outputs untouched. */
int nhip_ms_revert_batch(nhip_ctx *ctx, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out,
                         const nhip_ms_update_in *wit, nhip_ms_updated *out);

/* ---- witnesses resident on the device across blocks -----------------------------
 * A store owns the witnesses of nhip_ms_update_batch (same description: nhip_ms_update_in) in device memory of
 * its own and brings all of them across one block per nhip_ms_store_update: §6g for one job, its witness side
 * bound to the store.  Only the block, the plan's integer arrays, block_out and one status byte per witness cross
 * to or from the host; no path digest and no chunk word of a witness does after nhip_ms_store_append, or at all,
 * through nhip_ms_store_append_restored.  The host
 * keeps a mirror of the integers alone (index sets, leaf indices, the four offset arrays, the keys).
 * Witnesses are numbered 0 .. W-1 in insertion order; the positions are stable until nhip_ms_store_retain.
 * A store belongs to one nhip_ctx (which must outlive it) and to one tip; calls on it are serialized by the
 * context.  Status rules beyond nhip_ms_update_batch's, all failing closed:
 *   - unless the block ends NHIP_MS_OK the store is unchanged and every returned status is NHIP_MS_JOB_REJECTED;
 *   - NHIP_ERR_HIP / NHIP_ERR_OOM / NHIP_ERR_ARG leave the store unchanged;
 *   - a witness whose status after an update is not NHIP_MS_OK keeps its position and its planned slots, zero-filled
 *     (keys included); the status is sticky: every later update, read and check reports that first status, the slots
 *     stay zero and are planned by shape like any other's, until nhip_ms_store_retain drops the witness.
 * The gather kernel behind read and retain works in units of NHIP_MS_STORE_GATHER_UNIT 8-byte destination words
 * (twice as many u32 chunk words). */
#define NHIP_MS_STORE_GATHER_UNIT 1024
typedef struct nhip_ms_store nhip_ms_store;
/* initial capacities (0: a default); every capacity grows geometrically on demand, device to device */
typedef struct {
    size_t witnesses, aocl_digests, entries, path_digests, rel_words;
} nhip_ms_store_caps;
int nhip_ms_store_create(nhip_ctx *ctx, const nhip_ms_store_caps *initial, nhip_ms_store **out);
void nhip_ms_store_destroy(nhip_ms_store *store);
/* the totals, from the host mirror; any pointer may be NULL */
int nhip_ms_store_count(const nhip_ms_store *store, uint64_t *witnesses, uint64_t *aocl_digests, uint64_t *entries,
                        uint64_t *path_digests, uint64_t *rel_words);
/* n witnesses behind the existing ones (wit->wit_off is ignored); the shape checks of nhip_ms_update_batch */
int nhip_ms_store_append(nhip_ms_store *store, const nhip_ms_update_in *wit, size_t n);
/* block->n_jobs == 1; block_out as nhip_ms_apply_batch fills it; status: W bytes, or NULL */
int nhip_ms_store_update(nhip_ms_store *store, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out,
                         uint8_t *status);
/* The way back when the tip moves to another fork: nhip_ms_revert_batch for one job, its witness side bound to the
 * store, which stands at the accumulator after `block` and is taken to block->msa_before.  A caller who passes the
 * store's tip as msa_expected gets rule 2.e as the check that this block led to that tip.  The contract of
 * nhip_ms_store_update: unless the block ends NHIP_MS_OK the store is unchanged byte for byte and every status is
 * NHIP_MS_JOB_REJECTED; HIP, OOM and ARG errors leave it unchanged; sticky statuses carry over and new failures (a
 * witness born in the reverted block among them) become sticky; only the block, the plan's integer arrays, block_out
 * and W status bytes cross to or from the host. */
int nhip_ms_store_revert(nhip_ms_store *store, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out,
                         uint8_t *status);
/* The witnesses sel[0 .. n_sel) (any order, repeats allowed; sel == NULL with n_sel == W: all) in the layout of
 * nhip_ms_updated, with its two-call sizing; the count pass reads the mirror alone.  An index >= W is
 * NHIP_ERR_ARG with the outputs untouched.  One gather on the device, then one copy per array. */
int nhip_ms_store_read(nhip_ms_store *store, const uint64_t *sel, size_t n_sel, nhip_ms_updated *out);
/* keep: W bytes; the witnesses with keep[i] != 0 stay, in order */
int nhip_ms_store_retain(nhip_ms_store *store, const uint8_t *keep);
/* Per witness against msa, W bytes each: aocl_member = MmrMembershipProof::verify of its leaf under msa->aocl (1
 * for a removal record); valid / can_remove / status as nhip_ms_can_remove_batch decides its index set and
 * dictionary.  A sticky witness reports its sticky status and zeros.  Nothing of the store moves. */
int nhip_ms_store_check(nhip_ms_store *store, const nhip_msa *msa, uint8_t *aocl_member, uint8_t *valid,
                        uint8_t *can_remove, uint8_t *status);

/* ---- the archival mutator set resident on the device ----------------------------
 * ArchivalMutatorSet (util_types/mutator_set/archival_mutator_set.rs over util_types/archival_mmr.rs): every node of
 * the AOCL MMR and of the inactive-SWBF MMR, every chunk and the active window, in device memory of the archive's
 * own: the structure fresh witnesses come from.  An MMR of n leaves is kept as level arrays: level h holds the n >> h
 * nodes (h, k), each the root of the leaves [k 2^h, (k + 1) 2^h); the authentication path of leaf i is the nodes
 * (t, (i >> t) ^ 1) for t < ilog2(i ^ n), leaf sibling first, the shape nhip_mmr_verify_batch reads.  The chunks'
 * words (sorted ascending, repeats kept: Chunk::insert, chunk.rs:55-64) lie in a u32 arena behind an
 * (offset, length) table.  The host keeps a mirror of the integers alone (both leaf counts, the chunk table, the
 * window, the capacities) and no digest.  An archive belongs to one nhip_ctx (which must outlive it) and to one tip;
 * calls on it are serialized by the context.
 *   - NHIP_ERR_ARG, NHIP_ERR_OOM and NHIP_ERR_HIP before the first launch that writes archive state leave the archive
 *     unchanged; a HIP error behind such a launch poisons it: every later call returns NHIP_ERR_HIP, so that nothing
 *     is ever read from a half-written archive.
 *   - Digests are computed on the device only: load accepts leaves, chunk words and the window, nothing precomputed.
 * Load builds level h with a launch of its own while level h - 1 has more than NHIP_MS_ARCHIVE_TAIL_NODES nodes, and
 * all levels above with one workgroup per MMR. */
#define NHIP_MS_ARCHIVE_TAIL_NODES 256
typedef struct nhip_ms_archive nhip_ms_archive;
/* initial capacities (0: none): AOCL leaves, chunks, chunk words; every capacity grows geometrically on demand, device
 * to device */
typedef struct {
    size_t aocl_leafs, chunks, rel_words;
} nhip_ms_archive_caps;
int nhip_ms_archive_create(nhip_ctx *ctx, const nhip_ms_archive_caps *initial, nhip_ms_archive **out);
void nhip_ms_archive_destroy(nhip_ms_archive *archive);
/* the totals, from the host mirror; any pointer may be NULL.  rel_live: the chunk words the chunks own; rel_dead:
 * arena words no chunk owns any more. */
int nhip_ms_archive_count(const nhip_ms_archive *archive, uint64_t *aocl_leafs, uint64_t *chunks, uint64_t *n_active,
                          uint64_t *rel_live, uint64_t *rel_dead);
/* Bulk load into an empty archive: n_leafs AOCL leaves (addition records' canonical commitments, 5 words each), the
 * n_chunks chunks' words rel[rel_off[c] .. rel_off[c + 1]) and the window.  Uploads them once, hashes every chunk
 * (Tip5::hash(chunk)) and builds every level of both MMRs on the device.  NHIP_ERR_ARG before anything is touched: an
 * archive that is not empty, an unsorted chunk or window, offsets that do not start at 0 or that decrease, a relative
 * index >= 4096 in a chunk or >= 2^20 in the window, n_chunks != batch_index(n_leafs) (util_types/mutator_set.rs:74-76). */
int nhip_ms_archive_load(nhip_ms_archive *archive, const uint64_t *aocl_leaves, uint64_t n_leafs,
                         const uint64_t *rel_off, const uint32_t *rel, uint64_t n_chunks, const uint32_t *active,
                         uint64_t n_active);
/* The archive's MutatorSetAccumulator as one job's worth of nhip_ms_apply_out: both peak lists (read from the level
 * arrays on the device), the counts and the window (capacity active_off[1] - active_off[0] >= n_active, else
 * NHIP_ERR_ARG); verdict 1, status NHIP_MS_OK and bad_record UINT64_MAX where those pointers are present. */
int nhip_ms_archive_accumulator(nhip_ms_archive *archive, nhip_ms_apply_out *out);
/* ArchivalState::update_mutator_set's forward step (state/archival_state.rs:1242-1409) as an end state; block->n_jobs
 * == 1 and the accumulator outputs of block_out present (else NHIP_ERR_ARG).  The block runs through steps 1-5 of
 * nhip_ms_apply_batch with block->msa_before[0] checked against the archive's own accumulator first: both counts, the
 * window's length and words (against the mirror) and both peak lists (against the level arrays); any difference is
 * NHIP_MS_INCONSISTENT (verdict 0, bad_record UINT64_MAX, zero counts).  Unless the job ends NHIP_MS_OK the archive is
 * unchanged in every count and byte a later call can observe, and block_out is as nhip_ms_apply_batch fills it.  On
 * NHIP_MS_OK the AOCL gains the additions' commitments; every chunk c with b0 <= c < b1 is created from the part
 * [4096 (c - b0), 4096 (c - b0 + 1)) of the old window made relative (empty from c - b0 = 256 on); every chunk below b1
 * that the records' indices hit is merged with those indices, repeats kept; the SWBF MMR gets the new and the changed
 * leaves with all their ancestors; the window becomes the accumulator-after's.  A chunk that changes is written anew
 * at the arena's tail and its old words are dead; when dead words exceed live words after an apply the arena is
 * compacted into a second buffer with one gather and the two are swapped.  Every array grows geometrically, device to
 * device; all allocation and growth precede the first launch that writes archive state, and the mirror and the counts
 * advance only after the stream drains clean.  Afterwards nhip_ms_archive_accumulator equals what block_out reported. */
int nhip_ms_archive_apply(nhip_ms_archive *archive, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out);
/* The way back when the tip moves to another fork: ArchivalState::update_mutator_set's walk over an abandoned block
 * (state/archival_state.rs:1293-1335: revert_remove per removal record, then add_is_reversible / revert_add per
 * addition in reverse, archival_mutator_set.rs:417-490) as an end state.  The archive stands at the accumulator after
 * `block` and is taken to block->msa_before[0].  With n1 / b1 the archive's AOCL leaf and chunk counts, k additions,
 * n0 = n1 - k and b0 = batch_index(n0): the AOCL keeps its first n0 leaves and no node is hashed; the chunks [b0, b1)
 * are dropped; every chunk below b0 that a block index hits loses one copy of that index per occurrence the block
 * inserted (Chunk::subtract) and is written anew at the arena's tail, its old words dead; the rewritten chunks are
 * hashed and every SWBF node above one that exists at b0 is hashed again; the window becomes msa_before's.  Dead words
 * count and the arena compacts as after an apply; no capacity shrinks.
 *   1. block->n_jobs == 1 and the accumulator outputs of block_out present, else NHIP_ERR_ARG.
 *   2. The tip check, before anything is written: steps 1-5 of nhip_ms_apply_batch run on (msa_before, block), decide
 *      rules 2.b-2.e (a msa_expected is honoured) and fill block_out.  If the job ends NHIP_MS_OK, the accumulator it
 *      computed has to be the archive's own: both counts and the window word for word (against the mirror), both peak
 *      lists (against the level arrays).  Any difference, or counts no block can have led to, is
 *      NHIP_MS_UPDATE_MISMATCH ("this block did not lead to this tip"), reported as a 2.e failure is: verdict 0,
 *      bad_record UINT64_MAX.  Unless the job ends NHIP_MS_OK and the tip matches, the archive is unchanged in every
 *      count and byte a later call can observe.
 *   3. All allocation (arena growth for the tail writes, a longer window, the compaction's buffers) precedes the first
 *      launch that writes archive state; an error there leaves the archive as it was.
 *   4. The mirror and the counts move only after the stream drains clean; a HIP error behind a write poisons the archive.
 *   5. Never a guess: the subtraction flags a chunk that holds fewer copies of a block index than the block inserted,
 *      and after the writes the peaks are read back and compared with msa_before's at n0 and b0 (the reference's
 *      closing sanity assert), both on the drain that is due anyway.  A set flag or a difference poisons the archive
 *      and returns NHIP_ERR_HIP; nothing is reported as reverted.
 *   6. A block of 0 additions and 0 records is NHIP_MS_OK and changes nothing if the tip matches; a revert down to
 *      n0 == 0 leaves an empty archive that nhip_ms_archive_load accepts again.
 * On NHIP_MS_OK block_out holds the accumulator after the block, as nhip_ms_apply_batch fills it, and
 * nhip_ms_archive_accumulator equals msa_before. */
int nhip_ms_archive_revert(nhip_ms_archive *archive, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out);
/* ArchivalMmr::prove_membership_async (archival_mmr.rs:297-321) for n leaves of one MMR (which: 0 AOCL, 1 SWBF):
 * path_off n + 1, in digests.  Two-call sizing: with path_off and path NULL only *path_digests is written (from the
 * mirror alone); otherwise path_cap >= the total, else NHIP_ERR_ARG.  An index >= the leaf count is NHIP_ERR_ARG with
 * the outputs untouched.  One gather on the device, then one copy. */
int nhip_ms_archive_paths(nhip_ms_archive *archive, int which, const uint64_t *leaf_index, size_t n,
                          uint64_t *path_off, uint64_t *path, size_t path_cap, size_t *path_digests);
/* ArchivalMmr::get_leaf_range_inclusive_async (archival_mmr.rs:211-229): the leaves first .. first + n - 1 of one MMR;
 * a range that leaves the MMR is NHIP_ERR_ARG with `out` untouched. */
int nhip_ms_archive_leaves(nhip_ms_archive *archive, int which, uint64_t first, uint64_t n, uint64_t *out);
/* Fresh witnesses for n index sets (the layout nhip_absolute_index_sets writes), in the layout of nhip_ms_updated,
 * which nhip_ms_store_append reads.  With an AOCL leaf index it is ArchivalMutatorSet::restore_membership_proof
 * (archival_mutator_set.rs:298-346); with aocl_leaf_index == UINT64_MAX the dictionary alone, as
 * restore_membership_proof_privacy_preserving (:350-406) and the refresh of old removal records
 * (state/archival_state.rs:1156-1179) need it.  Per witness the status is the first failure of
 *   NHIP_MS_NOT_IN_AOCL   the leaf index is >= the leaf count, or the archive is empty (the reference's
 *                         RequestedAoclAuthPathOutOfBounds / MutatorSetIsEmpty);
 *   NHIP_MS_OUT_OF_RANGE  minimum + distance saturates u128, or a chunk index exceeds batch_index + 255;
 * such a witness owns no digest and no entry.  Otherwise: the AOCL path of ilog2(l ^ n) digests; a dictionary whose
 * keys are the witness's distinct chunk indices below the batch index b, strictly ascending (chunk_dictionary.rs:29-45),
 * each with the chunk's words and its path of ilog2(key ^ b) digests.  Every length and every status is an integer
 * decision of the plan; two-call sizing as nhip_ms_store_read (the count pass reads the mirror alone). */
int nhip_ms_archive_restore(nhip_ms_archive *archive, const uint64_t *minimum, const uint32_t *distances,
                            const uint64_t *aocl_leaf_index, size_t n, nhip_ms_updated *out);
/* The shape and every status of nhip_ms_archive_restore from integers alone (no context, host only): an archive of
 * aocl_leafs leaves whose chunk c holds chunk_len[c] words, n_chunks == batch_index(aocl_leafs) (else NHIP_ERR_ARG).
 * Writes the offset arrays, the keys, the totals and, when present, status; aocl_path, path and rel are left alone. */
int nhip_ms_archive_restore_plan(uint64_t aocl_leafs, const uint64_t *chunk_len, uint64_t n_chunks,
                                 const uint64_t *minimum, const uint32_t *distances, const uint64_t *aocl_leaf_index,
                                 size_t n, nhip_ms_updated *out);
/* nhip_ms_archive_restore_plan decided on the device, from the archive's own chunk table: the same outputs (status, the
 * four offset arrays, the keys, the totals; aocl_path, path and rel are left alone) with the two-call sizing of
 * nhip_ms_archive_restore, equal integer for integer to the host plan.  Only the index sets and the leaf indices go
 * up and only these integers come back; totals past the plan's limits are NHIP_ERR_OOM.  The kernels work on
 * NHIP_MS_RESTORE_WAVES witnesses per workgroup and scan in tiles of NHIP_MS_RESTORE_SCAN_WIDTH items, whose sums
 * NHIP_MS_RESTORE_CARRY_LANES lanes carry across the grid. */
#define NHIP_MS_RESTORE_WAVES 4
#define NHIP_MS_RESTORE_SCAN_WIDTH 256
#define NHIP_MS_RESTORE_CARRY_LANES 64
int nhip_ms_archive_restore_shape(nhip_ms_archive *archive, const uint64_t *minimum, const uint32_t *distances,
                                  const uint64_t *aocl_leaf_index, size_t n, nhip_ms_updated *out);
/* nhip_ms_archive_restore followed by nhip_ms_store_append of its output, device to device: afterwards the store
 * holds exactly what those two calls leave in it (device arrays, mirror, every later read, update, revert, retain
 * and check), and no path digest and no chunk word has crossed to the host.  The restore's shape is decided on the
 * device (nhip_ms_archive_restore_shape), the gather writes behind the store's totals, and only integers come back:
 * the statuses, the totals, the offset tails and the keys, which the store's mirror holds anyway.
 *   aocl_leaf  n x 5 words, as nhip_ms_update_in carries it, stored as given; NULL: a witness with a leaf index gets
 *              the archive's own level-0 digest at that index, one without gets zeros.
 *   status     n bytes or NULL: the restore's per-witness status.
 * All or nothing: unless every status is NHIP_MS_OK the store is unchanged and the return is NHIP_OK with the
 * statuses written; the caller filters and calls again.  n == 0 is NHIP_OK and changes nothing.  NHIP_ERR_ARG before
 * anything is touched: a NULL store or archive, an archive of another nhip_ctx than the store's, NULL inputs with
 * n > 0.  A poisoned archive is NHIP_ERR_HIP.  NHIP_ERR_OOM and NHIP_ERR_HIP leave the store as it was (every growth
 * precedes the first write, the mirror is committed behind a clean drain); the archive is only read. */
int nhip_ms_store_append_restored(nhip_ms_store *store, nhip_ms_archive *archive, const uint64_t *minimum,
                                  const uint32_t *distances, const uint64_t *aocl_leaf_index,
                                  const uint64_t *aocl_leaf, size_t n, uint8_t *status);

/* ---- a block file's mutator-set and transaction rules ---------------------------
 * Block::validate rules 2.a-2.l (protocol/consensus/block/mod.rs:811-891) for every (parent, child) pair of
 * scanned blocks, from the file's bytes: msa_before is the parent's Block::mutator_set_accumulator_after
 * (mod.rs:369-378,816), i.e. the parent body's accumulator plus the parent's two guesser-fee addition records
 * (block_kernel.rs:47-93).  Every digest is computed on the device and every status is the device's.
 *
 * nhip_blk_ms_params: NativeCurrency.hash() and TimeLock.hash() (type_scripts/native_currency.rs,
 * time_lock.rs) come from tasm-lib code generation, so they are parameters, canonical digests; the limit of
 * rules 2.j-2.l is MAX_NUM_INPUTS_OUTPUTS_ANNOUNCEMENTS = 1 << 14 (consensus_rule_set.rs:71-91). */
typedef struct {
    uint64_t native_currency_hash[5], time_lock_hash[5];
    uint32_t pow_tree_height;
    uint32_t max_num_inputs, max_num_outputs, max_num_announcements;
} nhip_blk_ms_params;
/* both digests zero (the caller fills them in), pow_tree_height 29, the three limits 1 << 14 */
void nhip_blk_ms_params_default(nhip_blk_ms_params *out);
/* nhip_blk_ms_walk (host only, hashes nothing): what rules 2.a-2.l and the guesser-fee records read of n scanned
 * blocks (blocks[i] from nhip_blk_scan of the same bytes with the same pow_tree_height <= 64; each is parsed
 * again from its offset, a malformed one is NHIP_ERR_DECODE), as integers and byte copies only.  Per block: the
 * header's height, timestamp and guesser_receiver_data; the kernel's fee and coinbase (i128 as two u64, low
 * first; coinbase_tag is the Option tag), timestamp and announcement count; the body's
 * mutator_set_accumulator (peak counts as serialized, saturated at 65; at most 64 peaks are stored, in 64
 * slots per block); the kernel's outputs (canonical commitments) and its inputs as they lie in the file, i.e.
 * in the packed reading of DESIGN.md §6f: rec_off / minimum / distances and the dictionaries with an entry's
 * key in chunk_index.  Two-call sizing, as nhip_ms_unpack_plan: with every array pointer NULL only the totals
 * are written; otherwise every array is present with its capacity, and NHIP_ERR_ARG if one is too small. */
typedef struct {
    uint64_t *height, *timestamp;                  /* n each */
    uint64_t *receiver_digest, *lock_script_hash;  /* n x 5 */
    uint64_t *fee, *coinbase;                      /* n x 2 */
    uint8_t *coinbase_tag;                         /* n */
    uint64_t *kernel_timestamp, *n_announcements;  /* n */
    uint64_t *aocl_num_leafs, *swbf_num_leafs;     /* n */
    uint32_t *aocl_n_peaks, *swbf_n_peaks;         /* n */
    uint64_t *aocl_peaks, *swbf_peaks;             /* n x 64 digests */
    uint64_t *active_off;                          /* n + 1, in u32 */
    uint32_t *active;                              /* active_cap: ActiveWindow::sbf */
    uint64_t *out_off;                             /* n + 1, in addition records */
    uint64_t *outputs;                             /* outputs_cap digests */
    uint64_t *rec_off;                             /* n + 1, in removal records */
    uint64_t *minimum;                             /* records_cap x 2 */
    uint32_t *distances;                           /* records_cap x 45 */
    uint64_t *entry_off;                           /* records_cap + 1 */
    uint64_t *chunk_index;                         /* entries_cap */
    uint64_t *path_off;                            /* entries_cap + 1, in digests */
    uint64_t *path;                                /* path_cap digests */
    uint64_t *rel_off;                             /* entries_cap + 1, in u32 */
    uint32_t *rel;                                 /* rel_cap */
    size_t active_cap, outputs_cap, records_cap, entries_cap, path_cap, rel_cap;
    size_t active_words, n_outputs, records, entries, path_digests, rel_words; /* out: the totals */
} nhip_blk_ms_parts;
int nhip_blk_ms_walk(const uint8_t *bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block *blocks,
                     size_t n, nhip_blk_ms_parts *out);
/* status of a block's guesser-fee records */
enum {
    NHIP_GUESSER_OK = 0,
    NHIP_GUESSER_NEGATIVE_FEE = 1 /* BlockBody::total_guesser_reward (block_body.rs:160-169): no records */
};
/* BlockKernel::guesser_fee_addition_records (block_kernel.rs:47-93) of n scanned blocks, one lane per (block,
 * UTXO): records[i] = [locked, unlocked], each commit(Tip5::hash(utxo), Block::hash, receiver_digest)
 * (util_types/mutator_set.rs:49-54), with timelocked = fee / 2, unlocked = fee - timelocked and the time lock
 * until header.timestamp + Timestamp::years(3) (a Goldilocks sum).  n_records[i] is 2, or 0 for a block at
 * height 0 or with a negative fee (its records are then zero); status[i] is NHIP_GUESSER_*.  digests: n x 5 as
 * nhip_blk_digests or nhip_blk_chain_check wrote them, or NULL to compute them here through nhip_blk_digests'
 * code (pow_tree_height <= 32).  The Utxo / Coin encodings are unpinned. */
int nhip_blk_guesser_fee_records(nhip_ctx *ctx, const uint8_t *bytes, size_t n_bytes, const nhip_blk_ms_params *params,
                                 const nhip_blk_block *blocks, size_t n, const uint64_t *digests, uint64_t *records,
                                 uint8_t *n_records, uint8_t *status);
/* block_validation_error.rs, in rule order; the first rule that fails is the status */
enum {
    NHIP_BLKMS_OK = 0,
    NHIP_BLKMS_SKIPPED = 1,                  /* parent_of[i] == -1: nothing checked */
    NHIP_BLKMS_UNPACK = 2,                   /* 2.a; ms_status = NHIP_MS_UNPACK_* */
    NHIP_BLKMS_PARENT_NEGATIVE_FEE = 3,      /* the `?` of mod.rs:816 */
    NHIP_BLKMS_PARENT_MSA_INCONSISTENT = 4,  /* divergence, failing closed (NHIP_MS_INCONSISTENT): also a parent
                                                accumulator with more than 64 peaks */
    NHIP_BLKMS_REMOVAL_RECORDS_VALIDITY = 5,   /* 2.b; ms_status = the first failing record's, bad_record = it */
    NHIP_BLKMS_REMOVAL_RECORDS_UNIQUENESS = 6, /* 2.c */
    NHIP_BLKMS_UPDATE_IMPOSSIBLE = 7,          /* 2.d */
    NHIP_BLKMS_UPDATE_INTEGRITY = 8,           /* 2.e; also a claimed accumulator with more than 64 peaks */
    NHIP_BLKMS_TRANSACTION_TIMESTAMP = 9,      /* 2.f */
    NHIP_BLKMS_COINBASE_TOO_BIG = 10,          /* 2.g */
    NHIP_BLKMS_NEGATIVE_COINBASE = 11,         /* 2.h */
    NHIP_BLKMS_NEGATIVE_FEE = 12,              /* 2.i */
    NHIP_BLKMS_TOO_MANY_INPUTS = 13,           /* 2.j: the unpacked inputs */
    NHIP_BLKMS_TOO_MANY_OUTPUTS = 14,          /* 2.k */
    NHIP_BLKMS_TOO_MANY_ANNOUNCEMENTS = 15     /* 2.l */
};
/* Rules 2.a-2.l for every (blocks[parent_of[i]], blocks[i]) pair: status[i] is NHIP_BLKMS_*, ms_status[i] the
 * NHIP_MS_* detail of rules 2.a-2.e (NHIP_MS_OK otherwise) and bad_record[i] the record nhip_ms_apply_batch_packed
 * blames (UINT64_MAX: none).  k_guesser_fee_records makes every block's records; pass A is nhip_ms_apply_batch over
 * (the parent body's accumulator, its records, no removals); pass B is nhip_ms_apply_batch_packed over (pass A's
 * accumulator, the child's packed inputs, its outputs, its body's accumulator as the expected one);
 * k_blk_ms_rules evaluates 2.f-2.l and combines the statuses.  Pass A's accumulators cross to the host between the
 * passes; the records' paths and chunks never do.  digests as above.  A parent index outside -1..n-1 or a null
 * pointer with a non-zero count is NHIP_ERR_ARG and a malformed block NHIP_ERR_DECODE, the outputs untouched. */
int nhip_blk_ms_check(nhip_ctx *ctx, const uint8_t *bytes, size_t n_bytes, const nhip_blk_ms_params *params,
                      const nhip_blk_block *blocks, size_t n, const int64_t *parent_of, const uint64_t *digests,
                      uint8_t *status, uint8_t *ms_status, uint64_t *bad_record);

/* ---- kernel timing (HIP events on the ctx stream around every kernel launch) ------------ */
int nhip_timing_enable(nhip_ctx *ctx, int on);
/* Total device time of the kernels launched since the last reset, and their count. */
int nhip_timing_read(nhip_ctx *ctx, double *total_ms, uint64_t *launches, int reset);

#ifdef __cplusplus
}
#endif
#endif /* NEPTUNE_HIP_H */
