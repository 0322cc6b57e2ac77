// The launch schedule of a STARK batch: which kernel instance runs at which size, with which grid,
// in which order, and which events bracket what.  plan_launch() decides all of it from the batch's
// shape and the tuning values, with integer arithmetic only; launch_phases (stark_kernels.hip) walks
// the plan and enqueues it.  Host only, no HIP call: tests/native/stark_launch_plan_check.cpp runs it
// against a restatement of the rules it replaced.  DESIGN.md §3a has the thresholds as a table.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "ab_env.hpp"
#include "kernels.hpp"

namespace nhip {

// ---- thresholds (each with the measurement it rests on; A/B builds override them, LaunchKnobs)
// batches of at most this many proofs climb every tree in its own workgroup (k_mp_climb), one
// launch for all levels, instead of one launch per level; they also run FRI on the main stream
static constexpr uint32_t MP_CLIMB_MAX_PROOFS = 32;
// batches of at most this many proofs hash their revealed rows in the 16-lane form (k_hash_rows_wide)
static constexpr uint32_t ROWS_WIDE_MAX_PROOFS = 32;
// k_ood_air<1024> (1,024 threads) up to this many proofs per batch, else <256>: below it one proof's
// evaluation is on the critical path and the CUs are idle
static constexpr uint32_t OOD_WIDE_MAX_PROOFS = 64;
// batches below this many proofs replay Fiat-Shamir on the two-row pair Tip5 (k_fs_replay_wide):
// one-collection latency 1.89 -> 1.65 ms, while from 512 proofs on (several steps in flight) the
// one-row form is 2-3% faster (profiles/r01i/ab_pair.log)
static constexpr uint32_t FS_PAIR_MAX_PROOFS = 512;
// batches of at least this many proofs replay Fiat-Shamir on the quad Tip5 (k_fs_replay_quad).
// 0.61x the row form's VALU instructions (profiles/r03g PMC), but fewer, longer replay waves: with
// 256-thread workgroups (one replay wave per SIMD of the CUs they land on) 4,096 proofs +1.5% and
// 2,048 +1.6% over the row form, 1,024 -3%; 64-thread workgroups -7 to -9% at every size, 512 /
// 1,024 threads -1 to -25% (profiles/r03g, 2 repetitions)
static constexpr uint32_t FS_QUAD_MIN_PROOFS = 2048;
static constexpr uint32_t FS_QUAD_WG = 256;  // k_fs_replay_quad workgroup size
// batches of at least this many proofs hash their revealed rows with the full rounds' MDS on the matrix
// cores (k_hash_rows<MW, true>, tip5_device.hpp mds_ark_planes): measured faster at 512, 1,024, 2,048 and
// 4,096 proofs (profiles/r09a); smaller batches, where a few waves per SIMD wait on one permutation's
// dependent chain, keep the VALU form
static constexpr uint32_t ROWS_PLANES_MIN_PROOFS = 512;
// batches below this many proofs hash their Merkle levels with the 7-wave k_mp_hash instance, larger
// ones with the 6-wave one.  7 waves: 2,048 proofs +1.3%, 1,024 +1.2%, 512 +3%; 4,096 -0.6%
// (profiles/r03ze, r03zf)
static constexpr uint32_t MP_SMALL_MAX_PROOFS = 4096;
// levels with at most this many hash ops run the 16-lane-row Tip5 (k_mp_hash_wide: latency-bound regime)
static constexpr uint64_t MP_WIDE_MAX_OPS = 48 * 1024;
// the last levels whose ops (multiproof + last-codeword parents) all fit this many rows are climbed
// by one workgroup in one launch (k_mp_hash_tail), up to MP_TAIL_LEVELS_MAX levels
#ifndef NHIP_MP_TAIL_MAX_OPS
#define NHIP_MP_TAIL_MAX_OPS 256
#endif
static constexpr uint64_t MP_TAIL_MAX_OPS = NHIP_MP_TAIL_MAX_OPS;
// Level-synchronous batches of deep trees (>= CLIMB_FROM_MIN_LEVELS hash levels: BASELINE config 5's
// height-23 proofs have 26) hand the rest of their trees to one per-tree climb launch (k_mp_climb
// from a start level) at the first level with at most CLIMB_FROM_OPS_DEFAULT hash ops: the top
// levels of a deep tree are launch-bound, not VALU-bound.  Measured
// (profiles/r05z/ab/climb_from_ab_r05q.txt): config 5's 64 proofs +3-6% at 4,096 ops; config 4's
// trees (<= 19 levels) are not affected (at 4,096 ops without the depth gate: 512 proofs -2 to -4%,
// 4,096 equal; 16K / 64K ops: worse).  nhip_set_climb_from_ops sets the threshold for every depth
// (tests: 0 = never).  A climb-from launch needs at least CLIMB_FROM_MIN_REST levels left.
static constexpr uint32_t CLIMB_FROM_MIN_LEVELS = 24;
static constexpr uint64_t CLIMB_FROM_OPS_DEFAULT = 4096;
static constexpr uint32_t CLIMB_FROM_MIN_REST = 3;
// hash levels launched before the OOD / FRI / DEEP chain is released; tuned on MI355X
static constexpr uint32_t AUX_AFTER_LEVEL_DEFAULT = 0;
// Oldest-first wave priority (age_priority, stark_kernels.hip): the AGE_PRIO_OLDEST oldest batch
// launches in flight run their hashing one priority level up, for batches of at least
// AGE_PRIO_MIN_PROOFS.  Measured (profiles/r05z/ab/age_prio_ab_r05w.txt, 3 alternating repetitions
// per run): config 4 in the driver's 20 steps at 4,096 proofs +1.4%, 2,048 +0.9%, 1,024 and 512
// equal.  Raising the sponge replay too: 512 -1 to -2% (round 5); 4,096 +0.6% and 2,048 equal,
// within the run-to-run spread (profiles/r06/ab_age_prio_fs.txt), so it stays off.
static constexpr uint32_t AGE_PRIO_OLDEST = 2;
static constexpr uint32_t AGE_PRIO_MIN_PROOFS = 2048;

// Fiat-Shamir replay form (k_fs_replay_wide / k_fs_replay_quad): 16-lane row, two-row pair, quad.
// nhip_set_fs_form forces one (tests and A/B runs).
enum FsForm { FS_ROW = 0, FS_PAIR = 1, FS_QUAD = 2 };

// ---- knobs: every tuning value the launch reads.  The defaults are the shipped verifier's; an A/B
// build (ab_env.hpp) reads each NHIP_* override once, at the first launch.
struct LaunchKnobs {
    uint32_t ood_wide_max = OOD_WIDE_MAX_PROOFS;    // NHIP_OOD_WIDE_MAX
    uint32_t rows_wide_max = ROWS_WIDE_MAX_PROOFS;  // NHIP_ROWS_WIDE_MAX
    uint32_t quad_wg = FS_QUAD_WG;                  // NHIP_QUAD_WG: 64..1024 in multiples of 64
    uint32_t quad_min = FS_QUAD_MIN_PROOFS;         // NHIP_FS_QUAD_MIN
    int fs_form_init = -1;      // NHIP_FS_FORM=row|pair|quad: nhip_set_fs_form's initial value
    int64_t age_prio = -1;      // NHIP_AGE_PRIO=k: k oldest launches raised at every size, 0 = off
    bool age_prio_fs = false;   // NHIP_AGE_PRIO_FS=1: the sponge replay raised as well
    bool fuse_fs_rows = true;   // NHIP_FUSE_SMALL=0 launches the replay and the row hashing apart
    bool fuse_plan_fri = true;  // NHIP_FUSE_PLAN_FRI=0 launches the plan and FRI apart
    uint32_t mp_small_max = MP_SMALL_MAX_PROOFS;        // NHIP_MP_SMALL_MAX
    uint32_t climb_max = MP_CLIMB_MAX_PROOFS;           // NHIP_CLIMB_MAX
    uint32_t aux_after_level = AUX_AFTER_LEVEL_DEFAULT;  // NHIP_AUX_AFTER_LEVEL
    int pad_packets = 0;  // NHIP_PAD_PACKETS: empty kernels after each kernel of the batch
    uint32_t rows_planes_min = ROWS_PLANES_MIN_PROOFS;  // NHIP_ROWS_PLANES_MIN (a huge value: never)
    bool mds_planes_mp = false;  // NHIP_MDS_PLANES_MP=1: k_mp_hash with the planes MDS in rounds 1-3 (A/B builds only)
};

inline unsigned long ab_unsigned(const char* name, unsigned long dflt) {
    const char* e = ab_env(name);
    return e ? std::strtoul(e, nullptr, 10) : dflt;
}

inline LaunchKnobs launch_knobs_from_env() {
    LaunchKnobs kn;
    kn.ood_wide_max = (uint32_t)ab_unsigned("NHIP_OOD_WIDE_MAX", kn.ood_wide_max);
    kn.rows_wide_max = (uint32_t)ab_unsigned("NHIP_ROWS_WIDE_MAX", kn.rows_wide_max);
    const uint32_t w = (uint32_t)ab_unsigned("NHIP_QUAD_WG", FS_QUAD_WG);
    kn.quad_wg = (w >= 64 && w <= 1024 && w % 64 == 0) ? w : FS_QUAD_WG;
    kn.quad_min = (uint32_t)ab_unsigned("NHIP_FS_QUAD_MIN", kn.quad_min);
    if (const char* v = ab_env("NHIP_FS_FORM"))
        kn.fs_form_init = v[0] == 'q' ? (int)FS_QUAD : v[0] == 'p' ? (int)FS_PAIR : v[0] == 'r' ? (int)FS_ROW : -1;
    kn.age_prio = (int64_t)ab_unsigned("NHIP_AGE_PRIO", (unsigned long)-1);
    if (const char* e = ab_env("NHIP_AGE_PRIO_FS")) kn.age_prio_fs = e[0] == '1';
    if (const char* e = ab_env("NHIP_FUSE_SMALL")) kn.fuse_fs_rows = e[0] != '0';
    if (const char* e = ab_env("NHIP_FUSE_PLAN_FRI")) kn.fuse_plan_fri = e[0] != '0';
    kn.mp_small_max = (uint32_t)ab_unsigned("NHIP_MP_SMALL_MAX", kn.mp_small_max);
    kn.climb_max = (uint32_t)ab_unsigned("NHIP_CLIMB_MAX", kn.climb_max);
    kn.aux_after_level = (uint32_t)ab_unsigned("NHIP_AUX_AFTER_LEVEL", kn.aux_after_level);
    kn.pad_packets = (int)ab_unsigned("NHIP_PAD_PACKETS", 0);
    kn.rows_planes_min = (uint32_t)ab_unsigned("NHIP_ROWS_PLANES_MIN", kn.rows_planes_min);
    if (const char* e = ab_env("NHIP_MDS_PLANES_MP")) kn.mds_planes_mp = e[0] == '1';
    return kn;
}
inline const LaunchKnobs& launch_knobs() {
    static const LaunchKnobs kn = launch_knobs_from_env();
    return kn;
}

// ---- events.  The cross-stream set is the fork / join points: recorded whenever the batch runs on
// two streams; the others only when the batch takes phase timestamps.
static constexpr uint32_t event_bit(StarkEvent e) { return 1u << (int)e; }
static constexpr uint32_t CROSS_STREAM_EVENTS = event_bit(EV_FORK) | event_bit(EV_DECODED) | event_bit(EV_FS_DONE) |
                                                event_bit(EV_PLAN_DONE) | event_bit(EV_FRI_DONE) |
                                                event_bit(EV_AUX_RELEASE) | event_bit(EV_DEEP_DONE);
static constexpr uint32_t ALL_EVENTS = (1u << STARK_EVENTS) - 1;

// ---- input: the batch's shape and the launch's modes
struct LaunchInput {
    uint32_t n, k, max_R;         // proofs, collinearity checks, most FRI rounds of a proof
    uint32_t mp_levels;           // multiproof plan levels, with
    const uint64_t* mp_cap_host;  // ... the op capacity of each
    uint32_t max_lcw;             // longest last codeword (a power of two)
    bool global_slots;            // the AIR's slots overflow LDS (air_gslot_n > 0)
    uint32_t air_block;           // k_ood_air<256>'s workgroup size for this AIR
    bool two_streams;
    bool phase_marks;    // take every phase timestamp (off in a captured graph)
    bool launch_events;  // dispatch begin / end events on the row and hash launches ...
    bool hash_events;    // ... which exist for the hash launches (a resident batch's own)
    int fs_form_forced;  // nhip_set_fs_form's value: -1 = by size
    int64_t climb_from_forced;  // nhip_set_climb_from_ops's value: -1 = by depth, 0 = never
};

// ---- output
enum class HashKind : uint8_t {
    Level6,  // k_mp_hash<NHIP_MP_WAVES>: one level, 6 waves
    Level7,  // k_mp_hash<NHIP_MP_WAVES_SMALL>: one level, 7 waves
    Wide,    // k_mp_hash_wide: one level on 16-lane rows
    Tail,    // k_mp_hash_tail: every level from `level` on, one workgroup
    Climb,   // k_mp_climb: every level from `level` on, one workgroup per (proof, tree)
};
struct HashStep {
    HashKind kind;
    uint32_t level;  // the level hashed, or the first of a tail / climb
    uint32_t grid;   // workgroups (Climb: proofs, by trees_per_proof + 1 in y)
    uint64_t arg;    // Wide: the level's multiproof op capacity; Level6/7: its multiproof workgroups
    int32_t slot;    // pair of per-launch events that times it, -1 = untimed
};
// one step per hash level at most; a proof's trees have at most LOG2_PH_MAX + log2 expansion levels
static constexpr uint32_t MAX_HASH_STEPS = 80;

struct LaunchPlan {
    bool ok = true;  // false: more hash levels than MAX_HASH_STEPS, nothing to launch
    bool two_streams;
    uint32_t recorded;  // the events this launch records (bit per StarkEvent)
    uint32_t trees_per_proof;
    uint32_t age_k, age_sponge_k;  // oldest-first priority of the hashing / of the sponge replay
    // Fiat-Shamir replay; fused with the 16-lane row hashing in k_fs_rows_small (fs_blocks replay
    // workgroups, then 3 x rows_gx hashing ones)
    FsForm fs_form;
    bool fused_fs_rows;
    uint32_t fs_grid, fs_block, fs_blocks, rows_gx;
    // Merkle plan; fused with FRI in k_plan_fri_small
    bool fused_plan_fri;
    uint32_t plan_block, plan_groups;  // k_mp_plan<plan_block>, grid (n, plan_groups)
    // row hashing (unless fused): grid (rows_grid, 3)
    bool rows_wide, rows_timed;
    uint32_t rows_grid;
    // Small batches: FRI on the main stream (it needs only the sponge samples), concurrent with the
    // plan and OOD on the aux stream, and DEEP waits for it; every tree climbed in one launch.  With
    // the climb that short, OOD -> FRI -> DEEP in a row would be the critical path.
    bool fri_on_main, one_climb;
    // OOD: k_ood_air<ood_block, MW, ood_global_slots> on ood_threads threads
    uint32_t ood_block, ood_threads;
    bool ood_global_slots;
    // Merkle hashing, in launch order.  The OOD / FRI / DEEP chain only needs the Fiat-Shamir samples,
    // but its kernels are latency-bound and hold CU resources for long: it is released before step
    // aux_release_step (n_steps: after the last), so that it overlaps the narrow top levels instead
    // of the wide, VALU-bound first ones.
    uint32_t hash_levels;
    uint32_t n_steps;  // = the mp_hash_launches nhip_stats reports
    uint32_t aux_release_step;
    HashStep steps[MAX_HASH_STEPS];
    uint32_t tail_caps[MP_TAIL_LEVELS_MAX];  // Tail: the multiproof op capacity of each of its levels
    // roots and verdicts: one workgroup, one launch (one stream: the aux chain is already in order)
    bool roots_one_launch;
    uint32_t n_records, roots_grid, verdicts_grid;
    PhaseBrackets spans;

    bool records(StarkEvent e) const { return (recorded >> (int)e) & 1u; }
};

inline LaunchPlan plan_launch(const LaunchInput& in, const LaunchKnobs& kn) {
    LaunchPlan p;
    const uint32_t n = in.n, k = in.k;
    const bool two = in.two_streams;
    p.two_streams = two;
    p.recorded = in.phase_marks ? ALL_EVENTS : (two ? CROSS_STREAM_EVENTS : 0u);
    p.trees_per_proof = 4 + in.max_R;
    p.age_k = kn.age_prio >= 0 ? (uint32_t)kn.age_prio : (n >= AGE_PRIO_MIN_PROOFS ? AGE_PRIO_OLDEST : 0u);
    p.age_sponge_k = kn.age_prio_fs ? p.age_k : 0u;
    const bool small = n <= kn.climb_max;
    p.fri_on_main = p.one_climb = small;

    // Fiat-Shamir.  Small batches: the sponge replay is the critical path and most SIMDs are idle, so
    // two rows per proof (pair form) for a shorter permutation; large ones: one row per proof (fewer
    // lane-instructions while the other steps' hashing fills the GPU); the largest: four lanes per
    // proof (quad form, fewer lane-instructions again).
    if (in.fs_form_forced >= 0) p.fs_form = (FsForm)in.fs_form_forced;
    else if (n < FS_PAIR_MAX_PROOFS) p.fs_form = FS_PAIR;
    else p.fs_form = n >= kn.quad_min ? FS_QUAD : FS_ROW;
    const uint64_t rows = (uint64_t)n * k;
    p.rows_wide = n <= kn.rows_wide_max;
    // one stream, pair form, 16-lane rows, untimed: the replay and the row hashing in one launch
    p.fused_fs_rows = kn.fuse_fs_rows && !two && p.fs_form == FS_PAIR && p.rows_wide && !in.launch_events;
    p.fs_block = 256;
    p.fs_blocks = p.rows_gx = 0;
    if (p.fused_fs_rows) {
        p.fs_blocks = (n * 32 + 255) / 256;
        p.rows_gx = (uint32_t)((rows * 16 + 255) / 256);
        p.fs_grid = p.fs_blocks + 3 * p.rows_gx;
    } else if (p.fs_form == FS_PAIR) {
        p.fs_grid = (n * 32 + 255) / 256;
    } else if (p.fs_form == FS_QUAD) {
        p.fs_block = kn.quad_wg;
        p.fs_grid = (n * 4 + kn.quad_wg - 1) / kn.quad_wg;
    } else {
        p.fs_grid = (n * 16 + 255) / 256;
    }

    // one stream, small, k <= 256: the plan and FRI in one launch
    p.fused_plan_fri = kn.fuse_plan_fri && !two && small && k <= 256;
    p.plan_block = k <= 128 ? 128 : 256;
    p.plan_groups = 1 + in.max_R;

    p.rows_timed = in.launch_events;
    if (p.rows_wide) {
        p.rows_grid = (uint32_t)((rows * 16 + 255) / 256);
    } else {
        const uint64_t gx = (rows + 255) / 256;
        p.rows_grid = gx > 16384 ? 16384u : (uint32_t)gx;
    }

    const bool ood_wide = n <= kn.ood_wide_max;
    p.ood_block = ood_wide ? 1024 : 256;
    p.ood_threads = ood_wide ? 1024 : in.air_block;
    p.ood_global_slots = in.global_slots;

    // Merkle hashing
    const uint32_t log2_lcw = 31 - __builtin_clz(in.max_lcw);
    const uint32_t hash_levels = in.mp_levels > log2_lcw ? in.mp_levels : log2_lcw;
    p.hash_levels = hash_levels;
    p.n_steps = 0;
    if (hash_levels > MAX_HASH_STEPS) {
        p.ok = false;
        return p;
    }
    auto cap_of = [&](uint32_t l) { return l < in.mp_levels ? in.mp_cap_host[l] : (uint64_t)0; };
    // last-codeword parents of level l (none from level 31 on: max_lcw has 32 bits)
    auto lcw_ops = [&](uint32_t l) { return l + 1 < 32 ? (uint64_t)(in.max_lcw >> (l + 1)) * n : (uint64_t)0; };
    auto step = [&](HashKind kind, uint32_t level, uint32_t grid, uint64_t arg) {
        const bool timed = in.launch_events && in.hash_events && p.n_steps < MAX_HASH_LAUNCHES;
        p.steps[p.n_steps] = HashStep{kind, level, grid, arg, timed ? (int32_t)p.n_steps : -1};
        ++p.n_steps;
    };
    if (small) {
        p.aux_release_step = 0;  // OOD right after the plan
        step(HashKind::Climb, 0, n, 0);
    } else {
        // first level of the tail climbed in one launch (every level from it on is small)
        uint32_t tail0 = hash_levels;
        while (tail0 > 0 && hash_levels - tail0 < MP_TAIL_LEVELS_MAX) {
            if (cap_of(tail0 - 1) + lcw_ops(tail0 - 1) > MP_TAIL_MAX_OPS) break;
            --tail0;
        }
        if (hash_levels - tail0 < 2) tail0 = hash_levels;  // a single small level: the per-level launch
        uint64_t climb_from = hash_levels >= CLIMB_FROM_MIN_LEVELS ? CLIMB_FROM_OPS_DEFAULT : 0;
        if (in.climb_from_forced >= 0) climb_from = (uint64_t)in.climb_from_forced;
        bool released = false;
        for (uint32_t l = 0; l < hash_levels; ++l) {
            if (!released && (l >= kn.aux_after_level || l == tail0)) {  // the tail is one workgroup
                p.aux_release_step = p.n_steps;
                released = true;
            }
            const uint64_t cap = cap_of(l), per_n = lcw_ops(l);
            // the rest of every tree climbed per (proof, tree group) in one launch once a level is small
            if (climb_from && cap + per_n <= climb_from && hash_levels - l >= CLIMB_FROM_MIN_REST) {
                step(HashKind::Climb, l, n, 0);
                break;
            }
            if (l == tail0) {
                for (uint32_t t = 0; t < MP_TAIL_LEVELS_MAX; ++t) p.tail_caps[t] = (uint32_t)cap_of(l + t);
                step(HashKind::Tail, l, 1, 0);
                break;
            }
            const uint32_t mp_blocks = (uint32_t)((cap + 255) / 256);
            const uint32_t lcw_blocks = (uint32_t)((per_n + 255) / 256);
            if (mp_blocks + lcw_blocks == 0) continue;
            if (cap + per_n <= MP_WIDE_MAX_OPS) step(HashKind::Wide, l, (uint32_t)(((cap + per_n) * 16 + 255) / 256), cap);
            else step(n < kn.mp_small_max ? HashKind::Level7 : HashKind::Level6, l, mp_blocks + lcw_blocks, mp_blocks);
        }
        if (!released) p.aux_release_step = p.n_steps;
    }

    p.n_records = n * p.trees_per_proof;
    p.roots_one_launch = !two && p.n_records + n <= ROOTS_ONE_WG;
    p.roots_grid = p.roots_one_launch ? 1 : (p.n_records + n + 255) / 256;
    p.verdicts_grid = (n + 255) / 256;

    // FRI on the main stream: timed from its own start event, and DEEP follows OOD.  Fused with the
    // plan (one stream), EV_FRI_START precedes k_plan_fri_small and EV_FRI_DONE follows the row
    // hashing, so the FRI span covers both of those launches.
    if (small) {
        p.spans.fri = {EV_FRI_START, EV_FRI_DONE};
        p.spans.deep = {EV_OOD_DONE, EV_DEEP_DONE};
    }
    return p;
}

}  // namespace nhip
