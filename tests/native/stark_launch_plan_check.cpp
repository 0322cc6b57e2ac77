// Host-side check of stark_launch_plan.hpp (run by tests/test_stark_launch_plan_host.py, plain and
// under ASan + UBSan).
//  1. old_launch() is a transcription of launch_phases as it was before the schedule was split from
//     the enqueue: the same ifs, loops and arithmetic in the same order, each HIP call replaced by a
//     record.  walk_plan() is the enqueue over a LaunchPlan, recording the same way.  The two record
//     lists must be equal for every case.
//  2. Properties of the plan and of its walk.
//  3. Every branch of the schedule must have been reached.
// Cases: every shape (n, k, max_R, levels, max_lcw, capacity profile) with a rotating sample of the
// modes, and every mode combination (streams, marks, timing, release level, forced form, forced
// climb-from, global slots, knob set) on a reduced set of shapes.
#include "stark_launch_plan.hpp"

#include <cstdio>
#include <vector>
using namespace nhip;

static uint64_t bad = 0, n_cases = 0;
static void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0) {
    if (!ok) {
        if (bad < 10) printf("FAIL %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
        ++bad;
    }
}

enum Op : uint8_t {
    MARK, WAIT, PAD, K_DECODE, K_FS_ROWS_SMALL, K_FS_PAIR, K_FS_QUAD, K_FS_ROW, K_PLAN_FRI_SMALL, K_PLAN_128,
    K_PLAN_256, K_ROWS_WIDE, K_ROWS, K_FRI, K_OOD_1024_GS, K_OOD_1024, K_OOD_256_GS, K_OOD_256, K_DEEP, K_CLIMB,
    K_TAIL, K_WIDE, K_HASH7, K_HASH6, K_ROOTS_VERDICTS, K_ROOTS, K_VERDICTS, OP_N
};
struct Rec {
    Op op;
    uint8_t stream;  // 0 main, 1 aux (the main stream's number when the batch runs on one)
    int32_t slot;    // timed slot, -1 none, -2 the row launch's pair
    uint32_t gx, gy, block;
    uint64_t a[4];  // the scalar arguments that are decisions; MARK / WAIT: a[0] = the event
    bool operator==(const Rec& o) const {
        return op == o.op && stream == o.stream && slot == o.slot && gx == o.gx && gy == o.gy && block == o.block &&
               a[0] == o.a[0] && a[1] == o.a[1] && a[2] == o.a[2] && a[3] == o.a[3];
    }
};
struct Log {
    Rec r[512];
    uint32_t n = 0;
    uint32_t launches = 0;
    uint32_t tail_caps[MP_TAIL_LEVELS_MAX] = {};
    void add(Op op, int stream, uint32_t gx, uint32_t gy, uint32_t block, int32_t slot = -1, uint64_t a0 = 0,
             uint64_t a1 = 0, uint64_t a2 = 0, uint64_t a3 = 0) {
        if (n < 512) r[n] = Rec{op, (uint8_t)stream, slot, gx, gy, block, {a0, a1, a2, a3}};
        ++n;
    }
};

// kernel constants of stark_kernels.hip the launch sites name
static constexpr uint32_t CLIMB_THREADS = 1024, TAIL_THREADS = 1024;

struct Case {
    LaunchInput in;
    LaunchKnobs kn;
};

// ---------------------------------------------------------------- 1a. the rules as they were
// `st` / `sa` are stream numbers; tm->x and b.x are read from the case.  The only departure from the
// text it restates: max_lcw >> (l + 1) is written lcw_shift(), 0 from a shift of 32 on (levels the
// verifier's proofs cannot have, which the timing-cap case needs).
static uint32_t lcw_shift(uint32_t max_lcw, uint32_t l) { return l + 1 < 32 ? max_lcw >> (l + 1) : 0u; }

static void old_launch(const Case& c, Log& L) {
    const LaunchInput& b = c.in;
    const LaunchKnobs& kn = c.kn;
    const uint32_t n = b.n;
    const uint32_t k = b.k;
    const uint32_t tpp = 4 + b.max_R;
    const int st = 0, sa = b.two_streams ? 1 : 0;
    const bool two = st != sa;
    constexpr uint32_t SYNC = (1u << 12) | (1u << 0) | (1u << 1) | (1u << 3) | (1u << 7) | (1u << 10) | (1u << 8);
    auto mark = [&](int i, int s) {
        if (b.phase_marks || (two && ((SYNC >> i) & 1u))) L.add(MARK, s, 0, 0, 0, -1, (uint64_t)i);
    };
    auto wait = [&](int s, int i) {
        if (two) L.add(WAIT, s, 0, 0, 0, -1, (uint64_t)i);
    };
    auto pad = [&](int s) {
        for (int i = 0; i < kn.pad_packets; ++i) L.add(PAD, s, 1, 1, 64);
    };
    const bool small = n <= kn.climb_max;
    const uint32_t age_k = kn.age_prio >= 0 ? (uint32_t)kn.age_prio : (n >= 2048 ? 2u : 0u);
    const uint32_t age_sponge_k = kn.age_prio_fs ? age_k : 0u;
    mark(12, st);
    wait(sa, 12);
    L.add(K_DECODE, sa, n, 1, 64);
    pad(sa);
    mark(0, sa);
    wait(st, 0);
    int ff;  // fs_form(n)
    if (b.fs_form_forced >= 0) ff = b.fs_form_forced;
    else if (n < 512) ff = 1;
    else ff = n >= kn.quad_min ? 2 : 0;
    const bool fused = kn.fuse_fs_rows && !two && ff == 1 && n <= kn.rows_wide_max && !b.launch_events;
    const uint64_t rows = (uint64_t)n * k;
    if (fused) {
        const uint32_t fs_blocks = (n * 32 + 255) / 256;
        const uint32_t rows_gx = (uint32_t)((rows * 16 + 255) / 256);
        L.add(K_FS_ROWS_SMALL, sa, fs_blocks + 3 * rows_gx, 1, 256, -1, fs_blocks, rows_gx, age_sponge_k);
    } else if (ff == 1)
        L.add(K_FS_PAIR, sa, (n * 32 + 255) / 256, 1, 256, -1, 0, 0, age_sponge_k);
    else if (ff == 2)
        L.add(K_FS_QUAD, sa, (n * 4 + kn.quad_wg - 1) / kn.quad_wg, 1, kn.quad_wg, -1, 0, 0, age_sponge_k);
    else
        L.add(K_FS_ROW, sa, (n * 16 + 255) / 256, 1, 256, -1, 0, 0, age_sponge_k);
    pad(sa);
    mark(1, sa);
    const bool fused2 = kn.fuse_plan_fri && !two && small && k <= 256;
    if (fused2) {
        mark(13, sa);
        L.add(K_PLAN_FRI_SMALL, sa, n * (1 + b.max_R) + n, 1, 256, -1, tpp, 1 + b.max_R);
    } else if (k <= 128)
        L.add(K_PLAN_128, sa, n, 1 + b.max_R, 128, -1, tpp);
    else
        L.add(K_PLAN_256, sa, n, 1 + b.max_R, 256, -1, tpp);
    pad(sa);
    mark(3, sa);
    if (!fused) {
        unsigned gx = (unsigned)((rows + 255) / 256);
        if (gx > 16384) gx = 16384;
        const int32_t rslot = b.launch_events ? -2 : -1;
        if (n <= kn.rows_wide_max) L.add(K_ROWS_WIDE, st, (unsigned)((rows * 16 + 255) / 256), 3, 256, rslot);
        else L.add(K_ROWS, st, gx, 3, 256, rslot, 0, 0, age_k);
    }
    pad(st);
    mark(2, st);
    if (small && fused2) {
        mark(7, st);
    } else if (small) {
        wait(st, 1);
        mark(13, st);
        L.add(K_FRI, st, n, 1, 256);
        pad(st);
        mark(7, st);
    }
    wait(st, 3);
    auto launch_aux_chain = [&]() {
        mark(10, st);
        if (!small) wait(sa, 10);
        mark(11, sa);
        const bool gs = b.global_slots;
        if (n <= kn.ood_wide_max) {
            if (gs) L.add(K_OOD_1024_GS, sa, n, 1, 1024);
            else L.add(K_OOD_1024, sa, n, 1, 1024);
        } else {
            if (gs) L.add(K_OOD_256_GS, sa, n, 1, b.air_block);
            else L.add(K_OOD_256, sa, n, 1, b.air_block);
        }
        pad(sa);
        mark(6, sa);
        if (small) {
            wait(sa, 7);
        } else {
            L.add(K_FRI, sa, n, 1, 256);
            mark(7, sa);
        }
        L.add(K_DEEP, sa, n, 1, 256);
        pad(sa);
        mark(8, sa);
    };
    uint32_t launches = 0;
    bool aux_started = false;
    if (small) {
        launch_aux_chain();
        aux_started = true;
        const bool timed = b.launch_events && b.hash_events;
        L.add(K_CLIMB, st, n, tpp + 1, CLIMB_THREADS, timed ? 0 : -1, 0u);
        pad(st);
        launches = 1;
    }
    const uint32_t log2_lcw = 31 - __builtin_clz(b.max_lcw);
    const uint32_t hash_levels = b.mp_levels > log2_lcw ? b.mp_levels : log2_lcw;
    uint32_t tail0 = hash_levels;
    while (tail0 > 0 && hash_levels - tail0 < 32) {
        const uint32_t l = tail0 - 1;
        const uint64_t ops = (l < b.mp_levels ? b.mp_cap_host[l] : 0) + (uint64_t)lcw_shift(b.max_lcw, l) * n;
        if (ops > 256) break;
        --tail0;
    }
    if (hash_levels - tail0 < 2) tail0 = hash_levels;
    for (uint32_t l = 0; l < hash_levels && !small; ++l) {
        if (!aux_started && (l >= kn.aux_after_level || l == tail0)) {
            launch_aux_chain();
            aux_started = true;
        }
        const bool timed = b.launch_events && launches < 64 && b.hash_events;
        const int32_t slot = timed ? (int32_t)launches : -1;
        {
            const uint64_t ops_l = (l < b.mp_levels ? b.mp_cap_host[l] : 0) + (uint64_t)lcw_shift(b.max_lcw, l) * n;
            uint64_t cf;  // climb_from_ops(hash_levels)
            if (b.climb_from_forced >= 0) cf = (uint64_t)b.climb_from_forced;
            else cf = hash_levels >= 24 ? 4096ull : 0ull;
            if (cf && ops_l <= cf && hash_levels - l >= 3) {
                L.add(K_CLIMB, st, n, tpp + 1, CLIMB_THREADS, slot, l);
                ++launches;
                break;
            }
        }
        if (l == tail0) {
            for (uint32_t t = l; t < hash_levels; ++t)
                L.tail_caps[t - l] = t < b.mp_levels ? (uint32_t)b.mp_cap_host[t] : 0u;
            L.add(K_TAIL, st, 1, 1, TAIL_THREADS, slot, l, hash_levels);
            ++launches;
            break;
        }
        const uint64_t cap = l < b.mp_levels ? b.mp_cap_host[l] : 0;
        const uint32_t mp_blocks = (uint32_t)((cap + 255) / 256);
        const uint64_t per = lcw_shift(b.max_lcw, l);
        const uint32_t lcw_blocks = (uint32_t)((per * n + 255) / 256);
        if (mp_blocks + lcw_blocks == 0) continue;
        const bool wide = cap + per * n <= 48 * 1024;
        if (wide) L.add(K_WIDE, st, (unsigned)(((cap + per * n) * 16 + 255) / 256), 1, 256, slot, l, cap);
        else if (n < kn.mp_small_max) L.add(K_HASH7, st, mp_blocks + lcw_blocks, 1, 256, slot, l, mp_blocks, age_k);
        else L.add(K_HASH6, st, mp_blocks + lcw_blocks, 1, 256, slot, l, mp_blocks, age_k);
        ++launches;
    }
    if (!aux_started) launch_aux_chain();
    L.launches = launches;
    mark(4, st);
    const uint32_t nrec = n * tpp;
    if (!two && nrec + n <= 1024) {
        L.add(K_ROOTS_VERDICTS, st, 1, 1, 1024, -1, nrec, tpp);
        mark(5, st);
    } else {
        L.add(K_ROOTS, st, (nrec + n + 255) / 256, 1, 256, -1, nrec, tpp);
        pad(st);
        mark(5, st);
        wait(st, 8);
        L.add(K_VERDICTS, st, (n + 255) / 256, 1, 256);
    }
    mark(9, st);
}

// ---------------------------------------------------------------- 1b. the enqueue over a plan
static void walk_plan(const LaunchPlan& p, const Case& c, Log& L) {
    const uint32_t n = c.in.n;
    const int st = 0, sa = p.two_streams ? 1 : 0;
    auto mark = [&](StarkEvent e, int s) {
        if (p.records(e)) L.add(MARK, s, 0, 0, 0, -1, (uint64_t)e);
    };
    auto wait = [&](int s, StarkEvent e) {
        if (p.two_streams) L.add(WAIT, s, 0, 0, 0, -1, (uint64_t)e);
    };
    auto pad = [&](int s) {
        for (int i = 0; i < c.kn.pad_packets; ++i) L.add(PAD, s, 1, 1, 64);
    };
    auto fri = [&](int s) { L.add(K_FRI, s, n, 1, 256); };
    mark(EV_FORK, st);
    wait(sa, EV_FORK);
    L.add(K_DECODE, sa, n, 1, 64);
    pad(sa);
    mark(EV_DECODED, sa);
    wait(st, EV_DECODED);
    // aux stream: Fiat-Shamir, plan
    if (p.fused_fs_rows) L.add(K_FS_ROWS_SMALL, sa, p.fs_grid, 1, p.fs_block, -1, p.fs_blocks, p.rows_gx, p.age_sponge_k);
    else
        L.add(p.fs_form == FS_PAIR ? K_FS_PAIR : p.fs_form == FS_QUAD ? K_FS_QUAD : K_FS_ROW, sa, p.fs_grid, 1,
              p.fs_block, -1, 0, 0, p.age_sponge_k);
    pad(sa);
    mark(EV_FS_DONE, sa);
    if (p.fused_plan_fri) {
        mark(EV_FRI_START, sa);
        L.add(K_PLAN_FRI_SMALL, sa, n * p.plan_groups + n, 1, 256, -1, p.trees_per_proof, p.plan_groups);
    } else {
        L.add(p.plan_block == 128 ? K_PLAN_128 : K_PLAN_256, sa, n, p.plan_groups, p.plan_block, -1, p.trees_per_proof);
    }
    pad(sa);
    mark(EV_PLAN_DONE, sa);
    // main stream: rows, FRI of a small batch
    if (!p.fused_fs_rows) {
        const int32_t rslot = p.rows_timed ? -2 : -1;
        if (p.rows_wide) L.add(K_ROWS_WIDE, st, p.rows_grid, 3, 256, rslot);
        else L.add(K_ROWS, st, p.rows_grid, 3, 256, rslot, 0, 0, p.age_k);
    }
    pad(st);
    mark(EV_ROWS_DONE, st);
    if (p.fri_on_main) {
        if (!p.fused_plan_fri) {
            wait(st, EV_FS_DONE);
            mark(EV_FRI_START, st);
            fri(st);
            pad(st);
        }
        mark(EV_FRI_DONE, st);
    }
    wait(st, EV_PLAN_DONE);
    auto aux_chain = [&]() {
        mark(EV_AUX_RELEASE, st);
        if (!p.fri_on_main) wait(sa, EV_AUX_RELEASE);
        mark(EV_AUX_START, sa);
        const Op ood = p.ood_block == 1024 ? (p.ood_global_slots ? K_OOD_1024_GS : K_OOD_1024)
                                           : (p.ood_global_slots ? K_OOD_256_GS : K_OOD_256);
        L.add(ood, sa, n, 1, p.ood_threads);
        pad(sa);
        mark(EV_OOD_DONE, sa);
        if (p.fri_on_main) {
            wait(sa, EV_FRI_DONE);
        } else {
            fri(sa);
            mark(EV_FRI_DONE, sa);
        }
        L.add(K_DEEP, sa, n, 1, 256);
        pad(sa);
        mark(EV_DEEP_DONE, sa);
    };
    for (uint32_t s = 0; s < p.n_steps; ++s) {
        if (s == p.aux_release_step) aux_chain();
        const HashStep& h = p.steps[s];
        switch (h.kind) {
            case HashKind::Climb: L.add(K_CLIMB, st, h.grid, p.trees_per_proof + 1, CLIMB_THREADS, h.slot, h.level); break;
            case HashKind::Tail:
                for (uint32_t t = 0; t < MP_TAIL_LEVELS_MAX; ++t) L.tail_caps[t] = p.tail_caps[t];
                L.add(K_TAIL, st, h.grid, 1, TAIL_THREADS, h.slot, h.level, p.hash_levels);
                break;
            case HashKind::Wide: L.add(K_WIDE, st, h.grid, 1, 256, h.slot, h.level, h.arg); break;
            case HashKind::Level7: L.add(K_HASH7, st, h.grid, 1, 256, h.slot, h.level, h.arg, p.age_k); break;
            case HashKind::Level6: L.add(K_HASH6, st, h.grid, 1, 256, h.slot, h.level, h.arg, p.age_k); break;
        }
    }
    if (p.one_climb) pad(st);
    if (p.aux_release_step == p.n_steps) aux_chain();
    L.launches = p.n_steps;
    mark(EV_HASH_DONE, st);
    if (p.roots_one_launch) {
        L.add(K_ROOTS_VERDICTS, st, p.roots_grid, 1, 1024, -1, p.n_records, p.trees_per_proof);
        mark(EV_ROOTS_DONE, st);
    } else {
        L.add(K_ROOTS, st, p.roots_grid, 1, 256, -1, p.n_records, p.trees_per_proof);
        pad(st);
        mark(EV_ROOTS_DONE, st);
        wait(st, EV_DEEP_DONE);
        L.add(K_VERDICTS, st, p.verdicts_grid, 1, 256);
    }
    mark(EV_VERDICTS, st);
}

// ---------------------------------------------------------------- 2. properties, 3. coverage
static uint64_t hits[OP_N], hit_single_small, hit_zero_ops, hit_timing_cap, hit_release_late, hit_not_ok;

static void check_properties(const LaunchPlan& p, const Case& c, const Log& L) {
    uint32_t mark_pos[2][STARK_EVENTS];  // [stream][event]: position of its record + 1
    for (auto& s : mark_pos)
        for (auto& e : s) e = 0;
    uint32_t n_ood = 0, n_steps = 0, n_marks = 0, n_waits = 0;
    for (uint32_t i = 0; i < L.n && i < 512; ++i) {
        const Rec& r = L.r[i];
        ++hits[r.op];
        if (r.op == MARK) {
            ++n_marks;
            expect(mark_pos[r.stream][r.a[0]] == 0, "an event is recorded once", r.a[0]);
            mark_pos[r.stream][r.a[0]] = i + 1;
        } else if (r.op == WAIT) {
            ++n_waits;
            expect((CROSS_STREAM_EVENTS >> r.a[0]) & 1u, "a waited event is in the cross-stream set", r.a[0]);
            expect(mark_pos[r.stream ^ 1][r.a[0]] != 0, "a waited event was recorded on the other stream", r.a[0], i);
        } else {
            expect(r.gx != 0 && r.gy != 0 && r.block != 0, "no zero grid", r.op, i);
            n_ood += r.op >= K_OOD_1024_GS && r.op <= K_OOD_256;
            n_steps += r.op >= K_CLIMB && r.op <= K_HASH6;
        }
    }
    expect(n_ood == 1, "the aux chain is released once", n_ood);
    expect(p.aux_release_step <= p.n_steps, "the release point is a step or the end");
    expect(n_steps == p.n_steps && L.launches == p.n_steps, "mp_hash_launches = the number of steps", n_steps, p.n_steps);
    if (!c.in.two_streams) expect(n_waits == 0, "one stream: no waits", n_waits);
    if (!c.in.two_streams && !c.in.phase_marks) expect(n_marks == 0, "one stream, no phase marks: no records", n_marks);
    if (c.in.two_streams && !c.in.phase_marks)
        expect(n_marks == (uint32_t)__builtin_popcount(CROSS_STREAM_EVENTS), "two streams: the cross-stream records");
    if (c.in.phase_marks) expect(n_marks == STARK_EVENTS - (p.fri_on_main ? 0u : 1u), "marks: every event", n_marks);
    const bool timed = c.in.launch_events && c.in.hash_events;
    for (uint32_t s = 0; s < p.n_steps; ++s) {
        const HashStep& h = p.steps[s];
        const bool rest = h.kind == HashKind::Tail || h.kind == HashKind::Climb;
        if (s) expect(h.level > p.steps[s - 1].level, "levels strictly increase", s);
        if (rest) expect(s + 1 == p.n_steps, "a tail or climb step is the last", s);
        expect(h.grid != 0, "no zero grid (step)", s);
        // (a small batch's one climb is launched whatever the trees' height)
        expect(p.one_climb || h.level < p.hash_levels, "a step's level is a hash level", s);
        expect(h.slot == (timed && s < MAX_HASH_LAUNCHES ? (int32_t)s : -1), "timed slots in order", s);
        if (timed && s >= MAX_HASH_LAUNCHES) ++hit_timing_cap;
    }
    if (p.aux_release_step && p.aux_release_step < p.n_steps) ++hit_release_late;
    // the phase brackets: both ends recorded when the batch takes phase marks
    if (c.in.phase_marks) {
        const PhaseBrackets& sp = p.spans;
        for (const PhaseSpan& s : {sp.decode, sp.fs, sp.rows, sp.plan, sp.hash[0], sp.hash[1], sp.roots, sp.ood, sp.fri,
                                   sp.deep, sp.total}) {
            const uint32_t a = mark_pos[0][s.from] | mark_pos[1][s.from], z = mark_pos[0][s.to] | mark_pos[1][s.to];
            expect(a && z && a < z, "a phase's bracket is recorded, begin before end", s.from, s.to);
        }
    }
}

static void run_case(const Case& c) {
    static Log A, B;
    ++n_cases;
    const LaunchPlan p = plan_launch(c.in, c.kn);
    if (!p.ok) {  // more levels than a plan holds: nothing is launched
        ++hit_not_ok;
        expect(c.in.mp_levels > MAX_HASH_STEPS, "a plan that is not ok has too many levels");
        return;
    }
    A.n = B.n = 0;
    for (uint32_t t = 0; t < MP_TAIL_LEVELS_MAX; ++t) A.tail_caps[t] = B.tail_caps[t] = 0;
    old_launch(c, A);
    walk_plan(p, c, B);
    bool same = A.n == B.n && A.n <= 512 && A.launches == B.launches;
    for (uint32_t i = 0; same && i < A.n; ++i) same = A.r[i] == B.r[i];
    for (uint32_t t = 0; same && t < MP_TAIL_LEVELS_MAX; ++t) same = A.tail_caps[t] == B.tail_caps[t];
    if (!same && bad < 10) {
        printf("MISMATCH n %u k %u R %u levels %u lcw %u two %d marks %d ev %d/%d fs %d cf %lld: %u vs %u records\n",
               c.in.n, c.in.k, c.in.max_R, c.in.mp_levels, c.in.max_lcw, c.in.two_streams, c.in.phase_marks,
               c.in.launch_events, c.in.hash_events, c.in.fs_form_forced, (long long)c.in.climb_from_forced, A.n, B.n);
        for (uint32_t i = 0; i < A.n && i < B.n && i < 512; ++i)
            if (!(A.r[i] == B.r[i])) {
                printf("  first difference at %u: op %d vs %d, grid %u vs %u\n", i, A.r[i].op, B.r[i].op, A.r[i].gx, B.r[i].gx);
                break;
            }
    }
    expect(same, "the plan's walk equals the restated launch");
    check_properties(p, c, B);
    // coverage of the schedule's own branches
    const uint32_t log2_lcw = 31 - __builtin_clz(c.in.max_lcw);
    const uint32_t hl = c.in.mp_levels > log2_lcw ? c.in.mp_levels : log2_lcw;
    if (!p.one_climb && hl) {
        auto ops = [&](uint32_t l) {
            return (l < c.in.mp_levels ? c.in.mp_cap_host[l] : 0) + (uint64_t)lcw_shift(c.in.max_lcw, l) * c.in.n;
        };
        if (ops(hl - 1) <= MP_TAIL_MAX_OPS && (hl == 1 || ops(hl - 2) > MP_TAIL_MAX_OPS)) ++hit_single_small;
        // the levels launched one by one: all of them, or those below a tail or climb step
        uint32_t swept = hl, per_level = p.n_steps;
        if (p.n_steps && (p.steps[p.n_steps - 1].kind == HashKind::Tail || p.steps[p.n_steps - 1].kind == HashKind::Climb))
            swept = p.steps[p.n_steps - 1].level, --per_level;
        uint32_t empty = 0;
        for (uint32_t l = 0; l < swept; ++l) empty += ops(l) == 0;
        expect(per_level + empty == swept, "one launch per level with ops", per_level, swept);
        if (empty) ++hit_zero_ops;
    }
}

// ---------------------------------------------------------------- cases
static const uint32_t NS[] = {1, 2, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097, 16384};
static const uint32_t KS[] = {1, 53, 128, 129, 256};
static const uint32_t RS[] = {0, 1, 7, 16};
// 70: more hash levels than MAX_HASH_LAUNCHES timed slots (no proof has them; the timing cap's case);
// 100: more than a plan holds
static const uint32_t LEVELS[] = {0, 1, 2, 3, 9, 19, 26, 28, 70, 100};
static const uint32_t LCWS[] = {1, 2, 512, 1u << 20};
enum Profile { ZERO, HALVING, ONE_FAT, TAIL_EXACT, TAIL_MORE, WIDE_EXACT, WIDE_MORE, CLIMB_EXACT, CLIMB_MORE, PROFILES };

// the capacity of every level so that its ops (capacity + last-codeword parents) are `total`, where they can be
static void fill_total(std::vector<uint64_t>& cap, uint32_t n, uint32_t max_lcw, uint64_t total) {
    for (uint32_t l = 0; l < cap.size(); ++l) {
        const uint64_t lcw = (uint64_t)lcw_shift(max_lcw, l) * n;
        cap[l] = total > lcw ? total - lcw : 0;
    }
}
static void fill_profile(std::vector<uint64_t>& cap, int profile, uint32_t n, uint32_t k, uint32_t max_lcw, int64_t cf_forced) {
    const uint32_t levels = (uint32_t)cap.size() - 1;  // one spare entry: mp_cap_host is never empty
    for (auto& c : cap) c = 0;
    const uint64_t cf = cf_forced > 0 ? (uint64_t)cf_forced : CLIMB_FROM_OPS_DEFAULT;
    switch (profile) {
        case ZERO: break;
        case HALVING:
            for (uint32_t l = 0; l < levels; ++l) cap[l] = l < 63 ? ((uint64_t)n * k) >> l : 0;
            break;
        case ONE_FAT:  // below the last level: the last one alone is small
            if (levels) cap[levels >= 2 ? levels - 2 : 0] = (uint64_t)n * k + MP_WIDE_MAX_OPS;
            break;
        case TAIL_EXACT: fill_total(cap, n, max_lcw, MP_TAIL_MAX_OPS); break;
        case TAIL_MORE: fill_total(cap, n, max_lcw, MP_TAIL_MAX_OPS + 1); break;
        case WIDE_EXACT: fill_total(cap, n, max_lcw, MP_WIDE_MAX_OPS); break;
        case WIDE_MORE: fill_total(cap, n, max_lcw, MP_WIDE_MAX_OPS + 1); break;
        case CLIMB_EXACT: fill_total(cap, n, max_lcw, cf); break;
        case CLIMB_MORE: fill_total(cap, n, max_lcw, cf + 1); break;
    }
    cap[levels] = 0;
}

static LaunchKnobs other_knobs() {
    LaunchKnobs kn;
    kn.ood_wide_max = 32;
    kn.rows_wide_max = 64;
    kn.quad_wg = 512;
    kn.quad_min = 1024;
    kn.age_prio = 3;
    kn.age_prio_fs = true;
    kn.fuse_fs_rows = false;
    kn.fuse_plan_fri = false;
    kn.mp_small_max = 1024;
    kn.climb_max = 64;
    kn.pad_packets = 1;
    return kn;
}

// the modes, numbered 0 .. N_MODES - 1
static const uint32_t AUX_AFTER[] = {0, 3, 1000};
static const int64_t CF_FORCED[] = {-1, 0, 1, 4096};
static constexpr uint32_t N_MODES = 2 * 2 * 3 * 3 * 4 * 4 * 2 * 2;
static void set_mode(Case& c, uint32_t m) {
    c.in.two_streams = m % 2; m /= 2;
    c.in.phase_marks = m % 2; m /= 2;
    const uint32_t ev = m % 3; m /= 3;  // off; on without hash events; on with them
    c.in.launch_events = ev != 0;
    c.in.hash_events = ev != 1;  // a resident batch has them whether or not it times a launch
    const uint32_t aux = AUX_AFTER[m % 3]; m /= 3;
    c.in.fs_form_forced = (int)(m % 4) - 1; m /= 4;
    c.in.climb_from_forced = CF_FORCED[m % 4]; m /= 4;
    c.in.global_slots = m % 2; m /= 2;
    c.kn = m % 2 ? other_knobs() : LaunchKnobs{};
    c.kn.aux_after_level = aux;
}

int main() {
    // the knobs' defaults are the shipped thresholds; outside an A/B build the environment changes nothing
    {
        const LaunchKnobs kn = launch_knobs_from_env(), d{};
        expect(kn.ood_wide_max == 64 && kn.rows_wide_max == 32 && kn.quad_wg == 256 && kn.quad_min == 2048 &&
                   kn.fs_form_init == -1 && kn.age_prio == -1 && !kn.age_prio_fs && kn.fuse_fs_rows && kn.fuse_plan_fri &&
                   kn.mp_small_max == 4096 && kn.climb_max == 32 && kn.aux_after_level == 0 && kn.pad_packets == 0,
               "knob defaults");
        expect(d.climb_max == kn.climb_max && d.quad_wg == kn.quad_wg, "default-constructed knobs are the defaults");
        expect(CROSS_STREAM_EVENTS == ((1u << 12) | (1u << 0) | (1u << 1) | (1u << 3) | (1u << 7) | (1u << 10) | (1u << 8)),
               "the cross-stream set");
        expect(STARK_EVENTS == 14, "14 events");
    }
    std::vector<uint64_t> cap;
    Case c{};
    c.in.air_block = 256;
    uint32_t rot = 0;
    for (uint32_t n : NS)
        for (uint32_t k : KS)
            for (uint32_t R : RS)
                for (uint32_t levels : LEVELS)
                    for (uint32_t lcw : LCWS)
                        for (int prof = 0; prof < PROFILES; ++prof) {
                            cap.assign(levels + 1, 0);
                            c.in.n = n, c.in.k = k, c.in.max_R = R, c.in.mp_levels = levels, c.in.max_lcw = lcw;
                            c.in.air_block = (n + k) % 2 ? 256 : 1024;
                            // every shape: 8 modes, rotating through all of them (1,009 is prime to N_MODES)
                            for (int i = 0; i < 8; ++i) {
                                rot = (rot + 1009) % N_MODES;
                                set_mode(c, rot);
                                fill_profile(cap, prof, n, k, lcw, c.in.climb_from_forced);
                                c.in.mp_cap_host = cap.data();
                                run_case(c);
                            }
                            // every mode on a reduced set of shapes
                            const bool reduced = k == 53 && R == 1 && lcw == 512 && (levels == 3 || levels == 19 || levels == 26 || levels == 70) &&
                                                 (prof == HALVING || prof == CLIMB_EXACT || prof == TAIL_MORE);
                            for (uint32_t m = 0; reduced && m < N_MODES; ++m) {
                                set_mode(c, m);
                                fill_profile(cap, prof, n, k, lcw, c.in.climb_from_forced);
                                c.in.mp_cap_host = cap.data();
                                run_case(c);
                            }
                        }
    static const char* names[OP_N] = {"mark", "wait", "pad", "k_decode", "k_fs_rows_small", "k_fs_replay_wide<pair>",
        "k_fs_replay_quad", "k_fs_replay_wide<row>", "k_plan_fri_small", "k_mp_plan<128>", "k_mp_plan<256>",
        "k_hash_rows_wide", "k_hash_rows", "k_fri", "k_ood_air<1024,gs>", "k_ood_air<1024>", "k_ood_air<256,gs>",
        "k_ood_air<256>", "k_deep_rows8", "k_mp_climb", "k_mp_hash_tail", "k_mp_hash_wide", "k_mp_hash<7>", "k_mp_hash<6>",
        "k_roots_verdicts_small", "k_mp_roots", "k_verdicts"};
    for (int i = 0; i < OP_N; ++i) {
        printf("hit %-24s %llu\n", names[i], (unsigned long long)hits[i]);
        expect(hits[i] != 0, "a launch kind was never reached", (uint64_t)i);
    }
    const struct {
        const char* name;
        uint64_t v;
    } branches[] = {{"single small level", hit_single_small}, {"zero-ops level skipped", hit_zero_ops},
                    {"timing cap", hit_timing_cap}, {"release between steps", hit_release_late},
                    {"too many levels", hit_not_ok}};
    for (const auto& b : branches) {
        printf("hit %-24s %llu\n", b.name, (unsigned long long)b.v);
        expect(b.v != 0, b.name);
    }
    printf("cases %llu bad %llu\n", (unsigned long long)n_cases, (unsigned long long)bad);
    return bad ? 1 : 0;
}
