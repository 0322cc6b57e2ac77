// The AIR object of the batched STARK verifier (include/neptune_hip.h: nhip_air_*): descriptor
// parsing and levelization, the compiler of k_ood_air's slot program (air_compile), the per-GPU
// device copies, and the parameter checks that tie a caller's nhip_stark_params to an AIR
// (dims_from, nhip_stark_params_default, nhip_proof_decodes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/neptune_hip.h"
#include "../../include/nhip_challenge_id.h"
#include "device_scope.hpp"
#include "goldilocks.hpp"
#include "kernels.hpp"
#include "stark.hpp"
#include "stark_host_internal.hpp"

using namespace nhip;

bool nhip::dims_from(const nhip_stark_params* sp, const nhip_air* air, Dims& D) {
    if (!sp || !air) return false;
    if (sp->num_collinearity_checks < 1 || sp->num_collinearity_checks > (uint32_t)MAX_CHECKS) return false;
    if (sp->log2_fri_expansion < 1 || sp->log2_fri_expansion > 8) return false;
    if (sp->num_main != air->dims_air.num_main || sp->num_aux != air->dims_air.num_aux) return false;
    if (sp->num_quotient_segments < 1 || sp->num_quotient_segments > 64) return false;
    if (sp->input_form != NHIP_INPUT_CANONICAL && sp->input_form != NHIP_INPUT_MONTGOMERY) return false;
    // DEEP kernel: carry-free accumulators (M + 3A row words, DEEP_ROW_WORDS_MAX), weights in LDS
    if (sp->num_main + 3ull * sp->num_aux >= DEEP_ROW_WORDS_MAX) return false;
    StarkDims& d = D.d;
    d.num_main = sp->num_main;
    d.num_aux = sp->num_aux;
    d.num_quot_seg = sp->num_quotient_segments;
    d.num_checks = sp->num_collinearity_checks;
    d.num_deep = 3;
    d.log2_expansion = sp->log2_fri_expansion;
    d.num_trace_randomizers = sp->num_collinearity_checks + 2 * 3;
    d.num_sampled = air->dims_air.num_sampled;
    d.num_constraints = air->dims_air.num_constraints;
    D.expansion = 1u << sp->log2_fri_expansion;
    D.mont_words = sp->input_form == NHIP_INPUT_MONTGOMERY ? 1u : 0u;
    if (deep_rows8_lds_bytes(d) > 160 * 1024 - 8192) return false;
    // the last FRI codeword has at most 2^(floor(log2 k) + 1 + log2 expansion) XFEs; bound its
    // Merkle-tree scratch (n x max_len digests)
    if ((1ull << (log2_u64(d.num_checks) + 1 + d.log2_expansion)) > 4096) return false;
    return true;
}

// The device copy of the compiled AIR on this context's GPU (uploaded on first use).
int nhip::air_upload(nhip_ctx* ctx, nhip_air* a, nhip_air::Dev* out) {
    std::lock_guard<std::mutex> g(a->mu);
    const int device = nhip_internal_device(ctx);
    for (const auto& d : a->devs)
        if (d.device == device) {
            *out = d;
            return NHIP_OK;
        }
    nhip_air::Dev d{device, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    auto free_dev = [&]() {
        for (int k = 0; k < 2; ++k) {
            if (d.d_prog[k]) (void)hipFree(d.d_prog[k]);
            if (d.d_prog_off[k]) (void)hipFree(d.d_prog_off[k]);
            if (d.d_consts[k]) (void)hipFree(d.d_consts[k]);
        }
    };
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        const OodProgram& pg = a->progs[k];
        e = hipMalloc(&d.d_prog[k], pg.prog.size() * sizeof(OodIns) + 16);
        if (e == hipSuccess) e = hipMalloc(&d.d_prog_off[k], pg.seg_off.size() * 4 + 4);
        if (e == hipSuccess) e = hipMalloc(&d.d_consts[k], pg.consts.size() * sizeof(Xfe) + 24);
        if (e == hipSuccess && !pg.prog.empty())
            e = hipMemcpy(d.d_prog[k], pg.prog.data(), pg.prog.size() * sizeof(OodIns), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(d.d_prog_off[k], pg.seg_off.data(), pg.seg_off.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && !pg.consts.empty())
            e = hipMemcpy(d.d_consts[k], pg.consts.data(), pg.consts.size() * sizeof(Xfe), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        free_dev();
        return hipfail(e);
    }
    try {
        a->devs.reserve(a->devs.size() + 1);
    } catch (const std::bad_alloc&) {
        free_dev();
        return NHIP_ERR_OOM;
    }
    a->devs.push_back(d);
    *out = d;
    return NHIP_OK;
}

// The program a batch of n proofs runs: the wide-step one up to NHIP_OOD_WIDE_PROG_MAX proofs (default
// 1,024), where one proof's evaluation latency matters more than proofs per CU.  Config 4 per-GPU
// shares (profiles/r04f): 512 proofs 416-419k proofs/s wide vs 398k narrow, 1,024: 427-430k vs 420k,
// 2,048: 368-374k vs 440k (8 steps in flight: the wide program's one workgroup per CU is the
// bottleneck there), 4,096: 425k vs 436-437k.
int nhip::ood_program_for(uint32_t n) {
    static const uint32_t lim = [] {
        const char* e = nhip::ab_env("NHIP_OOD_WIDE_PROG_MAX");
        return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 1024u;
    }();
    return n <= lim ? 1 : 0;
}

namespace {

// Instructions per step of the compiled AIR program: two per thread of k_ood_air's 256-thread
// workgroups (nhip_air_options.step_width sets another, tests of the compiler).
static constexpr uint32_t OOD_STEP_WIDTH = 512;
// Products of a step come in multiples of a wave where the ready list allows (air_compile).
static constexpr uint32_t OOD_MUL_QUOTA = 64;

// Compile the circuit into the slot program of k_ood_air (OodIns, stark.hpp): a sequence of
// steps, each a set of independent instructions the workgroup runs between two barriers, every
// value in a slot from the step that computes it to the step of its last use (a slot is reused
// from the step after).  The steps come from list scheduling with a liveness priority instead of
// the circuit's levels: a level-by-level program keeps every value of a wide level live at once
// (triton-air-sized circuits: ~13k slots, half of them past the LDS budget in global memory), while
// here each step takes up to `width` ready nodes, those that retire an operand (its last use) first,
// then in the order of the first constraint that needs them, so constraints are finished one after
// another and their values released (the same circuit: ~2.3k slots, all in LDS, 3x the steps).
// A step never takes a node past the LDS slot budget unless it retires a value or the step would be
// empty.  A constraint's value is copied (OOD_ACC) in the step after it is computed into its own slot
// of the top C slots (slots - C + c), and the kernel weighs all C of them in full waves after the last
// step: folded into the steps, each step paid one mostly idle wave of two XFE products per lane for
// its handful of constraints.  Within a step the instructions are grouped by kind (copies, products,
// sums, differences): a wave then runs one kind of XFE operation instead of the divergent union of
// several.
void air_compile(const nhip_air* a, const std::vector<uint32_t>& cons, uint32_t width, uint32_t slot_budget,
                 OodProgram& pg) {
    pg = OodProgram{};
    pg.width = width;
    const size_t NN = a->nodes.size();
    const auto is_op = [&](size_t i) {
        const uint32_t op = a->nodes[i].op;
        return op == AIR_ADD || op == AIR_SUB || op == AIR_MUL;
    };
    // nodes the constraints reach, each with the first constraint (descriptor order) that needs it
    std::vector<uint32_t> corder(NN, UINT32_MAX);
    {
        std::vector<uint32_t> st;
        for (size_t c = 0; c < cons.size(); ++c) {
            st.push_back(cons[c]);
            while (!st.empty()) {
                const uint32_t i = st.back();
                st.pop_back();
                if (corder[i] != UINT32_MAX) continue;
                corder[i] = (uint32_t)c;
                if (is_op(i)) {
                    st.push_back(a->nodes[i].a);
                    st.push_back(a->nodes[i].b);
                }
            }
        }
    }
    // every live value in a slot: inputs and constants are copied in (LOAD from the inputs or the
    // constant table), so the operands of ADD / SUB / MUL are slots only and the kernel reads them
    // from LDS without telling slots from constants (each constant is used about once)
    std::vector<uint32_t> ref(NN, 0), cidx(NN, 0);
    std::vector<uint8_t> slotted(NN, 0);  // live nodes (every one takes a slot)
    for (size_t i = 0; i < NN; ++i) {
        if (corder[i] == UINT32_MAX) continue;  // dead node
        if (a->nodes[i].op == AIR_CONST) {
            cidx[i] = (uint32_t)pg.consts.size();
            pg.consts.push_back(Xfe{a->nodes[i].k0, a->nodes[i].k1, a->nodes[i].k2});
        }
        slotted[i] = 1;
    }
    // remaining uses of each slotted value (operand occurrences + accumulations), pending operands of
    // each node, and the users of each value (CSR)
    std::vector<uint32_t> remaining(NN, 0), deps(NN, 0), uoff(NN + 1, 0);
    for (size_t i = 0; i < NN; ++i)
        if (slotted[i] && is_op(i))
            for (uint32_t o : {a->nodes[i].a, a->nodes[i].b})
                if (slotted[o]) ++remaining[o], ++deps[i], ++uoff[o + 1];
    for (uint32_t c : cons)
        if (slotted[c]) ++remaining[c];
    for (size_t i = 0; i < NN; ++i) uoff[i + 1] += uoff[i];
    std::vector<uint32_t> users(uoff[NN]);
    {
        std::vector<uint32_t> fill(uoff.begin(), uoff.end() - 1);
        for (size_t i = 0; i < NN; ++i)
            if (slotted[i] && is_op(i))
                for (uint32_t o : {a->nodes[i].a, a->nodes[i].b})
                    if (slotted[o]) users[fill[o]++] = (uint32_t)i;
    }
    std::vector<std::vector<uint32_t>> acc_of(NN);  // per node: the constraints whose value it is
    for (size_t c = 0; c < cons.size(); ++c) acc_of[cons[c]].push_back((uint32_t)c);
    std::vector<uint32_t> ready;
    for (size_t i = 0; i < NN; ++i)
        if (slotted[i] && deps[i] == 0) ready.push_back((uint32_t)i);
    // working slots; the C constraint slots above them take their share of the LDS first
    // (nhip_air_options.slot_budget lowers it: tests of the compiler)
    uint32_t budget = AIR_LDS_SLOTS_MAX > cons.size() + 256 ? AIR_LDS_SLOTS_MAX - (uint32_t)cons.size() : 256u;
    if (slot_budget) budget = std::min<uint32_t>(budget, std::max<uint32_t>(64u, slot_budget));
    std::vector<uint32_t> free_slots, to_free;
    uint32_t next_slot = 0, live = 0;
    std::vector<OodIns> cur, acc_next;
    std::vector<std::pair<int32_t, uint64_t>> key(NN);
    auto retires = [&](uint32_t i) {  // operands whose last use this node is
        if (!is_op(i)) return 0;
        const uint32_t x = a->nodes[i].a, y = a->nodes[i].b;
        int r = 0;
        if (slotted[x] && remaining[x] == (x == y ? 2u : 1u)) ++r;
        if (slotted[y] && y != x && remaining[y] == 1u) ++r;
        return r;
    };
    auto use = [&](uint32_t o) {  // a read of o in this step (its slot index is ref[o])
        if (slotted[o] && --remaining[o] == 0) to_free.push_back(ref[o]);
    };
    pg.prog_off.assign(1, 0);
    while (!ready.empty() || !acc_next.empty()) {
        cur.swap(acc_next);  // the accumulations of the values of the step before
        acc_next.clear();
        for (const OodIns& ins : cur)
            if (slotted[cons[ins.b]]) use(cons[ins.b]);
        for (uint32_t i : ready) key[i] = {-retires(i), ((uint64_t)corder[i] << 32) | i};
        std::sort(ready.begin(), ready.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
        // the step's constraint copies count against its width (width + a few would be one more,
        // nearly empty pass of the workgroup)
        const size_t room = width > cur.size() ? width - cur.size() : 1;
        std::vector<uint32_t> chosen, rest;
        for (uint32_t i : ready) {
            if (chosen.size() < room && (live < budget || key[i].first < 0 || chosen.empty())) {
                chosen.push_back(i);
                ++live;
            } else {
                rest.push_back(i);
            }
        }
        // Products in whole waves: a 64-lane pass of k_ood_air that holds one product pays an XFE
        // product on the whole wave, so the products past the last multiple of 64 (the step's lowest
        // priorities among them) wait for a later step, where they fill a wave with the products that
        // have become ready by then, unless that would leave the step empty or they retire a value
        // (waiting would hold the slot).  Ready sums, differences and copies take the room.
        {
            const auto is_mul = [&](uint32_t i) { return a->nodes[i].op == AIR_MUL; };
            size_t muls = 0;
            for (uint32_t i : chosen) muls += is_mul(i);
            size_t drop = muls % OOD_MUL_QUOTA;
            if (drop && (muls > drop || chosen.size() > muls)) {
                std::vector<uint32_t> kept, back;
                for (size_t k = chosen.size(); k-- > 0;) {
                    const uint32_t i = chosen[k];
                    if (drop && is_mul(i) && key[i].first == 0) {
                        back.push_back(i);
                        --drop;
                        --live;
                    } else {
                        kept.push_back(i);
                    }
                }
                std::reverse(kept.begin(), kept.end());
                chosen.swap(kept);
                std::vector<uint32_t> rest2;
                for (uint32_t i : rest) {
                    if (!is_mul(i) && chosen.size() < room && (live < budget || key[i].first < 0)) {
                        chosen.push_back(i);
                        ++live;
                    } else {
                        rest2.push_back(i);
                    }
                }
                rest.swap(rest2);
                rest.insert(rest.end(), back.begin(), back.end());
            }
        }
        ready.swap(rest);
        for (uint32_t i : chosen) {
            uint32_t sl;
            if (!free_slots.empty()) {
                sl = free_slots.back();
                free_slots.pop_back();
            } else {
                sl = next_slot++;
            }
            const AirNode& nd = a->nodes[i];
            if (nd.op == AIR_INPUT) {
                cur.push_back(OodIns{OOD_LOAD, OOD_REF_INPUT | (nd.a << 27) | nd.b, 0, sl});
            } else if (nd.op == AIR_CONST) {
                cur.push_back(OodIns{OOD_LOAD, OOD_REF_CONST | cidx[i], 0, sl});
            } else {
                cur.push_back(OodIns{nd.op, ref[nd.a], ref[nd.b], sl});
                use(nd.a);
                use(nd.b);
            }
            ref[i] = OOD_REF_SLOT | sl;
            for (uint32_t c : acc_of[i]) acc_next.push_back(OodIns{OOD_ACC, ref[i], c, 0});
        }
        for (uint32_t i : chosen)
            for (uint32_t k = uoff[i]; k < uoff[i + 1]; ++k)
                if (--deps[users[k]] == 0) ready.push_back(users[k]);
        // values whose last use was in this step: their slots take new values from the next step on
        live -= (uint32_t)to_free.size();
        free_slots.insert(free_slots.end(), to_free.begin(), to_free.end());
        to_free.clear();
        auto kind_rank = [](uint32_t op) {
            return op == OOD_LOAD || op == OOD_ACC ? 0 : (op == AIR_MUL ? 1 : (op == AIR_ADD ? 2 : 3));
        };
        std::stable_sort(cur.begin(), cur.end(),
                         [&](const OodIns& x, const OodIns& y) { return kind_rank(x.op) < kind_rank(y.op); });
        // the bounds of the step's segments: copies | products | sums and differences
        uint32_t bound = (uint32_t)pg.prog.size();
        for (int rank = 0; rank < 3; ++rank) {
            pg.seg_off.push_back(bound);
            for (const OodIns& ins : cur) bound += kind_rank(ins.op) == rank || (rank == 2 && kind_rank(ins.op) == 3);
        }
        pg.prog.insert(pg.prog.end(), cur.begin(), cur.end());
        pg.prog_off.push_back((uint32_t)pg.prog.size());
        cur.clear();
    }
    pg.seg_off.push_back((uint32_t)pg.prog.size());
    for (OodIns& ins : pg.prog)
        if (ins.op == OOD_ACC) ins.dst = next_slot + ins.b;
    pg.slots = next_slot + (uint32_t)cons.size();
}

}  // namespace

extern "C" {

void nhip_stark_params_default(nhip_stark_params* out) {
    if (!out) return;
    out->security_level = 160;
    out->log2_fri_expansion = 2;
    out->num_collinearity_checks = 80;  // security_level / log2_fri_expansion
    out->num_main = 379;
    out->num_aux = 88;
    out->num_quotient_segments = 4;
    out->input_form = NHIP_INPUT_CANONICAL;
}

int nhip_air_create(const uint64_t* w, size_t n, nhip_air** out) { return nhip_air_create_ex(w, n, nullptr, out); }

int nhip_air_create_ex(const uint64_t* w, size_t n, const nhip_air_options* opt, nhip_air** out) {
    if (!w || !out || n < 9) return NHIP_ERR_ARG;
    *out = nullptr;
    const nhip_air_options o = opt ? *opt : nhip_air_options{0, 0, 0};
    const uint32_t width = o.step_width ? o.step_width : OOD_STEP_WIDTH;
    if (width < 16 || width > (1u << 16)) return NHIP_ERR_ARG;
    if (w[0] != 0x41495231ull) return NHIP_ERR_ARG;
    const uint64_t M = w[1], A = w[2], K = w[3], NN = w[4];
    const uint64_t nc[4] = {w[5], w[6], w[7], w[8]};
    const uint64_t C = nc[0] + nc[1] + nc[2] + nc[3];
    // K: the sampled challenges, triton-air's Challenges::SAMPLE_COUNT (include/nhip_challenge_id.h);
    // the derived ones (K .. K + 3) read sampled ChallengeIds up to LookupTablePublicIndeterminate
    if (M > (1u << 20) || A > (1u << 20) || K != NHIP_CHALLENGE_SAMPLE_COUNT || NN > (1u << 24) || C > (1u << 24))
        return NHIP_ERR_ARG;
    if (n != 9 + 4 * NN + C) return NHIP_ERR_ARG;
    nhip_air* a = new (std::nothrow) nhip_air();
    if (!a) return NHIP_ERR_OOM;
    a->dims_air.num_main = (uint32_t)M;
    a->dims_air.num_aux = (uint32_t)A;
    a->dims_air.num_sampled = (uint32_t)K;
    a->dims_air.num_constraints = (uint32_t)C;
    a->nodes.resize(NN);
    std::vector<uint32_t> level(NN, 0);
    uint32_t max_level = 0;
    const uint64_t* nw = w + 9;
    for (uint64_t i = 0; i < NN; ++i) {
        const uint64_t op = nw[4 * i], x = nw[4 * i + 1], y = nw[4 * i + 2], z = nw[4 * i + 3];
        AirNode nd{};
        nd.op = (uint32_t)op;
        bool ok = true;
        if (op == AIR_INPUT) {
            const uint64_t lim = x == IN_MAIN_CURR || x == IN_MAIN_NEXT ? M
                                 : (x == IN_AUX_CURR || x == IN_AUX_NEXT ? A : (x == IN_CHALLENGE ? K + NHIP_NUM_DERIVED_CHALLENGES : 0));
            ok = x <= IN_CHALLENGE && y < lim;
            nd.a = (uint32_t)x;
            nd.b = (uint32_t)y;
        } else if (op == AIR_CONST) {
            nd.k0 = to_mont(x);
            nd.k1 = to_mont(y);
            nd.k2 = to_mont(z);
        } else if (op == AIR_ADD || op == AIR_SUB || op == AIR_MUL) {
            ok = x < i && y < i;
            nd.a = (uint32_t)x;
            nd.b = (uint32_t)y;
            if (ok) level[i] = 1 + std::max(level[x], level[y]);
        } else {
            ok = false;
        }
        if (!ok) {
            delete a;
            return NHIP_ERR_ARG;
        }
        a->nodes[i] = nd;
        max_level = std::max(max_level, level[i]);
    }
    a->level_off.assign(max_level + 2, 0);
    for (uint64_t i = 0; i < NN; ++i) a->level_off[level[i] + 1]++;
    for (uint32_t l = 0; l <= max_level; ++l) a->level_off[l + 1] += a->level_off[l];
    const uint64_t* cw = nw + 4 * NN;
    std::vector<uint32_t> cons(C);
    for (uint64_t i = 0; i < C; ++i) {
        if (cw[i] >= NN) {
            delete a;
            return NHIP_ERR_ARG;
        }
        cons[i] = (uint32_t)cw[i];
    }
    a->cons_off = make_uint4((uint32_t)nc[0], (uint32_t)(nc[0] + nc[1]), (uint32_t)(nc[0] + nc[1] + nc[2]), (uint32_t)C);
    air_compile(a, cons, width, o.slot_budget, a->progs[0]);
    air_compile(a, cons, 2 * width, o.slot_budget, a->progs[1]);
    if (o.lds_slots) a->lds_cap = std::min<uint32_t>(AIR_LDS_SLOTS_MAX, o.lds_slots);
    *out = a;
    return NHIP_OK;
}

void nhip_air_destroy(nhip_air* a) {
    if (!a) return;
    for (const auto& d : a->devs) {
        const DeviceScope device_scope(d.device);
        for (int k = 0; k < 2; ++k) {
            (void)hipFree(d.d_prog[k]);
            (void)hipFree(d.d_prog_off[k]);
            (void)hipFree(d.d_consts[k]);
        }
    }
    delete a;
}

int nhip_air_info(const nhip_air* a, uint32_t* num_nodes, uint32_t* num_levels, uint32_t* num_constraints) {
    if (!a) return NHIP_ERR_ARG;
    if (num_nodes) *num_nodes = (uint32_t)a->nodes.size();
    if (num_levels) *num_levels = (uint32_t)a->level_off.size() - 1;
    if (num_constraints) *num_constraints = a->dims_air.num_constraints;
    return NHIP_OK;
}

// Slots of the compiled AIR program: held in LDS, and past the LDS budget (global memory).
int nhip_air_slots(const nhip_air* a, uint32_t* lds_slots, uint32_t* global_slots) {
    if (!a) return NHIP_ERR_ARG;
    const uint32_t l = std::min<uint32_t>(a->progs[0].slots, a->lds_cap);
    if (lds_slots) *lds_slots = l;
    if (global_slots) *global_slots = a->progs[0].slots - l;
    return NHIP_OK;
}

int nhip_air_program(const nhip_air* a, uint32_t* step_off, size_t step_cap, uint32_t* ins, size_t ins_cap,
                     size_t* n_steps, size_t* n_ins) {
    if (!a) return NHIP_ERR_ARG;
    const OodProgram& pg = a->progs[0];
    const size_t ns = pg.prog_off.size() - 1, ni = pg.prog.size();
    if (n_steps) *n_steps = ns;
    if (n_ins) *n_ins = ni;
    if (step_off) {
        if (step_cap < ns + 1) return NHIP_ERR_ARG;
        std::memcpy(step_off, pg.prog_off.data(), (ns + 1) * 4);
    }
    if (ins) {
        if (ins_cap < 4 * ni) return NHIP_ERR_ARG;
        for (size_t i = 0; i < ni; ++i) {
            ins[4 * i] = pg.prog[i].op;
            ins[4 * i + 1] = pg.prog[i].a;
            ins[4 * i + 2] = pg.prog[i].b;
            ins[4 * i + 3] = pg.prog[i].dst;
        }
    }
    return NHIP_OK;
}

// The per-kind segments of the program's steps: 3 bounds per step (copies, products, sums and
// differences) and the end of the program.
int nhip_air_segments(const nhip_air* a, uint32_t* seg_off, size_t seg_cap, size_t* n_bounds) {
    if (!a) return NHIP_ERR_ARG;
    const OodProgram& pg = a->progs[0];
    if (n_bounds) *n_bounds = pg.seg_off.size();
    if (seg_off) {
        if (seg_cap < pg.seg_off.size()) return NHIP_ERR_ARG;
        std::memcpy(seg_off, pg.seg_off.data(), pg.seg_off.size() * 4);
    }
    return NHIP_OK;
}

// Host-only structural check (no GPU): 1 if the proof stream decodes with the expected item
// sequence and counts, else 0.  Used by CPU tests of the decoder and by callers that want to
// reject garbage before touching a device.
int nhip_proof_decodes(const nhip_air* air, const nhip_stark_params* sp, const nhip_claim* claim,
                       const nhip_proof* proof) {
    Dims D{};
    if (!claim || !proof || (proof->len && !proof->words) || !dims_from(sp, air, D)) return -NHIP_ERR_ARG;
    // the same walk k_decode runs, straight on the caller's words (proof_codec.hpp)
    ProofDesc pd;
    FsOp ops[fs_ops_for(MAX_FRI_ROUNDS)];
    uint64_t perms, perms_lcw;
    const ClaimLoc cl{0, (uint32_t)claim->input_len, (uint32_t)claim->output_len};
    const uint32_t f = D.mont_words ? decode_stream<true>(proof->words, 0, proof->len, cl, D, pd, ops, perms, perms_lcw)
                                    : decode_stream<false>(proof->words, 0, proof->len, cl, D, pd, ops, perms, perms_lcw);
    return f ? 0 : 1;
}

}  // extern "C"
