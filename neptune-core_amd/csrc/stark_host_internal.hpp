// What the host files of the batched STARK verifier share (internal, C++): the AIR object
// (air_host.cpp), the pinned-range registry (host_pinned.cpp), the context accessors of capi.hip, and
// the batch code's (stark_host.cpp) view of all three.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/neptune_hip.h"
#include "host_numa.hpp"
#include "kernels.hpp"
#include "stark.hpp"

// ctx internals live in capi.hip; access the stream / device via these helpers
extern "C" hipStream_t nhip_internal_stream(nhip_ctx* c);
extern "C" int nhip_internal_device(nhip_ctx* c);
extern "C" std::mutex* nhip_internal_mutex(nhip_ctx* c);
extern "C" void* nhip_internal_staging(nhip_ctx* c, size_t bytes);
extern "C" void* nhip_internal_verify_scratch(nhip_ctx* c, void* (*make)(), void (*freefn)(void*));
extern "C" const void* nhip_internal_topo(nhip_ctx* c);
extern "C" unsigned nhip_internal_host_threads(nhip_ctx* c);

// One compiled OOD program (air_compile): instructions, step offsets, constant table, slot count.
struct OodProgram {
    std::vector<nhip::OodIns> prog;
    std::vector<uint32_t> prog_off;
    // per-kind segments of each step (copies, products, sums and differences): 3 bounds per step + the
    // end, seg_off[3 s] == prog_off[s]; k_ood_air runs one loop per segment, so a wave runs one kind
    std::vector<uint32_t> seg_off;
    std::vector<nhip::Xfe> consts;
    uint32_t slots = 0;
    uint32_t width = 0;
};

struct nhip_air {
    nhip::StarkDims dims_air{};  // num_main, num_aux, num_sampled, num_constraints filled
    std::vector<nhip::AirNode> nodes;
    std::vector<uint32_t> level_off;  // node-level histogram (nhip_air_info)
    uint4 cons_off{};
    // compiled programs (see OodIns in stark.hpp, air_compile): [0] narrow steps (fewer live values:
    // more proofs per CU, for batches that fill the GPU), [1] wide steps (fewer barriers: lower
    // latency per proof, for smaller batches); a batch takes one by its size (ood_program_for)
    OodProgram progs[2];
    // slots held in LDS (the rest in the per-proof global area): AIR_LDS_SLOTS_MAX, or less when
    // nhip_air_options.lds_slots asks for it at creation (tests of the global-slot path)
    uint32_t lds_cap = nhip::AIR_LDS_SLOTS_MAX;
    // device copies, one per GPU that has used this AIR (read-only, so every context on that GPU
    // shares it; a group drives several contexts from one process, possibly concurrently);
    // created on first use, freed with the AIR
    struct Dev {
        int device;
        nhip::OodIns* d_prog[2];
        uint32_t* d_prog_off[2];  // the segment bounds (OodProgram::seg_off)
        nhip::Xfe* d_consts[2];
    };
    std::mutex mu;
    std::vector<Dev> devs;
};

namespace nhip {

inline int hipfail(hipError_t e) {
    return e == hipSuccess ? NHIP_OK : (e == hipErrorOutOfMemory ? NHIP_ERR_OOM : NHIP_ERR_HIP);
}
inline const HostTopo& ctx_topo(nhip_ctx* c) { return *(const HostTopo*)nhip_internal_topo(c); }

// ---- air_host.cpp
// The verifier's dimensions from the caller's parameters and the AIR; false = NHIP_ERR_ARG.
bool dims_from(const nhip_stark_params* sp, const nhip_air* air, Dims& D);
// The device copy of the compiled AIR on this context's GPU (uploaded on first use).
int air_upload(nhip_ctx* ctx, nhip_air* a, nhip_air::Dev* out);
// The program (index into nhip_air::progs) a batch of n proofs runs.
int ood_program_for(uint32_t n);

// ---- host_pinned.cpp
// Is [p, p + bytes) inside a pinned host range this library handed out or registered?
bool pinned_contains(const void* p, size_t bytes);

}  // namespace nhip
