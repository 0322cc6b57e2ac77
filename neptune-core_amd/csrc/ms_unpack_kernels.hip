// RemovalRecordList::try_unpack's hashes (block rule 2.a): the program the host plan wrote
// (csrc/ms_unpack_plan.cpp), run by one launch.
//
//  k_ms_unpack : one 256-thread workgroup per job, every phase strided over the job's items with barriers
//                between them (the shape of k_ms_apply); the job's slot arena (one canonical digest per known
//                node) is in global memory, so a job of any size runs.
//                  1  structure digests -> their slots (one lane per word), and Tip5::hash of every distinct
//                     chunk -> its leaf slot (one lane per chunk): the absorb loop of k_ms_chunk_auth with the
//                     12-bit fields taken straight from the packed words, the unpacked chunk never stored
//                  2  per height above the leaves, one hash_pair per parent op (dst, left, right); a parent
//                     needs given nodes and parents of the level below only, so a barrier per level is the
//                     reference's fixpoint.  At most 63 levels.
//                  3  gather: one lane per (path digest, word) copies its source slot to the unpacked path
//                The number of launches does not grow with the tree height or the number of jobs.  The leaves
//                share the launch: a workgroup's distinct chunks are few and of like size in a block's list, and a
//                launch of their own would only add a grid-wide wait before the first level.
//
// Every index the kernel follows was written by the host plan for this very call and is inside the buffers the
// call staged: slots < n_slots, copy_src < the input's path digests, leaf_words + the chunk's packed length
// <= the input's rel words, gather targets < the unpacked path digests.
#include "ms_device.hpp"

namespace nhip {

__global__ void __launch_bounds__(256) k_ms_unpack(MsUnpackDev u, size_t n_jobs) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint32_t tid = threadIdx.x;
    for (size_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {  // workgroup-uniform
        const MsUnpackJob jb = u.jobs[j];
        // 1. the given nodes
        for (uint64_t q = tid; q < 5 * jb.n_copy; q += blockDim.x) {
            const uint64_t c = jb.copy_off + q / 5, w = q % 5;
            u.arena[5 * (size_t)u.copy_slot[c] + w] = u.path_in[5 * (size_t)u.copy_src[c] + w];
        }
        for (uint64_t q = tid; q < jb.n_leaf; q += blockDim.x) {
            const uint64_t l = jb.leaf_off + q;
            const uint32_t* words = u.rel_in + u.leaf_words[l];
            uint64_t run[5];
            ms_chunk_sponge(u.leaf_cnt[l], [&](uint64_t i) {
                const uint32_t bit = 12u * ((uint32_t)i + 1u), w = bit >> 5, off = bit & 31u;
                const uint32_t hi = words[w];
                if (off <= 20u) return (hi >> (20u - off)) & 0xFFFu;
                return ((hi << (off - 20u)) | (words[w + 1] >> (52u - off))) & 0xFFFu;
            }, run, t5.lut);
            uint64_t* dst = u.arena + 5 * (size_t)u.leaf_slot[l];
#pragma unroll
            for (int k = 0; k < 5; ++k) dst[k] = from_mont(run[k]);
        }
        __syncthreads();
        // 2. the parents, level by level
        for (uint64_t lvl = 0; lvl < jb.n_levels; ++lvl) {
            const uint64_t beg = u.lvl[jb.lvl_off + lvl], end = u.lvl[jb.lvl_off + lvl + 1];
            for (uint64_t o = beg + tid; o < end; o += blockDim.x) {
                const uint64_t* l = u.arena + 5 * (size_t)u.op[3 * o + 1];
                const uint64_t* r = u.arena + 5 * (size_t)u.op[3 * o + 2];
                uint64_t s[16];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    s[k] = to_mont(l[k]);
                    s[5 + k] = to_mont(r[k]);
                }
                tip5_hash_pair_digest(s, t5.lut);
                uint64_t* dst = u.arena + 5 * (size_t)u.op[3 * o];
#pragma unroll
                for (int k = 0; k < 5; ++k) dst[k] = from_mont(s[k]);
            }
            __syncthreads();
        }
        // 3. the unpacked paths
        for (uint64_t q = tid; q < 5 * jb.n_gath; q += blockDim.x) {
            const uint64_t g = jb.gath_off + q / 5, w = q % 5;
            u.path_out[5 * (size_t)g + w] = u.arena[5 * (size_t)u.gath_src[g] + w];
        }
    }
}

hipError_t launch_ms_unpack(const MsUnpackDev& u, size_t n_jobs, hipStream_t st) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_unpack, dim3((unsigned)(n_jobs > 65536 ? 65536 : n_jobs)), dim3(256), 0, st, u, n_jobs);
    return hipGetLastError();
}

}  // namespace nhip
