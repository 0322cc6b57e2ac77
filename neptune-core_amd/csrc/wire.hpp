// Host side of the in-place feed path: how the proof spans of a wire buffer are laid
// into a device raw buffer for k_wire_words (wire_kernels.hip).  Shared by nhip_le_words_gpu (capi.hip)
// and the wire source of the batch fill step (stark_host.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/neptune_hip.h"
#include "kernels.hpp"

namespace nhip {

// Spans whose gap is at most this many bytes are uploaded as one run, gap included.  Between two proofs
// of a ProofCollection the gap is a length prefix, between two transactions a kernel (a few KB).  64 KB
// of link time (~1.2 us at ~54 GB/s) is well under the several microseconds one more copy call costs.
// (Arithmetic from those two figures, not a measurement.)
static constexpr uint64_t WIRE_RUN_GAP = 64 * 1024;

struct WireRun {
    uint64_t start, end;  // host bytes [start, end) of the wire buffer
    uint64_t pos;         // byte position in the device raw buffer
};
struct WirePlan {
    std::vector<WireRun> runs;
    std::vector<uint64_t> boff;  // per span: its first byte in the device raw buffer
    size_t raw_bytes = 0;        // device raw buffer size, tail padding included
};

inline bool wire_spans_ok(const nhip_span* spans, size_t n, size_t n_bytes) {
    for (size_t i = 0; i < n; ++i)
        if (spans[i].offset > n_bytes || spans[i].len > (n_bytes - spans[i].offset) / 8) return false;
    return true;
}

// Runs: the spans sorted by offset, neighbours merged while the gap is at most WIRE_RUN_GAP (spans may
// overlap or repeat: they fall into one run).  The runs lie back to back in the device buffer, each at
// a position congruent to its host address mod 64 (the buffer's base is 256-byte aligned), each followed
// by WIRE_TAIL_PAD bytes.  Zero-length spans are in no run.
inline void wire_plan(const uint8_t* bytes, const nhip_span* spans, size_t n, WirePlan& p) {
    p.runs.clear();
    p.boff.assign(n, 0);
    std::vector<size_t> order;
    order.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (spans[i].len) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return spans[a].offset < spans[b].offset; });
    for (size_t i : order) {
        const uint64_t s = spans[i].offset, e = s + 8 * spans[i].len;
        if (!p.runs.empty() && s <= p.runs.back().end + WIRE_RUN_GAP) p.runs.back().end = std::max(p.runs.back().end, e);
        else p.runs.push_back(WireRun{s, e, 0});
    }
    uint64_t cur = 0;
    for (WireRun& r : p.runs) {
        r.pos = ((cur + 63) & ~(uint64_t)63) + ((uintptr_t)(bytes + r.start) & 63u);
        cur = r.pos + (r.end - r.start) + WIRE_TAIL_PAD;
    }
    p.raw_bytes = (size_t)cur + WIRE_TAIL_PAD;
    for (size_t i : order) {
        auto it = std::upper_bound(p.runs.begin(), p.runs.end(), spans[i].offset,
                                   [](uint64_t o, const WireRun& r) { return o < r.start; });
        const WireRun& r = *(it - 1);
        p.boff[i] = r.pos + (spans[i].offset - r.start);
    }
}

// Upload the runs to d_raw on `st`.  is_pinned(ptr, bytes): the range is pinned host memory, DMA'd
// as it lies; any other run is copied byte for byte into `stage` (host memory of raw_bytes, laid out as
// the device buffer) and DMA'd from there.
template <class IsPinned>
inline hipError_t wire_upload(const WirePlan& p, const uint8_t* bytes, uint8_t* d_raw, uint8_t* stage, IsPinned is_pinned,
                              hipStream_t st) {
    for (const WireRun& r : p.runs) {
        const size_t len = (size_t)(r.end - r.start);
        const uint8_t* src = bytes + r.start;
        if (!is_pinned(src, len)) {
            if (!stage) return hipErrorInvalidValue;
            std::memcpy(stage + r.pos, src, len);
            src = stage + r.pos;
        }
        const hipError_t e = hipMemcpyAsync(d_raw + r.pos, src, len, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace nhip
