// Layout of one host-buffer call's device buffers inside the context workspace: buffers in
// declaration order, each rounded up to 256 bytes, a zero-byte buffer still one unit (a distinct
// non-null address).  Pure size_t arithmetic that reports overflow instead of wrapping.  Host only
// (no HIP), so that tests/native/stage_layout_check.cpp runs it under ASan + UBSan; the device half
// is Stage in ctx.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nhip {

static constexpr size_t STAGE_ALIGN = 256;
static constexpr unsigned STAGE_MAX_BUFS = 64;  // nhip_ms_update_batch declares 58

struct StageLayout {
    size_t off[STAGE_MAX_BUFS], bytes[STAGE_MAX_BUFS];
    size_t total = 0;
    unsigned n = 0;
    bool overflow = false;  // a size or the total left size_t, or more than STAGE_MAX_BUFS buffers

    // The next buffer: count * per elements of elem_bytes each.  Returns its slot (0 after an overflow).
    unsigned add(size_t count, size_t per, size_t elem_bytes) {
        size_t b = 0;
        if (n == STAGE_MAX_BUFS || __builtin_mul_overflow(count, per, &b) || __builtin_mul_overflow(b, elem_bytes, &b) ||
            b > SIZE_MAX - (STAGE_ALIGN - 1)) {
            overflow = true;
            return 0;
        }
        const size_t unit = ((b ? b : 1) + (STAGE_ALIGN - 1)) & ~(STAGE_ALIGN - 1);
        off[n] = total;
        bytes[n] = b;
        if (__builtin_add_overflow(total, unit, &total)) overflow = true;
        return n++;
    }
};

}  // namespace nhip
