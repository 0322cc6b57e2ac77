"""k_wire_words through its public seam nhip_le_words_gpu: the words of byte spans at any
byte shift, gathered and reduced mod p on the GPU, against the host nhip_le_words (the reference; the
comparison is bit-exact).

Shapes, the smallest at which the kernel can go wrong: a ~20 KB buffer of random bytes with the words 0,
p - 1, p, p + 5 and 2^64 - 1 forced into spans of every shift; spans starting at every byte offset 0..15
of a 16-byte line, of 0, 1, 2, 3, 31, 32, 33, 255, 256, 257 and 1025 words (below, at and past a wave, a
workgroup and a workgroup's tile; 32k words in all, so many workgroups and tiles that straddle spans,
zero-length spans included); a span at byte 0; a span whose last byte is the buffer's last byte;
overlapping spans, a repeated span, n == 0.  Each once from nhip_host_alloc memory (DMA'd as it lies) and
once from ordinary numpy memory (through the staging), with the buffer's start shifted by 0, 1 and 7
bytes inside its allocation so that the host address alignment differs from the span alignment."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = (1 << 64) - (1 << 32) + 1
N_BYTES = 20483
LENS = (0, 1, 2, 3, 31, 32, 33, 255, 256, 257, 1025)
SPECIAL = (0, P - 1, P, P + 5, (1 << 64) - 1)


def _case():
    rng = np.random.default_rng(2400)
    data = rng.integers(0, 256, size=N_BYTES, dtype=np.uint8)
    spans, k = [], 0
    for shift in range(16):
        for n in LENS:
            lines = (N_BYTES - 8 * n - 16) // 16
            spans.append((16 * ((k * 37 + 5) % lines) + shift, n))
            k += 1
    spans.append((0, 33))                     # starts at byte 0
    spans.append((N_BYTES - 8 * 33, 33))      # its last byte is the buffer's last byte (shift 3 of a line)
    spans.append((N_BYTES - 8 * 1025, 1025))  # the same for the longest span
    spans.append((1001, 300))                 # two overlapping spans ...
    spans.append((1001 + 8 * 100 + 3, 300))   # ... at different shifts
    spans.append(spans[40])                   # a repeated span
    spans.append(spans[7])
    spans.append((N_BYTES, 0))                # zero-length at the very end
    # the special words inside spans of every shift (written where a span's words 3.. lie)
    for shift in range(16):
        off, n = spans[shift * len(LENS) + LENS.index(31) + (shift % 3)]  # the 31-, 32- or 33-word span
        for j, v in enumerate(SPECIAL):
            data[off + 8 * (3 + j):off + 8 * (4 + j)] = np.frombuffer(int(v).to_bytes(8, "little"), dtype=np.uint8)
    return data, spans


@pytest.fixture(scope="module")
def case():
    from neptune_hip import _lib
    lib = _lib.load()
    data, spans = _case()
    want = []
    for off, n in spans:  # the reference: the host decode, span by span
        out = np.zeros(max(n, 1), dtype=np.uint64)
        assert lib.nhip_le_words(data.ctypes.data, data.size, off, n, out.ctypes.data) == _lib.NHIP_OK
        want.append(out[:n])
    want = np.concatenate(want)
    want.setflags(write=False)
    for v in SPECIAL:  # the forced words are in the reference, reduced
        assert (want == np.uint64(int(v) % P)).sum() >= 16
    return data, spans, want


class _Pinned:
    def __init__(self, lib, nbytes):
        self.lib = lib
        h = ctypes.c_void_p()
        assert lib.nhip_host_alloc(nbytes, ctypes.byref(h)) == 0
        self.ptr = h.value
        self.array = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(self.ptr), dtype=np.uint8)

    def close(self):
        self.array = None
        assert self.lib.nhip_host_free(self.ptr) == 0


@pytest.mark.parametrize("pinned", [True, False], ids=["host_alloc", "numpy"])
@pytest.mark.parametrize("lead", [0, 1, 7])
def test_le_words_gpu_is_bit_exact_with_the_host_decode(ctx, case, pinned, lead):
    import neptune_hip.stark as NS
    data, spans, want = case
    mem = _Pinned(ctx.lib, N_BYTES + 8) if pinned else None
    try:
        backing = mem.array if pinned else np.zeros(N_BYTES + 8, dtype=np.uint8)
        view = backing[lead:lead + N_BYTES]  # the buffer starts `lead` bytes into its allocation
        view[:] = data
        got = NS.le_words_gpu(ctx, view, spans)
        assert got.dtype == np.uint64 and got.shape == want.shape
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        # a second call on the same context (its workspace and staging are reused)
        sub = spans[5:9]
        lo = sum(n for _, n in spans[:5])
        assert (NS.le_words_gpu(ctx, view, sub) == want[lo:lo + sum(n for _, n in sub)]).all()
    finally:
        if mem:
            mem.close()


def test_le_words_gpu_empty_and_out_of_range(ctx, case):
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    data, spans, want = case
    assert NS.le_words_gpu(ctx, data, []).size == 0                   # n == 0
    assert NS.le_words_gpu(ctx, data, [(5, 0), (N_BYTES, 0)]).size == 0  # only zero-length spans
    assert NS.le_words_gpu(ctx, b"", []).size == 0
    for off, n in ((N_BYTES + 1, 0), (N_BYTES - 7, 1), (0, N_BYTES // 8 + 1), (8, (1 << 61))):
        with pytest.raises(_lib.NhipError, match="invalid argument"):
            NS.le_words_gpu(ctx, data, [(0, 4), (off, n)])
