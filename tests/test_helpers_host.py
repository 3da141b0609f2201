"""CPU: the refusals of the small helpers of csrc/pea_k_direct.hip -- pea_scale_inplace, pea_scale_inplace_multi, pea_weighted_sum,
pea_stitch_add and pea_stitch_finalize -- that launch nothing, with fake pointers, in the order the entry points make their checks; and
the calls that have nothing to do (n == 0, all counts 0, voxels == 0), which return PEA_OK without touching a pointer.
tests/test_gpu_helpers.py holds the kernels behind them to their references."""
import ctypes

import pytest

OK, E_NULL, E_DESC, E_ALIGN = 0, -1, -2, -5
F32, F16, BF16 = 0, 1, 2
P = ctypes.c_void_p
N = ctypes.c_size_t


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def p(a):
    return P(a) if a else None


# ---- pea_scale_inplace ----------------------------------------------------------------------------------------------------------------------
def test_scale_inplace(lib):
    scale = lambda buf, dtype=F32, n=8, sc=4096: lib.pea_scale_inplace(p(buf), dtype, N(n), p(sc), None)
    assert scale(0) == E_NULL and scale(1024, sc=0) == E_NULL
    assert scale(0, dtype=3) == E_NULL  # the pointers are judged first
    for dtype in (-1, 3, 7):
        assert scale(1024, dtype=dtype) == E_DESC and scale(1025, dtype=dtype) == E_DESC  # ... then the dtype, then the alignment
    for off in range(1, 16):  # an f32 buffer goes in quads: 16 bytes
        assert scale(1024 + off, F32) == E_ALIGN and scale(1024 + off, F32, n=0) == E_ALIGN
    for dtype in (F16, BF16):  # the 16-bit buffers: their element
        for off in (1, 3, 15):
            assert scale(1024 + off, dtype) == E_ALIGN
        for off in (2, 4, 6, 14):
            assert scale(1024 + off, dtype, n=0) == OK
    for off in (1, 2, 3):
        assert scale(1024, sc=4096 + off) == E_ALIGN and scale(1024, F16, sc=4096 + off) == E_ALIGN
    for dtype in (F32, F16, BF16):
        assert scale(1024, dtype, n=0) == OK  # nothing to do: no launch


# ---- pea_scale_inplace_multi ------------------------------------------------------------------------------------------------------------------
def multi(lib, bufs, counts, dtype=F32, sc=4096, nbuf=None, null_bufs=False, null_counts=False):
    b = (P * max(1, len(bufs)))(*[p(a) for a in bufs])
    c = (N * max(1, len(counts)))(*counts)
    return lib.pea_scale_inplace_multi(None if null_bufs else b, None if null_counts else c, len(bufs) if nbuf is None else nbuf, dtype, p(sc), None)


def test_scale_inplace_multi(lib):
    assert multi(lib, [1024], [0], null_bufs=True) == E_NULL and multi(lib, [1024], [0], null_counts=True) == E_NULL
    assert multi(lib, [1024], [0], sc=0) == E_NULL
    assert multi(lib, [1024], [0], nbuf=0) == E_DESC and multi(lib, [1024] * 9, [0] * 9) == E_DESC and multi(lib, [1024], [0], nbuf=-1) == E_DESC
    assert multi(lib, [1024] * 8, [0] * 8) == OK
    for dtype in (-1, 3):
        assert multi(lib, [1024], [0], dtype=dtype) == E_DESC
    for k in range(3):  # a NULL inside bufs, whatever its count
        bufs = [1024, 2048, 4096]
        bufs[k] = 0
        assert multi(lib, bufs, [0, 0, 0]) == E_NULL and multi(lib, bufs, [4, 4, 4], dtype=BF16) == E_NULL
    # alignment: the element size, for every buffer -- the f32 form takes an element-aligned buffer (its scalar route)
    for off in (1, 2, 3):
        assert multi(lib, [1024, 2048 + off], [0, 0], F32) == E_ALIGN and multi(lib, [1024 + off, 2048], [0, 0], F32) == E_ALIGN
    for off in (4, 8, 12):
        assert multi(lib, [1024, 2048 + off], [0, 0], F32) == OK
    for dtype in (F16, BF16):
        for off in (1, 3):
            assert multi(lib, [1024, 2048 + off], [0, 0], dtype) == E_ALIGN
        for off in (2, 6, 10):
            assert multi(lib, [1024 + off, 2048], [0, 0], dtype) == OK
    for off in (1, 2, 3):
        assert multi(lib, [1024], [0], sc=4096 + off) == E_ALIGN
    # the buffers are judged in order: the first fault answers
    assert multi(lib, [1025, 0], [0, 0]) == E_ALIGN and multi(lib, [0, 1025], [0, 0]) == E_NULL
    for nbuf in (1, 3, 8):  # all counts 0: nothing to do, no launch
        for dtype in (F32, F16, BF16):
            assert multi(lib, [1024 * (i + 1) for i in range(nbuf)], [0] * nbuf, dtype) == OK


# ---- pea_weighted_sum --------------------------------------------------------------------------------------------------------------------------
def test_weighted_sum(lib):
    ws = lambda rows=1024, stride=1, w=2048, n=4, out=4096: lib.pea_weighted_sum(p(rows), stride, p(w), n, p(out), None)
    assert ws(rows=0) == E_NULL and ws(w=0) == E_NULL and ws(out=0) == E_NULL
    assert ws(rows=0, n=0) == E_NULL  # the pointers first
    for n in (0, -1, 65, 1 << 20):
        assert ws(n=n) == E_DESC
    for stride in (0, -1, -11):
        assert ws(stride=stride) == E_DESC and ws(stride=stride, n=1) == E_DESC
    for off in (1, 2, 3):
        assert ws(rows=1024 + off) == E_ALIGN and ws(w=2048 + off) == E_ALIGN and ws(out=4096 + off) == E_ALIGN
        assert ws(rows=1024 + off, n=65) == E_DESC  # ... then the counts, then the alignment


# ---- pea_stitch_add / pea_stitch_finalize --------------------------------------------------------------------------------------------------
def test_stitch_add(lib):
    def add(out=1024, wmap=2048, vol=4096, wv=8192, C=3, vol_dims=(5, 9, 11), win=(2, 3, 5), at=(0, 0, 0)):
        return lib.pea_stitch_add(p(out), p(wmap), p(vol), p(wv), C, *vol_dims, *win, *at, None)

    for arg in ("out", "wmap", "vol", "wv"):
        assert add(**{arg: 0}) == E_NULL and add(**{arg: 0}, C=0) == E_NULL  # the pointers first
    assert add(C=0) == E_DESC and add(C=-1) == E_DESC
    # a window must have an extent and lie inside the volume
    for win in ((0, 3, 5), (2, 0, 5), (2, 3, 0), (-1, 3, 5)):
        assert add(win=win) == E_DESC
    for at in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert add(at=at) == E_DESC
    for at in ((4, 0, 0), (0, 7, 0), (0, 0, 7), (3, 6, 7), (5, 0, 0), (0, 9, 0), (0, 0, 11)):  # one voxel too far along an axis, or more
        assert add(at=at) == E_DESC
    for win in ((6, 9, 11), (5, 10, 11), (5, 9, 12)):
        assert add(win=win) == E_DESC
    for off in (1, 2, 3):
        for arg, base in (("out", 1024), ("wmap", 2048), ("vol", 4096), ("wv", 8192)):
            assert add(**{arg: base + off}) == E_ALIGN
        assert add(out=1024 + off, at=(4, 0, 0)) == E_DESC  # ... then the window, then the alignment


def test_stitch_finalize(lib):
    fin = lambda out=1024, wmap=2048, C=3, voxels=495: lib.pea_stitch_finalize(p(out), p(wmap), C, N(voxels), None)
    assert fin(out=0) == E_NULL and fin(wmap=0) == E_NULL and fin(out=0, C=0) == E_NULL
    assert fin(C=0) == E_DESC and fin(C=-2) == E_DESC
    for off in (1, 2, 3):
        assert fin(out=1024 + off) == E_ALIGN and fin(wmap=2048 + off) == E_ALIGN and fin(out=1024 + off, C=0) == E_DESC
    for C in (1, 3):
        assert fin(C=C, voxels=0) == OK  # nothing to do: no launch
