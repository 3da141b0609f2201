"""CPU: the fused 3D window inference (include/pea_infer.h: pea_infer_stitch_supported, pea_affinity_infer_stitch) -- the header and
the library agree on the two new symbols, every return code of the call is reached before anything is launched (dummy device
pointers, no GPU), the support query answers as documented, and VolumeStitcher.add_embedding refuses a CPU tensor."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NORM5 = [1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27]
OK, E_NULL, E_DESC, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -5
CIRCULAR, CROP_ZERO = 0, 1
FLAG_HALF_SHIFT, FLAG_CLAMP01, FLAG_LOSS_ACT = 4, 8, 64


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "pea_infer.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _desc(pkg, shifts=NORM5, D=16, dims=(18, 160, 160), dtype=0, border=CROP_ZERO, **kw):
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 3, 1, D, len(shifts)
    d.dims[:] = list(dims)
    d.border, d.dtype, d.norm, d.eps = border, dtype, 1, 1e-12
    for i, s in enumerate(shifts):
        o = [0, 0, 0]
        o[i % 3] = -s
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_header_declares_exactly_the_two_entry_points():
    assert declared_symbols() == ["pea_affinity_infer_stitch", "pea_infer_stitch_supported"]
    src = open(os.path.join(ROOT, "include", "pea_infer.h")).read()
    assert '#include "pea.h"' in src


def test_library_exports_both_and_the_tuple_matches_the_header(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in declared_symbols():
        assert hasattr(raw, name), name
    assert sorted(pkg._lib.EXPORTS_INFER) == declared_symbols()
    assert not set(pkg._lib.EXPORTS_INFER) & set(pkg._lib.EXPORTS)
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2


def _call(lib, d, e=0x10000, fill=1, wv=0x20000, out=0x30000, wm=0x40000, vol=(38, 320, 320), pos=(10, 80, 80)):
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    return lib.pea_affinity_infer_stitch(ctypes.byref(d), vp(e), fill, vp(wv), vp(out), vp(wm), vol[0], vol[1], vol[2], pos[0], pos[1],
                                         pos[2], None)


def test_every_error_code_is_returned_before_a_launch(pkg, lib):
    """host-only: the pointers are dummies, so anything but an early return would fault"""
    good = lambda **kw: _desc(pkg, **kw)
    # PEA_E_DESC: an invalid descriptor (pea_desc_validate), B != 1, a window that leaves the volume, a negative fill_shift,
    # 2 * fill_shift above a window dimension
    assert _call(lib, good(abi=7)) == E_DESC
    assert _call(lib, good(K=0)) == E_DESC
    assert _call(lib, good(B=2)) == E_DESC
    for pos in ((21, 80, 80), (10, 161, 80), (10, 80, 161), (-1, 80, 80), (10, -1, 80), (10, 80, -1)):
        assert _call(lib, good(), pos=pos) == E_DESC, pos
    assert _call(lib, good(), vol=(17, 320, 320), pos=(0, 0, 0)) == E_DESC
    assert _call(lib, good(), fill=-1) == E_DESC
    assert _call(lib, good(shifts=[1, 1, 1], dims=(1, 160, 160)), fill=1) == E_DESC
    assert _call(lib, good(shifts=[1, 1, 1], dims=(4, 160, 3)), fill=2) == E_DESC
    # PEA_E_NULL: each required pointer
    for kw in (dict(e=None), dict(wv=None), dict(out=None), dict(wm=None)):
        assert _call(lib, good(), **kw) == E_NULL, kw
    assert lib.pea_affinity_infer_stitch(None, None, 1, None, None, None, 1, 1, 1, 0, 0, 0, None) == E_NULL
    # PEA_E_ALIGN: a pointer that is not aligned to its element size
    assert _call(lib, good(), e=0x10002) == E_ALIGN
    assert _call(lib, good(dtype=1), e=0x10001) == E_ALIGN
    assert _call(lib, good(dtype=1), e=0x10002, fill=2) == E_UNSUPPORTED   # (2-byte aligned is enough for 16-bit storage)
    for kw in (dict(wv=0x20002), dict(out=0x30001), dict(wm=0x40002)):
        assert _call(lib, good(), **kw) == E_ALIGN, kw
    # PEA_E_UNSUPPORTED: wherever pea_infer_stitch_supported is 0
    assert _call(lib, good(border=CIRCULAR)) == E_UNSUPPORTED
    assert _call(lib, good(D=5)) == E_UNSUPPORTED
    assert _call(lib, good(), fill=2) == E_UNSUPPORTED
    assert _call(lib, good(flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT | FLAG_CLAMP01)) == E_UNSUPPORTED
    # the order of the table: descriptor errors before pointer errors before "unsupported"
    assert _call(lib, good(B=2, border=CIRCULAR), e=None) == E_DESC
    assert _call(lib, good(border=CIRCULAR), e=None) == E_NULL
    assert _call(lib, good(D=5), e=0x10002) == E_ALIGN


def test_supported_query(pkg, lib):
    q = lambda d, fill: lib.pea_infer_stitch_supported(ctypes.byref(d), fill)
    for shifts in (NORM5, [1, 1, 1]):
        for D in (16, 32):
            for dtype in (0, 1, 2):
                for fill in (0, 1):
                    assert q(_desc(pkg, shifts=shifts, D=D, dtype=dtype), fill) == 1, (shifts, D, dtype, fill)
    assert q(_desc(pkg, border=CIRCULAR), 1) == 0
    assert q(_desc(pkg, D=5), 1) == 0
    assert q(_desc(pkg), 2) == 0
    assert q(_desc(pkg, flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT | FLAG_CLAMP01), 1) == 0
    assert q(_desc(pkg, abi=7), 1) == 0       # an invalid descriptor
    assert lib.pea_infer_stitch_supported(None, 1) == 0


def test_add_embedding_raises_on_a_cpu_tensor(pkg):
    st = pkg.VolumeStitcher.__new__(pkg.VolumeStitcher)  # (the constructor itself wants a GPU; the check comes before any use of it)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.add_embedding(torch.zeros(1, 16, 4, 8, 8), (0, 0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.add_embedding(torch.zeros(1, 16, 4, 8, 8), (0, 0, 0), fused=False)
    with pytest.raises(RuntimeError):
        pkg.VolumeStitcher(12, (8, 16, 16), (4, 8, 8), "cpu")
