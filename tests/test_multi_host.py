"""CPU: the batched self losses (include/pea_multi.h: pea_multi_supported, pea_affinity_fwd_multi, pea_affinity_bwd_multi) -- the
header and the library agree on the three new symbols and include/pea.h keeps its own, the support query answers as the header
documents, every return code of the two calls is reached before anything is launched (dummy device pointers, no GPU), and the five
section functions take batched=False."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
CIRCULAR, CROP_ZERO, REPLICATE = 0, 1, 2
F32, F16, BF16 = 0, 1, 2
FLAG_HALF_SHIFT, FLAG_CLAMP01, FLAG_MASK_F32, FLAG_LOSS_ACT = 4, 8, 32, 64
CROSS = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-5, 0], [0, -5], [-9, 0], [0, -9], [-27, 0], [0, -27]]  # multi_offset([1, 3, 5, 9, 27], 4)


def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def desc2d(pkg, H=136, W=136, offsets=CROSS[:8], B=2, D=16, **kw):
    """a deep-supervision scale of the CVPPP loop: embedding_loss on [B, D, H, W] with offsets[:k]"""
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, B, D, len(offsets)
    d.dims[:] = [1, H, W]
    d.border, d.dtype, d.norm, d.eps = CIRCULAR, F32, 0, 1e-12
    for i, o in enumerate(offsets):
        d.offsets[i][:] = [0] + list(o)
        d.lam[i] = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def desc3d(pkg, dims=(4, 16, 24), shift=1, B=2, D=16, **kw):
    """a deep-supervision head of the AC3/AC4 loop: embedding_loss_norm1"""
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 3, B, D, 3
    d.dims[:] = list(dims)
    d.border, d.dtype, d.norm, d.eps = CROP_ZERO, F32, 1, 1e-12
    for i in range(3):
        o = [0, 0, 0]
        o[i] = -shift
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def cvppp_deep(pkg, **kw):
    """the four CVPPP deep-scale descriptors: 272^2 .. 34^2 with offsets[:8], [:6], [:4], [:2]"""
    return [desc2d(pkg, 272 >> j, 272 >> j, CROSS[:2 * (4 - j)], **kw) for j in range(4)]


def norm1_deep(pkg):
    return [desc3d(pkg, dims) for dims in ((18, 80, 80), (18, 40, 40), (18, 20, 20), (18, 10, 10))]


def supported(pkg, lib, descs, n=None):
    n = len(descs) if n is None else n
    arr = (ctypes.POINTER(pkg._lib.PeaDesc) * max(len(descs), 1))(*[ctypes.pointer(d) for d in descs])
    return lib.pea_multi_supported(arr, n)


def test_header_declares_exactly_the_three_entry_points(pkg):
    assert declared_symbols("pea_multi.h") == sorted(pkg._lib.EXPORTS_MULTI) == ["pea_affinity_bwd_multi", "pea_affinity_fwd_multi",
                                                                                 "pea_multi_supported"]
    src = open(os.path.join(ROOT, "include", "pea_multi.h")).read()
    assert '#include "pea.h"' in src
    assert re.search(r"#define\s+PEA_MULTI_MAX_N\s+4\b", src) and re.search(r"#define\s+PEA_MULTI_MAX_K\s+12\b", src)
    assert (pkg._lib.PEA_MULTI_MAX_N, pkg._lib.PEA_MULTI_MAX_K) == (4, 12)


def test_library_exports_them_and_pea_h_is_unchanged(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in pkg._lib.EXPORTS_MULTI:
        assert hasattr(raw, name), name
    assert not set(pkg._lib.EXPORTS_MULTI) & (set(pkg._lib.EXPORTS) | set(pkg._lib.EXPORTS_INFER))
    assert declared_symbols("pea.h") == sorted(pkg._lib.EXPORTS)  # the symbol list of pea.h: as before
    assert not set(declared_symbols("pea.h")) & set(pkg._lib.EXPORTS_MULTI)
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2


def test_entry_structs_match_the_header(pkg):
    """eight / five pointers, in the header's order"""
    assert ctypes.sizeof(pkg._lib.PeaMultiFwd) == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(pkg._lib.PeaMultiBwd) == 5 * ctypes.sizeof(ctypes.c_void_p)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_multi.h")).read(), flags=re.S)
    for name, cls in (("PeaMultiFwd", pkg._lib.PeaMultiFwd), ("PeaMultiBwd", pkg._lib.PeaMultiBwd)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        assert re.findall(r"\*\s*(\w+)\s*;", body) == [f[0] for f in cls._fields_], name


def test_supported_query(pkg, lib):
    q = lambda descs, n=None: supported(pkg, lib, descs, n)
    assert q(cvppp_deep(pkg)) == 1
    assert q(cvppp_deep(pkg, B=8)) == 1
    assert q(cvppp_deep(pkg, flags=FLAG_MASK_F32)) == 1
    assert q(norm1_deep(pkg)) == 1
    assert q(cvppp_deep(pkg)[:1]) == 1 and q(cvppp_deep(pkg)[:2]) == 1
    assert q([desc2d(pkg, D=32), desc3d(pkg)]) == 1           # entries may differ in every field
    assert q([], 0) == 0                                      # n = 0
    assert q(cvppp_deep(pkg) + [desc2d(pkg)]) == 0            # n = 5
    assert lib.pea_multi_supported(None, 1) == 0
    k13 = CROSS + [[-2, 0], [0, -2], [-4, 0]]
    assert q([desc2d(pkg, offsets=k13[:12])]) == 1 and q([desc2d(pkg, offsets=k13)]) == 0   # K = 13
    base = cvppp_deep(pkg)[:3]
    assert q(base + [desc2d(pkg, dtype=BF16)]) == 0
    assert q(base + [desc2d(pkg, dtype=F16)]) == 0
    assert q(base + [desc2d(pkg, D=64)]) == 0
    assert q(base + [desc2d(pkg, D=8)]) == 0
    assert q(base + [desc2d(pkg, border=REPLICATE)]) == 0
    assert q(base + [desc2d(pkg, flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT | FLAG_CLAMP01)]) == 0
    assert q(base + [desc2d(pkg, flags=FLAG_HALF_SHIFT | FLAG_CLAMP01)]) == 1                # (an activation of the map alone is fine)
    assert q(base + [desc2d(pkg, H=27, W=40, offsets=CROSS)]) == 0                           # an offset as long as the image
    assert q(base + [desc2d(pkg, H=28, W=40, offsets=CROSS)]) == 1
    assert q(base + [desc2d(pkg, abi=7)]) == 0                                               # an entry that does not validate
    assert q([desc3d(pkg, (511, 512, 512))]) == 1 and q([desc3d(pkg, (512, 512, 512))]) == 0  # S * max(D, K) fits int32, or not


DUMMY = dict(e=0x10000, target=0x20000, weight=0x30000, mask=None, affs=None, g_out=0x40000, loss_out=0x50000)


def fwd(pkg, lib, descs, over=None, n=None, ws=0x100000, ws_bytes=None):
    """pea_affinity_fwd_multi on dummy pointers; over: {entry index: {field: value}}"""
    tab = (pkg._lib.PeaMultiFwd * max(len(descs), 1))()
    for j, d in enumerate(descs):
        args = dict(DUMMY, desc=ctypes.pointer(d) if d is not None else None)
        args.update((over or {}).get(j, {}))
        for k, v in args.items():
            setattr(tab[j], k, v)
    n = len(descs) if n is None else n
    state = lib.pea_workspace_bytes(ctypes.byref(desc2d(pkg)))
    return lib.pea_affinity_fwd_multi(tab, n, ctypes.c_void_p(ws) if ws else None, n * state if ws_bytes is None else ws_bytes, None)


def bwd(pkg, lib, descs, over=None, n=None):
    tab = (pkg._lib.PeaMultiBwd * max(len(descs), 1))()
    for j, d in enumerate(descs):
        args = dict(desc=ctypes.pointer(d) if d is not None else None, e=0x10000, g=0x20000, dloss=None, de=0x30000)
        args.update((over or {}).get(j, {}))
        for k, v in args.items():
            setattr(tab[j], k, v)
    return lib.pea_affinity_bwd_multi(tab, len(descs) if n is None else n, None)


def test_forward_error_codes_are_returned_before_a_launch(pkg, lib):
    """host-only: the pointers are dummies, so anything but an early return would fault"""
    four = cvppp_deep(pkg)
    state = lib.pea_workspace_bytes(ctypes.byref(four[0]))
    # PEA_E_DESC: n out of range, an entry whose descriptor does not validate
    assert fwd(pkg, lib, four, n=0) == E_DESC
    assert fwd(pkg, lib, four + [desc2d(pkg)], n=5) == E_DESC
    assert fwd(pkg, lib, four[:3] + [desc2d(pkg, abi=7)]) == E_DESC
    assert fwd(pkg, lib, four[:3] + [desc2d(pkg, H=27, W=40, offsets=CROSS)]) == E_DESC
    # PEA_E_NULL: the table, a descriptor, each required pointer of any entry (g_out is required here)
    assert lib.pea_affinity_fwd_multi(None, 4, ctypes.c_void_p(0x100000), 4 * state, None) == E_NULL
    assert fwd(pkg, lib, four[:2] + [None]) == E_NULL
    for field in ("e", "target", "weight", "g_out", "loss_out"):
        for j in (0, 3):
            assert fwd(pkg, lib, four, {j: {field: None}}) == E_NULL, (field, j)
    # PEA_E_ALIGN
    for field in ("e", "target", "weight", "affs", "g_out", "loss_out"):
        assert fwd(pkg, lib, four, {2: {field: 0x60002}}) == E_ALIGN, field
    assert fwd(pkg, lib, four, ws=0x100004) == E_ALIGN
    # PEA_E_WORKSPACE: missing, or shorter than n states
    assert fwd(pkg, lib, four, ws=None) == E_WORKSPACE
    assert fwd(pkg, lib, four, ws_bytes=4 * state - 1) == E_WORKSPACE
    assert fwd(pkg, lib, four, ws_bytes=state) == E_WORKSPACE
    # PEA_E_UNSUPPORTED: wherever pea_multi_supported is 0 for a table of valid descriptors
    for bad in (dict(dtype=BF16), dict(D=64), dict(border=REPLICATE), dict(flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT)):
        assert fwd(pkg, lib, four[:3] + [desc2d(pkg, **bad)]) == E_UNSUPPORTED, bad
    assert fwd(pkg, lib, [desc2d(pkg, offsets=CROSS + [[-2, 0], [0, -2], [-4, 0]])]) == E_UNSUPPORTED
    # the order: descriptor errors before pointer errors before the workspace before "unsupported"
    assert fwd(pkg, lib, [desc2d(pkg, abi=7)], {0: {"e": None}}) == E_DESC
    assert fwd(pkg, lib, [desc2d(pkg, D=64)], {0: {"e": None}}) == E_NULL
    assert fwd(pkg, lib, [desc2d(pkg, D=64)], {0: {"g_out": 0x40002}}, ws=None) == E_ALIGN
    assert fwd(pkg, lib, [desc2d(pkg, D=64)], ws=None) == E_WORKSPACE


def test_backward_error_codes_are_returned_before_a_launch(pkg, lib):
    four = norm1_deep(pkg)
    assert bwd(pkg, lib, four, n=0) == E_DESC and bwd(pkg, lib, four + [desc3d(pkg)], n=5) == E_DESC
    assert bwd(pkg, lib, four[:3] + [desc3d(pkg, K=0)]) == E_DESC
    assert lib.pea_affinity_bwd_multi(None, 2, None) == E_NULL
    assert bwd(pkg, lib, [None]) == E_NULL
    for field in ("e", "g", "de"):
        assert bwd(pkg, lib, four, {1: {field: None}}) == E_NULL, field
    for field in ("e", "g", "dloss", "de"):
        assert bwd(pkg, lib, four, {3: {field: 0x70002}}) == E_ALIGN, field
    for bad in (dict(dtype=F16), dict(D=64), dict(border=REPLICATE)):
        assert bwd(pkg, lib, four[:3] + [desc3d(pkg, **bad)]) == E_UNSUPPORTED, bad
    assert bwd(pkg, lib, [desc3d(pkg, D=64)], {0: {"de": None}}) == E_NULL


def test_section_functions_take_batched_false(pkg):
    for name in ("cvppp_loss_section", "cvppp_loss_section_composed", "cvppp_validation_section", "ac3ac4_loss_section",
                 "ac3ac4_loss_section_composed"):
        p = inspect.signature(getattr(pkg, name)).parameters
        assert "batched" in p and p["batched"].default is False, name
    for name in ("embedding_loss_multi", "embedding_loss_norm1_multi", "MultiAffinityMSE"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    p = inspect.signature(pkg.embedding_loss_multi).parameters
    assert list(p)[:6] == ["embeddings", "targets", "weightmaps", "masks", "criterion", "offsets_list"] and p["need_affs"].default is False
    assert list(inspect.signature(pkg.embedding_loss_norm1_multi).parameters)[:6] == ["embeddings", "targets", "weightmaps", "criterion",
                                                                                      "affs0_weight", "shift"]
