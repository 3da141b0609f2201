"""CPU: connected components (include/pea_cc.h) -- the numpy restatement tests/cc_reference.py, which the GPU tests compare the kernels
with, is held to scipy.ndimage.label on every named case and on seeded random masks and to hand-written expectations that need no
library; the header and the library agree on the three new symbols, the ctypes mirror has the header's layout, pea_cc_validate and
pea_cc_workspace_bytes answer as the header says, every refusal of pea_cc_label is reached before anything is launched and in the
header's order (dummy device pointers, no GPU), and the Python entry points say what is wrong with a call before they look for a
device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from cc_reference import NEIGHBOURS, cases_2d, cases_3d, cases_ids, cc_reference, cc_reference_batch, random_mask
from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
U8, I32 = 0, 1
NEW = ["pea_cc_label", "pea_cc_validate", "pea_cc_workspace_bytes"]
SIZE_MAX = 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def first_occurrence_numbering(parts):
    """a partition given by any labelling (0 = background) renumbered 1 .. n in the order of each part's first pixel"""
    flat = parts.ravel()
    ids, first = np.unique(flat, return_index=True)
    order = [i for i in np.argsort(first) if ids[i] != 0]
    new = np.zeros(len(ids), np.int64)
    new[order] = np.arange(1, len(order) + 1)
    return new[np.searchsorted(ids, flat)].reshape(parts.shape).astype(np.int32)


def test_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    pairs = [(name, m) for name, m in cases_2d().items()] + [(name, m) for name, m in cases_3d().items()]
    pairs += [("seeded %d" % s, random_mask(400 + s, (0.2, 0.45, 0.59, 0.7)[s % 4], (17 + s, 23))) for s in range(12)]
    pairs += [("seeded 3d %d" % s, random_mask(500 + s, (0.15, 0.3, 0.5)[s % 3], (4, 9 + s, 11))) for s in range(6)]
    for name, m in pairs:
        for c in range(1, m.ndim + 1):
            ref, n = ndi.label(m, structure=ndi.generate_binary_structure(m.ndim, c))
            lab, (found, kept) = cc_reference(m, c)
            assert found == kept == n and np.array_equal(lab, ref), (name, c)
            # min_size: scipy's labels, sizes from bincount, threshold, renumbered in order
            sizes = np.bincount(ref.ravel())
            keep = sizes >= 5
            keep[0] = False
            want = np.where(keep, np.cumsum(keep), 0)[ref]
            lab5, (found5, kept5) = cc_reference(m, c, min_size=5)
            assert found5 == n and kept5 == int(keep.sum()) and np.array_equal(lab5, want), (name, c)
    # a multi-valued image: every value labelled on its own by scipy, the pieces numbered by their first pixel
    for name, m in cases_ids().items():
        for c in range(1, m.ndim + 1):
            parts, base = np.zeros(m.shape, np.int64), 0
            for v in np.unique(m):
                if v != 0:
                    ref, n = ndi.label(m == v, structure=ndi.generate_binary_structure(m.ndim, c))
                    parts += np.where(ref > 0, ref + base, 0)
                    base += n
            lab, (found, kept) = cc_reference(m, c)
            assert found == kept == base and np.array_equal(lab, first_occurrence_numbering(parts)), (name, c)


def test_hand_written_expectations():
    # a diagonal pair: two components in the 4-neighbourhood, one in the 8-neighbourhood
    d = np.array([[1, 0], [0, 1]], np.uint8)
    assert cc_reference(d, 1)[0].tolist() == [[1, 0], [0, 2]] and cc_reference(d, 1)[1] == (2, 2)
    assert cc_reference(d, 2)[0].tolist() == [[1, 0], [0, 1]] and cc_reference(d, 2)[1] == (1, 1)
    # a U whose first pixel is on the right arm, and a dot that comes after that pixel in raster order
    u = np.array([[0, 0, 0, 1],
                  [1, 0, 0, 1],
                  [1, 0, 0, 1],
                  [1, 1, 1, 1],
                  [0, 0, 0, 0],
                  [0, 1, 0, 0]], np.uint8)
    for c in (1, 2):
        lab, cnt = cc_reference(u, c)
        assert lab.tolist() == [[0, 0, 0, 1], [1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0], [0, 2, 0, 0]] and cnt == (2, 2)
    assert cc_reference(u, 1, min_size=2)[0][5, 1] == 0 and cc_reference(u, 1, min_size=2)[1] == (2, 1)
    assert cc_reference(u, 1, min_size=9)[1] == (2, 1) and cc_reference(u, 1, min_size=10)[1] == (2, 0)  # the U has nine pixels
    # a label image whose id 3 occurs in two separate places; adjacent different ids stay apart; a negative id is a value
    ids = np.array([[3, 3, 5, 0],
                    [0, 5, 5, -2],
                    [3, 0, -2, -2],
                    [3, 3, 0, 3]], np.int32)
    lab, cnt = cc_reference(ids, 1)
    assert lab.tolist() == [[1, 1, 2, 0], [0, 2, 2, 3], [4, 0, 3, 3], [4, 4, 0, 5]] and cnt == (5, 5)
    lab, cnt = cc_reference(ids, 2)  # the 8-neighbourhood joins nothing more: (3, 3) touches (2, 2) = -2 only
    assert lab.tolist() == [[1, 1, 2, 0], [0, 2, 2, 3], [4, 0, 3, 3], [4, 4, 0, 5]] and cnt == (5, 5)
    # dropping the middle component renumbers the later ones
    lab, cnt = cc_reference(ids, 1, min_size=3)
    assert lab.tolist() == [[0, 0, 1, 0], [0, 1, 1, 2], [3, 0, 2, 2], [3, 3, 0, 0]] and cnt == (5, 3)
    # 3D: a step along an edge is joined at connectivity 2, a step along a corner at 3 only
    e = np.zeros((2, 2, 2), np.uint8)
    e[0, 0, 0] = e[1, 1, 0] = 1
    assert [cc_reference(e, c)[1][0] for c in (1, 2, 3)] == [2, 1, 1]
    k = np.zeros((2, 2, 2), np.uint8)
    k[0, 0, 0] = k[1, 1, 1] = 1
    assert [cc_reference(k, c)[1][0] for c in (1, 2, 3)] == [2, 2, 1]
    # the batch form restarts the ids per image
    lab, cnt = cc_reference_batch(np.stack([d, np.zeros_like(d), d[::-1].copy()]), 1)
    assert lab.tolist() == [[[1, 0], [0, 2]], [[0, 0], [0, 0]], [[0, 1], [2, 0]]] and cnt.tolist() == [[2, 2], [0, 0], [2, 2]]
    # the neighbour lists are skimage's connectivity: offsets with at most `connectivity` non-zero steps
    for (ndim, c), offs in NEIGHBOURS.items():
        assert all(len(o) == ndim and max(abs(v) for v in o) == 1 and sum(abs(v) for v in o) <= c for o in offs)
        assert len(offs) == sum(1 for o in np.ndindex(*(3,) * ndim) if 0 < sum(abs(v - 1) for v in o) <= c)


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_exactly_the_three_entry_points(pkg, lib):
    assert declared_symbols("pea_cc.h") == sorted(pkg._lib.EXPORTS_CC) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    src = open(os.path.join(ROOT, "include", "pea_cc.h")).read()
    assert '#include "pea.h"' in src
    assert re.search(r"#define\s+PEA_CC_IN_U8\s+0\b", src) and re.search(r"#define\s+PEA_CC_IN_I32\s+1\b", src)
    assert (pkg._lib.CC_IN_U8, pkg._lib.CC_IN_I32) == (U8, I32)
    for cite in ("scripts_bbbc039v1/utils/postprocessing.py:43-48", "utils/merge_small.py:106", "convert_mask2ins.py:33", "raster order"):
        assert cite in src, cite
    # pea.h and the ABI version are as they were
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert not set(NEW) & set(pkg._lib.EXPORTS)


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaCcDesc
    assert ctypes.sizeof(D) == 9 * 4
    names = ["ndim", "B", "dims", "in_type", "connectivity", "min_size", "flags"]
    assert [f[0] for f in D._fields_] == names
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_cc.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaCcDesc \{(.*?)\} PeaCcDesc;", src, flags=re.S).group(1)
    declared = [n.split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*u?int32_t", "", decl.strip()).replace(" ", "").split(",")]
    assert declared == names
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 20, 24, 28, 32]


# ---- return codes ------------------------------------------------------------------------------------------------------------------------
IN, LABELS, MASK, COUNTS, WORK = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000


def desc(pkg, ndim=2, B=2, dims=(1, 37, 53), in_type=U8, connectivity=1, min_size=0, flags=0):
    d = pkg._lib.PeaCcDesc()
    d.ndim, d.B, d.in_type, d.connectivity, d.min_size, d.flags = ndim, B, in_type, connectivity, min_size, flags
    d.dims[:] = dims
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def label(pkg, lib, d="default", inp=IN, labels=LABELS, mask=MASK, counts=COUNTS, work=WORK, wbytes=None, **kw):
    """pea_cc_label on dummy pointers: anything but an early return would fault"""
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = lib.pea_cc_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    return lib.pea_cc_label(None if d is None else ctypes.byref(d), vp(inp), vp(labels), vp(mask), vp(counts), vp(work), wbytes, None)


BIG_IMAGE = dict(ndim=3, B=1, dims=(2, 1 << 15, 1 << 15))                 # Z * Y * X = 2^31: one pixel too many
HUGE = dict(ndim=3, B=2 ** 31 - 1, dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))


def test_validate(pkg, lib):
    v = lambda **kw: lib.pea_cc_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_cc_validate(None) == E_NULL and label(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(connectivity=2, in_type=I32, min_size=25) == OK and v(B=1, dims=(1, 1, 1)) == OK
    for c in (1, 2, 3):
        assert v(ndim=3, dims=(5, 37, 70), connectivity=c) == OK
    assert v(min_size=2 ** 31 - 1) == OK and v(**HUGE) == OK and v(**BIG_IMAGE) == OK
    bad = [dict(ndim=1), dict(ndim=4), dict(ndim=0), dict(ndim=-2),
           dict(B=0), dict(B=-1), dict(dims=(1, 0, 53)), dict(dims=(1, 37, 0)), dict(dims=(1, -1, 53)), dict(ndim=3, dims=(0, 37, 53)),
           dict(dims=(2, 37, 53)), dict(dims=(0, 37, 53)),                    # ndim == 2 with dims[0] != 1
           dict(connectivity=0), dict(connectivity=3), dict(connectivity=-1), dict(ndim=3, dims=(2, 3, 4), connectivity=4),
           dict(min_size=-1), dict(min_size=-2 ** 31),
           dict(in_type=2), dict(in_type=-1),
           dict(flags=1), dict(flags=1 << 31)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert label(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_cc_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    assert lib.pea_cc_workspace_bytes(None) == 0


def test_workspace_bytes(pkg, lib):
    nb = lambda **kw: lib.pea_cc_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    # two int32 words per pixel and two per 1024 pixels of an image
    assert nb(B=1, dims=(1, 1, 1)) == 8 * (1 + 1)
    assert nb(B=1, dims=(1, 32, 32)) == 8 * (1024 + 1) and nb(B=1, dims=(1, 1, 1025)) == 8 * (1025 + 2)
    assert nb(B=3, dims=(1, 70, 150)) == 3 * 8 * (10500 + 11)
    assert nb(ndim=3, B=2, dims=(5, 37, 70)) == 2 * 8 * (12950 + 13)
    # the element type, the connectivity and min_size do not change it
    assert nb(in_type=I32, connectivity=2, min_size=7) == nb()
    assert nb(**BIG_IMAGE) == 8 * (2 ** 31 + 2 ** 21) and nb(**HUGE) == SIZE_MAX


def test_label_refusals_before_a_launch_and_their_order(pkg, lib):
    # PEA_E_NULL: in, counts, or both outputs
    assert label(pkg, lib, inp=0) == E_NULL and label(pkg, lib, counts=0) == E_NULL and label(pkg, lib, labels=0, mask=0) == E_NULL
    # PEA_E_ALIGN: int32 pointers to 4 bytes; a uint8 in and mask_out at any address
    for skew in (1, 2, 3):
        assert label(pkg, lib, labels=LABELS + skew) == E_ALIGN and label(pkg, lib, counts=COUNTS + skew) == E_ALIGN, skew
        assert label(pkg, lib, work=WORK + skew) == E_ALIGN and label(pkg, lib, inp=IN + skew, in_type=I32) == E_ALIGN, skew
        assert label(pkg, lib, inp=IN + skew, mask=MASK + skew, work=0) == E_WORKSPACE, skew
    # PEA_E_WORKSPACE: missing or short
    need = lib.pea_cc_workspace_bytes(ctypes.byref(desc(pkg)))
    assert need > 0 and need % 8 == 0
    assert label(pkg, lib, work=0) == E_WORKSPACE and label(pkg, lib, wbytes=need - 1) == E_WORKSPACE and label(pkg, lib, wbytes=0) == E_WORKSPACE
    # PEA_E_UNSUPPORTED: 2^31 pixels in an image; more workgroups than a grid holds
    assert label(pkg, lib, **BIG_IMAGE) == E_UNSUPPORTED and label(pkg, lib, wbytes=SIZE_MAX, **HUGE) == E_UNSUPPORTED
    assert label(pkg, lib, ndim=2, B=1 << 21, dims=(1, 1 << 15, 1)) == E_UNSUPPORTED   # 2^31 tiles (1024 ragged ones an image), 2^26 runs
    assert label(pkg, lib, ndim=2, B=1 << 11, dims=(1, 1 << 10, 1 << 20)) == E_UNSUPPORTED  # 2^30 pixels an image, 2^31 runs of 1024
    # with one output only the other may be NULL: the call gets as far as the grid
    assert label(pkg, lib, labels=0, **BIG_IMAGE) == E_UNSUPPORTED and label(pkg, lib, mask=0, **BIG_IMAGE) == E_UNSUPPORTED
    assert label(pkg, lib, inp=IN + 4, in_type=I32, labels=LABELS + 12, **BIG_IMAGE) == E_UNSUPPORTED  # element-aligned: accepted
    # the stated order: descriptor, NULL, alignment, workspace, size
    assert label(pkg, lib, work=0, **BIG_IMAGE) == E_WORKSPACE and label(pkg, lib, wbytes=8, **BIG_IMAGE) == E_WORKSPACE
    assert label(pkg, lib, work=0, labels=LABELS + 2, **BIG_IMAGE) == E_ALIGN and label(pkg, lib, wbytes=0, work=WORK + 2, **BIG_IMAGE) == E_ALIGN
    assert label(pkg, lib, inp=0, labels=LABELS + 2, work=0, **BIG_IMAGE) == E_NULL
    assert label(pkg, lib, inp=0, labels=0, mask=0, counts=0, work=0, flags=2) == E_DESC
    assert label(pkg, lib, inp=0, labels=LABELS + 1, work=0, wbytes=0, connectivity=3) == E_DESC


# ---- the Python entry points ---------------------------------------------------------------------------------------------------------------
def test_python_entry_points(pkg):
    """no CPU fallback; a wrong shape, dtype or range is said before the device is looked at"""
    for name in pkg.CC_EXPORTS:
        assert hasattr(pkg, name), name
    from importlib import import_module
    post = import_module(pkg.__name__ + ".utils.postprocessing")
    assert post.remove_samll_object is pkg.remove_samll_object and pkg.postprocessing is post
    sig = inspect.signature(pkg.remove_samll_object)
    assert list(sig.parameters) == ["mask", "min_size"] and sig.parameters["min_size"].default == 25
    sig = inspect.signature(pkg.connected_components)
    assert list(sig.parameters) == ["x", "connectivity", "min_size", "mask"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, 0, False]
    sig = inspect.signature(pkg.foreground_mask)
    assert list(sig.parameters) == ["logits", "crop", "min_size"] and sig.parameters["min_size"].default == 0
    assert "merge_func" in post.__doc__ and "sequential" in post.__doc__ and not hasattr(post, "merge_func")

    m = torch.zeros(2, 6, 7, dtype=torch.uint8)
    for call in (lambda: pkg.connected_components(m), lambda: pkg.connected_components(m.bool(), connectivity=1, min_size=3, mask=True),
                 lambda: pkg.connected_components(m.to(torch.int32)[:, None].expand(2, 3, 6, 7), connectivity=3),
                 lambda: pkg.remove_samll_object(m), lambda: pkg.remove_samll_object(m[0]), lambda: pkg.remove_small_components(m, 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.foreground_mask(torch.zeros(2, 2, 6, 6), min_size=25)
    for bad in (torch.zeros(6, 7, dtype=torch.uint8), torch.zeros(1, 2, 3, 6, 7, dtype=torch.uint8), torch.zeros(7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[B, H, W\] or \[B, Z, H, W\]"):
            pkg.connected_components(bad)
    with pytest.raises(ValueError, match="empty"):
        pkg.connected_components(torch.zeros(2, 0, 7, dtype=torch.uint8))
    for dt in (torch.int64, torch.float32, torch.int16, torch.int8):
        with pytest.raises(TypeError, match="bool, uint8 or int32"):
            pkg.connected_components(m.to(dt))
        with pytest.raises(TypeError, match="bool, uint8 or int32"):
            pkg.remove_samll_object(m.to(dt))
    for c in (0, 3, -1):
        with pytest.raises(ValueError, match="connectivity"):
            pkg.connected_components(m, connectivity=c)
    with pytest.raises(ValueError, match="connectivity"):
        pkg.connected_components(m[:, None], connectivity=4)
    for ms in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="min_size"):
            pkg.connected_components(m, min_size=ms)
        with pytest.raises(ValueError, match="min_size"):
            pkg.remove_samll_object(m, min_size=ms)
    with pytest.raises(ValueError, match="min_size"):
        pkg.foreground_mask(torch.zeros(2, 2, 6, 6), min_size=-1)
    with pytest.raises(TypeError):
        pkg.connected_components(np.zeros((2, 6, 7), np.uint8))
    with pytest.raises(TypeError, match="bool or integers"):
        pkg.remove_samll_object(np.zeros((6, 7), np.float32))
    with pytest.raises(TypeError):
        pkg.remove_samll_object([[0, 1], [1, 0]])
