"""CPU: the small-segment merges (include/pea_merge.h) -- the two restatements of tests/merge_reference.py, which the GPU tests compare
the kernels with, agree with the fixtures made with the reference's own functions and with each other on 200 random images, ties
included.  The header and the library agree on the three new symbols, the ctypes mirror has the header's layout, every refusal of
pea_merge_validate and pea_merge_small is reached before anything is launched and in the header's order (dummy device pointers, no GPU),
pea_merge_workspace_bytes is monotone, and the Python entry points say what is wrong with a call before they look for a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import merge_reference as R
from conftest import GOLDEN, ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
RELABEL = 1
NEW = ["pea_merge_small", "pea_merge_validate", "pea_merge_workspace_bytes"]
SIZE_MAX = 2 ** 64 - 1
SETTINGS = (R.CVPPP_MERGE_PASSES, R.BBBC_MERGE_PASSES)


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def test_restatements_against_the_reference_chains():
    g = np.load(os.path.join(GOLDEN, "gmerge_chains.npz"))
    assert int(g["n"]) >= 6 and g["tie_free"].all() and {int(g["kind_%d" % k]) for k in range(int(g["n"]))} == {0, 1}
    for k in range(int(g["n"])):
        seg, passes = g["seg_%d" % k], SETTINGS[int(g["kind_%d" % k])]
        assert 21 <= min(seg.shape) and max(seg.shape) <= 69 and R.tie_free(seg, passes)
        a = R.aliased_passes(seg, passes)
        assert np.array_equal(R.chain(seg, passes), g["out_%d" % k]) and np.array_equal(a.labels, g["out_%d" % k]), k
        assert np.array_equal(R.chain(seg, passes, "desc"), g["out_%d" % k]), k
        lab, n = R.relabel(a.labels)
        assert np.array_equal(lab, g["relabel_%d" % k]) and n == lab.max(), k
        assert a.stat("merges") > 0 and a.stat("out_of_range") == 0


def test_restatements_against_the_reference_passes():
    g = np.load(os.path.join(GOLDEN, "gmerge_passes.npz"))
    assert int(g["n"]) >= 12 and g["tie_free"].all()
    seen = set()
    for k in range(int(g["n"])):
        seg, (t, w) = g["seg_%d" % k], (int(v) for v in g["pass_%d" % k])
        seen.add((t, w))
        assert np.array_equal(R.literal(seg, t, w), g["out_%d" % k]) and np.array_equal(R.aliased(seg, t, w), g["out_%d" % k]), k
        assert np.array_equal(R.literal(seg, t, w, "desc"), g["out_%d" % k]), k
        assert np.array_equal(R.relabel(g["out_%d" % k])[0], g["relabel_%d" % k]), k
    assert seen == set(R.CVPPP_MERGE_PASSES) | set(R.BBBC_MERGE_PASSES)


def test_the_two_restatements_agree_on_200_random_images_ties_included():
    rng = np.random.default_rng(20261021)
    tied = 0
    for k in range(200):
        seg = R.random_image(rng, 21, 45)
        passes = SETTINGS[k % 2]
        for ties in ("asc", "desc"):
            assert np.array_equal(R.chain(seg, passes, ties), R.aliased_passes(seg, passes, ties=ties).labels), (k, ties)
        tied += not R.tie_free(seg, passes)
    assert 0 < tied < 200  # both kinds occur: the tie rule is exercised, and tie-free images exist for the fixtures


def test_restatement_details():
    seg = np.zeros((21, 21), np.int64)
    seg[10, 10] = 5
    seg[10, 11] = 7
    seg[12:15, 12:15] = 9
    a = R.aliased_passes(seg, ((5, 5),))
    # 5 (1 pixel at (10, 10)): the crop rows 8 .. 12 holds 0 (most), 5, 7 and 9 (1 each): rank 1 is 5 itself by id ascending -> rank 2 = 7.
    # Then 7 (now 2 pixels, still judged by its stale size 1): 0, 7 (2), 9 (1): rank 1 is 7 itself -> rank 2 = 9.
    assert a.labels[10, 10] == 9 and a.labels[10, 11] == 9 and a.stats[:6] == [2, 2, 0, 0, 0, 1] and np.array_equal(a.labels, R.literal(seg, 5, 5))
    assert a.alias[5] == 9 and a.alias[7] == 9
    # ids outside [0, max_id] are written through and counted
    seg[0, 0] = 100
    b = R.aliased_passes(seg, ((5, 5),), max_id=20)
    assert b.labels[0, 0] == 100 and b.stat("out_of_range") == 1 and np.array_equal(b.labels[1:], a.labels[1:])
    lab, n = R.relabel(b.labels, max_id=20)
    assert n == 1 and lab[0, 0] == 100 and sorted(np.unique(lab).tolist()) == [0, 1, 100]


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------------------
def test_the_cases_hold_what_they_are_named_for():
    """the restatement's own counters, pass by pass, say that every edge case of the GPU tests' list is met (the GPU tests compare
    labels and stats with the same restatement exactly)"""
    from merge_cases import reference
    st = lambda name: reference(name)[3][0]
    pp = lambda name, p: st(name).per_pass[p]
    a = st("chain within a pass")  # 5 -> 7 -> 9 -> 11, then 20 reads the three hops; 7 and 9 are served on stale sizes
    assert a.stats[:6] == [4, 4, 0, 0, 0, 3] and set(a.labels[a.labels > 0].tolist()) == {11} and a.per_pass[0]["tie12"] == 2
    a = st("chain across passes")  # one merge a pass, 1 -> 2 -> 3 -> 4; the compress between passes keeps every read at one hop
    assert [q["merges"] for q in a.per_pass] == [1, 1, 1] and [q["chain"] for q in a.per_pass] == [0, 1, 1]
    assert a.alias[1:5].tolist() == [4, 4, 4, 4] and set(a.labels[a.labels > 0].tolist()) == {4}
    a = st("edges")  # 1, 2 skipped; 3 merged from a clipped crop; 6 alone in the background; 7 rank 0 of its own crop
    assert a.stat("negative") == 2 and a.stat("few") == 2 and a.labels[20, 20] != 3 and a.labels[10, 10] == 6 and (a.labels[4:6, 14:16] == 7).all()
    assert a.labels[0, 10] == 1 and a.labels[10, 0] == 2
    a = st("zero is small")
    assert (a.labels != 0).all() and a.stat("merges") == 2
    a = st("sparse ids")
    assert a.stat("merges") == 4 and a.labels.max() == 70000 and [q["merges"] for q in a.per_pass] == [2, 2, 0, 0]
    a = st("out of range")
    assert a.stat("out_of_range") == 4 and a.labels[3, 3] == -1 and a.labels[10, 11] == 2 ** 31 - 1 and a.labels[20, 30] == 5000
    assert st("threshold 0").stats[:4] == [0, 0, 0, 0]
    # windows 1, 4 and 45, each in its own pass: a window of 1 holds one id; the window of 45 serves 11 candidates that merge
    q = st("windows 1 4 45").per_pass
    assert (q[0]["candidates"], q[0]["few"]) == (23, 23) and (q[1]["merges"], q[1]["tie01"], q[1]["tie12"]) == (32, 3, 7)
    assert (q[2]["candidates"], q[2]["negative"], q[2]["merges"], q[2]["chain"]) == (40, 29, 11, 2)
    q = st("eight passes").per_pass
    assert len(q) == 8 and [x["merges"] for x in q] == [0, 12, 7, 3, 2, 0, 3, 2] and q[7]["candidates"] == 11
    assert len(st("one pass").per_pass) == 1 and pp("one pass", 0)["merges"] == 23
    # count ties at rank 0 / 1 and at rank 1 / 2, and images on which the tie rule decides
    assert (pp("23 x 37 tied", 0)["tie01"], pp("23 x 37 tied", 0)["tie12"]) == (2, 2) and (pp("21 x 21 tied", 0)["tie01"], pp("21 x 21 tied", 0)["tie12"]) == (1, 3)
    for name in ("21 x 21 tied", "23 x 37 tied"):
        segs, passes = reference(name)[:2]
        assert not R.tie_free(segs[0], passes)
    assert [r.stat("merges") for r in reference("batch of three")[3]] == [32, 76, 25]


# ---- exports -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_merge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_MERGE) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src
    for name, val in (("RELABEL", "1u"), ("MAX_PASSES", "8"), ("MAX_WINDOW", "45"), ("STATS", "8")):
        assert re.search(r"#define\s+PEA_MERGE_%s\s+%s\b" % (name, val), src), name
    for i, col in enumerate(pkg._lib.MERGE_STAT_COLUMNS[:6]):
        assert re.search(r"#define\s+PEA_MERGE_%s\s+%d\b" % (col.upper(), i), src), col
    assert pkg._lib.MERGE_STAT_COLUMNS == R.STAT_COLUMNS
    assert (pkg._lib.MERGE_RELABEL, pkg._lib.MERGE_MAX_PASSES, pkg._lib.MERGE_MAX_WINDOW, pkg._lib.MERGE_STATS) == (1, 8, 45, 8)
    for cite in ("THEN ID ASCENDING", "kind=\"stable\"", "uint16", "merge_func2", "NOTHING HAPPENS", "stale"):
        assert cite in src, cite
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert not set(NEW) & set(pkg._lib.EXPORTS)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "pea_merge" in open(os.path.join(ROOT, doc)).read(), doc
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "merge_objects" in integ and "uint16" in integ and "merge_small_objects" in integ
    assert "pea_k_merge.hip" in open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "pea_host.h")).read()


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaMergeDesc
    names = ["B", "Y", "X", "max_id", "n_passes", "threshold", "window", "flags"]
    assert [f[0] for f in D._fields_] == names and ctypes.sizeof(D) == 88
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 52, 84]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_merge.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaMergeDesc \{(.*?)\} PeaMergeDesc;", src, flags=re.S).group(1)
    fields = [f for decl in body.split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
    assert [re.sub(r"\[.*\]", "", f).strip() for f in fields] == names


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
PTR = {n: 0x10000000 * (i + 1) for i, n in enumerate(("seg", "out", "counts", "stats", "work"))}


def desc(pkg, B=2, Y=40, X=50, max_id=600, passes=R.CVPPP_MERGE_PASSES, flags=0, n_passes=None):
    d = pkg._lib.PeaMergeDesc()
    d.B, d.Y, d.X, d.max_id, d.flags = B, Y, X, max_id, flags
    d.n_passes = len(passes) if n_passes is None else n_passes
    for k, (t, w) in enumerate(passes):
        d.threshold[k], d.window[k] = t, w
    return d


def call(pkg, lib, d="default", wbytes=None, **kw):
    """pea_merge_small on dummy pointers: anything but an early return would fault"""
    p = dict(PTR)
    for k in list(kw):
        if k in p:
            p[k] = kw.pop(k)
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = lib.pea_merge_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    vp = lambda v: ctypes.c_void_p(v) if v else None
    return lib.pea_merge_small(None if d is None else ctypes.byref(d), vp(p["seg"]), vp(p["out"]), vp(p["counts"]), vp(p["stats"]), vp(p["work"]), wbytes, None)


def test_validate_and_its_order(pkg, lib):
    v = lambda **kw: lib.pea_merge_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_merge_validate(None) == E_NULL and call(pkg, lib, d=None) == E_NULL and lib.pea_merge_workspace_bytes(None) == 0
    assert v() == OK and v(passes=R.BBBC_MERGE_PASSES, flags=RELABEL) == OK and v(B=1, Y=1, X=1, max_id=0, passes=((0, 1),)) == OK
    assert v(passes=((2 ** 31 - 1, 45),) * 8, Y=45, X=45, max_id=2 ** 31 - 2, B=2 ** 31 - 1) == OK
    # entries from n_passes on are ignored
    assert v(passes=((5, 5), (-1, 0), (3, 99)), n_passes=1) == OK
    bad = [dict(flags=2), dict(flags=1 << 31), dict(B=0), dict(Y=0), dict(X=-3), dict(max_id=-1), dict(max_id=2 ** 31 - 1), dict(n_passes=0),
           dict(n_passes=9), dict(passes=((-1, 5),)), dict(passes=((5, 5), (5, 0))), dict(passes=((5, 46),), Y=100, X=100), dict(passes=((5, -5),))]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert call(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_merge_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    # a window above min(Y, X): valid, not served -- behind every descriptor check, before any pointer is looked at
    for kw in (dict(Y=20), dict(X=20), dict(passes=((5, 5), (1, 41))), dict(passes=((1, 2),), Y=1)):
        assert v(**kw) == E_UNSUPPORTED and call(pkg, lib, seg=0, work=0, **kw) == E_UNSUPPORTED, kw
        assert lib.pea_merge_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    assert v(Y=20, passes=((5, 21), (-1, 5))) == E_DESC and v(Y=21, X=21) == OK and v(Y=20, flags=2) == E_DESC
    assert call(pkg, lib, seg=0, out=0, work=0, flags=4) == E_DESC


def test_refusals_before_a_launch_and_their_order(pkg, lib):
    for name in ("seg", "out", "counts", "stats"):
        assert call(pkg, lib, **{name: 0}) == E_NULL, name
    for skew in (1, 2, 3):
        for name in ("seg", "out", "counts", "stats", "work"):
            assert call(pkg, lib, **{name: PTR[name] + skew}) == E_ALIGN, (name, skew)
    for name in ("stats", "work"):
        assert call(pkg, lib, **{name: PTR[name] + 4}) == E_ALIGN, name
    for name in ("seg", "out", "counts"):
        assert call(pkg, lib, work=0, **{name: PTR[name] + 4}) == E_WORKSPACE, name
    need = lib.pea_merge_workspace_bytes(ctypes.byref(desc(pkg)))
    assert call(pkg, lib, work=0) == E_WORKSPACE and call(pkg, lib, wbytes=need - 1) == E_WORKSPACE and call(pkg, lib, wbytes=0) == E_WORKSPACE
    # 2^31 pixels an image; more than 2^31 - 1 workgroups; out overlapping seg without being seg
    assert call(pkg, lib, wbytes=SIZE_MAX, Y=2 ** 16, X=2 ** 15) == E_UNSUPPORTED
    assert call(pkg, lib, wbytes=SIZE_MAX, B=2 ** 23, max_id=2 ** 16) == E_UNSUPPORTED and call(pkg, lib, wbytes=SIZE_MAX, B=2 ** 22, Y=2 ** 10, X=2 ** 10) == E_UNSUPPORTED
    assert call(pkg, lib, out=PTR["seg"] + 4) == E_UNSUPPORTED and call(pkg, lib, out=PTR["seg"] - 4 * (2 * 40 * 50 - 1)) == E_UNSUPPORTED
    # the stated order: descriptor, NULL, alignment, workspace, size
    assert call(pkg, lib, work=0, out=PTR["out"] + 2) == E_ALIGN
    assert call(pkg, lib, work=0, Y=2 ** 16, X=2 ** 15) == E_WORKSPACE
    assert call(pkg, lib, seg=0, work=0, out=PTR["out"] + 2) == E_NULL
    assert call(pkg, lib, seg=0, work=0, out=PTR["out"] + 2, n_passes=0) == E_DESC


def al8(x):
    return (x + 7) // 8 * 8


def test_workspace_bytes_is_monotone_in_each_extent(pkg, lib):
    nb = lambda **kw: lib.pea_merge_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    for name, values in (("B", range(1, 40)), ("max_id", range(0, 1200, 7))):
        sizes = [nb(**{name: v}) for v in values]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], name
    # the layout: 8 words per image, three moments of 8 bytes an id, alias, a candidate bit per id, root, rank, the scan's totals
    for B, max_id in ((1, 0), (2, 600), (3, 255), (1, 256), (5, 70)):
        N = max_id + 1
        assert nb(B=B, max_id=max_id) == 64 * B + 3 * 8 * B * N + 3 * al8(4 * B * N) + 8 * B * -(-N // 64) + al8(4 * B * -(-N // 256)), (B, max_id)
    assert nb(Y=21, X=3000, passes=R.BBBC_MERGE_PASSES, flags=RELABEL) == nb() and nb() % 8 == 0
    assert nb(B=2 ** 31 - 1, max_id=2 ** 31 - 2) == SIZE_MAX


# ---- the Python entry points -------------------------------------------------------------------------------------------------------------
def test_python_entry_points(pkg):
    from importlib import import_module
    for name in pkg.MERGE_EXPORTS:
        assert hasattr(pkg, name), name
    mod = import_module(pkg.__name__ + ".utils.merge_objects")
    post = import_module(pkg.__name__ + ".utils.postprocessing")
    assert mod is pkg.merge_objects and mod.merge_func is pkg.merge_func
    assert not hasattr(post, "merge_func") and not hasattr(post, "merge_small_object") and "merge_objects" in post.__doc__
    sig = inspect.signature(mod.merge_small_object)
    assert list(sig.parameters) == ["seg", "threshold", "window"] and [p.default for p in sig.parameters.values()][1:] == [5, 5]
    for f in (mod.merge_func, mod.merge_func_bbbc):
        sig = inspect.signature(f)
        assert list(sig.parameters) == ["seg", "step"] and sig.parameters["step"].default == 4
    assert list(inspect.signature(mod.relabel).parameters) == ["seg"]
    assert mod.CVPPP_MERGE_PASSES == pkg.CVPPP_MERGE_PASSES == R.CVPPP_MERGE_PASSES and mod.BBBC_MERGE_PASSES == pkg.BBBC_MERGE_PASSES == R.BBBC_MERGE_PASSES
    sig = inspect.signature(pkg.merge_small_objects)
    assert list(sig.parameters) == ["seg", "passes", "relabel", "max_id"]
    assert [p.default for p in sig.parameters.values()][1:] == [pkg.CVPPP_MERGE_PASSES, False, None]

    seg = torch.zeros(2, 30, 40, dtype=torch.int32)
    with pytest.raises(TypeError, match="torch.Tensor"):
        pkg.merge_small_objects(np.zeros((30, 40), np.int32))
    with pytest.raises(TypeError, match="int32"):
        pkg.merge_small_objects(seg.long())
    with pytest.raises(ValueError, match=r"\[Y, X\] or \[B, Y, X\]"):
        pkg.merge_small_objects(seg[None])
    with pytest.raises(ValueError, match="empty"):
        pkg.merge_small_objects(seg[:, :0])
    for passes in ((), ((1, 1),) * 9, ((1, 2, 3),)):
        with pytest.raises(ValueError, match="passes"):
            pkg.merge_small_objects(seg, passes=passes)
    with pytest.raises(ValueError, match="threshold"):
        pkg.merge_small_objects(seg, passes=((-1, 5),))
    with pytest.raises(ValueError, match="held in LDS"):
        pkg.merge_small_objects(seg, passes=((5, 101),))
    with pytest.raises(ValueError, match="may not exceed"):
        pkg.merge_small_objects(seg, passes=((5, 31),))
    with pytest.raises(ValueError, match="max_id"):
        pkg.merge_small_objects(seg, max_id=-1)
    with pytest.raises(TypeError, match="integers"):
        mod.merge_func(np.zeros((30, 40), np.float32))
    with pytest.raises(ValueError, match="outside"):
        mod.relabel(np.full((30, 40), -1))
    with pytest.raises(ValueError, match=r"\[Y, X\]"):
        mod.merge_func(np.zeros((40,), np.int32))
    if not torch.cuda.is_available():
        for f in (lambda: pkg.merge_small_objects(seg), lambda: pkg.merge_small_objects(seg[0], max_id=5, relabel=True), lambda: mod.merge_func(seg),
                  lambda: mod.merge_func(np.zeros((30, 40), np.uint16)), lambda: mod.relabel(seg[0]), lambda: mod.merge_small_object(seg, 20, 11)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f()
