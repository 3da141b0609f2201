"""CPU: the agglomeration of the fragment graph (include/pea_agglo.h) -- the two restatements of tests/agglo_reference.py, which the GPU
tests compare the kernels with, agree on every tie-free case (and no such case trips the sequential form's tie assertion); on tied cases
the round simulation does not depend on the order of the rows; the popped scores of a sequential run never decrease (reducibility).
The header and the library agree on the three new symbols, the ctypes mirrors have the header's layout, every refusal of
pea_agglo_validate and pea_agglo_merge is reached before anything is launched and in the header's order (dummy device pointers, no
GPU), pea_agglo_workspace_bytes is monotone, and the Python entry points say what is wrong with a call before they look for a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import agglo_reference as R
from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
RESUME, IGNORE_ZERO = 1, 2
NEW = ["pea_agglo_merge", "pea_agglo_validate", "pea_agglo_workspace_bytes"]
SIZE_MAX = 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TIE_FREE, ids=lambda c: c[0])
def test_the_two_restatements_agree_where_nothing_ties(case):
    name, make, linkage, thr = case
    g = make()
    root, popped = R.sequential(g, linkage, thr)  # (asserts at every pop that no other live edge has the popped score)
    sim = R.rounds(g, linkage, thr)
    assert np.array_equal(root, sim.root) and sim.merges == len(popped) and sim.mergeable() == 0, name
    assert sim.rounds <= sim.merges and (sim.merges == 0 or sim.rounds >= 1)
    # reducibility: the popped scores never decrease
    assert all(b >= a for a, b in zip(popped, popped[1:])) and all(s < np.float32(thr) for s in popped), name
    # root[i] is the smallest id of i's cluster
    for r in np.unique(root):
        assert r == np.flatnonzero(root == r).min()
    # rounds that run out leave a refinement, and the same rounds resumed give the same result
    few = R.rounds(g, linkage, thr, max_rounds=2)
    assert R.is_refinement(few.root, root) and (few.mergeable() > 0 or np.array_equal(few.root, root))
    assert np.array_equal(few.run(thr).root, root) and few.stats() == sim.stats()
    # a lower threshold merges a prefix: its partition refines this one
    assert R.is_refinement(R.rounds(g, linkage, np.float32(thr) / 2).root, root)


@pytest.mark.parametrize("case", R.TIED, ids=lambda c: c[0])
def test_tied_cases_do_not_depend_on_the_order_of_the_rows(case):
    name, make, linkage, thr = case
    g = make()
    a, b = R.rounds(g, linkage, thr), R.rounds(g.shuffled(7), linkage, thr)
    assert np.array_equal(a.root, b.root) and a.stats() == b.stats() and a.edges == b.edges, name
    assert a.merges > 0 and a.mergeable() == 0
    scores = [R.score(linkage, p) for p in R.clean(g, linkage)[0].values()]
    assert len(set(scores)) < len(scores) // 4, "the case is meant to tie"


def test_what_the_named_cases_promise():
    g = R.chain(70, True)
    assert (np.diff(g.value) > 0).all() and R.rounds(g, R.MEAN, 0.45).rounds == R.rounds(g, R.MEAN, 0.45).merges == 63
    assert (np.diff(R.chain(70, False).value) < 0).all()
    s = R.star(300)
    first = R.rounds(s, R.MEAN, 0.8, max_rounds=1)
    assert first.merges == 1 and len(first.edges) == 300 and len(s.uv) == 601  # the hubs merged: 300 pairs of parallel edges combined
    assert all(p[2] == int(s.weight[1 + i] + s.weight[301 + i]) for i, p in enumerate(first.edges[(1, 3 + i)] for i in range(300)))
    r = R.random_graph()
    assert len(r.uv) == 2500 and r.max_id == 600 and len(np.unique(r.uv, axis=0)) == 2500
    b = R.with_bad_rows(r)
    edges, no_edge, bad = R.clean(b, R.MEAN)
    assert (no_edge, bad) == (6, 6) and R.clean(b, R.MAX)[1:] == (6, 4) and R.clean(b, R.MEAN, True)[1] == 7 and len(edges) == 2501  # ((0, 7) is an edge without IGNORE_ZERO)
    assert len(b.uv) == 2500 + 250 + 13


def test_conversions_and_scores():
    # the fixed point: floor to a multiple of 2^-32, in two words
    for value, weight in ((0.3, 7), (-0.3, 7), (0.0, 5), (32768.0, 2 ** 31), (-32768.0, 2 ** 31), (1e-12, 1), (-1e-12, 1), (0.1, 0)):
        lo, hi, cnt = R.payload(R.MEAN, value, weight)
        p = value * float(weight)
        assert 0 <= lo < 2 ** 32 and cnt == weight
        if abs(p) < 2 ** 20:  # (p * 2^32 is exact in f64 there)
            assert hi * 2 ** 32 + lo == int(np.floor(np.float64(p) * 2.0 ** 32))
        assert hi == int(np.floor(p))
    assert R.score(R.MEAN, R.payload(R.MEAN, 0.1, 0)) == np.inf and R.combine(R.MEAN, (1, 2, 3), (0, 0, 0)) == (1, 2, 3)
    assert R.score(R.MEAN, R.payload(R.MEAN, 0.25, 8)) == np.float32(0.25)
    a, b = R.payload(R.MEAN, 0.2, 3), R.payload(R.MEAN, 0.6, 1)
    m = R.score(R.MEAN, R.combine(R.MEAN, a, b))
    assert R.score(R.MEAN, a) <= m <= R.score(R.MEAN, b) and abs(float(m) - 0.3) < 1e-7  # a weighted mean lies between its parts
    v = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 2.0, np.inf], np.float32)
    o = [R.ord32(x) for x in v]
    assert o == sorted(o) and len(set(o)) == len(o) and all(R.unord32(x).tobytes() == y.tobytes() for x, y in zip(o, v))
    assert R.score(R.MIN, R.combine(R.MIN, R.payload(R.MIN, 0.7, 1), R.payload(R.MIN, 0.2, 1))) == np.float32(0.2)
    assert R.score(R.MAX, R.combine(R.MAX, R.payload(R.MAX, 0.7, 1), R.payload(R.MAX, 0.2, 1))) == np.float32(0.7)
    labels, n = R.labels_of(np.array([0, 1, 1, 3, 1], np.int32), [5, 0, 2, 1, 0], True)
    assert labels.tolist() == [0, 0, 0, 1, 0] and n == 1  # root 1 is not present: its cluster is not numbered
    labels, n = R.labels_of(np.array([0, 1, 1, 3, 1], np.int32))
    assert labels.tolist() == [1, 2, 2, 3, 2] and n == 3


# ---- exports -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_agglo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_AGGLO) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src
    for name, val in (("RESUME", "1u"), ("IGNORE_ZERO", "2u"), ("MEAN", "0"), ("MIN", "1"), ("MAX", "2"), ("STATS", "8"), ("MAX_ROUNDS", "65536"),
                      ("MAX_EDGES", "1073741824")):
        assert re.search(r"#define\s+PEA_AGGLO_%s\s+%s\b" % (name, val), src), name
    for i, col in enumerate(pkg._lib.AGGLO_STAT_COLUMNS[:7]):
        assert re.search(r"#define\s+PEA_AGGLO_%s\s+%d\b" % (col.upper(), i), src), col
    assert (pkg._lib.AGGLO_RESUME, pkg._lib.AGGLO_IGNORE_ZERO, pkg._lib.AGGLO_STATS, pkg._lib.AGGLO_MAX_ROUNDS, pkg._lib.AGGLO_MAX_EDGES) == (1, 2, 8, 65536, 2 ** 30)
    assert pkg._lib.AGGLO_LINKAGES == R.LINKAGES
    for cite in ("Progress.", "Relation to the sequential procedure", "not waterz's", "discretize_queue=256", "REDUCIBLE", "HistogramQuantileAffinity",
                 "refused on the device"):
        assert cite in src, cite
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert not set(NEW) & set(pkg._lib.EXPORTS)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "pea_agglo" in open(os.path.join(ROOT, doc)).read(), doc
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "seg_waterz" in integ and "discretize_queue" in integ and "2^-24" in integ


def test_ctypes_mirrors_have_the_headers_layout(pkg):
    D = pkg._lib.PeaAggloDesc
    names = ["B", "max_id", "max_edges", "n_edges_stride", "linkage", "rounds", "threshold", "flags"]
    assert [f[0] for f in D._fields_] == names and ctypes.sizeof(D) == 40
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 16, 24, 28, 32, 36]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_agglo.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaAggloDesc \{(.*?)\} PeaAggloDesc;", src, flags=re.S).group(1)
    assert [decl.split()[-1] for decl in body.split(";") if decl.strip()] == names
    body = re.search(r"typedef struct PeaAggloBuffers \{(.*?)\} PeaAggloBuffers;", src, flags=re.S).group(1)
    fields = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert fields == [f[0] for f in pkg._lib.PeaAggloBuffers._fields_] and ctypes.sizeof(pkg._lib.PeaAggloBuffers) == 8 * len(fields)


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
PTR = {n: 0x10000000 * (i + 1) for i, n in enumerate(("uv", "n_edges", "value", "weight", "node_size", "root", "labels", "counts", "stats", "work"))}


def desc(pkg, B=2, max_id=600, max_edges=2500, n_edges_stride=8, linkage=0, rounds=3, threshold=0.5, flags=0):
    d = pkg._lib.PeaAggloDesc()
    d.B, d.max_id, d.max_edges, d.n_edges_stride, d.linkage, d.rounds, d.threshold, d.flags = B, max_id, max_edges, n_edges_stride, linkage, rounds, threshold, flags
    return d


def call(pkg, lib, d="default", wbytes=None, io=True, **kw):
    """pea_agglo_merge on dummy pointers: anything but an early return would fault"""
    p = dict(PTR)
    for k in list(kw):
        if k in p:
            p[k] = kw.pop(k)
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = lib.pea_agglo_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    buf = pkg._lib.PeaAggloBuffers()
    for k in p:
        if k != "work":
            setattr(buf, k, p[k] or None)
    return lib.pea_agglo_merge(None if d is None else ctypes.byref(d), ctypes.byref(buf) if io else None, ctypes.c_void_p(p["work"]) if p["work"] else None,
                               wbytes, None)


HUGE = dict(B=2 ** 31 - 1, max_id=2 ** 31 - 2, max_edges=2 ** 30)


def test_validate_and_its_order(pkg, lib):
    v = lambda **kw: lib.pea_agglo_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_agglo_validate(None) == E_NULL and call(pkg, lib, d=None) == E_NULL and lib.pea_agglo_workspace_bytes(None) == 0
    assert v() == OK and v(B=1, max_id=0, max_edges=1, n_edges_stride=0, rounds=0) == OK and v(flags=RESUME | IGNORE_ZERO) == OK
    assert v(linkage=2, rounds=65536, threshold=float("inf")) == OK and v(threshold=-1.0) == OK and v(**HUGE) == OK
    bad = [dict(flags=4), dict(flags=1 << 31), dict(B=0), dict(max_id=-1), dict(max_id=2 ** 31 - 1), dict(max_edges=0), dict(max_edges=2 ** 30 + 1),
           dict(n_edges_stride=-1), dict(linkage=3), dict(linkage=-1), dict(threshold=float("nan")), dict(rounds=-1), dict(rounds=65537)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert call(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_agglo_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    # a descriptor is refused before a NULL pointer, a short workspace or a size is looked at
    assert call(pkg, lib, uv=0, root=0, work=0, linkage=5, **HUGE) == E_DESC and call(pkg, lib, io=False, rounds=-1) == E_DESC


def test_refusals_before_a_launch_and_their_order(pkg, lib):
    assert call(pkg, lib, io=False) == E_NULL
    for name in ("uv", "n_edges", "value", "root", "stats", "weight", "labels", "counts"):
        assert call(pkg, lib, **{name: 0}) == E_NULL, name
    assert call(pkg, lib, weight=0, linkage=1, work=0) == E_WORKSPACE and call(pkg, lib, weight=0, linkage=2, work=0) == E_WORKSPACE  # read under MEAN only
    assert call(pkg, lib, labels=0, counts=0, node_size=0, work=0) == E_WORKSPACE  # optional
    assert call(pkg, lib, wbytes=SIZE_MAX, **HUGE) == E_UNSUPPORTED  # more than 2^31 - 1 workgroups
    assert call(pkg, lib, wbytes=SIZE_MAX, B=2 ** 23, max_id=2 ** 16) == E_UNSUPPORTED and call(pkg, lib, B=2 ** 22, max_id=2 ** 16, max_edges=1, work=0) == E_WORKSPACE
    for skew in (1, 2, 3):
        for name in ("uv", "root", "labels", "counts", "n_edges", "value", "weight", "node_size", "stats", "work"):
            assert call(pkg, lib, **{name: PTR[name] + skew}) == E_ALIGN, (name, skew)
    for name in ("n_edges", "value", "weight", "node_size", "stats", "work"):
        assert call(pkg, lib, **{name: PTR[name] + 4}) == E_ALIGN, name
    for name in ("uv", "root", "labels", "counts"):
        assert call(pkg, lib, work=0, **{name: PTR[name] + 4}) == E_WORKSPACE, name
    need = lib.pea_agglo_workspace_bytes(ctypes.byref(desc(pkg)))
    assert call(pkg, lib, work=0) == E_WORKSPACE and call(pkg, lib, wbytes=need - 1) == E_WORKSPACE and call(pkg, lib, wbytes=0) == E_WORKSPACE
    assert call(pkg, lib, work=0, flags=RESUME) == E_WORKSPACE
    # the stated order: descriptor, NULL, size, alignment, workspace
    assert call(pkg, lib, work=0, root=PTR["root"] + 2) == E_ALIGN
    assert call(pkg, lib, work=0, root=PTR["root"] + 2, **HUGE) == E_UNSUPPORTED
    assert call(pkg, lib, uv=0, work=0, root=PTR["root"] + 2, **HUGE) == E_NULL
    assert call(pkg, lib, uv=0, work=0, root=PTR["root"] + 2, rounds=-1, **HUGE) == E_DESC


def al8(x):
    return (x + 7) // 8 * 8


def test_workspace_bytes_is_monotone_in_each_extent(pkg, lib):
    nb = lambda **kw: lib.pea_agglo_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    for name, values in (("B", range(1, 40)), ("max_id", range(0, 1200, 7)), ("max_edges", [1, 2, 31, 32, 33, 100, 2500, 4096, 4097, 10 ** 6])):
        sizes = [nb(**{name: v}) for v in values]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], name
    # the layout: the header, 16 words per image, two tables of four words a slot, best, root, rank, the scan's totals
    for B, max_id, E in ((1, 0, 1), (2, 600, 2500), (3, 255, 32), (1, 256, 33), (5, 70, 69)):
        cap = 64
        while cap < 2 * E:
            cap *= 2
        N = max_id + 1
        want = 8 * 8 + 8 * 16 * B + 8 * B * 2 * 4 * cap + 8 * B * N + 2 * al8(4 * B * N) + al8(4 * B * -(-N // 256))
        assert nb(B=B, max_id=max_id, max_edges=E) == want, (B, max_id, E)
    assert nb(rounds=0, linkage=2, threshold=3.0, n_edges_stride=1, flags=RESUME | IGNORE_ZERO) == nb() and nb() % 8 == 0
    assert nb(**HUGE) == SIZE_MAX


# ---- the Python entry points -------------------------------------------------------------------------------------------------------------
def test_python_entry_points(pkg):
    from importlib import import_module
    for name in pkg.AGGLO_EXPORTS:
        assert hasattr(pkg, name), name
    mod = import_module(pkg.__name__ + ".utils.seg_waterz")
    assert mod is pkg.utils.seg_waterz and mod.seg_waterz is pkg.seg_waterz
    assert list(inspect.signature(pkg.seg_waterz).parameters) == ["affs", "mask"] and inspect.signature(pkg.seg_waterz).parameters["mask"].default is None
    sig = inspect.signature(mod.agglomerate)  # waterz's
    assert list(sig.parameters) == ["affs", "thresholds", "fragments", "scoring_function", "discretize_queue"]
    assert sig.parameters["fragments"].default is None and sig.parameters["discretize_queue"].default == 0
    sig = inspect.signature(pkg.agglomerate)
    assert list(sig.parameters)[:7] == ["affs", "thresholds", "fragments", "linkage", "offsets", "rounds", "max_id"]
    assert sig.parameters["linkage"].default == "mean" and sig.parameters["rounds"].default is None
    assert list(inspect.signature(pkg.agglomerate_graph).parameters)[:3] == ["rag_or_uv", "value", "weight"]

    # the scoring strings: the reference's, waterz's default, the min / max forms on the COST; anything else names itself
    ref_sf = "OneMinus<EdgeStatisticValue<RegionGraphType, MeanAffinityProvider<RegionGraphType, ScoreValue>>>"
    assert mod.scoring_linkage(ref_sf) == "mean" and mod.scoring_linkage("OneMinus<MeanAffinity<RegionGraphType, ScoreValue>>") == "mean"
    assert mod.scoring_linkage("OneMinus<MinAffinity<RegionGraphType, ScoreValue>>") == "max"
    assert mod.scoring_linkage("OneMinus<MaxAffinity<RegionGraphType,ScoreValue>>") == "min"
    a = np.zeros((3, 4, 20, 30), np.float32)
    quantile = "OneMinus<HistogramQuantileAffinity<RegionGraphType, 50, ScoreValue, 256>>"
    for sf in (quantile, "MeanAffinity<RegionGraphType, ScoreValue>", "nonsense"):
        with pytest.raises(NotImplementedError, match=re.escape(sf)):
            mod.agglomerate(a, [0.5], scoring_function=sf)
    for th in ([0.5, 0.3], [0.2, 0.8, 0.7], [], [float("nan")]):
        with pytest.raises(ValueError, match="ascending|empty"):
            pkg.agglomerate(a, th, fragments="watershed")
        with pytest.raises(ValueError, match="ascending|empty"):
            mod.agglomerate(a, th)
    with pytest.raises(ValueError, match="linkage"):
        pkg.agglomerate(a, [0.5], fragments="watershed", linkage="median")
    with pytest.raises(TypeError, match="fragments is required"):
        pkg.agglomerate(a, [0.5])
    with pytest.raises(ValueError, match="only named way"):
        pkg.agglomerate(a, [0.5], fragments="mahotas")
    with pytest.raises(ValueError, match="does not go with"):
        pkg.agglomerate(a, [0.5], fragments=np.zeros((4, 20, 31), np.int32))
    with pytest.raises(ValueError, match=r"\[K, Y, X\] or \[K, Z, Y, X\]"):
        pkg.agglomerate(a[0, 0], [0.5], fragments="watershed")
    with pytest.raises(ValueError, match="local channels"):
        pkg.agglomerate(a[:2], [0.5], fragments="watershed")
    with pytest.raises(ValueError, match=r"\[2, H, W\]"):
        pkg.seg_waterz(a)
    with pytest.raises(ValueError, match="mask"):
        pkg.seg_waterz(a[:2, 0], np.ones((20, 31)))
    with pytest.raises(TypeError, match="floats"):
        pkg.seg_waterz(np.zeros((2, 20, 30), np.int32))
    with pytest.raises(TypeError, match="value is required"):
        pkg.agglomerate_graph(np.array([[1, 2]]), threshold=0.5)
    with pytest.raises(TypeError, match="weight"):
        pkg.agglomerate_graph(np.array([[1, 2]]), np.array([0.5]), threshold=0.5)
    with pytest.raises(ValueError, match="linkage"):
        pkg.agglomerate_graph(np.array([[1, 2]]), np.array([0.5]), threshold=0.5, linkage="ward")
    if not torch.cuda.is_available():
        for f in (lambda: next(pkg.agglomerate(a, [0.5], fragments="watershed")), lambda: pkg.seg_waterz(a[:2, 0]),
                  lambda: next(mod.agglomerate(a, [0.3, 0.5])), lambda: pkg.seg_waterz(torch.zeros(2, 20, 30)),
                  lambda: pkg.agglomerate_graph(np.array([[1, 2]]), np.array([0.5]), np.array([3]), threshold=0.5)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f()
    assert mod.relabel(np.array([5, 2, 2, 9], np.int32)).tolist() == [2, 1, 1, 3] and mod.relabel(np.array([[4]], np.uint8)).dtype == np.uint8
    seg = np.array([[0, 7, 7], [3, 3, 9]], np.uint64)
    assert mod.relabel(seg).tolist() == [[0, 2, 2], [1, 1, 3]] and mod.relabel(np.zeros((2, 2), np.int32)).tolist() == [[0, 0], [0, 0]]
    assert mod.relabel(torch.tensor([[0, 7, 7], [3, 3, 9]])).tolist() == [[0, 2, 2], [1, 1, 3]]
