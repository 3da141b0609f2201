"""CPU: the region adjacency graph (include/pea_rag.h) -- the numpy restatement tests/rag_reference.py, which the GPU tests compare the
kernels with, is held to a brute-force dictionary walk over the voxels on a handful of tiny volumes and to hand-written expectations;
the header and the library agree on the five new symbols, the ctypes mirrors have the header's layout, pea_rag_validate and
pea_rag_workspace_bytes answer as the header says, every refusal of pea_rag_build and pea_rag_project is reached before anything is
launched and in the header's order (dummy device pointers, no GPU); probs_to_costs is the reference's formula in float64; mc_baseline
says what is wrong with a call before it looks for a device and its boundary map is the reference's."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from rag_reference import (LOCAL3, hub_image, probs_to_costs_f64, project_reference, rag_brute, rag_reference, stub_solver, volume,
                           volume_ref, voronoi)

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
NEW = ["pea_rag_build", "pea_rag_project", "pea_rag_validate", "pea_rag_workspace_bytes", "pea_rag_workspace_init"]
SIZE_MAX = 2 ** 64 - 1
KEYS = ("uv", "size", "count", "min", "max", "node_size", "stats")


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def same(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)
    for k in ("mean", "bmean"):
        assert np.allclose(a[k], b[k], rtol=0, atol=1e-12), (what, k)


def test_restatement_against_the_brute_force_walk():
    rng = np.random.default_rng(0)
    cases = []
    for seed, shape, n in ((1, (1, 7, 9), 5), (2, (3, 5, 6), 7), (3, (2, 1, 11), 4), (4, (4, 6, 1), 6), (5, (1, 1, 1), 1)):
        f = voronoi(shape, n, seed)
        a = (rng.random((5,) + shape, dtype=np.float32) * 4 - 2).astype(np.float32)
        b = rng.random(shape, dtype=np.float32)
        offs = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 2, -3], [1, -2, 0]]
        cases.append((f, a, offs, b))
    for f, a, offs, b in cases:
        for kw in (dict(), dict(one_minus=True), dict(ignore_zero=True), dict(max_id=int(f.max()) + 3), dict(max_id=max(0, int(f.max()) - 2))):
            same(rag_reference(f, a, offs, b, **kw), rag_brute(f, a, offs, b, **kw), (f.shape, kw))
        same(rag_reference(f), rag_brute(f), f.shape)
    # bad ids, bad samples, negative samples
    f, a, offs, b = cases[1][0].copy(), cases[1][1].copy(), cases[1][2], cases[1][3].copy()
    f[0, 0, 0], f[1, 2, 3], f[2, 4, 5] = -1, 99, -2 ** 31
    a[0, 1], a[1, 0, 3], a[2, 2, 2], a[3, 1, 1, 4] = np.nan, np.inf, 1e30, -np.inf
    b[1, 1], b[0, 2, 2] = np.nan, -1e30
    for kw in (dict(max_id=6), dict(max_id=6, one_minus=True, ignore_zero=True)):
        r = rag_reference(f, a, offs, b, **kw)
        same(r, rag_brute(f, a, offs, b, **kw), kw)
        assert r["stats"][3] == 3 and r["stats"][5] > 0


def test_hand_written_expectations():
    f = np.array([[[0, 0, 1], [2, 2, 1]]], np.int32)
    a = np.array([[[[.5, .25, .75], [1., 0., -1.]]], [[[9., 9., 9.], [.5, .125, 2.]]]], np.float32)  # (0, 0, -1) then (0, -1, 0)
    b = np.array([[[1., 2., 3.], [4., 5., 6.]]], np.float32)
    r = rag_reference(f, a, [[0, 0, -1], [0, -1, 0]], b)
    assert r["uv"].tolist() == [[0, 1], [0, 2], [1, 2]] and r["size"].tolist() == [1, 2, 1]
    # (0, 1): the sample sits at p = (0, 2), q = p + (0, 0, -1); (1, 2): at p = (1, 2); (0, 2): the two vertical pairs, p in row 1
    assert r["count"].tolist() == [1, 2, 1] and r["mean"].tolist() == [0.75, 0.3125, -1.0]
    assert r["min"].tolist() == [0.75, 0.125, -1.0] and r["max"].tolist() == [0.75, 0.5, -1.0]
    assert r["bmean"].tolist() == [2.5, (1 + 4 + 2 + 5) / 4, 5.5]
    assert r["node_size"].tolist() == [2, 2, 2] and r["stats"].tolist() == [3, 0, 0, 0, 0, 0, 0, 0]
    r = rag_reference(f, a, [[0, 0, -1], [0, -1, 0]], b, ignore_zero=True, one_minus=True)
    assert r["uv"].tolist() == [[1, 2]] and r["mean"].tolist() == [2.0] and r["node_size"].tolist() == [2, 2, 2]
    # a long-range offset joins 0 and 1 across the image (they touch) and 2 and 1 ... and one that meets a pair that does not touch
    g = np.array([[[0, 5, 1, 5, 2]]], np.int32)
    r = rag_reference(g, np.ones((1, 1, 1, 5), np.float32), [[0, 0, -2]])
    assert r["uv"].tolist() == [[0, 5], [1, 5], [2, 5]] and r["count"].tolist() == [0, 0, 0] and r["stats"][4] == 2
    assert r["mean"].tolist() == [0, 0, 0] and r["min"].tolist() == [0, 0, 0]
    # row ends: the last voxel of a row and the first of the next are no neighbours
    h = np.array([[[7, 7, 3], [4, 7, 7]]], np.int32)
    assert rag_reference(h)["uv"].tolist() == [[3, 7], [4, 7]]
    # the hub touches more than 1024 others
    r = rag_reference(hub_image()[None][0])
    assert (r["uv"][:, 0] == 1).sum() == 1025 and r["stats"][0] == 1025 + 1  # and the split block's two ids touch
    # the shared volumes: long-range channels meet pairs that do not touch, both images differ
    for kind in ("2d", "3d"):
        ref = volume_ref(kind)
        assert all(r["stats"][4] > 0 and r["stats"][0] > 20 for r in ref) and ref[0]["stats"][0] != ref[1]["stats"][0]
    # projection and the stub solver
    seg, bad = project_reference(np.array([[0, 2, 5, -1]], np.int32), np.array([10, 11, 12], np.int32))
    assert seg.tolist() == [[10, 12, 0, 0]] and bad == 2
    assert stub_solver(5, np.array([[0, 1], [1, 2], [3, 4]]), np.array([-1.0, 2.0, -0.5])).tolist() == [1, 1, 3, 4, 4]


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "pea_rag.h")).read()


def test_header_declares_exactly_the_five_entry_points(pkg, lib):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src))) == sorted(pkg._lib.EXPORTS_RAG) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in header()
    for name, val in (("PEA_RAG_ONE_MINUS", "1u"), ("PEA_RAG_IGNORE_ZERO", "2u"), ("PEA_RAG_MAX_K", "32"), ("PEA_RAG_MIN_CAPACITY", "64"),
                      ("PEA_RAG_STATS", "8")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, val), header()), name
    L = pkg._lib
    assert (L.RAG_ONE_MINUS, L.RAG_IGNORE_ZERO, L.RAG_MAX_K, L.RAG_MIN_CAPACITY, L.RAG_STATS) == (1, 2, 32, 64, 8)
    for i, name in enumerate(("N_EDGES", "N_EDGES_DROPPED", "N_PAIRS_DROPPED", "N_NO_ID", "N_NOT_TOUCHING", "N_SKIPPED")):
        assert re.search(r"#define\s+PEA_RAG_%s\s+%d\b" % (name, i), header()), name
    assert lib.pea_version() == L.PEA_ABI_VERSION == 2 and not set(NEW) & set(L.EXPORTS)


def test_ctypes_mirrors_have_the_headers_layout(pkg):
    D, IO = pkg._lib.PeaRagDesc, pkg._lib.PeaRagBuffers
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)

    def declared(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        out = []
        for decl in body.split(";"):
            decl = re.sub(r"^\s*(const\s+)?(u?int(32|64)_t|float|double)\s*", "", decl.strip())
            out += [n.replace("*", "").split("[")[0].strip() for n in decl.split(",") if n.strip()]
        return out

    names = ["ndim", "B", "dims", "K", "offsets", "max_id", "capacity", "max_edges", "flags"]
    assert [f[0] for f in D._fields_] == names == declared("PeaRagDesc")
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 20, 24, 408, 416, 424, 432] and ctypes.sizeof(D) == 440
    io = ["fragments", "affs", "boundary", "uv", "size", "count", "mean", "bmean", "min", "max", "node_size", "stats"]
    assert [f[0] for f in IO._fields_] == io == declared("PeaRagBuffers") and ctypes.sizeof(IO) == 8 * len(io)


# ---- return codes ------------------------------------------------------------------------------------------------------------------------
BASE = 0x10000000
PTRS = {n: BASE * (i + 1) for i, n in enumerate(("fragments", "affs", "boundary", "uv", "size", "count", "mean", "bmean", "min", "max",
                                                 "node_size", "stats"))}
WORK = 0x70000000 << 4


def desc(pkg, ndim=2, B=2, dims=(1, 37, 53), K=2, offsets=((0, -1, 0), (0, 0, -1)), max_id=40, capacity=256, max_edges=100, flags=0):
    d = pkg._lib.PeaRagDesc()
    d.ndim, d.B, d.K, d.max_id, d.capacity, d.max_edges, d.flags = ndim, B, K, max_id, capacity, max_edges, flags
    d.dims[:] = dims
    for k, o in enumerate(offsets):
        d.offsets[k][:] = o
    return d


def build(pkg, lib, d="default", work=WORK, wbytes=None, io="default", **kw):
    """pea_rag_build on dummy pointers: anything but an early return would fault"""
    ptrs = dict(PTRS)
    for k in list(kw):
        if k in ptrs:
            ptrs[k] = kw.pop(k)
    if isinstance(d, str):
        d = desc(pkg, **kw)
    b = pkg._lib.PeaRagBuffers()
    for k, v in ptrs.items():
        setattr(b, k, v or None)
    if wbytes is None:
        wbytes = lib.pea_rag_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    return lib.pea_rag_build(None if d is None else ctypes.byref(d), None if io is None else ctypes.byref(b),
                             ctypes.c_void_p(work) if work else None, wbytes, None)


BIG_IMAGE = dict(ndim=3, B=1, dims=(2, 1 << 15, 1 << 15))  # Z * Y * X = 2^31: one voxel too many
HUGE = dict(ndim=3, B=2 ** 31 - 1, dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))


def test_validate(pkg, lib):
    v = lambda **kw: lib.pea_rag_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_rag_validate(None) == E_NULL and build(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(flags=3) == OK and v(K=0) == OK and v(max_id=0) == OK and v(B=1, dims=(1, 1, 1)) == OK
    assert v(ndim=3, dims=(5, 19, 23), K=32, offsets=[(-k, k, 0) for k in range(32)]) == OK
    assert v(capacity=64) == OK and v(capacity=2 ** 31) == OK and v(max_edges=1) == OK and v(max_id=2 ** 31 - 1) == OK
    assert v(offsets=((0, -100, 0), (0, 0, 2 ** 31 - 1))) == OK  # any reach: such a channel has no sample
    bad = [dict(flags=4), dict(flags=1 << 31), dict(K=33), dict(K=-1), dict(ndim=1), dict(ndim=4), dict(B=0), dict(dims=(1, 0, 53)),
           dict(dims=(1, 37, -1)), dict(ndim=3, dims=(0, 37, 53)), dict(dims=(2, 37, 53)), dict(offsets=((1, 0, 0), (0, 0, -1))),
           dict(max_id=-1), dict(capacity=0), dict(capacity=32), dict(capacity=96), dict(capacity=2 ** 32), dict(capacity=-64),
           dict(max_edges=0), dict(max_edges=-5)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert build(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_rag_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    assert v(**BIG_IMAGE) == E_UNSUPPORTED and v(**HUGE) == E_UNSUPPORTED
    # the stated order: flags, K, ndim, extents, max_id, capacity, max_edges, then the size of the image
    assert v(flags=8, **BIG_IMAGE) == E_DESC and v(capacity=100, **BIG_IMAGE) == E_DESC and v(max_edges=0, **BIG_IMAGE) == E_DESC
    assert lib.pea_rag_workspace_bytes(None) == 0


def test_workspace_bytes(pkg, lib):
    nb = lambda **kw: lib.pea_rag_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    # a header of 8 words, 32 words per image, 64 bytes and two int32 per (image, slot), three int32 per (image, id)
    assert nb(B=1, capacity=64, max_id=0) == 8 * 8 + 8 * 32 + 64 * 72 + 12 + 4
    assert nb(B=2, capacity=256, max_id=40) == 8 * 8 + 2 * (8 * 32 + 256 * 72 + 41 * 12)
    assert nb(B=3, capacity=1024, max_id=9) == 8 * 8 + 3 * (8 * 32 + 1024 * 72 + 10 * 12)
    # the image, the offsets, max_edges and the flags play no part
    assert nb(dims=(1, 5, 5), K=0, max_edges=7, flags=3) == nb()
    assert nb() % 8 == 0 and nb(capacity=512) > nb() and nb(max_id=41) >= nb()
    assert nb(B=2 ** 31 - 1, capacity=2 ** 31, max_id=2 ** 31 - 1) == SIZE_MAX


def test_build_refusals_before_a_launch_and_their_order(pkg, lib):
    assert build(pkg, lib, io=None) == E_NULL
    for name in ("fragments", "uv", "stats"):
        assert build(pkg, lib, **{name: 0}) == E_NULL, name
    for skew in (1, 2, 3):
        for name in PTRS:
            assert build(pkg, lib, work=0, **{name: PTRS[name] + skew}) == E_ALIGN, (name, skew)
        assert build(pkg, lib, wbytes=0, work=WORK + skew) == E_ALIGN
    for name in ("size", "count", "mean", "bmean", "node_size", "stats"):  # 64-bit elements: 4 is not enough
        assert build(pkg, lib, work=0, **{name: PTRS[name] + 4}) == E_ALIGN, name
    assert build(pkg, lib, work=WORK + 4, wbytes=0) == E_ALIGN
    need = lib.pea_rag_workspace_bytes(ctypes.byref(desc(pkg)))
    assert build(pkg, lib, work=0) == E_WORKSPACE and build(pkg, lib, wbytes=need - 1) == E_WORKSPACE and build(pkg, lib, wbytes=0) == E_WORKSPACE
    # element-aligned pointers and missing optional ones get as far as the workspace
    opt = {n: 0 for n in ("affs", "boundary", "size", "count", "mean", "bmean", "min", "max", "node_size")}
    assert build(pkg, lib, work=0, **opt) == E_WORKSPACE
    assert build(pkg, lib, work=0, fragments=PTRS["fragments"] + 4, affs=PTRS["affs"] + 12, uv=PTRS["uv"] + 4, min=PTRS["min"] + 4) == E_WORKSPACE
    # a grid above 2^31 - 1 workgroups: the edge pass (2^21 images of 2^20 voxels), the sample pass (K times as many), the slot passes,
    # the clear (ids, rows)
    big = dict(wbytes=SIZE_MAX)
    assert build(pkg, lib, B=1 << 21, dims=(1, 1 << 10, 1 << 10), **big) == E_UNSUPPORTED
    assert build(pkg, lib, B=1 << 17, dims=(1, 1 << 10, 1 << 10), K=32, offsets=[(0, 0, 1)] * 32, **big) == E_UNSUPPORTED
    assert build(pkg, lib, B=1 << 17, dims=(1, 1 << 10, 1 << 10), K=32, offsets=[(0, 0, 1)] * 32, affs=0, work=0) == E_WORKSPACE  # no map, no pass
    assert build(pkg, lib, B=1 << 10, capacity=1 << 31, **big) == E_UNSUPPORTED
    assert build(pkg, lib, B=1 << 10, max_id=2 ** 31 - 1, **big) == E_UNSUPPORTED
    assert build(pkg, lib, B=1 << 10, max_edges=2 ** 40, **big) == E_UNSUPPORTED
    # the stated order: descriptor, NULL, alignment, workspace, grid
    assert build(pkg, lib, B=1 << 21, dims=(1, 1 << 10, 1 << 10), work=0) == E_WORKSPACE
    assert build(pkg, lib, B=1 << 21, dims=(1, 1 << 10, 1 << 10), work=0, uv=PTRS["uv"] + 2) == E_ALIGN
    assert build(pkg, lib, B=1 << 21, dims=(1, 1 << 10, 1 << 10), work=0, uv=PTRS["uv"] + 2, stats=0) == E_NULL
    assert build(pkg, lib, work=0, uv=PTRS["uv"] + 2, stats=0, flags=4) == E_DESC
    assert build(pkg, lib, work=0, stats=0, **BIG_IMAGE) == E_UNSUPPORTED  # what validate refuses comes first


def test_init_and_project_refusals(lib):
    init = lambda p, n: lib.pea_rag_workspace_init(ctypes.c_void_p(p) if p else None, n, None)
    assert init(0, 64) == E_NULL and init(WORK + 4, 64) == E_ALIGN and init(WORK, 56) == E_WORKSPACE and init(WORK, 68) == E_WORKSPACE
    F, N, SEG, BAD = (ctypes.c_void_p(BASE * i) for i in (1, 2, 3, 4))
    p = lambda n=100, f=F, nl=N, m=7, s=SEG, bad=BAD: lib.pea_rag_project(n, f, nl, m, s, bad, None)
    assert p(n=0) == E_DESC and p(m=0) == E_DESC and p(n=-1, f=None) == E_DESC
    assert p(f=None) == E_NULL and p(nl=None) == E_NULL and p(s=None) == E_NULL
    for skew in (1, 2, 3):
        assert p(f=ctypes.c_void_p(BASE + skew)) == E_ALIGN and p(s=ctypes.c_void_p(3 * BASE + skew)) == E_ALIGN
        assert p(nl=ctypes.c_void_p(2 * BASE + skew)) == E_ALIGN
    assert p(bad=ctypes.c_void_p(4 * BASE + 4)) == E_ALIGN
    assert p(n=2 ** 43, bad=None) == E_UNSUPPORTED and p(n=2 ** 43, s=None) == E_NULL


# ---- the costs -------------------------------------------------------------------------------------------------------------------------------
def test_probs_to_costs_is_the_references_formula(pkg):
    p = np.concatenate([np.linspace(0, 1, 101), np.random.default_rng(1).random(50)])
    for beta in (0.5, 0.25, 0.9):
        got = pkg.probs_to_costs(p, beta)
        assert got.dtype == np.float64 and np.allclose(got, probs_to_costs_f64(p, beta), rtol=1e-15, atol=1e-15)
        assert np.array_equal(pkg.probs_to_costs(p.astype(np.float32), beta), probs_to_costs_f64(p.astype(np.float32), beta))
    assert pkg.probs_to_costs(np.array([0.5]))[0] == pytest.approx(0.0, abs=1e-15)
    assert inspect.signature(pkg.probs_to_costs).parameters["beta"].default == 0.5
    got = pkg.probs_to_costs(p[:0])
    assert got.shape == (0,)
    sizes = np.arange(1, len(p) + 1)
    want = probs_to_costs_f64(p) * (sizes / sizes.max())
    assert np.allclose(pkg.transform_probabilities_to_costs(p, edge_sizes=sizes), want, rtol=1e-15, atol=0)
    assert np.allclose(pkg.transform_probabilities_to_costs(p, edge_sizes=7 * sizes), want, rtol=1e-15, atol=0)  # a constant factor cancels
    want2 = probs_to_costs_f64(p, 0.3) * (sizes / sizes.max()) ** 2.0
    assert np.allclose(pkg.transform_probabilities_to_costs(p, 0.3, sizes, 2.0), want2, rtol=1e-15, atol=0)
    assert np.array_equal(pkg.transform_probabilities_to_costs(p), pkg.probs_to_costs(p))
    with pytest.raises(ValueError, match="shape"):
        pkg.transform_probabilities_to_costs(p, edge_sizes=sizes[:-1])
    doc = pkg.transform_probabilities_to_costs.__doc__
    assert "elf" in doc and "nifty" in doc and "not checked" in doc


# ---- the Python entry points ---------------------------------------------------------------------------------------------------------------
def test_python_entry_points(pkg):
    for name in pkg.RAG_EXPORTS:
        assert hasattr(pkg, name), name
    sig = inspect.signature(pkg.region_adjacency)
    assert list(sig.parameters)[:4] == ["fragments", "affs", "offsets", "boundary"]
    for name, default in (("one_minus", False), ("ignore_zero", False), ("max_id", None), ("capacity", None), ("max_edges", None)):
        assert sig.parameters[name].default is default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert "round trip" in pkg.region_adjacency.__doc__ and "graphed" in pkg.region_adjacency.__doc__
    for name in ("n_nodes", "uv", "sizes", "counts", "mean", "min", "max", "boundary_mean", "node_sizes", "stats", "costs"):
        assert name in pkg.RegionAdjacency.__doc__ or hasattr(pkg.RegionAdjacency, name), name
    assert list(inspect.signature(pkg.RegionAdjacency.costs).parameters)[1:] == ["beta", "weighting_exponent"]
    assert list(inspect.signature(pkg.mc_baseline).parameters) == ["affs", "fragments", "solver"]
    assert list(inspect.signature(pkg.multicut_multi).parameters) == ["affs", "offsets", "fragments", "solver"]
    assert list(inspect.signature(pkg.project_node_labels).parameters)[:2] == ["fragments", "node_labels"]
    from importlib import import_module
    rag = import_module(pkg.__name__ + ".harness.rag")
    assert [rag.default_capacity(s) for s in (1, 37 * 53, 520 * 696, 100 * 1024 * 1024)] == [256, 256, 16384, 1 << 22]

    f = torch.zeros(5, 6, 7, dtype=torch.int32)
    a = torch.zeros(3, 5, 6, 7)
    if not torch.cuda.is_available():
        for call in (lambda: pkg.region_adjacency(f), lambda: pkg.region_adjacency(f.numpy(), a.numpy(), LOCAL3, a[0].numpy(), max_id=3),
                     lambda: pkg.project_node_labels(f, torch.zeros(3, dtype=torch.int64)),
                     lambda: pkg.mc_baseline(a, f, solver=stub_solver), lambda: pkg.multicut_multi(a.numpy(), LOCAL3, f.numpy(), stub_solver)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    for bad in (torch.zeros(7, dtype=torch.int32), torch.zeros(1, 2, 3, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"\[Y, X\] or \[Z, Y, X\]"):
            pkg.region_adjacency(bad)
    with pytest.raises(ValueError, match=r"\[B, Y, X\] or \[B, Z, Y, X\]"):
        pkg.region_adjacency(torch.zeros(6, 7, dtype=torch.int32), batched=True)
    with pytest.raises(ValueError, match="empty"):
        pkg.region_adjacency(torch.zeros(0, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs offsets"):
        pkg.region_adjacency(f, a)
    with pytest.raises(ValueError, match="offsets without affs"):
        pkg.region_adjacency(f, offsets=LOCAL3)
    with pytest.raises(ValueError, match="does not go with"):
        pkg.region_adjacency(f, a[:, :4], LOCAL3)
    with pytest.raises(ValueError, match="does not go with"):
        pkg.region_adjacency(f, a[0], LOCAL3)
    for offs in (LOCAL3[:2], [[0, 1]] * 3):
        with pytest.raises(ValueError, match="offsets must hold"):
            pkg.region_adjacency(f, a, offs)
    with pytest.raises(ValueError, match="1 .. 32"):
        pkg.region_adjacency(f, torch.zeros(33, 5, 6, 7), [[0, 0, 1]] * 33)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.region_adjacency(f, boundary=a[0, :4])
    with pytest.raises(TypeError):
        pkg.region_adjacency([[0, 1]])
    with pytest.raises(TypeError):
        pkg.region_adjacency(f, a.tolist(), LOCAL3)
    with pytest.raises(ValueError, match="vector"):
        pkg.project_node_labels(f, torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        pkg.project_node_labels(f, [1, 2])


def test_mc_baseline_arguments_and_boundary_map(pkg):
    from importlib import import_module
    lmc = import_module(pkg.__name__ + ".utils.lmc")
    assert pkg.lmc is lmc and lmc.mc_baseline is pkg.mc_baseline and lmc.probs_to_costs is pkg.probs_to_costs
    assert lmc.OFFSETS_3D == [[-1, 0, 0], [0, -1, 0], [0, 0, -1]] and lmc.OFFSETS_2D == [[-1, 0], [0, -1]]
    assert "required" in lmc.__doc__ and "solver" in lmc.__doc__ and "nifty" in lmc.__doc__
    f, a, _ = volume("3d")
    f, a = f[0], a[0, :3]
    # the boundary map: the reference's np.maximum(affs[1], affs[2]) of affs = 1 - affs; channels 0, 1 of an image
    inv = 1 - a
    want = np.maximum(inv[1], inv[2])
    got = lmc.boundary_map(a)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want)
    got = lmc.boundary_map(torch.from_numpy(a.copy()))
    assert isinstance(got, torch.Tensor) and np.array_equal(got.numpy(), want)
    a2 = a[:2, 0]
    assert np.array_equal(lmc.boundary_map(a2), np.maximum(1 - a2[0], 1 - a2[1])) and lmc.boundary_channels(2) == (0, 1)
    # arguments, before any device is looked for
    with pytest.raises(TypeError, match="fragments is required"):
        pkg.mc_baseline(a)
    with pytest.raises(TypeError, match="fragments is required"):
        pkg.multicut_multi(a, solver=stub_solver)
    with pytest.raises(TypeError, match="numpy array or a torch.Tensor"):
        pkg.mc_baseline(a.tolist(), f, stub_solver)
    with pytest.raises(ValueError, match=r"\[Y, X\] or \[Z, Y, X\]"):
        pkg.mc_baseline(a, f[None], stub_solver)
    with pytest.raises(ValueError, match="does not go with"):
        pkg.mc_baseline(a[:, :3], f, stub_solver)
    with pytest.raises(ValueError, match="needs as many offsets"):
        pkg.mc_baseline(a[:2], f, stub_solver)  # three offsets, two channels
    with pytest.raises(ValueError, match="needs as many offsets"):
        pkg.multicut_multi(a, [[-1, 0, 0]], f, stub_solver)
    with pytest.raises(ValueError, match="in-plane channels"):
        pkg.multicut_multi(a[:1], [[-1, 0, 0]], f, stub_solver)
    # the default solver says what is missing
    try:
        import nifty  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="nifty"):
            lmc.nifty_multicut(3, np.array([[0, 1]]), np.array([1.0]))
