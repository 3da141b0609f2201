"""CPU: the watershed fragments (include/pea_ws.h) -- the numpy / scipy restatement tests/ws_reference.py, which the GPU tests compare
the kernels with, is held to properties that need no second implementation of it: the Kruskal flood to the minimax property by a
multi-source Dijkstra with max as the path cost, and to scipy.ndimage.watershed_ift on uint8 planes whose cut has no tie that the two
break differently; the plateau maxima and the distance transform to hand-written expectations.  The header and the library agree on
the five new symbols, the ctypes mirror has the header's layout, pea_ws_validate and the two workspace queries answer as the header
says, every refusal of pea_ws_seeds and pea_ws_flood is reached before anything is launched and in the header's order (dummy device
pointers, no GPU), and the Python entry points say what is wrong with a call before they look for a device."""
import ctypes
import heapq
import inspect
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import ws_reference as R
from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
STACK_IDS, FIELD = 1, 2
NEW = ["pea_ws_flood", "pea_ws_flood_workspace_bytes", "pea_ws_seeds", "pea_ws_seeds_workspace_bytes", "pea_ws_validate"]
SIZE_MAX = 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatement: the flood ----------------------------------------------------------------------------------------------------------
def minimax_to_seeds(h, seeds):
    """[Y, X] -> int64 [Y, X]: the smallest, over all paths from the pixel to any seeded pixel, of the largest edge weight
    max(ord(h[p]), ord(h[q])) on the path (-1 for a seeded pixel: the empty path): a multi-source Dijkstra with max as the path cost"""
    Y, X = h.shape
    o = R.ord32(h).astype(np.int64)
    cost = np.full((Y, X), np.iinfo(np.int64).max, np.int64)
    heap = []
    for y, x in zip(*np.nonzero(seeds)):
        cost[y, x] = -1
        heap.append((-1, int(y), int(x)))
    heapq.heapify(heap)
    while heap:
        c, y, x = heapq.heappop(heap)
        if c > cost[y, x]:
            continue
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < Y and 0 <= nx < X:
                nc = max(c, int(max(o[y, x], o[ny, nx])))
                if nc < cost[ny, nx]:
                    cost[ny, nx] = nc
                    heapq.heappush(heap, (nc, ny, nx))
    return cost


def forest_path_maxima(shape, seeds, taken):
    """the largest edge weight on every pixel's path to the seeded pixel of its tree, through the taken edges only"""
    Y, X = shape
    adj = [[] for _ in range(Y * X)]
    for p, q, w in taken:
        adj[p].append((q, w))
        adj[q].append((p, w))
    out = np.full(Y * X, np.iinfo(np.int64).max, np.int64)
    stack = [int(i) for i in np.nonzero(np.asarray(seeds).ravel())[0]]
    for i in stack:
        out[i] = -1
    while stack:
        p = stack.pop()
        for q, w in adj[p]:
            if out[q] == np.iinfo(np.int64).max:
                out[q] = max(out[p], w)
                stack.append(q)
    return out.reshape(Y, X)


def flood_planes():
    """(name, h float32 [Y, X], seeds int32 [Y, X]): integer heights with ties everywhere, floats, signed zeros, walls, a ramp"""
    rng = np.random.default_rng(77)
    out = []
    for t in range(8):
        Y, X = int(rng.integers(1, 14)), int(rng.integers(1, 19))
        h = rng.integers(0, 4, (Y, X)).astype(np.float32) if t % 2 == 0 else rng.standard_normal((Y, X)).astype(np.float32)
        s = np.zeros((Y, X), np.int32)
        for i in range(int(rng.integers(1, 6))):
            s[rng.integers(0, Y), rng.integers(0, X)] = i + 1
        out.append(("random %d" % t, h, s))
    h = rng.integers(-1, 2, (9, 11)).astype(np.float32) * np.float32(0.0)  # +0.0 and -0.0
    h[4] = np.inf
    s = np.zeros((9, 11), np.int32)
    s[0, 0], s[8, 10], s[8, 0] = 3, 1, 2
    out.append(("zeros and a wall", h, s))
    s = np.zeros((8, 8), np.int32)
    s[0, 0] = 1
    out.append(("ramp", np.arange(64, dtype=np.float32).reshape(8, 8), s))
    return out


def test_kruskal_has_the_minimax_property():
    for name, h, s in flood_planes():
        labels, taken = R.kruskal_flood(h, s, forest=True)
        assert (labels > 0).all() and set(np.unique(labels)) <= set(np.unique(s[s > 0]).tolist()), name
        assert np.array_equal(labels[s > 0], s[s > 0]), name
        # a spanning forest: one tree per seeded pixel, every other pixel hooked once
        assert len(taken) == h.size - int((s > 0).sum()), name
        assert np.array_equal(forest_path_maxima(h.shape, s, taken), minimax_to_seeds(h, s)), name


def test_ord32_is_order_preserving():
    v = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 2.0, np.inf], np.float32)
    o = R.ord32(v).astype(np.int64)
    assert (np.diff(o) > 0).all()
    assert R.ord32(np.float32(0.0)) == 0x80000000 and R.ord32(np.float32(-0.0)) == 0x7FFFFFFF


def monotone_basins(seed, transpose):
    """a uint8 plane of strictly monotone basins, one row (or, transposed, one column: scipy's watershed_ift joins the last pixel of
    a row to the first of the next, so a plane of several rows leaks between its side borders): a profile that rises from each seed
    with growing steps up to a one-pixel ridge whose two steps are larger still.  watershed_ift costs a path by the largest height DIFFERENCE on it,
    the header by the largest height; on slopes whose steps grow with the height the two orders agree.  They differ on the ridge pixel
    alone: by heights it ties between its two neighbours, and the header's key gives it to the edge of smaller index, the LEFT one; by
    differences it goes to the HIGHER neighbour.  The profile makes the left neighbour of every ridge the higher one, so the cut has no
    tie that the two break differently."""
    rng = np.random.default_rng(seed)

    def slope(n):  # heights 1 .. n steps above a seed, the steps growing by one
        first = int(rng.integers(1, 4))
        return np.cumsum(np.arange(first, first + n)).tolist()

    nb = int(rng.integers(2, 5))
    prof, cols = [0], [0]
    for b in range(1, nb):
        up, down = slope(int(rng.integers(2, 7))), slope(int(rng.integers(2, 7)))
        while up[-1] <= down[-1]:
            up.append(up[-1] + (up[-1] - up[-2]) + 1)
        ridge = up[-1] + max(up[-1] - up[-2], down[-1] - down[-2]) + 1
        prof += up + [ridge] + down[::-1] + [0]
        cols.append(len(prof) - 1)
    prof = np.array(prof)
    assert prof.max() <= 255
    h = prof.astype(np.uint8)[None]
    m = np.zeros(h.shape, np.int16)
    for i, c in enumerate(cols):
        m[0, c] = i + 1
    return (h.T.copy(), m.T.copy()) if transpose else (h, m)


def test_kruskal_against_watershed_ift():
    for seed in range(24):
        h, m = monotone_basins(seed, transpose=seed % 2 == 1)
        want = ndi.watershed_ift(h, m)
        got = R.kruskal_flood(h.astype(np.float32), m.astype(np.int32))
        assert len(np.unique(want)) == int(m.max()) and np.array_equal(got, want), (seed, h.ravel(), got.ravel(), want.ravel())


def test_flood_reference_size_filter_and_numbering():
    # a row of three basins, the middle one a single low pixel between walls: seeds 5, 9 (one pixel), 7
    h = np.array([[0, 0, 0, 9, 1, 9, 0, 0, 0, 0]], np.float32)
    s = np.array([[5, 0, 0, 0, 9, 0, 0, 0, 7, 0]], np.int32)
    lab, cnt, zeros = R.flood_reference(h[None], s[None])
    assert lab[0].tolist() == [[1, 1, 1, 1, 3, 3, 2, 2, 2, 2]] and cnt.tolist() == [[3, 3]] and zeros.tolist() == [0]  # ascending seed id
    lab, cnt, _ = R.flood_reference(h[None], s[None], min_size=3)
    # 9's two pixels go to a neighbour: every edge of the two walls weighs 9, and the edges of smaller index come first
    assert lab[0].tolist() == [[1, 1, 1, 1, 1, 1, 2, 2, 2, 2]] and cnt.tolist() == [[3, 2]]
    lab, cnt, _ = R.flood_reference(h[None], s[None], min_size=5)
    assert cnt.tolist() == [[3, 3]] and lab[0].tolist() == [[1, 1, 1, 1, 3, 3, 2, 2, 2, 2]]  # none would remain: the first flood
    both = np.concatenate([h[None], h[None], h[None]]), np.concatenate([s[None], np.zeros_like(s)[None], s[None]])
    lab, cnt, zeros = R.flood_reference(*both, stack_ids=True)
    assert lab[2].tolist() == [[4, 4, 4, 4, 6, 6, 5, 5, 5, 5]] and not lab[1].any() and zeros.tolist() == [0, 10, 0] and cnt[1].tolist() == [0, 0]
    lab, _, _ = R.flood_reference(both[0], np.where(both[1] == 9, 10 ** 6, both[1]))  # an id above Y * X is no seed
    assert lab[0].tolist() == [[1, 1, 1, 1, 1, 1, 2, 2, 2, 2]]


# ---- the restatement: distance transform and seeds -------------------------------------------------------------------------------------------
def test_dt2_and_plateau_maxima_by_hand():
    b = np.zeros((1, 4, 5), np.float32)
    assert (R.dt2_reference(b, 0.5) == 41).all()
    b[0, 0, 0] = 1
    yy, xx = np.mgrid[0:4, 0:5]
    assert np.array_equal(R.dt2_reference(b, 0.5)[0], yy ** 2 + xx ** 2)
    assert np.array_equal(R.dt2_reference(b, 1.0)[0], np.full((4, 5), 41))  # > threshold, not >=
    # a diagonal two-pixel plateau: one maximum in the 8-neighbourhood, two seeds in the 4-; not a maximum in the 4-neighbourhood
    # sense either way round is irrelevant: each pixel is then a plateau of its own and a maximum
    d = np.array([[1, 1, 1, 1], [1, 5, 1, 1], [1, 1, 5, 1], [1, 1, 1, 1]], np.float32)
    assert R.plateau_maxima(d, 2).astype(int).tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert R.seeds_reference(d[None], 2, 1)[0][0].tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]]
    assert R.seeds_reference(d[None], 2, 2)[1].tolist() == [1]
    # a plateau with one higher neighbour is no maximum; a flat plane is one; a maximum on the border counts
    d = np.array([[3, 3, 3, 4], [3, 3, 3, 0], [0, 0, 0, 0], [7, 0, 0, 0]], np.float32)
    assert R.plateau_maxima(d, 2).astype(int).tolist() == [[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]]
    assert R.plateau_maxima(np.full((3, 3), 2.0), 1).all() and R.seeds_reference(np.zeros((1, 3, 3)))[1].tolist() == [1]
    d = np.array([[0.0, -0.0], [-0.0, 0.0]], np.float32)  # signed zeros are one plateau
    assert R.plateau_maxima(d, 1).all()


def test_gauss_reference_is_the_headers_filter():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 9, 13))
    for sigma in (0.5, 1.0, 2.0):
        r = R.gauss_radius(sigma)
        w = np.exp(-0.5 * np.arange(-r, r + 1) ** 2 / float(np.float32(sigma)) ** 2)
        w /= w.sum()
        pad = np.pad(x[0], r, mode="reflect")  # numpy's 'reflect' is scipy's 'mirror'
        rows = sum(w[k] * pad[r:-r, k:k + 13] for k in range(2 * r + 1))
        pad = np.pad(rows, ((r, r), (0, 0)), mode="reflect")
        want = sum(w[k] * pad[k:k + 9] for k in range(2 * r + 1))
        assert np.abs(R.gauss_reference(x, sigma)[0] - want).max() < 1e-13, sigma
    assert R.gauss_radius(2.0) == 6 and R.gauss_radius(0.5) == 2 and R.gauss_radius(10.5) == 32
    assert np.array_equal(R.gauss_reference(x, 0.0), x)


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_five_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_ws.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_WS) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src
    assert re.search(r"#define\s+PEA_WS_STACK_IDS\s+1u\b", src) and re.search(r"#define\s+PEA_WS_FIELD\s+2u\b", src)
    assert re.search(r"#define\s+PEA_WS_MAX_RADIUS\s+32\b", src)
    assert (pkg._lib.WS_STACK_IDS, pkg._lib.WS_FIELD, pkg._lib.WS_MAX_RADIUS) == (STACK_IDS, FIELD, 32)
    for cite in ("distance_transform_watershed", "fragment.py", "NaN", "every loop still ends", "not vigra's"):
        assert cite in src, cite
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert not set(NEW) & set(pkg._lib.EXPORTS)


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaWsDesc
    names = ["N", "Y", "X", "threshold", "sigma_seeds", "sigma_weights", "alpha", "maxima_connectivity", "seed_connectivity", "min_size", "flags"]
    assert ctypes.sizeof(D) == 11 * 4 and [f[0] for f in D._fields_] == names
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_ws.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaWsDesc \{(.*?)\} PeaWsDesc;", src, flags=re.S).group(1)
    declared = [n for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(u?int32_t|float)", "", decl.strip()).replace(" ", "").split(",")]
    assert declared == names
    assert [getattr(D, n).offset for n in names] == list(range(0, 44, 4))


# ---- return codes ------------------------------------------------------------------------------------------------------------------------
PTR = {n: 0x10000000 * (i + 1) for i, n in enumerate(("boundary", "dt2", "dts", "hmap", "seeds", "counts", "work", "labels", "stats"))}


def desc(pkg, N=3, Y=37, X=53, threshold=0.25, sigma_seeds=2.0, sigma_weights=2.0, alpha=0.9, maxima_connectivity=2, seed_connectivity=1,
         min_size=0, flags=0):
    d = pkg._lib.PeaWsDesc()
    d.N, d.Y, d.X, d.threshold, d.sigma_seeds, d.sigma_weights, d.alpha = N, Y, X, threshold, sigma_seeds, sigma_weights, alpha
    d.maxima_connectivity, d.seed_connectivity, d.min_size, d.flags = maxima_connectivity, seed_connectivity, min_size, flags
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def seeds_call(pkg, lib, d="default", wbytes=None, **kw):
    """pea_ws_seeds on dummy pointers: anything but an early return would fault"""
    p = dict(PTR)
    for k in list(kw):
        if k in p:
            p[k] = kw.pop(k)
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = lib.pea_ws_seeds_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    return lib.pea_ws_seeds(None if d is None else ctypes.byref(d), vp(p["boundary"]), vp(p["dt2"]), vp(p["dts"]), vp(p["hmap"]), vp(p["seeds"]),
                            vp(p["counts"]), vp(p["work"]), wbytes, None)


def flood_call(pkg, lib, d="default", wbytes=None, **kw):
    p = dict(PTR)
    for k in list(kw):
        if k in p:
            p[k] = kw.pop(k)
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = lib.pea_ws_flood_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    return lib.pea_ws_flood(None if d is None else ctypes.byref(d), vp(p["hmap"]), vp(p["seeds"]), vp(p["labels"]), vp(p["counts"]), vp(p["stats"]),
                            vp(p["work"]), wbytes, None)


BIG_PLANE = dict(N=1, Y=1 << 15, X=1 << 15)   # Y * X = 2^30: one pixel too many for the edge index
HUGE = dict(N=2 ** 31 - 1, Y=2 ** 31 - 1, X=2 ** 31 - 1)


def test_validate(pkg, lib):
    v = lambda **kw: lib.pea_ws_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_ws_validate(None) == E_NULL and seeds_call(pkg, lib, d=None) == E_NULL and flood_call(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(N=1, Y=1, X=1) == OK and v(sigma_seeds=0.0, sigma_weights=0.0, alpha=0.0) == OK and v(alpha=1.0) == OK
    assert v(maxima_connectivity=1, seed_connectivity=2, min_size=2 ** 31 - 1, flags=STACK_IDS | FIELD) == OK
    assert v(**HUGE) == OK and v(**BIG_PLANE) == OK and v(sigma_seeds=100.0) == OK and v(threshold=-3.0) == OK
    bad = [dict(N=0), dict(Y=0), dict(X=0), dict(N=-1), dict(Y=-5),
           dict(threshold=float("nan")), dict(threshold=float("inf")), dict(sigma_seeds=-1.0), dict(sigma_seeds=float("nan")),
           dict(sigma_weights=-0.5), dict(sigma_weights=float("inf")), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")),
           dict(maxima_connectivity=0), dict(maxima_connectivity=3), dict(seed_connectivity=0), dict(seed_connectivity=3),
           dict(min_size=-1), dict(flags=4), dict(flags=1 << 31)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert seeds_call(pkg, lib, **kw) == E_DESC and flood_call(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_ws_seeds_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
        assert lib.pea_ws_flood_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    assert lib.pea_ws_seeds_workspace_bytes(None) == 0 and lib.pea_ws_flood_workspace_bytes(None) == 0


def al8(x):
    return (x + 7) // 8 * 8


def test_workspace_bytes(pkg, lib):
    ns = lambda **kw: lib.pea_ws_seeds_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    nf = lambda **kw: lib.pea_ws_flood_workspace_bytes(ctypes.byref(desc(pkg, **kw)))

    def cc_bytes(N, Y, X):
        d = pkg._lib.PeaCcDesc()
        d.ndim, d.B, d.in_type, d.connectivity, d.min_size, d.flags = 2, N, 1, 1, 0, 0
        d.dims[:] = [1, Y, X]
        return lib.pea_cc_workspace_bytes(ctypes.byref(d))

    for N, Y, X in ((1, 1, 1), (3, 70, 150), (1, 64, 64), (2, 1, 37)):
        S = Y * X
        # flood: root, par, seed (4 bytes a pixel), the slots (8), a counter per id 0 .. S, 64 words per plane
        assert nf(N=N, Y=Y, X=X) == 3 * al8(4 * N * S) + 8 * N * S + al8(4 * N * (S + 1)) + 256 * N
        # seeds: six images of 4 bytes a pixel, a flag per id 0 .. S, the mask, four words per plane, pea_cc_label's workspace
        assert ns(N=N, Y=Y, X=X) == 6 * al8(4 * N * S) + al8(4 * N * (S + 1)) + al8(N * S) + al8(16 * N) + cc_bytes(N, Y, X)
        assert ns(N=N, Y=Y, X=X) % 8 == 0 and nf(N=N, Y=Y, X=X) % 8 == 0
    # nothing but the extents changes them
    assert ns(sigma_seeds=0.0, alpha=0.1, maxima_connectivity=1, min_size=9, flags=FIELD) == ns()
    assert nf(min_size=9, flags=STACK_IDS) == nf()
    assert ns(**HUGE) == SIZE_MAX and nf(**HUGE) == SIZE_MAX
    assert nf(**BIG_PLANE) == 20 * 2 ** 30 + al8(4 * (2 ** 30 + 1)) + 256


def test_seeds_refusals_before_a_launch_and_their_order(pkg, lib):
    assert seeds_call(pkg, lib, boundary=0) == E_NULL and seeds_call(pkg, lib, seeds=0) == E_NULL and seeds_call(pkg, lib, counts=0) == E_NULL
    # the optional outputs may be NULL; with PEA_WS_FIELD dt2 and hmap must be
    assert seeds_call(pkg, lib, flags=FIELD) == E_NULL and seeds_call(pkg, lib, flags=FIELD, dt2=0) == E_NULL
    assert seeds_call(pkg, lib, flags=FIELD, hmap=0) == E_NULL
    for skew in (1, 2, 3):
        for name in ("boundary", "dt2", "dts", "hmap", "seeds", "counts", "work"):
            assert seeds_call(pkg, lib, **{name: PTR[name] + skew}) == E_ALIGN, (name, skew)
    assert seeds_call(pkg, lib, work=PTR["work"] + 4) == E_ALIGN  # the workspace to 8 bytes
    need = lib.pea_ws_seeds_workspace_bytes(ctypes.byref(desc(pkg)))
    assert seeds_call(pkg, lib, work=0) == E_WORKSPACE and seeds_call(pkg, lib, wbytes=need - 1) == E_WORKSPACE and seeds_call(pkg, lib, wbytes=0) == E_WORKSPACE
    # PEA_E_UNSUPPORTED: the plane, the squared distance, the radius of a Gaussian that is used
    assert seeds_call(pkg, lib, **BIG_PLANE) == E_UNSUPPORTED and seeds_call(pkg, lib, wbytes=SIZE_MAX, **HUGE) == E_UNSUPPORTED
    assert seeds_call(pkg, lib, N=1, Y=1, X=1 << 16) == E_UNSUPPORTED          # Y^2 + X^2 = 2^32 + 1
    assert seeds_call(pkg, lib, N=1, Y=1, X=1 << 16, sigma_seeds=0.0, hmap=0) == E_UNSUPPORTED
    assert seeds_call(pkg, lib, sigma_seeds=10.9) == E_UNSUPPORTED              # radius 33
    assert seeds_call(pkg, lib, sigma_weights=10.9) == E_UNSUPPORTED
    for huge in (1e9, 7.2e8, 3e38):  # 3 sigma + 0.5 does not fit an int: decided before the conversion, nothing is launched
        assert lib.pea_ws_validate(ctypes.byref(desc(pkg, sigma_seeds=huge, sigma_weights=huge))) == OK
        assert seeds_call(pkg, lib, sigma_seeds=huge) == E_UNSUPPORTED and seeds_call(pkg, lib, sigma_weights=huge) == E_UNSUPPORTED, huge
        assert seeds_call(pkg, lib, sigma_seeds=huge, flags=FIELD, dt2=0, hmap=0) == E_UNSUPPORTED, huge
        assert seeds_call(pkg, lib, N=1, Y=4096, X=4096, sigma_seeds=huge, sigma_weights=huge) == E_UNSUPPORTED, huge
    assert seeds_call(pkg, lib, Y=6) == E_UNSUPPORTED and seeds_call(pkg, lib, X=6) == E_UNSUPPORTED  # radius 6 >= min(Y, X)
    assert seeds_call(pkg, lib, N=1, Y=1, X=1) == E_UNSUPPORTED
    assert seeds_call(pkg, lib, N=1 << 21, Y=1 << 15, X=1, sigma_seeds=0.0, sigma_weights=0.0) == E_UNSUPPORTED  # 2^31 tiles
    # the stated order: descriptor, NULL, alignment, workspace, size
    assert seeds_call(pkg, lib, work=0, **BIG_PLANE) == E_WORKSPACE and seeds_call(pkg, lib, wbytes=8, **BIG_PLANE) == E_WORKSPACE
    assert seeds_call(pkg, lib, work=0, dts=PTR["dts"] + 2, **BIG_PLANE) == E_ALIGN
    assert seeds_call(pkg, lib, seeds=0, dts=PTR["dts"] + 2, work=0, **BIG_PLANE) == E_NULL
    assert seeds_call(pkg, lib, boundary=0, seeds=0, counts=0, work=0, flags=8) == E_DESC
    # a Gaussian that is not used is not looked at: sigma_weights without hmap
    assert seeds_call(pkg, lib, sigma_weights=10.9, hmap=0, work=0) == E_WORKSPACE


def test_flood_refusals_before_a_launch_and_their_order(pkg, lib):
    for name in ("hmap", "seeds", "labels", "counts", "stats"):
        assert flood_call(pkg, lib, **{name: 0}) == E_NULL, name
    for skew in (1, 2, 3):
        for name in ("hmap", "seeds", "labels", "counts", "stats", "work"):
            assert flood_call(pkg, lib, **{name: PTR[name] + skew}) == E_ALIGN, (name, skew)
    assert flood_call(pkg, lib, work=PTR["work"] + 4) == E_ALIGN
    need = lib.pea_ws_flood_workspace_bytes(ctypes.byref(desc(pkg)))
    assert flood_call(pkg, lib, work=0) == E_WORKSPACE and flood_call(pkg, lib, wbytes=need - 1) == E_WORKSPACE
    assert flood_call(pkg, lib, **BIG_PLANE) == E_UNSUPPORTED and flood_call(pkg, lib, wbytes=SIZE_MAX, **HUGE) == E_UNSUPPORTED
    assert flood_call(pkg, lib, N=1 << 13, Y=1 << 15, X=(1 << 15) - 1) == E_UNSUPPORTED  # more than 2^31 - 1 workgroups
    # stacked ids are int32 sums of kept counts, at most one per pixel: N * Y * X < 2^31 under PEA_WS_STACK_IDS only
    assert flood_call(pkg, lib, N=4, Y=1 << 15, X=(1 << 15) - 1, work=0) == E_WORKSPACE
    assert flood_call(pkg, lib, N=2, Y=1 << 15, X=1 << 14, flags=STACK_IDS, work=0) == E_WORKSPACE   # 2^30 pixels: served
    assert flood_call(pkg, lib, N=4, Y=1 << 15, X=1 << 14, flags=STACK_IDS) == E_UNSUPPORTED         # 2^31
    assert flood_call(pkg, lib, N=4, Y=1 << 15, X=1 << 14, flags=STACK_IDS, work=0) == E_WORKSPACE   # the stated order
    # the flood does not look at the seeds' fields beyond their validity: a radius it never uses
    assert flood_call(pkg, lib, sigma_seeds=50.0, work=0) == E_WORKSPACE
    assert flood_call(pkg, lib, work=0, **BIG_PLANE) == E_WORKSPACE
    assert flood_call(pkg, lib, work=0, labels=PTR["labels"] + 2, **BIG_PLANE) == E_ALIGN
    assert flood_call(pkg, lib, hmap=0, labels=PTR["labels"] + 2, work=0, **BIG_PLANE) == E_NULL
    assert flood_call(pkg, lib, hmap=0, seeds=0, labels=0, counts=0, stats=0, work=0, min_size=-1) == E_DESC


# ---- the Python entry points ---------------------------------------------------------------------------------------------------------------
def test_python_entry_points(pkg):
    """no CPU fallback; a wrong shape, dtype or range is said before the device is looked at"""
    for name in pkg.WS_EXPORTS:
        assert hasattr(pkg, name), name
    from importlib import import_module
    frag = import_module(pkg.__name__ + ".utils.fragment")
    assert pkg.fragment is frag
    for name in ("elf_watershed", "watershed", "relabel", "remove_small"):
        assert callable(getattr(frag, name)), name
    sig = inspect.signature(pkg.watershed_seeds)
    assert list(sig.parameters)[:5] == ["boundary", "threshold", "sigma_seeds", "sigma_weights", "alpha"]
    assert [sig.parameters[n].default for n in ("sigma_seeds", "sigma_weights", "alpha", "maxima_connectivity", "seed_connectivity")] == [2., 2., .9, 2, 1]
    sig = inspect.signature(pkg.seeded_watershed)
    assert list(sig.parameters) == ["hmap", "seeds", "min_size", "stack_ids"] and [p.default for p in sig.parameters.values()][2:] == [0, False]
    sig = inspect.signature(pkg.distance_transform_watershed)  # elf's name, argument order and defaults
    assert list(sig.parameters)[:6] == ["boundary", "threshold", "sigma_seeds", "sigma_weights", "min_size", "alpha"]
    assert [sig.parameters[n].default for n in ("sigma_weights", "min_size", "alpha")] == [2., 100, .9]
    assert sig.parameters["threshold"].default is inspect.Parameter.empty and sig.parameters["sigma_seeds"].default is inspect.Parameter.empty

    b = torch.zeros(2, 40, 50)
    s = torch.zeros(2, 40, 50, dtype=torch.int32)
    if not torch.cuda.is_available():
        for call in (lambda: pkg.watershed_seeds(b, .25), lambda: pkg.watershed_seeds(b[0], .25, 0., 0.), lambda: pkg.plateau_maxima(b),
                     lambda: pkg.seeded_watershed(b, s), lambda: pkg.seeded_watershed(b[0], s[0], 5, True),
                     lambda: pkg.distance_transform_watershed(b, .25, 2.), lambda: pkg.distance_transform_watershed(b.numpy(), .25, 2.),
                     lambda: frag.elf_watershed(torch.zeros(3, 2, 40, 50)), lambda: frag.watershed(np.zeros((3, 2, 40, 50), np.float32), "grid"),
                     lambda: pkg.mc_baseline(torch.zeros(3, 2, 40, 50), "watershed", lambda n, uv, c: np.zeros(n, np.int64))):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    for bad in (torch.zeros(7), torch.zeros(1, 2, 3, 4)):
        with pytest.raises(ValueError, match=r"\[Y, X\] or \[N, Y, X\]"):
            pkg.watershed_seeds(bad, .25)
        with pytest.raises(ValueError, match=r"\[Y, X\] or \[N, Y, X\]"):
            pkg.seeded_watershed(bad, bad.to(torch.int32))
    with pytest.raises(ValueError, match="empty"):
        pkg.watershed_seeds(torch.zeros(2, 0, 7), .25)
    for dt in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            pkg.watershed_seeds(b.to(dt), .25)
        with pytest.raises(TypeError, match="float32"):
            pkg.seeded_watershed(b.to(dt), s)
    with pytest.raises(TypeError, match="int32"):
        pkg.seeded_watershed(b, s.to(torch.int64))
    with pytest.raises(TypeError):
        pkg.watershed_seeds(b.numpy(), .25)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.seeded_watershed(b, s[:, :30])
    for ms in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="min_size"):
            pkg.seeded_watershed(b, s, min_size=ms)
    for thr in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            pkg.watershed_seeds(b, thr)
    for a in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            pkg.watershed_seeds(b, .25, alpha=a)
    for sg in (-1.0, float("nan"), float("inf"), 10.9, 13.5):  # negative, not finite, radius 33, radius 41 >= 40
        with pytest.raises(ValueError, match="sigma_seeds"):
            pkg.watershed_seeds(b, .25, sg)
        with pytest.raises(ValueError, match="sigma_weights"):
            pkg.watershed_seeds(b, .25, 1., sg)
        with pytest.raises(ValueError, match="sigma"):
            pkg.plateau_maxima(b, sg)
    for c in (0, 3, None):
        with pytest.raises(ValueError, match="maxima_connectivity"):
            pkg.watershed_seeds(b, .25, maxima_connectivity=c)
        with pytest.raises(ValueError, match="seed_connectivity"):
            pkg.plateau_maxima(b, seed_connectivity=c)
    # elf's arguments that are not served
    for kw in (dict(pixel_pitch=(1, 2)), dict(apply_nonmax_suppression=True), dict(mask=np.ones((40, 50), bool))):
        with pytest.raises(NotImplementedError, match="not served"):
            pkg.distance_transform_watershed(b, .25, 2., **kw)
    with pytest.raises(ValueError, match=r"\[Y, X\] or \[Z, Y, X\]"):
        pkg.distance_transform_watershed(np.zeros((1, 2, 40, 50), np.float32), .25, 2.)
    with pytest.raises(TypeError, match="floats"):
        pkg.distance_transform_watershed(np.zeros((40, 50), np.int32), .25, 2.)
    with pytest.raises(ValueError, match="seed_method"):
        frag.watershed(torch.zeros(3, 2, 40, 50), "random")
    with pytest.raises(ValueError, match="C >= 3"):
        frag.elf_watershed(torch.zeros(2, 2, 40, 50))
    with pytest.raises(TypeError, match="numpy array or a torch.Tensor"):
        frag.watershed([[1.0]], "grid")
    # utils/lmc.py: None still raises, the string asks for the device fragments, any other string is refused
    a = torch.zeros(3, 2, 40, 50)
    with pytest.raises(TypeError, match="fragments is required"):
        pkg.mc_baseline(a)
    with pytest.raises(ValueError, match="watershed"):
        pkg.mc_baseline(a, "elf")
    with pytest.raises(ValueError, match="needs as many offsets"):
        pkg.multicut_multi(a, [[-1, 0, 0]], "watershed")
    with pytest.raises(ValueError, match=r"\[K, Y, X\] or \[K, Z, Y, X\]"):
        pkg.mc_baseline(torch.zeros(3, 4), "watershed")
    assert "watershed" in pkg.lmc.__doc__ and pkg.lmc.WATERSHED == "watershed"


def test_relabel_and_remove_small_are_the_references(pkg):
    frag = pkg.fragment
    seg = torch.tensor([[0, 7, 7, 3], [3, 3, 0, 12], [12, 7, 7, 7]], dtype=torch.int32)
    assert frag.relabel(seg).tolist() == [[0, 2, 2, 1], [1, 1, 0, 3], [3, 2, 2, 2]] and frag.relabel(seg).dtype == torch.int32
    assert frag.relabel(torch.zeros(2, 3, dtype=torch.int64)).tolist() == [[0, 0, 0], [0, 0, 0]]
    assert frag.remove_small(seg, 3).tolist() == [[0, 7, 7, 3], [3, 3, 0, 0], [0, 7, 7, 7]]
    assert frag.remove_small(seg, 4).tolist() == [[0, 7, 7, 0], [0, 0, 0, 0], [0, 7, 7, 7]]
    assert torch.equal(frag.remove_small(seg, 1), seg)
    with pytest.raises(TypeError):
        frag.relabel(seg.numpy())


def test_synth_membranes(pkg):
    from importlib import import_module
    synth = import_module(pkg.__name__ + ".utils.synth")
    b, cells = synth.synth_membranes(2, 70, 150, 12, seed=5)
    assert b.shape == cells.shape == (2, 70, 150) and b.dtype == np.float32 and cells.dtype == np.int32
    assert set(np.unique(b).tolist()) == {np.float32(0.05).item(), 1.0} and 0.05 < (b == 1).mean() < 0.4
    assert len(np.unique(cells[0])) >= 8 and not np.array_equal(b[0], b[1])
    b2, _ = synth.synth_membranes(2, 70, 150, 12, seed=5)
    assert np.array_equal(b, b2)
    walls = synth.synth_membranes(1, 70, 150, 12, seed=5, gaps_per_plane=0)[0]
    assert int((walls == 1).sum()) - int((b[:1] == 1).sum()) in range(1, 13)  # six gaps of two pixels (gaps may overlap)
