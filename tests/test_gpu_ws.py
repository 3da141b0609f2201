"""GPU: the watershed fragments on the device (include/pea_ws.h, csrc/pea_k_ws.hip) through the C ABI, through watershed_seeds,
seeded_watershed, distance_transform_watershed, utils/fragment.py and utils/lmc.py, against the numpy / scipy restatement
tests/ws_reference.py (which test_ws_host.py holds to a Dijkstra, to scipy.ndimage.watershed_ift and to hand-written expectations).

dt2, the seeds and the flood are exact integers: those comparisons are torch.equal.  dts and hmap are held to bounds derived from the
arithmetic (tolerances() below), never from what the kernels give.  The seeds are compared with the restatement run on the device's own
dts, read back, and the flood with Kruskal on the device's own hmap and seeds, so an exact stage is never hostage to a rounded one.
Every C call of this file runs in a guard-banded arena (arena.py): the inputs come back untouched, every element of every output is
written, nothing else changes; the workspace is lent as it is -- filled with the arena's pattern, never prepared -- and each call runs
twice on the same workspace.

Case sizing: 3 x 70 x 150 is two whole 32-tiles and a ragged one on both axes (pea_cc_label's tile; the Gaussian's is 64 x 32) and 41
runs of 256 pixels with a ragged one; three planes exercise plane isolation and id stacking.  1 x 1 x 1, 1 x 1 x 37 and 1 x 37 x 1 are
the degenerate extents, 64 x 64 and 1 x 4096 the ramps whose hooks form long chains."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import ws_reference as R
from arena import Arena

pytestmark = pytest.mark.gpu
STACK_IDS, FIELD = 1, 2
N3, Y3, X3 = 3, 70, 150
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def tt(a):
    return torch.tensor(np.asarray(a))


def make_desc(pkg, shape, threshold=0.25, sigma_seeds=2.0, sigma_weights=2.0, alpha=0.9, mc=2, sc=1, min_size=0, flags=0):
    d = pkg._lib.PeaWsDesc()
    d.N, d.Y, d.X = shape
    d.threshold, d.sigma_seeds, d.sigma_weights, d.alpha = threshold, sigma_seeds, sigma_weights, alpha
    d.maxima_connectivity, d.seed_connectivity, d.min_size, d.flags = mc, sc, min_size, flags
    return d


def twice(call, outs):
    """run `call` twice (the second time on the workspace as the first left it) -> the outputs as clones, equal both times"""
    first = None
    for _ in range(2):
        call()
        torch.cuda.synchronize()
        got = [None if t is None else t.clone() for t in outs]
        if first is not None:
            assert all(a is None or torch.equal(a, b) for a, b in zip(first, got)), "the second call on the same workspace differs"
        first = got
    return first


def seeds_raw(pkg, dev, boundary, skew=(0, 0, 0, 0, 0, 0), **kw):
    """pea_ws_seeds on numpy boundary [N, Y, X] in an arena -> dict(dt2, dts, hmap, seeds, counts) of device clones (dt2 and hmap None
    with PEA_WS_FIELD).  skew: bytes (boundary, dt2, dts, hmap, seeds, counts)."""
    L = pkg._lib.lib()
    b = np.ascontiguousarray(boundary, dtype=np.float32)
    d = make_desc(pkg, b.shape, **kw)
    field = bool(d.flags & FIELD)
    nb = L.pea_ws_seeds_workspace_bytes(ctypes.byref(d))
    assert nb % 8 == 0 and nb >= 29 * b.size
    ar = Arena(nb + 24 * b.size + (1 << 15), dev)
    B = ar.fill(ar.carve(b.shape, torch.float32, skew[0], name="boundary"), tt(b))
    dt2 = None if field else ar.carve(b.shape, torch.int32, skew[1], name="dt2")
    dts = ar.carve(b.shape, torch.float32, skew[2], name="dts")
    hmap = None if field else ar.carve(b.shape, torch.float32, skew[3], name="hmap")
    seeds = ar.carve(b.shape, torch.int32, skew[4], name="seeds")
    counts = ar.carve((b.shape[0],), torch.int32, skew[5], name="counts")
    ws = ar.carve((1, nb // 4), torch.int32, 8, name="workspace")
    outs = twice(lambda: pkg._lib.check(L.pea_ws_seeds(ctypes.byref(d), vp(B), vp(dt2), vp(dts), vp(hmap), vp(seeds), vp(counts), vp(ws), nb, None),
                                        "pea_ws_seeds"), (dt2, dts, hmap, seeds, counts))
    ar.check(written=[t for t in (dt2, dts, hmap, seeds, counts) if t is not None], untouched=[B], scratch=[ws])
    return dict(zip(("dt2", "dts", "hmap", "seeds", "counts"), outs))


def flood_raw(pkg, dev, h, seeds, min_size=0, flags=0, skew=(0, 0, 0, 0, 0)):
    """pea_ws_flood on numpy h, seeds [N, Y, X] in an arena -> (labels, counts [N, 2], stats [N, 2]) as device clones"""
    L = pkg._lib.lib()
    h, seeds = np.ascontiguousarray(h, dtype=np.float32), np.ascontiguousarray(seeds, dtype=np.int32)
    d = make_desc(pkg, h.shape, min_size=min_size, flags=flags)
    nb = L.pea_ws_flood_workspace_bytes(ctypes.byref(d))
    assert nb % 8 == 0 and nb >= 24 * h.size
    ar = Arena(nb + 16 * h.size + (1 << 15), dev)
    H = ar.fill(ar.carve(h.shape, torch.float32, skew[0], name="hmap"), tt(h))
    S = ar.fill(ar.carve(h.shape, torch.int32, skew[1], name="seeds"), tt(seeds))
    labels = ar.carve(h.shape, torch.int32, skew[2], name="labels")
    counts = ar.carve((h.shape[0], 2), torch.int32, skew[3], name="counts")
    stats = ar.carve((h.shape[0], 2), torch.int32, skew[4], name="stats")
    ws = ar.carve((1, nb // 4), torch.int32, 8, name="workspace")
    outs = twice(lambda: pkg._lib.check(L.pea_ws_flood(ctypes.byref(d), vp(H), vp(S), vp(labels), vp(counts), vp(stats), vp(ws), nb, None),
                                        "pea_ws_flood"), (labels, counts, stats))
    ar.check(written=[labels, counts, stats], untouched=[H, S], scratch=[ws])
    return outs


# ---- 1. distance transform, smoothing, seeds ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_batches():
    """two batches [3, 70, 150] (never modified): random sparse, one pixel in a corner, all boundary | none, a full column at a tile
    edge, random dense"""
    rng = np.random.default_rng(11)
    a = np.zeros((N3, Y3, X3), np.float32)
    a[0] = np.where(rng.random((Y3, X3)) < 0.004, 1.0, 0.1 * rng.random((Y3, X3)))
    a[1, Y3 - 1, X3 - 1] = 0.8
    a[2] = 0.3 + 0.7 * rng.random((Y3, X3))
    b = np.zeros((N3, Y3, X3), np.float32)
    b[0] = 0.2 * rng.random((Y3, X3))
    b[1, :, 32] = 1.0
    b[1] += (0.1 * rng.random((Y3, X3))).astype(np.float32)
    b[2] = np.where(rng.random((Y3, X3)) < 0.3, 0.9, 0.05)
    for x in (a, b):
        x.setflags(write=False)
    return {"sparse | corner | all": a, "none | column | dense": b}


def tolerances(boundary, dt2, sigma_seeds, sigma_weights, alpha):
    """the bounds on |dts - float64| and |hmap - float64| per plane, from the arithmetic alone:
      one separable pass of 2r + 1 f32 products and sums   (2r + 2) * 2^-24 * max|in|;  two passes  4 (r + 2) * 2^-24 * max|in|
      the weights' one rounding                              2^-24 * max|in|
      sqrtf: 1 ulp                                           2^-23 * max|dt| (an ulp of a value is at most 2^-23 of it)
      hmap before smoothing: a dozen f32 operations on values in [0, max(1, max|boundary|)]   16 * 2^-24 * that scale, added"""
    tol_s, tol_w = [], []
    pre = R.hmap_pre_reference(boundary, dt2, alpha)
    for n in range(len(boundary)):
        dmax = math.sqrt(float(dt2[n].max()))
        rs, rw = (R.gauss_radius(sigma_seeds) if sigma_seeds else None), (R.gauss_radius(sigma_weights) if sigma_weights else None)
        tol_s.append(((4 * (rs + 2) + 1) * EPS if rs is not None else 0.0) * dmax + 2 * EPS * dmax)
        scale = max(1.0, float(np.abs(boundary[n]).max()))
        tol_w.append(((4 * (rw + 2) + 1) * EPS if rw is not None else 0.0) * float(np.abs(pre[n]).max()) + 16 * EPS * scale)
    return np.array(tol_s)[:, None, None], np.array(tol_w)[:, None, None]


def check_seeds_call(what, pkg, dev, b, threshold=0.25, sigma_seeds=2.0, sigma_weights=2.0, alpha=0.9, mc=2, sc=1, **kw):
    got = seeds_raw(pkg, dev, b, threshold=threshold, sigma_seeds=sigma_seeds, sigma_weights=sigma_weights, alpha=alpha, mc=mc, sc=sc, **kw)
    dt2 = R.dt2_reference(b, threshold)
    assert torch.equal(got["dt2"].cpu(), tt(dt2)), what
    tol_s, tol_w = tolerances(b, dt2, sigma_seeds, sigma_weights, alpha)
    err_s = np.abs(got["dts"].cpu().numpy().astype(np.float64) - R.dts_reference(dt2, sigma_seeds))
    err_w = np.abs(got["hmap"].cpu().numpy().astype(np.float64) - R.hmap_reference(b, dt2, sigma_weights, alpha))
    print(what, "dts err / bound per plane", (err_s.max((1, 2)) / np.maximum(tol_s[:, 0, 0], 1e-300)).round(3).tolist(),
          "hmap err / bound", (err_w.max((1, 2)) / tol_w[:, 0, 0]).round(3).tolist(), "seeds", got["counts"].tolist())
    assert (err_s <= tol_s).all(), what
    assert (err_w <= tol_w).all(), what
    rs, rc = R.seeds_reference(got["dts"].cpu().numpy(), mc, sc)  # on the device's own dts
    assert torch.equal(got["counts"].cpu(), tt(rc)) and torch.equal(got["seeds"].cpu(), tt(rs)), what
    return got


@pytest.mark.parametrize("name", sorted(boundary_batches()))
def test_distance_transform_smoothing_and_seeds(pkg, dev, name):
    b = boundary_batches()[name]
    got = check_seeds_call(name, pkg, dev, b)
    dt2 = got["dt2"].cpu().numpy()
    if name.startswith("sparse"):
        yy, xx = np.mgrid[0:Y3, 0:X3]
        assert np.array_equal(dt2[1], (yy - (Y3 - 1)) ** 2 + (xx - (X3 - 1)) ** 2) and not dt2[2].any()
        assert got["counts"][2].item() == 1 and bool((got["seeds"][2] == 1).all())  # an all-boundary plane: dts is flat, one seed
    else:
        assert (dt2[0] == Y3 * Y3 + X3 * X3).all() and got["counts"][0].item() == 1
        assert np.array_equal(dt2[1], np.broadcast_to((np.arange(X3) - 32) ** 2, (Y3, X3)))
    # the other parameters: no smoothing, a wide Gaussian (radius 32), the 4-neighbourhood, alpha at its ends
    check_seeds_call(name + " sigma 0", pkg, dev, b, sigma_seeds=0.0, sigma_weights=0.0, alpha=0.0, mc=1, sc=2)
    check_seeds_call(name + " sigma 10.5 / 0.7", pkg, dev, b, threshold=0.5, sigma_seeds=10.5, sigma_weights=0.7, alpha=1.0)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 37), (1, 37, 1), (2, 5, 3)])
def test_degenerate_extents(pkg, dev, shape):
    rng = np.random.default_rng(shape[1] * 100 + shape[2])
    b = np.where(rng.random(shape) < 0.3, 1.0, 0.0).astype(np.float32)
    for bb in (b, np.zeros(shape, np.float32), np.ones(shape, np.float32)):
        check_seeds_call("degenerate %s" % (shape,), pkg, dev, bb, sigma_seeds=0.0, sigma_weights=0.0)
    if min(shape[1:]) >= 3:
        check_seeds_call("degenerate %s sigma 0.5" % (shape,), pkg, dev, b, sigma_seeds=0.5, sigma_weights=0.6)  # radius 2 < 3


@functools.lru_cache(maxsize=None)
def crafted_fields():
    """[3, 70, 150] integer-valued fields (never modified): ties everywhere | flat | hand-placed plateaus"""
    rng = np.random.default_rng(12)
    f = np.zeros((N3, Y3, X3), np.float32)
    f[0] = rng.integers(0, 6, (Y3, X3))
    f[1] = 3.0
    p = f[2]
    p[10, 10] = p[11, 11] = 5                 # a diagonal two-pixel plateau: one maximum under connectivity 2, two seeds under 1
    p[20:23, 29:35] = 4                       # a plateau across the tile border x = 32 ...
    p[21, 35] = 6                             # ... with one higher neighbour on the far side: not a maximum (the 6 is one)
    p[40:43, 29:35] = 4                       # the same plateau without it: a maximum
    p[0, 70:75] = 2                           # a maximum on the image border
    p[Y3 - 1, X3 - 1] = 1                     # and in the corner
    p[30:68, 60:140] = 7                      # a plateau larger than a tile
    p[50, 100] = 6.5                          # a dent inside it is no maximum, and the plateau stays one
    p[5, 100], p[5, 101] = 0.0, -0.0          # signed zeros are one value
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("mc,sc", [(2, 1), (1, 1), (2, 2), (1, 2)])
def test_plateau_maxima_of_a_crafted_field(pkg, dev, mc, sc):
    f = crafted_fields()
    got = seeds_raw(pkg, dev, f, sigma_seeds=0.0, mc=mc, sc=sc, flags=FIELD)
    assert got["dt2"] is None and got["hmap"] is None
    assert torch.equal(got["dts"].cpu(), tt(f))  # sigma == 0: the field itself, integer-valued
    rs, rc = R.seeds_reference(got["dts"].cpu().numpy(), mc, sc)
    print("crafted field", mc, sc, "seeds", got["counts"].tolist(), "ref", rc.tolist())
    assert torch.equal(got["counts"].cpu(), tt(rc)) and torch.equal(got["seeds"].cpu(), tt(rs))
    s = got["seeds"].cpu().numpy()
    assert got["counts"][1].item() == 1 and (s[1] == 1).all()
    p = s[2]
    if mc == 2:
        assert p[10, 10] > 0 and p[11, 11] > 0 and (p[10, 10] == p[11, 11]) == (sc == 2)
    assert not p[20:23, 29:35].any() and p[21, 35] > 0 and (p[40:43, 29:35] == p[40, 29]).all() and p[40, 29] > 0
    assert (p[0, 70:75] > 0).all() and p[Y3 - 1, X3 - 1] > 0 and p[31, 61] > 0 and p[50, 100] == 0 and p[49, 100] == p[31, 61]
    # a smoothed field goes through the same filter as dts
    got = seeds_raw(pkg, dev, f, sigma_seeds=1.0, mc=mc, sc=sc, flags=FIELD)
    ref = R.gauss_reference(f, 1.0)
    bound = (4 * (3 + 2) + 1) * EPS * 7.0
    assert float(np.abs(got["dts"].cpu().numpy() - ref).max()) <= bound
    rs, rc = R.seeds_reference(got["dts"].cpu().numpy(), mc, sc)
    assert torch.equal(got["counts"].cpu(), tt(rc)) and torch.equal(got["seeds"].cpu(), tt(rs))


# ---- 2. the flood ----------------------------------------------------------------------------------------------------------------------------
def random_seeds(rng, shape, n, ids=None):
    s = np.zeros(shape, np.int32)
    for plane in s:
        pos = rng.choice(plane.size, size=n, replace=False)
        plane.ravel()[pos] = np.arange(1, n + 1) if ids is None else ids
    return s


@functools.lru_cache(maxsize=None)
def flood_cases():
    """name -> (h float32 [N, Y, X], seeds int32 [N, Y, X]), never modified"""
    rng = np.random.default_rng(13)
    shape = (N3, Y3, X3)
    c = {}
    c["integer heights"] = (rng.integers(0, 4, shape).astype(np.float32), random_seeds(rng, shape, 9))
    c["random floats"] = (rng.standard_normal(shape).astype(np.float32), random_seeds(rng, shape, 25))
    h = (rng.integers(-2, 3, shape) * rng.choice([0.0, 1.0, 0.5], shape)).astype(np.float32)
    h[np.logical_and(h == 0, rng.random(shape) < 0.5)] = -0.0
    c["negative heights and signed zeros"] = (h, random_seeds(rng, shape, 12))
    h = rng.random(shape).astype(np.float32)
    h[:, 33, :] = np.inf
    h[:, :, 64] = np.inf
    h[:, 10:20, 100:110] = np.inf  # a block of wall: its inside is reached through +inf alone
    c["inf walls"] = (h, random_seeds(rng, shape, 6))
    s = random_seeds(rng, shape, 7)
    s[1] = 0
    c["no seeds in one plane"] = (rng.integers(0, 3, shape).astype(np.float32), s)
    c["a seed on every pixel"] = (rng.random(shape).astype(np.float32), np.broadcast_to(np.arange(1, Y3 * X3 + 1, dtype=np.int32).reshape(Y3, X3), shape).copy())
    s = np.zeros(shape, np.int32)
    s[0, 35, 75], s[1, 0, 0], s[2, Y3 - 1, X3 - 1] = 1, 1, 1
    c["one seed"] = (rng.integers(0, 2, shape).astype(np.float32), s)
    s = np.zeros(shape, np.int32)
    s[:, 2:45, 3:50] = 2       # seeded regions larger than a tile, one id in two places
    s[:, 5:60, 90:148] = 1
    s[:, 66:69, 20:120] = 2
    c["seeded regions larger than a tile"] = (rng.random(shape).astype(np.float32), s)
    # ids that are not consecutive, one above Y * X and a negative one (both read as 0)
    c["sparse ids"] = (rng.integers(0, 5, shape).astype(np.float32), random_seeds(rng, shape, 6, ids=np.array([7, 300, Y3 * X3, Y3 * X3 + 1, -4, 41])))
    for h, s in c.values():
        h.setflags(write=False)
        s.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def flood_ref(name, min_size=0, stack=False):
    h, s = flood_cases()[name]
    return R.flood_reference(h, s, min_size, stack)


def max_rounds(Y, X):
    return int(math.ceil(math.log2(Y * X))) + 1 if Y * X > 1 else 1


def check_flood(what, pkg, dev, h, s, min_size=0, flags=0, ref=None, **kw):
    rl, rc, rz = ref if ref is not None else R.flood_reference(h, s, min_size, bool(flags & STACK_IDS))
    labels, counts, stats = flood_raw(pkg, dev, h, s, min_size, flags, **kw)
    print(what, "min_size", min_size, "flags", flags, "counts", counts.tolist(), "stats", stats.tolist(), "bound", max_rounds(*h.shape[1:]))
    assert torch.equal(counts.cpu(), tt(rc)), what
    assert torch.equal(labels.cpu(), tt(rl)), what
    assert torch.equal(stats[:, 1].cpu(), tt(rz)), what
    assert int(stats[:, 0].max()) <= max_rounds(*h.shape[1:]) and int(stats[:, 0].min()) >= 0, what
    return labels, counts, stats


@pytest.mark.parametrize("name", sorted(flood_cases()))
def test_flood_is_kruskal(pkg, dev, name):
    h, s = flood_cases()[name]
    labels, counts, stats = check_flood(name, pkg, dev, h, s, ref=flood_ref(name))
    if name == "no seeds in one plane":
        # (the trees of a plane without seeds still merge, round by round, into one that has no label)
        assert not bool(labels[1].any()) and stats[1, 1].item() == Y3 * X3 and counts[1].tolist() == [0, 0] and stats[0, 1].item() == 0
    if name == "a seed on every pixel":
        assert torch.equal(labels.cpu(), tt(s)) and stats[:, 0].tolist() == [0, 0, 0]
    if name == "one seed":
        assert bool((labels == 1).all()) and counts.tolist() == [[1, 1]] * 3
    if name == "sparse ids":
        assert counts.tolist() == [[4, 4]] * 3 and int(labels.max()) == 4
    # numbering: with PEA_WS_STACK_IDS plane n is offset by the kept counts of the planes before it
    stacked, counts2, _ = check_flood(name + " stacked", pkg, dev, h, s, flags=STACK_IDS, ref=flood_ref(name, 0, True))
    off = torch.cumsum(counts2[:, 1], 0) - counts2[:, 1]
    assert torch.equal(stacked, torch.where(labels > 0, labels + off[:, None, None].to(torch.int32), labels))


@pytest.mark.parametrize("shape", [(1, 64, 64), (1, 1, 4096), (1, 4096, 1), (1, 1, 1), (1, 1, 37), (1, 37, 1)])
def test_ramps_hook_long_chains(pkg, dev, shape):
    """h[p] = p with one seed at p = 0: every pixel's smallest edge leads one step towards the seed, so one round hooks chains as long
    as a row, a column (64 x 64) or the whole plane (1 x 4096: 4095 hooks); the same ramp reversed; the degenerate extents"""
    S = shape[1] * shape[2]
    for h in (np.arange(S, dtype=np.float32).reshape(shape), np.arange(S, dtype=np.float32)[::-1].reshape(shape).copy()):
        s = np.zeros(shape, np.int32)
        s.ravel()[0] = 1
        labels, counts, stats = check_flood("ramp %s" % (shape,), pkg, dev, h, s)
        assert bool((labels == 1).all()) and stats[0, 1].item() == 0
        if S > 1:
            s.ravel()[S - 1] = 2
            check_flood("ramp %s two seeds" % (shape,), pkg, dev, h, s)
        check_flood("ramp %s no seed" % (shape,), pkg, dev, h, np.zeros(shape, np.int32))


@functools.lru_cache(maxsize=None)
def pockets():
    """[3, 70, 150]: plane 0 is three bowls around the seeds 2, 7 and 11 (the height grows with the distance to the nearest of them)
    and two 3 x 3 pockets of height 0 behind walls of height 5, each with a seed (5 and 9); plane 1 random heights with 40 seeds;
    plane 2 has no seed"""
    rng = np.random.default_rng(14)
    h = np.zeros((N3, Y3, X3), np.float32)
    s = np.zeros((N3, Y3, X3), np.int32)
    yy, xx = np.mgrid[0:Y3, 0:X3]
    outside = (((35, 20), 2), ((35, 75), 7), ((35, 130), 11))
    h[0] = np.min([np.hypot(yy - y, xx - x) for (y, x), _ in outside], axis=0) / 200.0
    for (y, x), sid in outside:
        s[0, y, x] = sid
    for (y, x), sid in (((12, 45), 5), ((55, 100), 9)):
        h[0, y - 2:y + 3, x - 2:x + 3] = 5.0
        h[0, y - 1:y + 2, x - 1:x + 2] = 0.0
        s[0, y, x] = sid
    h[1] = rng.random((Y3, X3))
    s[1] = random_seeds(rng, (1, Y3, X3), 40)[0]
    h.setflags(write=False)
    s.setflags(write=False)
    return h, s


def test_min_size_removes_seeds_and_floods_again(pkg, dev):
    h, s = pockets()
    plain, counts, _ = check_flood("pockets", pkg, dev, h, s)
    assert counts[0].tolist() == [5, 5] and counts[2].tolist() == [0, 0]
    sizes = np.bincount(plain[0].cpu().numpy().ravel())[1:]  # ids 1 .. 5 for the seeds 2, 5, 7, 9, 11
    # a pocket is its nine pixels and those of its wall that it wins (every edge of the wall weighs 5: the edge index decides)
    assert 9 <= sizes[1] <= 25 and 9 <= sizes[3] <= 25 and min(sizes[0], sizes[2], sizes[4]) > 2000
    # two seeds fall below 50 and their area goes to the neighbours
    labels, counts, stats = check_flood("pockets min_size 50", pkg, dev, h, s, 50)
    assert counts[0].tolist() == [5, 3] and 0 < counts[1, 1].item() < 40 and counts[1, 0].item() == 40
    lab = labels.cpu().numpy()
    assert lab[0].min() == 1 and lab[0].max() == 3 and np.array_equal(lab[0] == 1, np.isin(plain[0].cpu().numpy(), (1, 2)) | (lab[0] == 1))
    assert np.bincount(lab[0].ravel())[1:].sum() == Y3 * X3 and stats[2, 1].item() == Y3 * X3 and stats[0, 1].item() == 0
    check_flood("pockets min_size 50 stacked", pkg, dev, h, s, 50, STACK_IDS)
    # a plane in which none would remain keeps its first flood: no fragment of plane 0 or 1 has 9000 of the 10500 pixels
    labels, counts, _ = check_flood("pockets min_size 9000", pkg, dev, h, s, 9000)
    assert counts[0].tolist() == [5, 5] and counts[1].tolist() == [40, 40] and torch.equal(labels, plain)
    one = np.zeros_like(s)
    one[:, 3, 3] = 1
    _, counts, _ = check_flood("one seed min_size 9000", pkg, dev, h, one, 9000)
    assert counts.tolist() == [[1, 1]] * 3
    for ms in (1, 2, 9, 26):  # 0 and 1 filter nothing
        _, counts, _ = check_flood("pockets", pkg, dev, h, s, ms)
        assert counts[0].tolist() == [5, 5 if ms <= 9 else 3], ms


def test_skewed_pointers_give_the_same_bits(pkg, dev):
    h, s = flood_cases()["integer heights"]
    ref = flood_ref("integer heights", 30, True)
    aligned = check_flood("aligned", pkg, dev, h, s, 30, STACK_IDS, ref=ref)
    for skew in ((4, 12, 8, 4, 12), (12, 4, 4, 8, 4)):
        got = check_flood("skew %s" % (skew,), pkg, dev, h, s, 30, STACK_IDS, ref=ref, skew=skew)
        assert all(torch.equal(a, b) for a, b in zip(got, aligned)), skew
    b = boundary_batches()["sparse | corner | all"]
    aligned = seeds_raw(pkg, dev, b)
    for skew in ((4, 8, 12, 4, 8, 12), (12, 4, 8, 12, 4, 4)):
        got = seeds_raw(pkg, dev, b, skew=skew)
        assert all(torch.equal(got[k], aligned[k]) for k in aligned), skew


def test_stacked_ids_over_more_planes_than_a_step_of_the_offsets(pkg, dev):
    """k_ws_offsets takes 256 planes a step with a carry: 257 planes of 2 x 2 with one seed each, so the last plane's offset is 256"""
    N = 257
    h = torch.zeros((N, 2, 2), dtype=torch.float32, device=dev)
    s = torch.zeros((N, 2, 2), dtype=torch.int32, device=dev)
    s[:, 1, 0] = 3  # (any id in 1 .. Y * X is a seed id)
    w = pkg.seeded_watershed(h, s, stack_ids=True)
    want = torch.arange(1, N + 1, dtype=torch.int32, device=dev)[:, None, None].expand(N, 2, 2)
    assert torch.equal(w.labels, want) and w.counts.tolist() == [[1, 1]] * N and int(w.stats[:, 1].sum()) == 0
    assert torch.equal(pkg.seeded_watershed(h, s).labels, torch.ones_like(s))  # not stacked: every plane starts at 1


# ---- 3. the Python layer, end to end -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def membranes():
    """[3, 70, 150]: planes 0 and 1 are Voronoi cell walls with two-pixel gaps (utils/synth.py); plane 2 is two cells behind one
    straight wall at x = 75 with a two-pixel gap at y = 35, 36 -> (boundary, cells)"""
    import __graft_entry__ as ge
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    b, cells = synth.synth_membranes(N3, Y3, X3, 12, seed=21, gap=2, gaps_per_plane=6)
    b[2], cells[2] = 0.05, 1
    b[2, :, 75] = 1.0
    b[2, 35:37, 75] = 0.05
    cells[2, :, 76:] = 2
    b.setflags(write=False)
    return b, cells


def test_distance_transform_watershed_end_to_end(pkg, dev):
    b, _ = membranes()
    B = tt(b).to(dev)
    labels, max_id = pkg.distance_transform_watershed(B, .25, 2., min_size=20)
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.shape == B.shape and max_id.is_cuda and max_id.dim() == 0
    # the reference chain, fed stage by stage with the device's intermediates
    s = pkg.watershed_seeds(B, .25, 2., 2., .9)
    assert torch.equal(s.dt2.cpu(), tt(R.dt2_reference(b, .25)))
    rs, rc = R.seeds_reference(s.dts.cpu().numpy(), 2, 1)
    assert torch.equal(s.seeds.cpu(), tt(rs)) and torch.equal(s.counts.cpu(), tt(rc))
    rl, rcnt, _ = R.flood_reference(s.hmap.cpu().numpy(), s.seeds.cpu().numpy(), 20, True)
    print("end to end: seeds", rc.tolist(), "fragments", rcnt.tolist(), "max_id", int(max_id))
    assert torch.equal(labels.cpu(), tt(rl)) and int(max_id) == int(rcnt[:, 1].sum()) == int(labels.max())
    w = pkg.seeded_watershed(s.hmap, s.seeds, min_size=20, stack_ids=True)
    assert torch.equal(w.labels, labels) and torch.equal(w.counts.cpu(), tt(rcnt)) and int(w.stats[:, 1].sum()) == 0
    # every label is 4-connected: splitting the label image into its connected pieces finds as many pieces as ids
    cc = pkg.connected_components(labels, connectivity=1)
    assert torch.equal(cc.counts[:, 0].cpu(), tt(rcnt[:, 1]))
    # the gap in the wall does not merge the two cells; connected components of the thresholded map do merge them
    lab = labels[2]
    assert bool((lab[:, :75] != lab[35, 110]).all()) and bool((lab[:, 76:] != lab[35, 40]).all())
    merged = pkg.connected_components((B <= .25), connectivity=1).labels[2]
    assert merged[35, 40].item() == merged[35, 110].item() != 0
    # one plane in, one plane out; numpy in, numpy out, through the device
    l2, m2 = pkg.distance_transform_watershed(B[2], .25, 2., min_size=20)
    assert l2.shape == (Y3, X3) and torch.equal(torch.unique(l2), torch.arange(1, int(m2) + 1, dtype=torch.int32, device=dev))
    ln, mn = pkg.distance_transform_watershed(b.copy(), .25, 2., min_size=20)
    assert isinstance(ln, np.ndarray) and ln.dtype == np.int32 and isinstance(mn, int) and np.array_equal(ln, rl) and mn == int(max_id)
    # strided input: a dense copy is made
    wide = torch.zeros((N3, Y3, 2 * X3), device=dev)
    wide[:, :, ::2] = B
    assert torch.equal(pkg.distance_transform_watershed(wide[:, :, ::2], .25, 2., min_size=20)[0], labels)


def affs_of(b):
    """an affinity volume [3, Z, Y, X] whose boundary map max(1 - a[1], 1 - a[2]) is b"""
    return np.stack([np.ones_like(b), 1 - b, 1 - 0.5 * b]).astype(np.float32)


def test_fragment_module(pkg, dev):
    b, _ = membranes()
    affs = affs_of(b[:2])
    A = tt(affs).to(dev)
    frag = pkg.fragment
    got = frag.elf_watershed(A)
    want = pkg.distance_transform_watershed(torch.maximum(1 - A[1], 1 - A[2]), .25, 2.)[0]
    assert got.dtype == torch.int32 and torch.equal(got, want) and int(got.max()) > 2
    gn = frag.elf_watershed(affs)
    assert isinstance(gn, np.ndarray) and gn.dtype == np.uint64 and np.array_equal(gn, want.cpu().numpy())
    xy = (1.0 - 0.5 * (A[1] + A[2])).cpu().numpy()  # the device's own height map
    grid = np.zeros(xy.shape, np.int32)
    grid[:, ::10, ::10] = np.arange(1, 7 * 15 + 1).reshape(7, 15)
    seeds = {"grid": grid, "minima": R.seeds_reference(-xy, 1, 1)[0],
             "maxima_distance": R.seeds_reference(R.dt2_reference(xy, np.nextafter(np.float32(0.5), np.float32(0))).astype(np.float32), 1, 1)[0]}
    for method in ("grid", "minima", "maxima_distance"):
        got = frag.watershed(A, method)
        want = R.flood_reference(xy, seeds[method], 0, True)[0]
        print("fragment.watershed", method, "fragments", int(got.max()))
        assert torch.equal(got.cpu(), tt(want)), method
    assert int(frag.watershed(A, "grid").max()) == 2 * 105


def test_mc_baseline_makes_its_fragments_on_the_device(pkg, dev):
    b, _ = membranes()
    affs = affs_of(b)
    A = tt(affs).to(dev)
    fragments = pkg.distance_transform_watershed(torch.maximum(1 - A[1], 1 - A[2]), .25, 2.)[0]
    seen = {}

    def pair_up(n_nodes, uvs, costs):  # a trivial solver: fragments 2k and 2k + 1 become one piece
        seen["n"] = n_nodes
        return np.arange(n_nodes) // 2

    seg = pkg.mc_baseline(A, "watershed", solver=pair_up)
    assert seg.is_cuda and seg.shape == fragments.shape and seen["n"] == int(fragments.max()) + 1
    f, g = fragments.cpu().numpy().ravel(), seg.cpu().numpy().ravel()
    # every piece is a union of fragments: a fragment lies in one piece, and the pieces are those of the solver
    first = np.zeros(f.max() + 1, np.int64)
    first[f] = g
    assert np.array_equal(first[f], g) and len(np.unique(g)) == len(np.unique(f // 2))
    assert torch.equal(seg, pkg.mc_baseline(A, fragments, solver=pair_up))
    assert torch.equal(seg, pkg.multicut_multi(A, None, "watershed", pair_up))
    sn = pkg.mc_baseline(affs, "watershed", solver=pair_up)
    assert isinstance(sn, np.ndarray) and np.array_equal(sn, seg.cpu().numpy())


def test_graphed_call_replays_the_eager_result(pkg, dev):
    b, _ = membranes()
    B = tt(b).to(dev)

    def step(B):
        labels, max_id = pkg.distance_transform_watershed(B, .25, 2., min_size=20)
        return labels, max_id

    eager = [t.clone() for t in step(B)]
    g = pkg.graphed(step, B)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a, c) for a, c in zip(got, eager))
    B.copy_(tt(np.ascontiguousarray(b[::-1, :, ::-1])))  # the input buffer refilled: the replay floods what it holds now
    got = [t.clone() for t in g.replay()]
    again = step(B)
    assert all(torch.equal(a, c) for a, c in zip(got, again)) and not torch.equal(got[0], eager[0])
