"""A numpy restatement of include/pea_rag.h (the region adjacency graph with affinity and boundary statistics), for the tests: pair
codes, np.unique, np.add.at and float64 sums of the f32 terms (rag_reference), a brute-force dictionary version that walks the voxels
one by one (rag_brute), the projection, a stub multicut solver on a host union-find, and the volumes the tests share.

Everything works on ONE image [Z, Y, X] (a 2D image is Z = 1); rag_reference_batch stacks.  Offsets are (dz, dy, dx)."""
import functools

import numpy as np

MAX_ABS = np.float32(32768.0)  # 2^15: a larger term is skipped
STAT_NAMES = ("edges", "edges_dropped", "pairs_dropped", "no_id", "not_touching", "skipped")
NORM5 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9]]  # local and long range
LOCAL3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]


def _part(frag, max_id, ignore_zero):
    ok = (frag >= 0) & (frag <= max_id)
    return ok & ~((frag == 0) & bool(ignore_zero))


def _pq_slices(shape, off):
    """the slices of p and of q = p + off that keep both inside the image; None: no such p"""
    ps, qs = [], []
    for n, o in zip(shape, off):
        if abs(o) >= n:
            return None
        ps.append(slice(max(0, -o), n - max(0, o)))
        qs.append(slice(max(0, o), n - max(0, -o)))
    return tuple(ps), tuple(qs)


def _term_ok(x):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (np.abs(x) <= MAX_ABS)


def rag_reference(frag, affs=None, offsets=None, boundary=None, max_id=None, one_minus=False, ignore_zero=False):
    """-> dict: uv int32 [n, 2] sorted, size / count int64 [n], mean / bmean float64 [n], min / max float32 [n], node_size int64
    [max_id + 1], stats int64 [8]"""
    frag = np.asarray(frag)
    assert frag.ndim == 3
    max_id = int(frag.max()) if max_id is None else int(max_id)
    M = max_id + 1
    part = _part(frag, max_id, ignore_zero)
    f64 = frag.astype(np.int64)
    codes, bterms = [], []
    for axis in range(3):
        sl = _pq_slices(frag.shape, [int(a == axis) for a in range(3)])
        if sl is None:
            continue
        p, q = sl
        m = part[p] & part[q] & (f64[p] != f64[q])
        codes.append((np.minimum(f64[p], f64[q]) * M + np.maximum(f64[p], f64[q]))[m])
        if boundary is not None:
            bterms.append((boundary[p][m], boundary[q][m]))
    codes = np.concatenate(codes) if codes else np.zeros(0, np.int64)
    edges = np.unique(codes)
    n = len(edges)
    idx = np.searchsorted(edges, codes)
    size = np.zeros(n, np.int64)
    np.add.at(size, idx, 1)
    skipped = 0
    bsum = np.zeros(n, np.float64)
    if boundary is not None and n:
        for side in range(2):
            t = np.concatenate([bt[side] for bt in bterms]).astype(np.float32)
            ok = _term_ok(t)
            skipped += int((~ok).sum())
            np.add.at(bsum, idx[ok], t[ok].astype(np.float64))
    count, ssum = np.zeros(n, np.int64), np.zeros(n, np.float64)
    mn, mx = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
    not_touching = 0
    if affs is not None:
        for k, off in enumerate(offsets):
            sl = _pq_slices(frag.shape, off)
            if sl is None:
                continue
            p, q = sl
            m = part[p] & part[q] & (f64[p] != f64[q])
            c = (np.minimum(f64[p], f64[q]) * M + np.maximum(f64[p], f64[q]))[m]
            x = np.asarray(affs[k], np.float32)[p][m]
            if one_minus:
                x = (np.float32(1.0) - x).astype(np.float32)
            i = np.searchsorted(edges, c)
            hit = (i < n)
            hit[hit] = edges[i[hit]] == c[hit]
            not_touching += int((~hit).sum())
            ok = _term_ok(x) & hit
            skipped += int((hit & ~ok).sum())
            np.add.at(count, i[ok], 1)
            np.add.at(ssum, i[ok], x[ok].astype(np.float64))
            np.minimum.at(mn, i[ok], x[ok])
            np.maximum.at(mx, i[ok], x[ok])
    has = count > 0
    mean = np.where(has, ssum / np.maximum(count, 1), 0.0)
    inb = (frag >= 0) & (frag <= max_id)
    stats = np.zeros(8, np.int64)
    stats[0], stats[3], stats[4], stats[5] = n, int((~inb).sum()), not_touching, skipped
    return {"uv": np.stack([edges // M, edges % M], axis=1).astype(np.int32).reshape(n, 2), "size": size, "count": count, "mean": mean,
            "bmean": bsum / np.maximum(2 * size, 1), "min": np.where(has, mn, np.float32(0)).astype(np.float32),
            "max": np.where(has, mx, np.float32(0)).astype(np.float32), "node_size": np.bincount(frag[inb].ravel(), minlength=M).astype(np.int64),
            "stats": stats}


def rag_brute(frag, affs=None, offsets=None, boundary=None, max_id=None, one_minus=False, ignore_zero=False):
    """the same contract, voxel by voxel into a dictionary (exact rational sums through Python floats of few terms)"""
    frag = np.asarray(frag)
    Z, Y, X = frag.shape
    max_id = int(frag.max()) if max_id is None else int(max_id)

    def part(v):
        return 0 <= v <= max_id and not (ignore_zero and v == 0)

    def ok(x):
        return bool(np.isfinite(x)) and abs(float(x)) <= 32768.0

    E, skipped, not_touching, no_id = {}, 0, 0, 0
    node = np.zeros(max_id + 1, np.int64)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                u = int(frag[z, y, x])
                if 0 <= u <= max_id:
                    node[u] += 1
                else:
                    no_id += 1
                for dz, dy, dx in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
                    qz, qy, qx = z + dz, y + dy, x + dx
                    if qz >= Z or qy >= Y or qx >= X:
                        continue
                    v = int(frag[qz, qy, qx])
                    if u == v or not part(u) or not part(v):
                        continue
                    e = E.setdefault((min(u, v), max(u, v)), {"size": 0, "b": [], "s": []})
                    e["size"] += 1
                    if boundary is not None:
                        for t in (np.float32(boundary[z, y, x]), np.float32(boundary[qz, qy, qx])):
                            if ok(t):
                                e["b"].append(float(t))
                            else:
                                skipped += 1
    if affs is not None:
        for k, (dz, dy, dx) in enumerate(offsets):
            for z in range(Z):
                for y in range(Y):
                    for x in range(X):
                        qz, qy, qx = z + dz, y + dy, x + dx
                        if not (0 <= qz < Z and 0 <= qy < Y and 0 <= qx < X):
                            continue
                        u, v = int(frag[z, y, x]), int(frag[qz, qy, qx])
                        if u == v or not part(u) or not part(v):
                            continue
                        e = E.get((min(u, v), max(u, v)))
                        if e is None:
                            not_touching += 1
                            continue
                        s = np.float32(affs[k][z, y, x])
                        if one_minus:
                            s = np.float32(np.float32(1.0) - s)
                        if ok(s):
                            e["s"].append(s)
                        else:
                            skipped += 1
    keys = sorted(E)
    n = len(keys)
    out = {"uv": np.array(keys, np.int32).reshape(n, 2), "size": np.array([E[k]["size"] for k in keys], np.int64),
           "count": np.array([len(E[k]["s"]) for k in keys], np.int64),
           "mean": np.array([float(np.sum(np.array(E[k]["s"], np.float64))) / len(E[k]["s"]) if E[k]["s"] else 0.0 for k in keys], np.float64),
           "bmean": np.array([float(np.sum(np.array(E[k]["b"], np.float64))) / (2 * E[k]["size"]) for k in keys], np.float64),
           "min": np.array([min(E[k]["s"]) if E[k]["s"] else 0.0 for k in keys], np.float32),
           "max": np.array([max(E[k]["s"]) if E[k]["s"] else 0.0 for k in keys], np.float32), "node_size": node}
    stats = np.zeros(8, np.int64)
    stats[0], stats[3], stats[4], stats[5] = n, no_id, not_touching, skipped
    out["stats"] = stats
    return out


def rag_reference_batch(frags, affs=None, offsets=None, boundary=None, **kw):
    """a list of rag_reference results, one per image of frags [B, Z, Y, X] (affs [B, K, Z, Y, X], boundary [B, Z, Y, X])"""
    return [rag_reference(frags[b], None if affs is None else affs[b], offsets, None if boundary is None else boundary[b], **kw)
            for b in range(len(frags))]


def mean_bound(value):
    """how far a device mean may lie from the exact one: one floor of 2^-32 per term in a mean of them, the sum rounded to f64 once and
    one f64 division (include/pea_rag.h)"""
    return 2.0 ** -32 + 2.0 ** -52 * np.abs(value)


# ---- after the graph ---------------------------------------------------------------------------------------------------------------------
def project_reference(frag, node_labels):
    frag, node_labels = np.asarray(frag), np.asarray(node_labels)
    ok = (frag >= 0) & (frag < len(node_labels))
    return np.where(ok, node_labels[np.where(ok, frag, 0)], 0).astype(np.int32), int((~ok).sum())


def stub_solver(n_nodes, uvs, costs):
    """(n_nodes, uvs, costs) -> node_labels as mc_baselines.multicut gives them: every edge of NEGATIVE cost is merged with a host
    union-find; a node's label is the smallest node of its part plus one"""
    parent = list(range(n_nodes))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for (u, v), c in zip(np.asarray(uvs).tolist(), np.asarray(costs).tolist()):
        if c < 0:
            a, b = find(u), find(v)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(a) + 1 for a in range(n_nodes)], np.int64)


def probs_to_costs_f64(probs, beta=0.5):
    """the formula of the reference's mc_baselines.probs_to_costs in float64"""
    p = np.asarray(probs, np.float64)
    c = (0.999 - 0.001) * p + 0.001
    return np.log((1.0 - c) / c) + np.log((1.0 - beta) / beta)


# ---- the shared volumes (read-only) ---------------------------------------------------------------------------------------------------------
def voronoi(shape, n, seed, first_id=0):
    """an over-segmentation: every voxel takes the id of the nearest of n random seeds (z counted four times as far)"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(0, s, n) for s in shape], axis=1).astype(np.float64)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    w = np.array([4.0, 1.0, 1.0])
    d = (((g[..., None, :] - pts) * w) ** 2).sum(-1)
    return (d.argmin(-1) + first_id).astype(np.int32)


def _ro(a):
    a.setflags(write=False)
    return a


SHAPE_2D, SHAPE_3D = (1, 37, 53), (5, 19, 23)


@functools.lru_cache(maxsize=None)
def volume(kind):
    """-> (frags int32 [2, Z, Y, X], affs f32 [2, 9, Z, Y, X], boundary f32 [2, Z, Y, X]), different content per image"""
    shape = SHAPE_2D if kind == "2d" else SHAPE_3D
    rng = np.random.default_rng(11 if kind == "2d" else 12)
    frags = np.stack([voronoi(shape, 14, 3), voronoi(shape, 23, 4, first_id=2)])
    affs = rng.random((2, len(NORM5)) + shape, dtype=np.float32)
    boundary = rng.random((2,) + shape, dtype=np.float32)
    return _ro(frags), _ro(affs), _ro(boundary)


def offsets_for(kind):
    """the norm5 offsets; for an image the channels that step along z are replaced by in-plane long-range ones"""
    if kind == "3d":
        return NORM5
    return [[0, -1, 0], [0, 0, -1], [0, -1, -1], [0, -3, 0], [0, 0, -3], [0, 2, 5], [0, -9, 0], [0, 0, -9], [0, -27, 0]]


@functools.lru_cache(maxsize=None)
def volume_ref(kind, one_minus=False, ignore_zero=False):
    f, a, b = volume(kind)
    return rag_reference_batch(f, a, offsets_for(kind), b, max_id=int(f.max()), one_minus=one_minus, ignore_zero=ignore_zero)


@functools.lru_cache(maxsize=None)
def hub_image():
    """96 x 96: 2 x 2 blocks, each its own id >= 2, separated by one-pixel lines of id 1, which so touches 32 * 32 = 1024 .. others"""
    f = np.ones((1, 96, 96), np.int32)
    ids = np.arange(2, 2 + 32 * 32, dtype=np.int32).reshape(32, 32)
    for dy in (0, 1):
        for dx in (0, 1):
            f[0, dy::3, dx::3] = ids
    f[0, 1, 1] = 1030  # the corner of a block that lies at two lines: one more neighbour of the hub, more than 1024
    return _ro(f)
