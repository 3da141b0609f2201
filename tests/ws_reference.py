"""A numpy / scipy restatement of every stage of include/pea_ws.h (a plain helper: the GPU tests compare the kernels with it and
test_ws_host.py holds it to scipy and to a Dijkstra).

  dt2_reference         scipy.ndimage.distance_transform_edt, squared and rounded to int
  gauss_reference       scipy.ndimage.gaussian_filter(truncate=3.0, mode='mirror') in float64
  plateau_maxima        plateau maxima by scipy.ndimage.label per distinct value
  seeds_reference       the components of that mask, numbered by scipy.ndimage.label (raster order of the first pixel)
  kruskal_flood         the minimum spanning forest relative to the seeds: Kruskal with union-find over the keys of the header
  flood_reference       the batch form: size filter and second flood, renumbering, stacked ids, counts, pixels left 0
All functions take and return numpy arrays; planes are [Y, X], batches [N, Y, X]."""
import numpy as np
import scipy.ndimage as ndi


def ord32(h):
    """the order-preserving uint32 image of a float32 array (-0.0 below +0.0)"""
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


# ---- distance transform, smoothing ---------------------------------------------------------------------------------------------------------
def dt2_reference(boundary, threshold):
    """[N, Y, X] float32 -> int32: squared distance to the nearest pixel with boundary > threshold, Y^2 + X^2 in a plane without"""
    out = np.empty(boundary.shape, np.int32)
    for n, b in enumerate(boundary):
        m = b > np.float32(threshold)
        if not m.any():
            out[n] = b.shape[0] ** 2 + b.shape[1] ** 2
        else:
            out[n] = np.rint(ndi.distance_transform_edt(~m) ** 2).astype(np.int32)
    return out


def gauss_radius(sigma):
    return int(3.0 * float(np.float32(sigma)) + 0.5)


def gauss_reference(x, sigma):
    """[N, Y, X] -> float64, each plane on its own; sigma == 0: the input"""
    x = np.asarray(x, np.float64)
    if float(sigma) == 0.0:
        return x.copy()
    return np.stack([ndi.gaussian_filter(p, float(np.float32(sigma)), truncate=3.0, mode="mirror") for p in x])


def dts_reference(dt2, sigma_seeds):
    return gauss_reference(np.sqrt(dt2.astype(np.float64)), sigma_seeds)


def hmap_pre_reference(boundary, dt2, alpha):
    """alpha * boundary + (1 - alpha) * (1 - (dt - dmin) / (dmax - dmin)) in float64, the quotient 0 where the extrema are equal"""
    a = float(np.float32(alpha))
    out = np.empty(boundary.shape, np.float64)
    for n in range(len(boundary)):
        dt = np.sqrt(dt2[n].astype(np.float64))
        lo, hi = dt.min(), dt.max()
        q = (dt - lo) / (hi - lo) if hi > lo else np.zeros_like(dt)
        out[n] = a * boundary[n].astype(np.float64) + (1.0 - a) * (1.0 - q)
    return out


def hmap_reference(boundary, dt2, sigma_weights, alpha):
    return gauss_reference(hmap_pre_reference(boundary, dt2, alpha), sigma_weights)


# ---- seeds ------------------------------------------------------------------------------------------------------------------------------------
def _structure(connectivity):
    return ndi.generate_binary_structure(2, connectivity)


def plateau_maxima(d, connectivity=2):
    """[Y, X] -> bool: the pixels of the plateaus (maximal sets of equal value, connected under `connectivity`) none of whose pixels
    has a strictly higher neighbour; the border is allowed"""
    d = np.asarray(d)
    Y, X = d.shape
    pad = np.full((Y + 2, X + 2), -np.inf, np.float64)
    pad[1:-1, 1:-1] = d
    higher, equal = np.zeros((Y, X), bool), np.zeros((Y, X), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy == 0 and dx == 0) or (dy and dx and connectivity < 2):
                continue
            nb = pad[1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]
            higher |= nb > d
            equal |= nb == d
    ismax = ~higher
    for v in np.unique(d[equal & ~higher]):  # plateaus of more than one pixel that may still be maxima
        lab, _ = ndi.label(d == v, structure=_structure(connectivity))
        bad = np.unique(lab[higher & (d == v)])
        ismax[np.isin(lab, bad[bad > 0])] = False
    return ismax


def seeds_reference(dts, maxima_connectivity=2, seed_connectivity=1):
    """[N, Y, X] -> (seeds int32 [N, Y, X], counts int32 [N])"""
    seeds, counts = np.zeros(dts.shape, np.int32), np.zeros(len(dts), np.int32)
    for n, d in enumerate(dts):
        seeds[n], counts[n] = ndi.label(plateau_maxima(d, maxima_connectivity), structure=_structure(seed_connectivity))
    return seeds, counts


# ---- the flood ----------------------------------------------------------------------------------------------------------------------------------
def edge_keys(h):
    """[Y, X] float32 -> (keys uint64 sorted ascending, p, q): every 4-neighbour pair with key (max(ord(h[p]), ord(h[q])) << 32) |
    (2 p + dir)"""
    Y, X = h.shape
    o = ord32(h).astype(np.uint64).ravel()
    idx = np.arange(Y * X, dtype=np.int64).reshape(Y, X)
    px, py = idx[:, :-1].ravel(), idx[:-1, :].ravel()
    p = np.concatenate([px, py])
    q = np.concatenate([px + 1, py + X])
    d = np.concatenate([np.zeros(len(px), np.uint64), np.ones(len(py), np.uint64)])
    keys = (np.maximum(o[p], o[q]) << np.uint64(32)) | (np.uint64(2) * p.astype(np.uint64) + d)
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys)
    return keys[order], p[order], q[order]


def kruskal_flood(h, seeds, forest=False):
    """[Y, X] float32 and int [Y, X] (0 = none) -> the seed id of every pixel's tree (0 in a plane without seeds): Kruskal over the
    edges by key, an edge skipped iff both ends are in one tree or both trees hold a seed.  forest: also the list of taken edges."""
    Y, X = h.shape
    keys, ps, qs = edge_keys(h)
    parent = list(range(Y * X))
    lab = [int(v) for v in np.asarray(seeds).ravel()]
    taken = []

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for k, p, q in zip(keys.tolist(), ps.tolist(), qs.tolist()):
        a, b = find(p), find(q)
        if a == b or (lab[a] and lab[b]):
            continue
        parent[a] = b
        if lab[a]:
            lab[b] = lab[a]
        if forest:
            taken.append((p, q, k >> 32))
    out = np.array([lab[find(x)] for x in range(Y * X)], np.int32).reshape(Y, X)
    return (out, taken) if forest else out


def flood_reference(h, seeds, min_size=0, stack_ids=False):
    """[N, Y, X] -> (labels int32, counts int32 [N, 2], zeros int32 [N]) as include/pea_ws.h states them; seed ids outside
    1 .. Y * X are read as 0"""
    N, Y, X = h.shape
    labels, counts, zeros = np.zeros((N, Y, X), np.int32), np.zeros((N, 2), np.int32), np.zeros(N, np.int32)
    offset = 0
    for n in range(N):
        s = np.where((seeds[n] >= 1) & (seeds[n] <= Y * X), seeds[n], 0)
        first = kruskal_flood(h[n], s)
        ids, sizes = np.unique(first[first > 0], return_counts=True)
        keep = ids[sizes >= min_size] if min_size > 1 else ids
        final = first
        if min_size > 1 and 0 < len(keep) < len(ids):
            final = kruskal_flood(h[n], np.where(np.isin(s, keep), s, 0))
        if len(keep) == 0:
            keep = ids
        new = np.zeros(Y * X + 1, np.int32)
        new[keep] = np.arange(1, len(keep) + 1)
        lab = new[final]
        counts[n] = (len(ids), len(keep))
        zeros[n] = int((lab == 0).sum())
        labels[n] = np.where(lab > 0, lab + (offset if stack_ids else 0), 0)
        offset += len(keep)
    return labels, counts, zeros


def chain_reference(boundary, threshold, sigma_seeds, sigma_weights=2.0, min_size=100, alpha=0.9):
    """the whole chain in float64 / exact integers on [N, Y, X] -> labels with stacked ids (what distance_transform_watershed
    computes, up to the rounding of dts and hmap)"""
    dt2 = dt2_reference(boundary, threshold)
    seeds, _ = seeds_reference(dts_reference(dt2, sigma_seeds).astype(np.float32))
    hmap = hmap_reference(boundary, dt2, sigma_weights, alpha).astype(np.float32)
    return flood_reference(hmap, seeds, min_size, True)[0]
