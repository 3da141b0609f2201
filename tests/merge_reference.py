"""The small-segment merges of include/pea_merge.h restated twice in numpy and Python integers (a plain helper, no test):

  literal(seg, threshold, window)   the reference's merge_small_object line by line -- the image is rewritten, np.unique once per pass and
                                    once per crop -- with its np.argsort made stable (or ties ranked the other way round: ties="desc")
  aliased(seg, threshold, window)   the form the kernels take: an alias per id, integer moments that add under a merge, the image never
                                    rewritten; it also counts what pea_merge_small leaves in stats

tests/test_merge_host.py holds the two to each other and to the fixtures made with the reference's own functions; the GPU tests compare
the kernels with `chain` (passes of `aliased`) bit for bit.  Ids are non-negative integers; windows do not exceed the image.
"""
import numpy as np

CVPPP_MERGE_PASSES = ((5, 5), (20, 11), (50, 11), (300, 21))
BBBC_MERGE_PASSES = ((5, 5), (25, 11), (50, 11), (100, 21))
STAT_COLUMNS = ("candidates", "merges", "negative", "few", "out_of_range", "chain", "reserved", "reserved")


def _rank(ids, counts, ties):
    """positions of `ids` (ascending) by count descending, then id ascending ("asc", the library's rule) or descending ("desc")"""
    if ties == "asc":
        return np.argsort(-counts, kind="stable")
    return np.lexsort((-ids, -counts))


def _target(ids, counts, i, ties):
    """the id that candidate i takes, given the crop's ascending ids and their counts (three or more)"""
    rank = _rank(ids, counts, ties)
    if ids[rank[0]] == 0:
        return int(ids[rank[2]]) if ids[rank[1]] == i else int(ids[rank[1]])
    return int(ids[rank[0]])


def literal(seg, threshold=5, window=5, ties="asc"):
    """the reference's loop on a copy of seg [Y, X]"""
    seg = np.array(seg, dtype=np.int64)
    assert seg.ndim == 2 and window <= min(seg.shape) and seg.min() >= 0
    uid, uc = np.unique(seg, return_counts=True)
    for i, size in zip(uid.tolist(), uc.tolist()):
        if size > threshold:
            continue
        rows, cols = np.where(seg == i)
        r0 = int(rows.sum()) // rows.size - window // 2
        c0 = int(cols.sum()) // cols.size - window // 2
        if r0 < 0 or c0 < 0:  # (the reference's negative slice start: an empty crop)
            continue
        ids, counts = np.unique(seg[r0:r0 + window, c0:c0 + window], return_counts=True)
        if len(ids) > 2:
            seg[seg == i] = _target(ids, counts, i, ties)
    return seg


class Aliased(object):
    """labels int64 [Y, X]; stats: the eight columns of pea_merge_small; alias: the table after the last pass; per_pass: for every pass a
    dict of its own candidates, merges, negative, few, chain (the longest chain met in that pass), tie01 and tie12 (candidates whose
    crop's rank 0 and 1, rank 1 and 2 had equal counts)"""

    def __init__(self, labels, stats, alias, per_pass=()):
        self.labels, self.stats, self.alias, self.per_pass = labels, stats, alias, list(per_pass)

    def stat(self, name):
        return self.stats[STAT_COLUMNS.index(name)]


def aliased_passes(seg, passes, max_id=None, ties="asc"):
    """the passes in order on one alias table -> Aliased.  Pixels whose id lies outside [0, max_id] count for nothing and stay."""
    seg = np.asarray(seg).astype(np.int64)
    Y, X = seg.shape
    max_id = int(seg.max()) if max_id is None else int(max_id)
    N = max_id + 1
    ok = (seg >= 0) & (seg <= max_id)
    flat = np.where(ok, seg, 0).ravel()
    w = ok.ravel().astype(np.int64)
    rr, cc = np.indices(seg.shape)
    n = np.bincount(flat, weights=w, minlength=N).astype(np.int64)
    sr = np.bincount(flat, weights=w * rr.ravel(), minlength=N).astype(np.int64)
    sc = np.bincount(flat, weights=w * cc.ravel(), minlength=N).astype(np.int64)
    alias = np.arange(N)
    stats = [0] * 8
    stats[4] = int((~ok).sum())

    def find(v):
        hops = 0
        while alias[v] != v:
            v = alias[v]
            hops += 1
        return v, hops

    per_pass = []
    for p, (threshold, window) in enumerate(passes):
        assert 1 <= window <= min(Y, X) and threshold >= 0
        size0 = n.copy()
        before, mine = list(stats), dict(chain=0, tie01=0, tie12=0)
        for i in np.flatnonzero((size0 > 0) & (size0 <= threshold)).tolist():
            assert n[i] > 0  # pixels leave an id only when it is served
            stats[0] += 1
            r0 = int(sr[i]) // int(n[i]) - window // 2
            c0 = int(sc[i]) // int(n[i]) - window // 2
            if r0 < 0 or c0 < 0:
                stats[2] += 1
                continue
            count = {}
            for r in range(r0, min(r0 + window, Y)):
                for c in range(c0, min(c0 + window, X)):
                    if ok[r, c]:
                        v, hops = find(int(seg[r, c]))
                        stats[5] = max(stats[5], hops)
                        mine["chain"] = max(mine["chain"], hops)
                        count[v] = count.get(v, 0) + 1
            if len(count) <= 2:
                stats[3] += 1
                continue
            ids = np.array(sorted(count))
            top = sorted(count.values(), reverse=True)
            mine["tie01"] += top[0] == top[1]
            mine["tie12"] += top[1] == top[2]
            t = _target(ids, np.array([count[v] for v in ids.tolist()]), i, ties)
            if t != i:
                stats[1] += 1
                alias[i] = t
                n[t] += n[i]; sr[t] += sr[i]; sc[t] += sc[i]
                n[i] = sr[i] = sc[i] = 0
        mine.update(candidates=stats[0] - before[0], merges=stats[1] - before[1], negative=stats[2] - before[2], few=stats[3] - before[3])
        per_pass.append(mine)
        if p + 1 < len(passes):  # between passes every chain becomes one link
            alias = np.array([find(v)[0] for v in range(N)])
    root = np.array([find(v)[0] for v in range(N)])
    labels = np.where(ok, root[np.where(ok, seg, 0)], seg)
    return Aliased(labels, stats, root, per_pass)


def aliased(seg, threshold=5, window=5, ties="asc"):
    return aliased_passes(seg, ((threshold, window),), ties=ties).labels


def chain(seg, passes, ties="asc"):
    """the passes of `literal` in order"""
    for threshold, window in passes:
        seg = literal(seg, threshold, window, ties)
    return seg


def relabel(seg, max_id=None):
    """the reference's relabel with ids outside [0, max_id] written through -> (labels, n)"""
    seg = np.asarray(seg).astype(np.int64)
    ok = (seg > 0) if max_id is None else (seg > 0) & (seg <= max_id)
    ids = np.unique(seg[ok])
    out = seg.copy()
    out[ok] = np.searchsorted(ids, seg[ok]) + 1
    return out, int(ids.size)


def tie_free(seg, passes):
    """True iff ranking equal counts the other way round gives the same image in every pass: the reference's unstable argsort cannot
    have mattered"""
    seg = np.array(seg, dtype=np.int64)
    for threshold, window in passes:
        a, b = literal(seg, threshold, window, "asc"), literal(seg, threshold, window, "desc")
        if not np.array_equal(a, b):
            return False
        seg = a
    return True


def random_image(rng, lo=21, hi=69):
    """blocks, random specks and holes (the images of the fixtures)"""
    Y, X = (int(v) for v in rng.integers(lo, hi + 1, 2))
    g = int(rng.integers(4, 12))
    seg = ((np.arange(Y)[:, None] // g) * ((X + g - 1) // g) + np.arange(X)[None, :] // g + 1).astype(np.int64)
    specks = rng.random((Y, X)) < 0.08
    seg[specks] = rng.integers(0, seg.max() + 40, int(specks.sum()))
    seg[rng.random((Y, X)) < 0.15] = 0
    return seg
