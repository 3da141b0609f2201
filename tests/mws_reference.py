"""The mutex watershed of include/pea_mws.h restated three times in numpy / plain Python (a helper of test_mws_host.py and
test_gpu_mws.py, no test of its own):

  sequential(g)    (a) the definition: the edges by descending key through a union-find, a set of excluded roots per root
  naive(g)         (b) the same order, but "exclusive?" is answered by scanning every earlier repulsive edge that became an exclusion
  rounds(g)        (c) the round rule of the header as a simulation: prune, best, decide, hook, compress, carry, rebuild
  rounds_trace(g)  (c) again, returning what the header fixes after every round: the partition, the rounds used and the counts of
                   undecided, merged and active edges -- the integers of the stats columns of a call whose rounds ran out

A graph g comes from edges(x, offsets, n_attractive, strides, mask, input) of ONE image x [K, Z, Y, X].  Every function returns the flat
label image in the numbering of the header: clusters 1 .. n in raster order of their first pixel, invalid pixels 0.
"""
import numpy as np

IN_AFFS, IN_ELF, IN_WEIGHTS = 0, 1, 2
INPUTS = {"affs": IN_AFFS, "elf": IN_ELF, "weights": IN_WEIGHTS}
ONE = np.float32(1.0)


def ord32(w):
    """the order-preserving uint32 image of float32 values (-0.0 below +0.0)"""
    b = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def weights(x, attractive, input):
    """float32 weights of float32 x by the header's table: exactly these roundings"""
    x = np.asarray(x, np.float32)
    if input == IN_AFFS:
        c = ONE - x
        return (ONE - c) if attractive else c
    if input == IN_ELF:
        return (ONE - x) if attractive else x
    return x


def keys(w, eid):
    return (ord32(w).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - eid.astype(np.uint64))


class Graph(object):
    """the existing edges of one image: p, q (flat pixels), att (bool), w (float32), eid, key (uint64), sorted by DESCENDING key;
    valid (bool [S]); missing = dict(stride, mask, nan, outside)"""


def edges(x, offsets, n_attractive, strides=None, mask=None, input=IN_AFFS):
    x = np.asarray(x, np.float32)
    K, Z, Y, X = x.shape
    S = Z * Y * X
    strides = [1, 1, 1] if strides is None else [1] * (3 - len(strides)) + [int(s) for s in strides]
    valid = np.ones(S, bool) if mask is None else (np.asarray(mask).reshape(S) != 0)
    zz, yy, xx = (a.reshape(S) for a in np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij"))
    pix = np.arange(S, dtype=np.int64)
    g = Graph()
    g.S, g.valid, g.missing = S, valid, dict(stride=0, mask=0, nan=0, outside=0)
    P, Q, A, W, E = [], [], [], [], []
    for k, off in enumerate(offsets):
        off = [0] * (3 - len(off)) + [int(o) for o in off]
        att = k < n_attractive
        qz, qy, qx = zz + off[0], yy + off[1], xx + off[2]
        ok = (qz >= 0) & (qz < Z) & (qy >= 0) & (qy < Y) & (qx >= 0) & (qx < X)
        g.missing["outside"] += int((~ok).sum())
        q = np.where(ok, (qz * Y + qy) * X + qx, 0)
        m = ok & ~(valid & valid[q])
        g.missing["mask"] += int(m.sum())
        ok &= ~m
        if not att:
            m = ok & ((zz % strides[0] != 0) | (yy % strides[1] != 0) | (xx % strides[2] != 0))
            g.missing["stride"] += int(m.sum())
            ok &= ~m
        w = weights(x[k].reshape(S), att, input)
        m = ok & np.isnan(w)
        g.missing["nan"] += int(m.sum())
        ok &= ~m
        P.append(pix[ok]); Q.append(q[ok]); W.append(w[ok]); A.append(np.full(int(ok.sum()), att)); E.append(k * S + pix[ok])
    g.p, g.q, g.w, g.att, g.eid = (np.concatenate(v) for v in (P, Q, W, A, E))
    g.key = keys(g.w, g.eid)
    order = np.argsort(g.key, kind="stable")[::-1]
    for name in ("p", "q", "w", "att", "eid", "key"):
        setattr(g, name, getattr(g, name)[order])
    return g


def raster(root, valid):
    """a root (any representative) per pixel -> ids 1 .. n in raster order of the clusters' first pixels, 0 where not valid"""
    out = np.zeros(len(root), np.int32)
    r = np.asarray(root)[valid]
    _, first, inv = np.unique(r, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int32)
    rank[np.argsort(first, kind="stable")] = np.arange(1, len(first) + 1)
    out[valid] = rank[inv]
    return out


def _find(par, a):
    while par[a] != a:
        par[a] = par[par[a]]
        a = par[a]
    return a


def sequential(g, limit=None, with_exclusions=False):
    """(a).  limit: stop after that many edges of the order (a prefix of the procedure).  with_exclusions: -> (labels, the number of
    distinct unordered pairs of exclusive roots as the procedure stands at its end: half the sum of the set sizes)"""
    par = list(range(g.S))
    excl = {}
    n = len(g.p) if limit is None else limit
    for p, q, att in zip(g.p[:n].tolist(), g.q[:n].tolist(), g.att[:n].tolist()):
        a, b = _find(par, p), _find(par, q)
        if a == b:
            continue
        ea, eb = excl.get(a), excl.get(b)
        if not att:
            if ea is None:
                ea = excl[a] = set()
            if eb is None:
                eb = excl[b] = set()
            ea.add(b)
            eb.add(a)
            continue
        if ea is not None and b in ea:
            continue
        if ea is not None and eb is not None and len(ea) > len(eb):
            a, b, ea, eb = b, a, eb, ea
        par[a] = b  # a's exclusions go to b; everyone who excluded a now excludes b
        if ea is not None:
            if eb is None:
                eb = excl[b] = set()
            for c in ea:
                excl[c].discard(a)
                excl[c].add(b)
                eb.add(c)
            del excl[a]
    labels = raster(np.array([_find(par, i) for i in range(g.S)]), g.valid)
    if not with_exclusions:
        return labels
    assert all(par[r] == r and r not in e and all(r in excl[c] for c in e) for r, e in excl.items()), "the sets are not symmetric on roots"
    return labels, sum(len(e) for e in excl.values()) // 2


def naive(g):
    """(b): a label image kept flat, and every earlier exclusion edge scanned for every attractive edge between two clusters"""
    lab = np.arange(g.S)
    rp, rq = [], []
    for p, q, att in zip(g.p.tolist(), g.q.tolist(), g.att.tolist()):
        a, b = lab[p], lab[q]
        if a == b:
            continue
        if not att:
            rp.append(p)
            rq.append(q)
            continue
        if rp:
            la, lb = lab[np.array(rp)], lab[np.array(rq)]
            if bool((((la == a) & (lb == b)) | ((la == b) & (lb == a))).any()):
                continue
        lab[lab == b] = a
    return raster(lab, g.valid)


def rounds(g, max_rounds=None, prune_table=True):
    """(c) -> (labels, rounds in which an edge was decided, edges left undecided: those that survived the last prune and were not
    decided since)"""
    return _simulate(g, max_rounds, prune_table, None, False, None)[0]


def rounds_trace(g, max_rounds=None, history=None, states=False, hooks=None):
    """(c) -> (labels, used, undecided_slots, merged, active) as the state stands after the last round run, the round's rebuild of the
    table and the death of duplicate exclusions included.  used: the rounds in which an edge was decided.  undecided_slots: the edges
    whose state is still "undecided", those that the next round's prune would kill among them (what the kernels count; not the third
    value of rounds()).  merged, active: the edges decided as merges, the active exclusions.  A round whose prune leaves nothing ends
    the procedure and is no round of `used`: with max_rounds = n <= the rounds needed the state is the one after n rounds, without the
    prune of round n + 1; with more, or None, the one after the last prune (undecided_slots == 0).
    history: a list that receives the same tuple after every round of `used`.  states: the state bytes (0 undecided, 1 dead, 2 merged,
    3 active exclusion, in the order of g's edges) are appended to every tuple.  hooks: a list that receives, per round, (the parent of
    every root as the round hooked them, before any compression; the pointer doublings that changed a pointer)."""
    return _simulate(g, max_rounds, True, history, states, hooks)[1]


def _simulate(g, max_rounds, prune_table, history, states, hooks):
    S = g.S
    n = len(g.p)
    state = np.zeros(n, np.uint8)  # 0 undecided, 1 dead, 2 merged, 3 active exclusion
    root = np.arange(S)
    hascon = np.zeros(S, bool)
    table = np.zeros(0, np.int64)
    used = 0
    und = n

    def snapshot():
        out = (raster(root, g.valid), used, int((state == 0).sum()), int((state == 2).sum()), int((state == 3).sum()))
        return out + (state.copy(),) if states else out

    while max_rounds is None or used < max_rounds:
        # prune, on the state as the round finds it
        u = np.nonzero(state == 0)[0]
        ra, rb = root[g.p[u]], root[g.q[u]]
        dead = ra == rb
        if prune_table:
            dead |= np.isin(np.minimum(ra, rb) * S + np.maximum(ra, rb), table)
        state[u[dead]] = 1
        u, ra, rb = u[~dead], ra[~dead], rb[~dead]
        und = len(u)
        if not und:
            break
        key = g.key[u]
        best = np.zeros(S, np.uint64)
        np.maximum.at(best, ra, key)
        np.maximum.at(best, rb, key)
        ba, bb = best[ra] == key, best[rb] == key
        att = g.att[u]
        pa, pb = att & ba & (bb | ~hascon[ra]), att & bb & (ba | ~hascon[rb])
        if not prune_table:  # without the prune a mutual best still has to ask the table
            both = att & ba & bb & hascon[ra] & hascon[rb] & np.isin(np.minimum(ra, rb) * S + np.maximum(ra, rb), table)
            state[u[both]] = 1
            pa &= ~both
            pb &= ~both
        act = ~att & (ba | bb)
        par = np.arange(S)
        m = pa & pb
        par[np.maximum(ra[m], rb[m])] = np.minimum(ra[m], rb[m])
        m = pa & ~pb
        par[ra[m]] = rb[m]
        m = pb & ~pa
        par[rb[m]] = ra[m]
        state[u[pa | pb]] = 2
        state[u[act]] = 3
        hascon[ra[act]] = True
        hascon[rb[act]] = True
        used += 1
        und -= int((pa | pb | act).sum())
        hooked, doublings = par, 0
        while True:  # compress by pointer jumping
            nxt = par[par]
            if np.array_equal(nxt, par):
                break
            par = nxt
            doublings += 1
        if hooks is not None:
            hooks.append((hooked, doublings))
        moved = np.nonzero(hascon & (par != np.arange(S)))[0]
        hascon[par[moved]] = True
        root = par[root]
        a = np.nonzero(state == 3)[0]
        ra, rb = root[g.p[a]], root[g.q[a]]
        assert not (ra == rb).any(), "an exclusion inside one cluster"
        code = np.minimum(ra, rb) * S + np.maximum(ra, rb)
        table, firsts = np.unique(code, return_index=True)
        dup = np.ones(len(a), bool)
        dup[firsts] = False
        state[a[dup]] = 1
        if history is not None:
            history.append(snapshot())
    return (raster(root, g.valid), used, und), snapshot()


def segment(x, offsets, n_attractive, strides=None, mask=None, input=IN_AFFS, with_rounds=False):
    """a batch x [B, K, Z, Y, X] (mask [B, Z, Y, X] or None) through (a) -> labels int32 [B, Z, Y, X], counts [B], missing int [B, 4] in
    the order of the header's stats columns: stride, mask, nan, outside.  with_rounds: two more, per image -- the exclusive pairs at
    the end of (a), and the rounds that (c) used, whose partition is held to (a)'s on the way"""
    x = np.asarray(x, np.float32)
    labels = np.zeros((x.shape[0],) + x.shape[2:], np.int32)
    counts = np.zeros(x.shape[0], np.int32)
    missing = np.zeros((x.shape[0], 4), np.int64)
    exclusions, used = np.zeros(x.shape[0], np.int64), np.zeros(x.shape[0], np.int64)
    for b in range(x.shape[0]):
        g = edges(x[b], offsets, n_attractive, strides, None if mask is None else mask[b], input)
        lab, exclusions[b] = sequential(g, with_exclusions=True)
        labels[b] = lab.reshape(x.shape[2:])
        counts[b] = lab.max() if lab.size else 0
        missing[b] = [g.missing[k] for k in ("stride", "mask", "nan", "outside")]
        if with_rounds:
            sim, used[b], left, merged, active = rounds_trace(g)
            assert np.array_equal(sim, lab) and left == 0 and active == exclusions[b] and merged == int(g.valid.sum()) - counts[b]
    return (labels, counts, missing, exclusions, used) if with_rounds else (labels, counts, missing)


def is_refinement(fine, coarse):
    """every cluster of `fine` lies inside one cluster of `coarse` (label images of one shape; 0 = invalid in both)"""
    f, c = np.asarray(fine).ravel(), np.asarray(coarse).ravel()
    if not np.array_equal(f == 0, c == 0):
        return False
    pairs = np.unique(np.stack([f, c]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1]


def graph_cases(seed, Y, X, strides, kind, masked):
    """a seeded 2D image for the host tests: 8 offsets of which 2 attract (the long ranges reach 3 and 9) -> (x [8, 1, Y, X] affinities,
    offsets, mask or None)"""
    rng = np.random.default_rng(seed)
    offsets = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-3, -3], [-9, 0], [0, -9], [3, -3]]
    if kind == "noise":
        x = rng.random((8, 1, Y, X))
    elif kind == "ties":
        x = np.full((8, 1, Y, X), 0.5)
    else:
        blob = rng.integers(0, 4, ((Y + 4) // 5, (X + 4) // 5)).repeat(5, 0).repeat(5, 1)[:Y, :X]
        x = np.zeros((8, 1, Y, X))
        for k, (dy, dx) in enumerate(offsets):
            same = np.zeros((Y, X), bool)
            if abs(dy) >= Y or abs(dx) >= X:
                continue
            ys, xs = slice(max(0, -dy), Y - max(0, dy)), slice(max(0, -dx), X - max(0, dx))
            yq, xq = slice(max(0, dy), Y - max(0, -dy)), slice(max(0, dx), X - max(0, -dx))
            same[ys, xs] = blob[ys, xs] == blob[yq, xq]
            x[k, 0] = same
        if kind == "blobs":
            x = 0.8 * x + 0.1 + 0.1 * rng.random(x.shape)
        elif kind == "quantised":
            x = np.round((0.6 * x + 0.4 * rng.random(x.shape)) * 4) / 4
    mask = (rng.random((1, Y, X)) < 0.8).astype(np.uint8) if masked else None
    return x.astype(np.float32), offsets, mask
