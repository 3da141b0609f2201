"""The agglomeration of include/pea_agglo.h restated twice in numpy and Python integers, with the header's exact conversions and
roundings (a helper, no test of its own):

  sequential(g, thr)   "pop the live edge of lowest score, merge if below the threshold, rescore" -- waterz without queue
                       discretisation.  It ASSERTS at every pop that no other live edge has the popped score: a case that trips the
                       assertion is not a valid case for the comparison with the round rule.
  Rounds(g)            a simulation of the round rule: .run(thr, rounds) continues from where it stands, as PEA_AGGLO_RESUME does, and
                       .stats() gives the columns of the C call.

and the graph cases that test_agglo_host.py and test_gpu_agglo.py share.  A graph is Graph(uv [E, 2] int32, value [E] float64, weight
[E] int64, max_id); clean() turns its rows into {(u, v): payload} as the set-up of the C call does."""
import math

import numpy as np

MEAN, MIN, MAX = 0, 1, 2
LINKAGES = {"mean": MEAN, "min": MIN, "max": MAX}
ROUNDS, LIVE, MERGEABLE, MERGES, CLUSTERS, NO_EDGE, BAD_VALUE = range(7)
F32 = np.float32
INF = F32(np.inf)


def ord32(x):
    """the order-preserving uint32 image of an f32 (pea_ws.h), as a Python int"""
    b = int(np.asarray(x, F32).view(np.uint32))
    return (~b) & 0xFFFFFFFF if b >> 31 else b | 0x80000000


def unord32(o):
    b = o ^ 0x80000000 if o >> 31 else (~o) & 0xFFFFFFFF
    return np.array(b, np.uint32).view(F32)[()]


class Graph(object):
    def __init__(self, uv, value, weight, max_id):
        self.uv = np.ascontiguousarray(uv, np.int32).reshape(-1, 2)
        self.value = np.ascontiguousarray(value, np.float64)
        self.weight = np.ascontiguousarray(weight, np.int64)
        self.max_id = int(max_id)
        assert len(self.uv) == len(self.value) == len(self.weight)

    def shuffled(self, seed):
        p = np.random.default_rng(seed).permutation(len(self.uv))
        return Graph(self.uv[p], self.value[p], self.weight[p], self.max_id)


def payload(linkage, value, weight):
    """one row's payload: MEAN (low word, high word, count) of the fixed-point sum, MIN / MAX the ord of (float)value"""
    if linkage == MEAN:
        p = float(value) * float(int(weight))  # one f64 rounding
        whole = math.floor(p)
        frac = int((p - whole) * 4294967296.0)  # exact: p - whole is exact in [0, 1)
        return (frac, int(whole), int(weight))
    return ord32(F32(value))


def combine(linkage, p, q):
    if linkage == MEAN:
        return (p[0] + q[0], p[1] + q[1], p[2] + q[2])
    return min(p, q) if linkage == MIN else max(p, q)


def score(linkage, p):
    """-> np.float32"""
    if linkage == MEAN:
        lo, hi, cnt = p
        if cnt == 0:
            return INF
        s = float(hi + (lo >> 32)) + float(lo & 0xFFFFFFFF) / 4294967296.0  # the sum rounded to f64 once
        return F32(s / float(cnt))
    return unord32(p)


def clean(g, linkage, ignore_zero=False, n=None):
    """the set-up: -> ({(u, v): payload}, rows that were no edge, rows refused for their value)"""
    edges, no_edge, bad = {}, 0, 0
    n = len(g.uv) if n is None else max(0, min(int(n), len(g.uv)))
    for (u, v), val, w in zip(g.uv[:n].tolist(), g.value[:n].tolist(), g.weight[:n].tolist()):
        if u >= v or u < 0 or v > g.max_id or (ignore_zero and u == 0):
            no_edge += 1
        elif not abs(val) <= 32768.0 or (linkage == MEAN and not 0 <= w <= 2 ** 31):
            bad += 1
        else:
            p = payload(linkage, val, w)
            edges[(u, v)] = combine(linkage, edges[(u, v)], p) if (u, v) in edges else p
    return edges, no_edge, bad


def _merge(linkage, edges, root, a, b):
    """cluster b joins a < b: every live edge re-keyed, parallel edges combined"""
    root[root == b] = a
    out = {}
    for (x, y), p in edges.items():
        x, y = (a if x == b else x), (a if y == b else y)
        if x == y:
            continue
        k = (min(x, y), max(x, y))
        out[k] = combine(linkage, out[k], p) if k in out else p
    return out


def _rescore(linkage, edges, old_edges, old_scored):
    """{edge: (ord, score)}; what an unchanged edge had is kept"""
    out = {}
    for k, p in edges.items():
        if k in old_edges and old_edges[k] == p:
            out[k] = old_scored[k]
        else:
            s = score(linkage, p)
            out[k] = (ord32(s), s)
    return out


def sequential(g, linkage, thr, ignore_zero=False, check_ties=True):
    """-> (root int32 [max_id + 1], the popped scores in order)"""
    thr = F32(thr)
    edges, _, _ = clean(g, linkage, ignore_zero)
    root = np.arange(g.max_id + 1, dtype=np.int32)
    popped = []
    scored = _rescore(linkage, edges, {}, {})
    while edges:
        k = min(scored, key=lambda e: (scored[e][0], e))
        o, s = scored[k]
        if not s < thr:
            break
        if check_ties:
            assert sum(1 for v in scored.values() if v[1] == s) == 1, "two live edges share the popped score %r" % (s,)
        popped.append(s)
        new = _merge(linkage, edges, root, *k)
        scored = _rescore(linkage, new, edges, scored)
        edges = new
    return root, popped


class Rounds(object):
    """the round rule; .root is the state, .run(thr, rounds) enqueues rounds as one C call does"""

    def __init__(self, g, linkage, ignore_zero=False, n=None):
        self.linkage = linkage
        self.edges, self.no_edge, self.bad = clean(g, linkage, ignore_zero, n)
        self.root = np.arange(g.max_id + 1, dtype=np.int32)
        self.rounds = self.merges = 0
        self.thr = None
        self.scored = _rescore(linkage, self.edges, {}, {})

    def run(self, thr, rounds=1 << 30):
        thr = F32(thr)
        assert self.thr is None or ord32(thr) >= ord32(self.thr), "a resumed call may not lower the threshold"
        self.thr = thr
        for _ in range(rounds):
            best = {}
            scored = self.scored
            for (a, b), (o, s) in scored.items():
                hi = o << 32
                best[a] = min(best.get(a, 1 << 64), hi | b)
                best[b] = min(best.get(b, 1 << 64), hi | a)
            pairs = [(a, b) for (a, b), (o, s) in scored.items() if s < thr and best[a] == (o << 32 | b) and best[b] == (o << 32 | a)]
            if not pairs:
                assert not any(s < thr for o, s in scored.values()), "progress: a round that can merge does merge"
                break
            assert len({x for pr in pairs for x in pr}) == 2 * len(pairs), "the mutual bests of a round form a matching"
            hook = np.arange(len(self.root), dtype=np.int32)
            for a, b in pairs:
                hook[b] = a
            self.root = hook[self.root]
            out = {}
            for (x, y), p in self.edges.items():
                x, y = int(hook[x]), int(hook[y])
                if x != y:
                    k = (min(x, y), max(x, y))
                    out[k] = combine(self.linkage, out[k], p) if k in out else p
            self.scored = _rescore(self.linkage, out, self.edges, scored)
            self.edges = out
            self.rounds += 1
            self.merges += len(pairs)
        return self

    def mergeable(self):
        return sum(1 for o, s in self.scored.values() if s < self.thr)

    def stats(self, node_size=None, ignore_zero=False):
        """the eight columns of the C call's stats"""
        return [self.rounds, len(self.edges), self.mergeable(), self.merges, labels_of(self.root, node_size, ignore_zero)[1], self.no_edge, self.bad, 0]


def rounds(g, linkage, thr, ignore_zero=False, max_rounds=1 << 30, n=None):
    return Rounds(g, linkage, ignore_zero, n).run(thr, max_rounds)


def labels_of(root, node_size=None, ignore_zero=False):
    """-> (labels int32, count): the clusters whose root is present numbered 1 .. n in ascending root id; 0 for an id that is not present"""
    n = len(root)
    present = np.ones(n, bool) if node_size is None else np.asarray(node_size) > 0
    if ignore_zero:
        present = present.copy()
        present[0] = False
    numbered = (root == np.arange(n)) & present
    rank = np.where(numbered, np.cumsum(numbered), 0).astype(np.int32)
    return np.where(present, rank[root], 0).astype(np.int32), int(numbered.sum())


def is_refinement(part, final):
    """every cluster of `part` lies inside one cluster of `final` (root arrays or label arrays)"""
    part, final = np.asarray(part).ravel(), np.asarray(final).ravel()
    first = {}
    for a, b in zip(part.tolist(), final.tolist()):
        if first.setdefault(a, b) != b:
            return False
    return True


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def chain(n=70, rising=True, seed=1):
    """ids 1 .. n in a row.  Rising scores: only the first edge left is a mutual best, one merge per round from the near end.  Falling
    scores: the last edge is its ends' best, one merge per round from the far end (the merged mean lies above the next edge's score)"""
    rng = np.random.default_rng(seed)
    uv = np.stack([np.arange(1, n), np.arange(2, n + 1)], 1)
    base = np.sort(rng.random(n - 1) * 0.5 + 0.01)
    value = base if rising else base[::-1]
    weight = rng.integers(1, 40, n - 1)
    return Graph(uv, value, weight, n)


def star(leaves=300, seed=2):
    """two hubs 1 and 2 joined by the cheapest edge, each joined to every leaf 3 .. leaves + 2: after the first round the merged hub
    holds a long row of parallel edges, and then collects one leaf per round"""
    rng = np.random.default_rng(seed)
    ids = np.arange(3, leaves + 3)
    uv = np.concatenate([[[1, 2]], np.stack([np.full(leaves, 1), ids], 1), np.stack([np.full(leaves, 2), ids], 1)])
    value = np.concatenate([[0.001], rng.random(2 * leaves) * 0.9 + 0.05])
    weight = rng.integers(1, 1000, len(uv))
    return Graph(uv, value, weight, leaves + 2)


def random_graph(nodes=600, edges=2500, seed=3, max_id=None):
    rng = np.random.default_rng(seed)
    pairs = set()
    while len(pairs) < edges:
        a, b = rng.integers(1, nodes + 1, 2).tolist()
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    uv = np.array(sorted(pairs))
    return Graph(uv, rng.random(edges), rng.integers(1, 5000, edges), nodes if max_id is None else max_id)


def with_bad_rows(g, seed=4):
    """duplicates of a tenth of the rows (new values), and rows that are no edge or refused for their value, shuffled in"""
    rng = np.random.default_rng(seed)
    E = len(g.uv)
    dup = rng.choice(E, E // 10, replace=False)
    bad_uv = np.array([[5, 5], [9, 3], [-1, 4], [3, g.max_id + 1], [0, 7], [2 ** 31 - 1, 4], [-7, -2]] +
                      [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12]])
    bad_val = np.array([.1] * 7 + [np.nan, np.inf, -np.inf, 32768.5, .2, .3])
    bad_wt = np.array([1] * 7 + [1, 1, 1, 1, -1, 2 ** 31 + 1])
    h = Graph(np.concatenate([g.uv, g.uv[dup], bad_uv]), np.concatenate([g.value, rng.random(len(dup)), bad_val]),
              np.concatenate([g.weight, rng.integers(0, 50, len(dup)), bad_wt]), g.max_id)
    return h.shuffled(seed)


def tied(kind, seed=5):
    """graphs on which scores tie: constant values, values in steps of 0.1, small integers (for MIN / MAX)"""
    g = random_graph(120, 400, seed)
    rng = np.random.default_rng(seed + 100)
    if kind == "constant":
        return Graph(g.uv, np.full(400, 0.25), np.full(400, 3), g.max_id)
    if kind == "steps":
        return Graph(g.uv, rng.integers(0, 10, 400) * 0.1, rng.integers(1, 4, 400), g.max_id)
    return Graph(g.uv, rng.integers(0, 6, 400).astype(np.float64), np.ones(400), g.max_id)


# (name, graph factory, linkage, threshold): no two live edges share a score when they are popped -- test_agglo_host.py checks it
TIE_FREE = [
    ("single below", lambda: Graph([[1, 2]], [0.3], [4], 3), MEAN, 0.5),
    ("single above", lambda: Graph([[1, 2]], [0.7], [4], 3), MEAN, 0.5),
    ("single at", lambda: Graph([[1, 2]], [0.5], [4], 3), MEAN, 0.5),
    ("chain rising", lambda: chain(70, True), MEAN, 0.45),
    ("chain falling", lambda: chain(70, False), MEAN, 0.45),
    ("star", lambda: star(300), MEAN, 0.8),
    ("random mean", lambda: random_graph(), MEAN, 0.35),
    ("random min", lambda: random_graph(), MIN, 0.05),
    ("random max", lambda: random_graph(), MAX, 0.6),
    ("bad rows mean", lambda: with_bad_rows(random_graph()), MEAN, 0.35),
    ("bad rows max", lambda: with_bad_rows(random_graph()), MAX, 0.6),
]
TIED = [
    ("constant mean", lambda: tied("constant"), MEAN, 0.5),
    ("constant min", lambda: tied("constant"), MIN, 0.5),
    ("steps mean", lambda: tied("steps"), MEAN, 0.45),
    ("steps max", lambda: tied("steps"), MAX, 0.45),
    ("integers min", lambda: tied("integers"), MIN, 3.0),
    ("integers max", lambda: tied("integers"), MAX, 3.0),
]
