"""GPU: the agglomeration of the fragment graph on the device (include/pea_agglo.h, csrc/pea_k_agglo.hip) through the C ABI, through
pea.agglomerate_graph / pea.agglomerate and through utils/seg_waterz.py, against the two restatements of tests/agglo_reference.py
(which test_agglo_host.py holds to each other): the sequential procedure on the tie-free cases, the simulation of the round rule on
the tied ones, including stats and the rounds used.

root, labels, counts and every column of stats are integers that the definition fixes: every comparison is torch.equal /
np.array_equal, no tolerance anywhere.  Every C call of this file runs in a guard-banded arena (arena.py): the inputs come back
untouched, every element of every output is written, nothing else changes; the workspace is lent as it is -- filled with the arena's
pattern, never prepared.  The edge counts sit in a [B, 8] table and are read with a stride of 8, as pea_rag_build's stats are; the rows
past an image's count hold edges that would change the result if they were read.

Case sizing: 600 nodes and 2500 edges are three runs of 256 ids and ten of rows, a table of 8192 slots = 32 workgroups with colliding
probes; a chain of 70 takes one merge per round; 300 leaves put 300 pairs of parallel edges on one cluster."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import agglo_reference as R
from arena import Arena

pytestmark = pytest.mark.gpu
RESUME, IGNORE_ZERO = 1, 2
CASES = {c[0]: c for c in R.TIE_FREE + R.TIED}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def tt(a):
    return torch.tensor(np.asarray(a))


def vp(t):
    return None if t is None else t.data_ptr()


class Call(object):
    """pea_agglo_merge on a list of graphs (one per image, one max_id) in an arena; run(thr, rounds, resume) enqueues one call and returns
    (root, labels, counts, stats) as device clones; check() holds the arena to its contract"""

    def __init__(self, pkg, dev, graphs, linkage, ignore_zero=False, node_size=None, skew=(0, 0, 0, 0, 0), extra_rows=7, extra_ws=0, labels=True):
        self.pkg, self.L, self.linkage, self.flags = pkg, pkg._lib.lib(), linkage, IGNORE_ZERO if ignore_zero else 0
        B, self.max_id = len(graphs), graphs[0].max_id
        self.B = B
        assert all(g.max_id == self.max_id for g in graphs)
        E = self.E = max(1, max(len(g.uv) for g in graphs) + extra_rows)
        rng = np.random.default_rng(99)
        uv = np.sort(rng.integers(1, self.max_id + 1, (B, E, 2)), axis=2).astype(np.int32)  # past the counts: edges that must not be read
        value, weight = rng.random((B, E)) * 0.01, rng.integers(1, 9, (B, E))
        counts = np.full((B, 8), -5, np.int64)
        for b, g in enumerate(graphs):
            n = len(g.uv)
            uv[b, :n], value[b, :n], weight[b, :n], counts[b, 0] = g.uv, g.value, g.weight, n
        N = self.max_id + 1
        d = self.desc(0.0, 0, 0)
        self.nb = self.L.pea_agglo_workspace_bytes(ctypes.byref(d)) + extra_ws
        ar = self.ar = Arena(self.nb + 28 * B * E + 24 * B * N + (1 << 15), dev)
        self.uv = ar.fill(ar.carve((B, E, 2), torch.int32, skew[0], name="uv"), tt(uv))
        self.ne = ar.fill(ar.carve((B, 8), torch.int64, name="n_edges"), tt(counts))
        self.value = ar.fill(ar.carve((B, E), torch.float64, skew[1], name="value"), tt(value))
        self.weight = ar.fill(ar.carve((B, E), torch.int64, skew[1], name="weight"), tt(weight))
        self.node_size = None if node_size is None else ar.fill(ar.carve((B, N), torch.int64, name="node_size"), tt(np.asarray(node_size, np.int64)))
        self.root = ar.carve((B, N), torch.int32, skew[2], name="root")
        self.labels = ar.carve((B, N), torch.int32, skew[3], name="labels") if labels else None
        self.counts = ar.carve((B,), torch.int32, skew[3], name="counts") if labels else None
        self.stats = ar.carve((B, 8), torch.int64, skew[4], name="stats")
        self.ws = ar.carve((1, self.nb // 8), torch.int64, 8, name="workspace")

    def desc(self, thr, rounds, flags):
        d = self.pkg._lib.PeaAggloDesc()
        d.B, d.max_id, d.max_edges, d.n_edges_stride, d.linkage = self.B, self.max_id, self.E, 8, self.linkage
        d.rounds, d.threshold, d.flags = rounds, thr, flags | self.flags
        return d

    def run(self, thr, rounds, resume=False):
        d = self.desc(thr, rounds, RESUME if resume else 0)
        io = self.pkg._lib.PeaAggloBuffers()
        io.uv, io.n_edges, io.value, io.weight, io.node_size = vp(self.uv), vp(self.ne), vp(self.value), vp(self.weight), vp(self.node_size)
        io.root, io.labels, io.counts, io.stats = vp(self.root), vp(self.labels), vp(self.counts), vp(self.stats)
        self.pkg._lib.check(self.L.pea_agglo_merge(ctypes.byref(d), ctypes.byref(io), ctypes.c_void_p(self.ws.data_ptr()), self.nb, None), "pea_agglo_merge")
        torch.cuda.synchronize()
        return tuple(None if t is None else t.clone() for t in (self.root, self.labels, self.counts, self.stats))

    def complete(self, thr, batch=16, limit=1024, resume=False):
        out = self.run(thr, batch, resume)
        done = batch
        while int(out[3][:, R.MERGEABLE].max()) > 0:
            assert done < limit, "not complete after %d rounds" % done
            out = self.run(thr, batch, True)
            done += batch
        return out

    def check(self):
        wr = [self.root, self.stats] + ([self.labels, self.counts] if self.labels is not None else [])
        un = [self.uv, self.ne, self.value, self.weight] + ([] if self.node_size is None else [self.node_size])
        self.ar.check(written=wr, untouched=un, scratch=[self.ws])


@functools.lru_cache(maxsize=None)
def reference(name, ignore_zero=False):
    """(graph, linkage, threshold, the finished round simulation) of a case: computed once, shared, never written"""
    _, make, linkage, thr = CASES[name]
    g = make()
    return g, linkage, thr, R.rounds(g, linkage, thr, ignore_zero)


def same(got, sim, node_size=None, ignore_zero=False, b=0, what=""):
    """image b of a result against a round simulation: every integer that the header fixes"""
    root, labels, counts, stats = got
    print(what, "stats", stats[b].tolist())
    assert np.array_equal(root[b].cpu().numpy(), sim.root), what
    want_labels, n = R.labels_of(sim.root, node_size, ignore_zero)
    if labels is not None:
        assert np.array_equal(labels[b].cpu().numpy(), want_labels) and int(counts[b]) == n, what
    assert stats[b].tolist() == sim.stats(node_size, ignore_zero), what


# ---- graph-level cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.TIE_FREE])
def test_equals_the_sequential_procedure(pkg, dev, name):
    g, linkage, thr, sim = reference(name)
    c = Call(pkg, dev, [g], linkage)
    got = c.complete(thr, batch=64)
    c.check()
    same(got, sim, what=name)
    seq_root, popped = R.sequential(g, linkage, thr)
    assert np.array_equal(got[0][0].cpu().numpy(), seq_root) and int(got[3][0, R.MERGES]) == len(popped), name
    if name == "single below":
        assert got[0].tolist() == [[0, 1, 1, 3]] and got[1].tolist() == [[1, 2, 2, 3]] and got[2].tolist() == [3]
    if name in ("single above", "single at"):
        assert got[0].tolist() == [[0, 1, 2, 3]] and got[3][0, :4].tolist() == [0, 1, 0, 0]
    if name.startswith("chain"):
        assert int(got[3][0, R.ROUNDS]) == int(got[3][0, R.MERGES]) == 63  # one merge per round
    if name == "star":
        assert int(got[3][0, R.ROUNDS]) > 250


@pytest.mark.parametrize("name", [c[0] for c in R.TIED])
def test_tied_cases_equal_the_round_simulation(pkg, dev, name):
    g, linkage, thr, sim = reference(name)
    for graph in (g, g.shuffled(11)):  # the order of the rows does not show
        c = Call(pkg, dev, [graph], linkage)
        got = c.complete(thr, batch=64)
        c.check()
        same(got, sim, what=name)


def test_zero_edges_and_three_images_of_different_size(pkg, dev):
    g, linkage, thr, sim = reference("random mean")
    small = R.Graph(g.uv[:40], g.value[:40], g.weight[:40], g.max_id)
    empty = R.Graph(np.zeros((0, 2)), [], [], g.max_id)
    c = Call(pkg, dev, [empty], R.MEAN)
    got = c.run(0.5, 3)
    c.check()
    assert got[0][0].tolist() == list(range(g.max_id + 1)) and got[3][0].tolist() == [0, 0, 0, 0, g.max_id + 1, 0, 0, 0]
    c = Call(pkg, dev, [g, empty, small], linkage)  # image isolation, and the per-image finished word: the images end at different rounds
    got = c.complete(thr, batch=8)
    c.check()
    same(got, sim, b=0, what="full")
    same(got, R.rounds(empty, linkage, thr), b=1, what="empty")
    same(got, R.rounds(small, linkage, thr), b=2, what="small")
    assert len({int(v) for v in got[3][:, R.ROUNDS]}) == 3


def test_ignore_zero_node_sizes_and_no_labels(pkg, dev):
    g = R.random_graph(200, 700, seed=21)
    uv = g.uv.copy()
    uv[::9, 0] = 0  # rows with an end 0: edges without the flag, no edges with it
    g = R.Graph(uv, g.value, g.weight, g.max_id)
    sizes = np.random.default_rng(22).integers(0, 3, g.max_id + 1)
    for iz in (False, True):
        sim = R.rounds(g, R.MEAN, 0.4, iz)
        assert (sim.no_edge > 0) == iz
        c = Call(pkg, dev, [g], R.MEAN, ignore_zero=iz, node_size=sizes[None])
        got = c.complete(0.4)
        c.check()
        same(got, sim, sizes, iz, what="ignore_zero=%s" % iz)
    c = Call(pkg, dev, [g], R.MEAN, labels=False)  # labels and counts are optional
    got = c.complete(0.4)
    c.check()
    assert np.array_equal(got[0][0].cpu().numpy(), R.rounds(g, R.MEAN, 0.4).root)


def test_round_budget_and_resume_on_the_rising_chain(pkg, dev):
    g, linkage, thr, sim = reference("chain rising")
    c = Call(pkg, dev, [g], linkage)
    got = c.run(thr, 10)
    same(got, R.rounds(g, linkage, thr, max_rounds=10), what="10 rounds")
    assert int(got[3][0, R.ROUNDS]) == int(got[3][0, R.MERGES]) == 10 and int(got[3][0, R.MERGEABLE]) == 53  # 63 merges in all
    got = c.run(thr, 30, resume=True)
    same(got, R.rounds(g, linkage, thr, max_rounds=40), what="40 rounds")
    got = c.run(thr, 30, resume=True)
    c.check()
    same(got, sim, what="70 rounds")


def test_one_round_at_a_time_resumed_equals_the_one_shot_call(pkg, dev):
    g, linkage, thr, sim = reference("random mean")
    one = Call(pkg, dev, [g], linkage)
    shot = one.run(thr, 64)
    one.check()
    same(shot, sim, what="one shot")
    step = Call(pkg, dev, [g], linkage)
    got = step.run(thr, 1)
    n = 1
    while int(got[3][0, R.MERGEABLE]) > 0:
        assert n < 64
        if n in (1, 2, 5, 12):  # the rounds ran out: a refinement of the final partition
            assert R.is_refinement(got[0][0].cpu().numpy(), sim.root) and not np.array_equal(got[0][0].cpu().numpy(), sim.root), n
            same(got, R.rounds(g, linkage, thr, max_rounds=n), what="%d rounds" % n)
        got = step.run(thr, 1, resume=True)
        n += 1
    step.check()
    assert n == sim.rounds and all(torch.equal(a, b) for a, b in zip(got, shot))
    again = step.run(thr, 3, resume=True)  # extra rounds change nothing
    assert all(torch.equal(a, b) for a, b in zip(again, shot))
    zero = Call(pkg, dev, [g], linkage).run(thr, 0)  # no round: every id is its own cluster
    assert zero[0][0].tolist() == list(range(g.max_id + 1)) and zero[3][0, :4].tolist() == [0, 2500, sim_mergeable_at_start(g, linkage, thr), 0]


def sim_mergeable_at_start(g, linkage, thr):
    return R.rounds(g, linkage, thr, max_rounds=0).mergeable()


def test_rising_thresholds_resumed_equal_fresh_calls_and_a_lower_one_is_refused(pkg, dev):
    g = R.random_graph()
    c = Call(pkg, dev, [g], R.MEAN)
    sim = R.Rounds(g, R.MEAN)
    for i, thr in enumerate((0.3, 0.5, 0.8)):
        got = c.complete(thr, resume=i > 0)
        fresh = Call(pkg, dev, [g], R.MEAN).complete(thr)
        # the partition and the edges left are those of a fresh call; the rounds and merges of the resumed run add up over its calls
        assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1]) and torch.equal(got[2], fresh[2])
        assert got[3][0, 1:3].tolist() == fresh[3][0, 1:3].tolist() and got[3][0, R.MERGES] == fresh[3][0, R.MERGES]
        same(got, sim.run(thr), what="threshold %r" % thr)
    last = got
    refused = c.run(0.5, 4, resume=True)  # lower than 0.8: refused on the device, -1 everywhere, the workspace stands
    c.check()
    assert all(bool((t == -1).all()) for t in refused)
    other = Call(pkg, dev, [g], R.MEAN)
    other.complete(0.3)
    other.linkage = R.MAX
    assert all(bool((t == -1).all()) for t in other.run(0.3, 1, resume=True))  # another linkage
    never = Call(pkg, dev, [g], R.MEAN)
    assert all(bool((t == -1).all()) for t in never.run(0.3, 1, resume=True))  # a workspace that no set-up wrote
    never.check()
    again = c.run(0.8, 2, resume=True)
    assert all(torch.equal(a, b) for a, b in zip(again, last))


def test_alignment_workspace_size_and_two_runs_give_the_same_bits(pkg, dev):
    g, linkage, thr, sim = reference("bad rows mean")
    base = Call(pkg, dev, [g], linkage)
    first = base.run(thr, 40)
    second = base.run(thr, 40)  # on the workspace as the first call left it
    base.check()
    same(first, sim, what="aligned")
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for skew, extra in (((4, 8, 4, 12, 8), 0), ((12, 24, 8, 4, 16), 4096)):
        c = Call(pkg, dev, [g], linkage, skew=skew, extra_ws=extra)
        got = c.run(thr, 40)
        c.check()
        assert all(torch.equal(a, b) for a, b in zip(got, first)), skew


# ---- the Python layer and the end-to-end chain ---------------------------------------------------------------------------------------------
def test_agglomerate_graph(pkg, dev):
    g, linkage, thr, sim = reference("random max")
    out = pkg.agglomerate_graph(g.uv, g.value, threshold=thr, linkage="max", max_id=g.max_id)
    assert out.complete and np.array_equal(out.root.cpu().numpy(), sim.root) and out.stats.tolist() == sim.stats()
    assert out.labels.dtype == torch.int32 and out.counts.dim() == 0 and int(out.counts) == sim.stats()[R.CLUSTERS]
    g, linkage, thr, sim = reference("random mean")
    few = pkg.agglomerate_graph(tt(g.uv).to(dev), tt(g.value).to(dev), tt(g.weight).to(dev), threshold=thr, rounds=2)
    assert not few.complete and R.is_refinement(few.root.cpu().numpy(), sim.root)
    more = few.resume(thr)
    assert more.complete and np.array_equal(more.root.cpu().numpy(), sim.root) and more.stats.tolist() == sim.stats()
    with pytest.raises(ValueError, match="lower"):
        more.resume(thr / 2)
    two = pkg.agglomerate_graph(np.stack([g.uv, g.uv]), np.stack([g.value, g.value]), np.stack([g.weight, g.weight]), threshold=thr, batched=True,
                                n_edges=[2500, 40])
    assert np.array_equal(two.root[0].cpu().numpy(), sim.root) and int(two.stat("live")[1]) + int(two.stat("merges")[1]) <= 40


def cells(shape, seed):
    """affinities [ndim, ...] of synthetic cells (utils/synth.py synth_membranes) with a little seeded noise -> (affs, boundary) float32"""
    import __graft_entry__ as ge
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    planes = 1 if len(shape) == 2 else shape[0]
    b, _ = synth.synth_membranes(planes, shape[-2], shape[-1], 7, seed, noise=0.2)
    b = np.clip(b, 0, 1).astype(np.float32)
    n = int(np.prod(shape))
    affs = []
    for k in range(len(shape)):
        ax = k + (3 - len(shape))
        nb = np.maximum(b, np.roll(b, 1, axis=ax))
        noise = synth.hash_uniform(np.arange(n, dtype=np.uint64), seed + 10 + k).reshape(b.shape)
        affs.append(np.clip(1 - nb - 0.05 * noise, 0, 1))
    affs = np.stack(affs).astype(np.float32)
    return (affs[:, 0], b[0]) if len(shape) == 2 else (affs, b)


def fragments_of(pkg, dev, boundary):
    """the package's watershed: of a volume the distance-transform watershed plane by plane, of an image the flood from a grid of seeds
    six pixels apart (about 50 fragments on 37 x 41: an over-segmentation with something to merge at every threshold)"""
    b = tt(boundary).to(dev)
    if b.dim() == 3:
        return pkg.distance_transform_watershed(b, .25, 1., sigma_weights=1., min_size=4)[0]
    seeds, _ = pkg.fragment.get_seeds(b[None], "grid", seed_distance=6)
    return pkg.seeded_watershed(b[None].contiguous(), seeds, min_size=0, stack_ids=True).labels[0]


@pytest.mark.parametrize("shape", [(37, 41), (5, 12, 20)], ids=["37x41", "5x12x20"])
def test_end_to_end_on_the_packages_fragments(pkg, dev, shape):
    affs, boundary = cells(shape, 31 + len(shape))
    A = tt(affs).to(dev)
    frag = fragments_of(pkg, dev, boundary)
    offsets = [[-1, 0], [0, -1]] if len(shape) == 2 else [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    rag = pkg.region_adjacency(frag, A, offsets, one_minus=True, ignore_zero=True)
    g = R.Graph(rag.uv, rag.mean, rag.counts, rag.n_nodes - 1)  # the RAG's own outputs
    assert len(g.uv) >= 8, "the fragments are too few for the test to say anything"
    F = frag.cpu().numpy()
    thresholds = (0.2, 0.5, 0.8)
    segs = list(pkg.agglomerate(A, thresholds, fragments=frag))
    want = []
    for thr, seg in zip(thresholds, segs):
        root, popped = R.sequential(g, R.MEAN, thr, ignore_zero=True)
        labels, n = R.labels_of(root, rag.node_sizes, True)
        want.append(labels[F])
        print(shape, "threshold", thr, "fragments", rag.n_nodes - 1, "edges", len(g.uv), "merges", len(popped), "segments", n)
        assert seg.dtype == torch.int32 and seg.is_cuda and np.array_equal(seg.cpu().numpy(), want[-1]), thr
    assert int(want[0].max()) > int(want[-1].max()) >= 1  # the thresholds differ in what they merge
    # through the C chain by hand: pea_rag_build's tables as they are -> merge -> pea_rag_project
    out = pkg.agglomerate_graph(rag, threshold=0.5, ignore_zero=True)
    assert out.complete and torch.equal(pkg.project_node_labels(frag, out.labels), segs[1])
    for link, col in (("min", rag.min), ("max", rag.max)):
        got = pkg.agglomerate_graph(rag, threshold=0.5, linkage=link, ignore_zero=True)
        sim = R.rounds(R.Graph(rag.uv, col, rag.counts, rag.n_nodes - 1), R.LINKAGES[link], 0.5, True)
        assert np.array_equal(got.root.cpu().numpy(), sim.root) and got.stats.tolist() == sim.stats(rag.node_sizes, True), link
    # numpy in, numpy out through the device
    seg_np = list(pkg.agglomerate(affs, [0.5], fragments=F))[0]
    assert isinstance(seg_np, np.ndarray) and np.array_equal(seg_np, want[1])
    mod = pkg.utils.seg_waterz
    if len(shape) == 3:  # the waterz-shaped call; its own fragments are the package's default watershed
        sf = "OneMinus<EdgeStatisticValue<RegionGraphType, MeanAffinityProvider<RegionGraphType, ScoreValue>>>"
        got = list(mod.agglomerate(A, [0.5], fragments=frag, scoring_function=sf, discretize_queue=256))[0]
        assert torch.equal(got, segs[1])
        own = list(mod.agglomerate(affs, [0.2, 0.8]))
        assert len(own) == 2 and own[0].dtype == np.uint64 and own[0].shape == shape and R.is_refinement(own[0], own[1])
        got = list(mod.agglomerate(A, [0.5], fragments=frag, scoring_function="OneMinus<MinAffinity<RegionGraphType, ScoreValue>>"))[0]
        link = pkg.agglomerate_graph(rag, threshold=0.5, linkage="max", ignore_zero=True)
        assert torch.equal(got, pkg.project_node_labels(frag, link.labels))


def test_seg_waterz_tensor_and_numpy(pkg, dev):
    affs, boundary = cells((37, 41), 33)
    A = tt(affs).to(dev)
    mask = np.ones((37, 41), np.uint8)
    mask[:6, :9] = 0
    mod = pkg.utils.seg_waterz
    for m in (None, mask):
        seg, frag = pkg.seg_waterz(A, None if m is None else tt(m).to(dev))
        assert seg.is_cuda and seg.dtype == torch.int32 and frag.dtype == torch.int32 and seg.shape == frag.shape == (37, 41)
        F = frag.cpu().numpy()
        assert np.array_equal(F, np.where(mask if m is not None else 1, mod.gen_fragment(A).cpu().numpy(), 0))
        rag = pkg.region_adjacency(frag, A, [[-1, 0], [0, -1]], one_minus=True, ignore_zero=True)
        root, _ = R.sequential(R.Graph(rag.uv, rag.mean, rag.counts, rag.n_nodes - 1), R.MEAN, 0.5, ignore_zero=True)
        want = R.labels_of(root, rag.node_sizes, True)[0][F]
        assert np.array_equal(seg.cpu().numpy(), want) and ((want == 0) == (F == 0)).all()
        sn, fn = pkg.seg_waterz(affs, m)
        assert isinstance(sn, np.ndarray) and sn.dtype == fn.dtype == np.uint64 and np.array_equal(sn, want) and np.array_equal(fn, F)
        assert np.array_equal(mod.relabel(sn), sn) and torch.equal(mod.relabel(seg), seg)  # already 1 .. n
    assert int(want.max()) >= 1


def test_graphed_call_with_fixed_rounds_replays_the_eager_result(pkg, dev):
    affs, boundary = cells((37, 41), 35)
    A = tt(affs).to(dev)
    frag = fragments_of(pkg, dev, boundary)
    max_id = int(frag.max())

    def step(A):
        return tuple(pkg.agglomerate(A, [0.3, 0.6], fragments=frag, rounds=48, max_id=max_id, capacity=1024, max_edges=512))

    eager = [t.clone() for t in step(A)]
    want = [t.clone() for t in pkg.agglomerate(A, [0.3, 0.6], fragments=frag)]
    assert all(torch.equal(a, b) for a, b in zip(eager, want))
    g = pkg.graphed(step, A)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
    A.copy_(tt(cells((37, 41), 36)[0]).to(dev))  # the input buffer refilled: the replay agglomerates what it holds now
    got = [t.clone() for t in g.replay()]
    assert all(torch.equal(a, b) for a, b in zip(got, [t.clone() for t in pkg.agglomerate(A, [0.3, 0.6], fragments=frag, rounds=48, max_id=max_id)]))
