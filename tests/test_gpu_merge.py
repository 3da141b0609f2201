"""GPU: the small-segment merges on the device (include/pea_merge.h, csrc/pea_k_merge.hip) through the C ABI, through
pea.merge_small_objects and through utils/merge_objects.py, against the alias-table restatement of tests/merge_reference.py (which
test_merge_host.py holds to the literal restatement and to the fixtures made with the reference's own functions).

labels, counts and every column of stats are integers that the definition fixes: every comparison is torch.equal / np.array_equal, no
tolerance anywhere.  Every C call of this file runs in a guard-banded arena (arena.py): the input comes back untouched, every element
of every output is written, nothing else changes; the workspace is lent as it is -- filled with the arena's pattern, never prepared.

Case sizing: 21 x 21 is the smallest image that admits the window 21 of the reference's last pass; 23 x 37 has rows that straddle a
wave's run of 256 pixels and a ragged last quad; the random images have some 60 to 150 ids (one run of 256 ids), the sparse case
70001 ids (274 runs); a window of 45 fills half of the crop table's 4096 slots and takes eight strides of the workgroup over the crop."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import merge_reference as R
from arena import Arena
from conftest import GOLDEN
from merge_cases import CASES, fixed, reference

pytestmark = pytest.mark.gpu
RELABEL = 1
E_UNSUPPORTED = -3
CAND, MERGES, NEGATIVE, FEW, OUT_OF_RANGE, CHAIN = range(6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def tt(a):
    return torch.tensor(np.asarray(a))


class Call(object):
    """pea_merge_small on images [B, Y, X] in an arena; run(relabel) enqueues one call and returns (labels, counts, stats) as device
    clones; check() holds the arena to its contract"""

    def __init__(self, pkg, dev, segs, passes, max_id, skew=(0, 0, 0, 0), extra_ws=0, in_place=False):
        self.pkg, self.L, self.passes, self.max_id, self.in_place = pkg, pkg._lib.lib(), passes, max_id, in_place
        self.B, self.Y, self.X = segs.shape
        self.nb = self.L.pea_merge_workspace_bytes(ctypes.byref(self.desc(0))) + extra_ws
        assert self.nb > extra_ws
        ar = self.ar = Arena(self.nb + 8 * segs.size + (1 << 15), dev)
        self.seg = ar.fill(ar.carve(segs.shape, torch.int32, skew[0], name="seg"), tt(segs.astype(np.int32)))
        self.out = self.seg if in_place else ar.carve(segs.shape, torch.int32, skew[1], name="out")
        self.counts = ar.carve((self.B,), torch.int32, skew[2], name="counts")
        self.stats = ar.carve((self.B, 8), torch.int64, skew[3], name="stats")
        self.ws = ar.carve((1, self.nb // 8), torch.int64, 8, name="workspace")

    def desc(self, flags):
        d = self.pkg._lib.PeaMergeDesc()
        d.B, d.Y, d.X, d.max_id, d.n_passes, d.flags = self.B, self.Y, self.X, self.max_id, len(self.passes), flags
        for k, (t, w) in enumerate(self.passes):
            d.threshold[k], d.window[k] = t, w
        return d

    def raw(self, relabel=False):
        d = self.desc(RELABEL if relabel else 0)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return self.L.pea_merge_small(ctypes.byref(d), p(self.seg), p(self.out), p(self.counts), p(self.stats), p(self.ws), self.nb, None)

    def run(self, relabel=False):
        self.pkg._lib.check(self.raw(relabel), "pea_merge_small")
        torch.cuda.synchronize()
        return self.out.clone(), self.counts.clone(), self.stats.clone()

    def check(self):
        wr = [self.counts, self.stats] + ([] if self.in_place else [self.out])
        self.ar.check(written=wr, untouched=[] if self.in_place else [self.seg], scratch=[self.ws] + ([self.seg] if self.in_place else []))


def same(got, refs, max_id, relabel, what=""):
    """a result against the restatement of every image: every integer that the header fixes"""
    labels, counts, stats = got
    for b, ref in enumerate(refs):
        print(what, "image", b, "stats", stats[b].tolist())
        want, n = R.relabel(ref.labels, max_id)
        assert np.array_equal(labels[b].cpu().numpy(), want if relabel else ref.labels), (what, b)
        assert int(counts[b]) == n, (what, b)
        assert stats[b].tolist() == ref.stats, (what, b)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_through_the_c_abi(pkg, dev, name):
    segs, passes, max_id, refs = reference(name)
    for relabel in (False, True):
        c = Call(pkg, dev, segs, passes, max_id)
        same(c.run(relabel), refs, max_id, relabel, name)
        c.check()


def test_pointers_workspace_and_in_place(pkg, dev):
    segs, passes, max_id, refs = reference("batch of three")
    # element-aligned pointers: seg, out and counts 4 bytes off a 16-byte boundary, stats 8 off; a larger workspace; out == seg
    for kw in (dict(skew=(4, 12, 4, 8)), dict(skew=(8, 4, 12, 24), extra_ws=4096), dict(in_place=True), dict(in_place=True, skew=(12, 0, 0, 0))):
        for relabel in (False, True):
            c = Call(pkg, dev, segs, passes, max_id, **kw)
            same(c.run(relabel), refs, max_id, relabel, str(kw))
            c.check()
    # the same call twice on one workspace: scratch, not state
    c = Call(pkg, dev, segs, passes, max_id)
    first = c.run(True)
    again = c.run(True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    c.check()


def test_a_window_above_the_image_is_refused_before_a_launch(pkg, dev):
    segs = reference("one pass")[0]
    c = Call(pkg, dev, segs, ((20, 11),), int(segs.max()))
    c.passes = ((20, 11), (5, 25))  # 25 > min(23, 37)
    assert c.raw() == E_UNSUPPORTED
    torch.cuda.synchronize()
    c.ar.check(untouched=[c.seg])
    with pytest.raises(ValueError, match="may not exceed"):
        pkg.merge_small_objects(c.seg, passes=c.passes)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
def test_merge_small_objects_batches_strides_and_max_id(pkg, dev):
    segs, passes, max_id, refs = reference("batch of three")
    ar = Arena(16 * segs.size + (1 << 14), dev)
    x = ar.fill(ar.carve_batch_strided(segs.shape, torch.int32, 37, skew_bytes=4, name="seg"), tt(segs.astype(np.int32)))  # ragged batch stride
    out = pkg.merge_small_objects(x, passes)  # max_id=None: seg.max()
    same((out.labels, out.counts, out.stats), refs, max_id, False, "strided")
    assert out.labels.shape == x.shape and out.counts.shape == (3,) and out.stats.shape == (3, 8) and out.stats.dtype == torch.int64
    assert torch.equal(out.stat("merges"), out.stats[:, 1])
    out = pkg.merge_small_objects(x, passes, relabel=True, max_id=max_id + 1000)  # a larger id space: the same result
    same((out.labels, out.counts, out.stats), refs, max_id, True, "strided, relabel")
    one = pkg.merge_small_objects(x[1], passes, relabel=True)
    assert torch.equal(one.labels, out.labels[1]) and one.counts.dim() == 0 and one.stats.shape == (8,)
    ar.check(untouched=[x])
    # a smaller max_id: the ids above it are written through and counted
    small = pkg.merge_small_objects(x[0], passes, max_id=20)
    ref = R.aliased_passes(segs[0], passes, 20)
    assert np.array_equal(small.labels.cpu().numpy(), ref.labels) and small.stats.tolist() == ref.stats and ref.stat("out_of_range") > 0


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def test_reference_fixtures_through_merge_objects(pkg, dev):
    mod = importlib.import_module(pkg.__name__ + ".utils.merge_objects")
    g = load("gmerge_chains.npz")
    for k in range(int(g["n"])):
        f = (mod.merge_func, mod.merge_func_bbbc)[int(g["kind_%d" % k])]
        seg = g["seg_%d" % k].astype(np.uint16)  # the dtype of the validation loops
        keep = seg.copy()
        out = f(seg)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint16 and np.array_equal(out, g["out_%d" % k]) and np.array_equal(seg, keep), k
        assert np.array_equal(mod.relabel(out), g["relabel_%d" % k]), k
        t = tt(g["seg_%d" % k]).to(dev)
        got = f(t)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), g["out_%d" % k]), k
        assert np.array_equal(mod.relabel(got).cpu().numpy(), g["relabel_%d" % k]), k
        # PEA_MERGE_RELABEL in the same call
        passes = (pkg.CVPPP_MERGE_PASSES, pkg.BBBC_MERGE_PASSES)[int(g["kind_%d" % k])]
        fused = pkg.merge_small_objects(t, passes, relabel=True)
        assert np.array_equal(fused.labels.cpu().numpy(), g["relabel_%d" % k]) and int(fused.counts) == g["relabel_%d" % k].max(), k
    g = load("gmerge_passes.npz")
    for k in range(int(g["n"])):
        t, w = (int(v) for v in g["pass_%d" % k])
        assert np.array_equal(mod.merge_small_object(g["seg_%d" % k], threshold=t, window=w), g["out_%d" % k]), k
        got = mod.merge_small_object(tt(g["seg_%d" % k]).to(dev), t, w)
        assert np.array_equal(got.cpu().numpy(), g["out_%d" % k]), k
        assert np.array_equal(mod.relabel(g["out_%d" % k][None])[0], g["relabel_%d" % k]), k  # [B, Y, X]


def test_graphed_chain_replays_the_eager_result(pkg, dev):
    from mws_cases import CASES as MWS_CASES
    x, offsets, nA, strides, mask, input = MWS_CASES["quantised"]()
    X = tt(x[:, :, 0]).to(dev)
    S = int(X.shape[-2] * X.shape[-1])
    gt = tt(np.stack([fixed(21, 37, 41), fixed(22, 37, 41)]).astype(np.int32)).to(dev)

    def step(X):
        mws = pkg.mutex_watershed(X, offsets, strides, rounds=48)
        seg = pkg.merge_small_objects(mws.labels, pkg.CVPPP_MERGE_PASSES, relabel=True, max_id=S)
        return seg.labels, seg.counts, seg.stats, pkg.segmentation_scores(seg.labels, gt).table, mws.labels

    eager = [t.clone() for t in step(X)]
    g = pkg.graphed(step, X)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a, c) for a, c in zip(got, eager))
    # the eager result is the restatement's on the watershed's labels
    for b in range(2):
        ref = R.aliased_passes(eager[4][b].cpu().numpy(), R.CVPPP_MERGE_PASSES, S)
        want, n = R.relabel(ref.labels, S)
        assert np.array_equal(eager[0][b].cpu().numpy(), want) and int(eager[1][b]) == n and eager[2][b].tolist() == ref.stats
    assert int(eager[2][:, MERGES].min()) > 0
    X.copy_(tt(np.ascontiguousarray(x[::-1, :, 0])))  # the input buffer refilled: the replay merges what it holds now
    got = [t.clone() for t in g.replay()]
    assert torch.equal(got[0], eager[0].flip(0)) and torch.equal(got[2], eager[2].flip(0))
