"""GPU: the mutex watershed on the device (include/pea_mws.h, csrc/pea_k_mws.hip) through the C ABI, through pea.mutex_watershed and
through seg_mutex, against the sequential definition restated in tests/mws_reference.py (which test_mws_host.py holds to a naive
second form and to a simulation of the round rule).

labels, counts and the missing-edge columns of stats are integers that the definition fixes: every comparison is torch.equal /
np.array_equal, no tolerance anywhere.  Every C call of this file runs in a guard-banded arena (arena.py): the inputs come back
untouched, every element of every output is written, nothing else changes; the workspace is lent as it is -- filled with the arena's
pattern, never prepared.

Case sizing: 37 x 41 is six runs of 256 pixels with a ragged one; 3 x 300 has a row that crosses a run; 33 x 65 x 2 and 5 x 12 x 20 step
along z; three images of different content exercise image isolation; reaches 9 and 27 leave channels with few or no edges."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import mws_reference as R
from arena import Arena

pytestmark = pytest.mark.gpu
RESUME = 1
ROUNDS, UNDECIDED, MERGES, EXCLUSIONS = 0, 1, 2, 3
OFF2 = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-3, -3], [-9, 0], [0, -9], [3, -3]]
# K = 10, two attractive; (-1, 0, 0) has edges only where Z > 1 and (-3, -3, -3) only where Z > 3; the reach 27 leaves few rows
OFF10 = [[0, -1, 0], [0, 0, -1], [-1, 0, 0], [0, -3, 0], [0, 0, -3], [0, -9, 0], [0, 0, -9], [0, -27, 0], [0, 0, -27], [-3, -3, -3]]
# 3 attractive + 9 repulsive
OFF12 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9], [-1, -3, -3], [0, 3, -3], [-4, 0, 0]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def tt(a):
    return torch.tensor(np.asarray(a))


def off3(offsets):
    return [[0] * (3 - len(o)) + list(o) for o in offsets]


def make_desc(pkg, x, offsets, n_attractive, strides, input, rounds, flags):
    d = pkg._lib.PeaMwsDesc()
    d.B, d.K, d.Z, d.Y, d.X = x.shape
    d.n_attractive, d.input, d.rounds, d.flags = n_attractive, input, rounds, flags
    for k, o in enumerate(off3(offsets)):
        d.offsets[k][:] = o
    d.strides[:] = [1] * (3 - len(strides)) + list(strides)
    return d


class Call(object):
    """pea_mws_segment on numpy x [B, K, Z, Y, X] (mask [B, Z, Y, X] or None) in an arena; run(rounds, resume) enqueues one call and
    returns (labels, counts, stats) as device clones; check() holds the arena to its contract"""

    def __init__(self, pkg, dev, x, offsets, n_attractive=2, strides=(1, 1), mask=None, input=R.IN_AFFS, skew=(0, 0, 0, 0, 0)):
        self.pkg, self.L = pkg, pkg._lib.lib()
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.args = (x, offsets, n_attractive, strides, input)
        d = make_desc(pkg, x, offsets, n_attractive, strides, input, 0, 0)
        self.nb = self.L.pea_mws_workspace_bytes(ctypes.byref(d))
        S = x[0, 0].size
        assert self.nb % 8 == 0 and self.nb >= (25 + x.shape[1]) * x.shape[0] * S
        ar = self.ar = Arena(self.nb + x.nbytes + 16 * x.shape[0] * S + (1 << 15), dev)
        self.X = ar.fill(ar.carve(x.shape, torch.float32, skew[0], name="x"), tt(x))
        self.M = None if mask is None else ar.fill(ar.carve(mask.shape, torch.uint8, skew[1], name="mask"), tt(np.asarray(mask, np.uint8)))
        self.labels = ar.carve((x.shape[0],) + x.shape[2:], torch.int32, skew[2], name="labels")
        self.counts = ar.carve((x.shape[0],), torch.int32, skew[3], name="counts")
        self.stats = ar.carve((x.shape[0], 8), torch.int32, skew[4], name="stats")
        self.ws = ar.carve((1, self.nb // 4), torch.int32, 8, name="workspace")

    def run(self, rounds, resume=False):
        d = make_desc(self.pkg, *self.args, rounds, RESUME if resume else 0)
        self.pkg._lib.check(self.L.pea_mws_segment(ctypes.byref(d), vp(self.X), vp(self.M), vp(self.labels), vp(self.counts), vp(self.stats),
                                                   vp(self.ws), self.nb, None), "pea_mws_segment")
        torch.cuda.synchronize()
        return self.labels.clone(), self.counts.clone(), self.stats.clone()

    def complete(self, batch=8, limit=1024):
        """rounds in batches, resumed, until no image has an undecided edge"""
        out = self.run(batch)
        done = batch
        while int(out[2][:, UNDECIDED].max()) > 0:
            assert done < limit, "not complete after %d rounds" % done
            out = self.run(batch, resume=True)
            done += batch
        return out

    def check(self):
        self.ar.check(written=[self.labels, self.counts, self.stats], untouched=[self.X] + ([] if self.M is None else [self.M]), scratch=[self.ws])


@functools.lru_cache(maxsize=None)
def reference(name):
    x, offsets, nA, strides, mask, input = CASES[name]()
    return R.segment(x, off3(offsets), nA, [1] * (3 - len(strides)) + list(strides), mask, input)


def blobs(rng, B, Z, Y, X, offsets, cell=6):
    """clean affinities [B, K, Z, Y, X] of random block labels: 1 where both ends carry one label, 0 elsewhere"""
    lab = rng.integers(0, 5, (B, -(-Z // 2), -(-Y // cell), -(-X // cell))).repeat(2, 1).repeat(cell, 2).repeat(cell, 3)[:, :Z, :Y, :X]
    x = np.zeros((B, len(offsets), Z, Y, X), np.float32)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    for k, (dz, dy, dx) in enumerate(off3(offsets)):
        qz, qy, qx = zz + dz, yy + dy, xx + dx
        ok = (qz >= 0) & (qz < Z) & (qy >= 0) & (qy < Y) & (qx >= 0) & (qx < X)
        same = np.zeros((B, Z, Y, X), bool)
        same[:, ok] = lab[:, zz[ok], yy[ok], xx[ok]] == lab[:, qz[ok], qy[ok], qx[ok]]
        x[:, k] = same
    return x


def noisy(rng, clean):
    return (0.8 * clean + 0.1 + 0.1 * rng.random(clean.shape)).astype(np.float32)


def case(seed, B, Z, Y, X, offsets, nA=2, strides=(1, 1), kind="blobs", mask=None, input=R.IN_AFFS):
    def make():
        rng = np.random.default_rng(seed)
        if kind == "noise":
            x = rng.random((B, len(offsets), Z, Y, X)).astype(np.float32)
        elif kind == "equal":
            x = np.full((B, len(offsets), Z, Y, X), 0.5, np.float32)
        else:
            x = blobs(rng, B, Z, Y, X, offsets)
            if kind == "blobs":
                x = noisy(rng, x)
            elif kind == "quantised":
                x = (np.round((0.6 * x + 0.4 * rng.random(x.shape)) * 4) / 4).astype(np.float32)
        m = None
        if mask == "random":
            m = (rng.random((B, Z, Y, X)) < 0.8).astype(np.uint8)
        elif mask == "isolated":  # image 0: valid pixels that touch no other one, and a small valid block; image 1: nothing valid
            m = np.zeros((B, Z, Y, X), np.uint8)
            m[0, :, ::4, ::5] = 1
            m[0, :, 8:14, 21:30] = 1
        if input == R.IN_WEIGHTS:  # a NaN here and there, signed zeros, an infinity
            x = (x - 0.5).astype(np.float32)
            x[rng.random(x.shape) < 0.02] = np.nan
            x[rng.random(x.shape) < 0.1] = 0.0
            x[rng.random(x.shape) < 0.1] = -0.0
            x[rng.random(x.shape) < 0.01] = np.inf
            x[rng.random(x.shape) < 0.01] = -np.inf
        x.setflags(write=False)
        return x, offsets, nA, strides, m, input
    return make


CASES = {
    "1x1": case(1, 1, 1, 1, 1, OFF2),
    "1x7": case(2, 1, 1, 1, 7, OFF2),
    "3x300": case(3, 1, 1, 3, 300, OFF2, strides=(1, 2)),
    "37x41 K10 B3": case(4, 3, 1, 37, 41, OFF10, strides=(1, 2, 2)),
    "2x33x65 K10 B3": case(5, 3, 2, 33, 65, OFF10, strides=(1, 3, 3)),
    "5x12x20 K12": case(6, 2, 5, 12, 20, OFF12, nA=3, strides=(1, 2, 2)),
    "strides 1 1": case(7, 1, 1, 37, 41, OFF2, strides=(1, 1)),
    "strides 2 2": case(7, 1, 1, 37, 41, OFF2, strides=(2, 2)),
    "strides 5 5": case(7, 1, 1, 37, 41, OFF2, strides=(5, 5)),
    "strides 1 3": case(7, 1, 1, 37, 41, OFF2, strides=(1, 3)),
    "mask isolated and empty": case(8, 2, 1, 37, 41, OFF2, strides=(1, 1), mask="isolated"),
    "mask random": case(9, 2, 1, 37, 41, OFF2, strides=(2, 2), mask="random"),
    "quantised": case(10, 2, 1, 37, 41, OFF2, strides=(2, 2), kind="quantised"),
    "all equal": case(11, 1, 1, 37, 41, OFF2, strides=(1, 1), kind="equal"),
    "all equal strides 2 2": case(11, 1, 1, 37, 41, OFF2, strides=(2, 2), kind="equal"),
    "clean": case(12, 2, 1, 37, 41, OFF2, strides=(1, 1), kind="clean"),
    "noise": case(13, 2, 1, 37, 41, OFF2, strides=(1, 1), kind="noise"),
    "noise 3D": case(14, 1, 5, 12, 20, OFF12, nA=3, strides=(1, 1, 1), kind="noise"),
    "nan and zeros": case(15, 2, 1, 37, 41, OFF2, strides=(1, 2), kind="noise", mask="random", input=R.IN_WEIGHTS),
    "all attractive": case(16, 2, 1, 37, 41, OFF2, nA=8, strides=(1, 1), mask="random"),
    "elf input": case(17, 1, 1, 37, 41, OFF2, strides=(2, 2), input=R.IN_ELF),
}


def check(what, got, ref, mask):
    labels, counts, stats = (t.cpu().numpy() for t in got)
    rl, rc, rm = ref
    print(what, "counts", counts.tolist(), "stats", stats.tolist())
    assert np.array_equal(stats[:, 4:8], rm), what            # missing by stride, mask, NaN, outside
    assert (stats[:, UNDECIDED] == 0).all(), what
    assert np.array_equal(counts, rc), what
    assert np.array_equal(labels, rl), what
    valid = np.full(rl.shape, True) if mask is None else mask != 0
    # every merge takes one cluster away; the exclusions are pairs of clusters
    assert np.array_equal(stats[:, MERGES], valid.reshape(len(rc), -1).sum(1) - rc), what
    assert (stats[:, EXCLUSIONS] >= 0).all() and (stats[:, EXCLUSIONS] <= rc.astype(np.int64) * (rc - 1) // 2).all(), what
    assert ((labels == 0) == ~valid).all(), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_sequential_definition(pkg, dev, name):
    x, offsets, nA, strides, mask, input = CASES[name]()
    c = Call(pkg, dev, x[:, :, :, :, :], offsets, nA, strides, mask, input)
    got = c.complete()
    c.check()
    check(name, got, reference(name), mask)
    if name == "1x1":
        assert got[0].tolist() == [[[[1]]]] and got[2][0, :4].tolist() == [0, 0, 0, 0]
    if name == "mask isolated and empty":
        assert got[1].tolist()[1] == 0 and not bool(got[0][1].any()) and got[1].tolist()[0] >= 60  # singletons, label 0, counts = 0
    if name == "all attractive":
        assert got[2][:, EXCLUSIONS].tolist() == [0, 0]  # one cluster per connected valid region
    if name == "all equal":
        assert got[2][0, ROUNDS].item() < 40  # ties by edge id alone: the prune keeps the rounds few


def test_input_modes_order_the_edges_as_their_weights(pkg, dev):
    """the kernel's weights are the header's, bit for bit: handing it the reference's float32 weights as they are gives the same
    partition as the affinities, on a map where fl(1 - fl(1 - a)) != a decides ties"""
    rng = np.random.default_rng(20)
    a = (rng.integers(0, 6, (1, 8, 1, 37, 41)) * np.float32(0.1) + rng.integers(0, 3, (1, 8, 1, 37, 41)) * np.float32(2.0 ** -25)).astype(np.float32)
    assert (R.weights(a[:, :2], True, R.IN_AFFS) != a[:, :2]).any()
    w = np.concatenate([R.weights(a[:, :2], True, R.IN_AFFS), R.weights(a[:, 2:], False, R.IN_AFFS)], 1)
    c = np.float32(1) - a
    ref = R.segment(a, off3(OFF2), 2, [1, 2, 2], None, R.IN_AFFS)
    for x, input in ((a, R.IN_AFFS), (w, R.IN_WEIGHTS), (c, R.IN_ELF)):
        call = Call(pkg, dev, x, OFF2, 2, (2, 2), None, input)
        got = call.complete()
        call.check()
        check("input %d" % input, got, ref, None)
    # and taken as plain weights the affinities give another partition: the modes are not the same map
    other = R.segment(a, off3(OFF2), 2, [1, 2, 2], None, R.IN_WEIGHTS)
    assert not np.array_equal(other[0], ref[0])


def test_one_round_at_a_time_resumed_equals_the_one_shot_call(pkg, dev):
    name = "37x41 K10 B3"
    x, offsets, nA, strides, mask, input = CASES[name]()
    one = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    shot = one.run(64)
    one.check()
    check(name + " one shot", shot, reference(name), mask)
    step = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = step.run(1)
    n = 1
    final = reference(name)[0]
    while int(got[2][:, UNDECIDED].max()) > 0:
        assert n < 64
        if n in (1, 2, 5, 12):  # the rounds ran out: a refinement of the final partition, image by image
            assert all(R.is_refinement(got[0][b].cpu().numpy(), final[b]) for b in range(len(final))), n
            assert n > 1 or not np.array_equal(got[0].cpu().numpy(), final)
        got = step.run(1, resume=True)
        n += 1
    step.check()
    print("rounds one at a time:", n, "stats", got[2].tolist())
    assert all(torch.equal(a, b) for a, b in zip(got, shot))
    # the images end at different rounds; their stats say how many each one used, and a round more changes nothing
    assert int(shot[2][:, ROUNDS].max()) <= n <= int(shot[2][:, ROUNDS].max()) + 2
    again = step.run(3, resume=True)
    assert all(torch.equal(a, b) for a, b in zip(again, shot))
    zero = Call(pkg, dev, x, offsets, nA, strides, mask, input).run(0)  # no round: every pixel is its own cluster
    S = 37 * 41
    assert torch.equal(zero[0].cpu(), torch.arange(1, S + 1, dtype=torch.int32).reshape(1, 1, 37, 41).expand(3, 1, 37, 41)) and zero[1].tolist() == [S] * 3
    assert (zero[2][:, UNDECIDED] > 0).all() and zero[2][:, :1].tolist() == [[0]] * 3


def test_two_runs_give_the_same_bits(pkg, dev):
    for name in ("noise", "2x33x65 K10 B3"):
        x, offsets, nA, strides, mask, input = CASES[name]()
        c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
        first = c.run(64)
        second = c.run(64)  # on the workspace as the first call left it
        c.check()
        other = Call(pkg, dev, x, offsets, nA, strides, mask, input).run(64)
        assert all(torch.equal(a, b) for a, b in zip(first, second)) and all(torch.equal(a, b) for a, b in zip(first, other)), name
        check(name, first, reference(name), mask)


def test_element_aligned_pointers_in_a_guard_band(pkg, dev):
    name = "mask random"
    x, offsets, nA, strides, mask, input = CASES[name]()
    aligned = Call(pkg, dev, x, offsets, nA, strides, mask, input).complete()
    for skew in ((4, 1, 12, 4, 8), (12, 3, 4, 12, 4)):
        c = Call(pkg, dev, x, offsets, nA, strides, mask, input, skew=skew)
        got = c.complete()
        c.check()
        assert all(torch.equal(a, b) for a, b in zip(got, aligned)), skew
    check(name, aligned, reference(name), mask)


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_python_call_runs_to_completion(pkg, dev):
    for name in ("37x41 K10 B3", "5x12x20 K12", "mask random", "strides 5 5"):
        x, offsets, nA, strides, mask, input = CASES[name]()
        two_d = len(offsets[0]) == 2
        X = tt(x[:, :, 0] if two_d else x).to(dev)
        M = None if mask is None else tt(mask[:, 0] if two_d else mask).to(dev)
        out = pkg.mutex_watershed(X, offsets, strides, M, n_attractive=nA)
        rl, rc, rm = reference(name)
        assert out.labels.dtype == torch.int32 and out.labels.shape == (X.shape[:1] + X.shape[2:])
        assert np.array_equal(out.labels.cpu().numpy().reshape(rl.shape), rl) and np.array_equal(out.counts.cpu().numpy(), rc), name
        assert int(out.stat("undecided").max()) == 0 and np.array_equal(out.stats[:, 4:].cpu().numpy(), rm)
        if M is not None:  # a bool mask, and pea.foreground_mask's own output (uint8 [B, H, W])
            assert torch.equal(pkg.mutex_watershed(X, offsets, strides, M.bool(), n_attractive=nA).labels, out.labels)
            logits = torch.stack([torch.zeros_like(M, dtype=torch.float32), M.float() - 0.5], 1)
            fg = pkg.foreground_mask(logits)
            assert torch.equal(fg, M) and torch.equal(pkg.mutex_watershed(X, offsets, strides, fg, n_attractive=nA).labels, out.labels)
        one = pkg.mutex_watershed(X[1 % len(X)], offsets, strides, None if M is None else M[1 % len(X)], n_attractive=nA)  # one image in, one out
        assert torch.equal(one.labels, out.labels[1 % len(X)]) and one.counts.dim() == 0 and one.stats.shape == (8,)
    # a view that is not dense is copied
    x, offsets, nA, strides, mask, input = CASES["strides 2 2"]()
    wide = torch.zeros((1, 8, 37, 82), device=dev)
    wide[..., ::2] = tt(x[:, :, 0]).to(dev)
    assert np.array_equal(pkg.mutex_watershed(wide[..., ::2], offsets, strides).labels.cpu().numpy(), reference("strides 2 2")[0][:, 0])


def test_graphed_call_with_fixed_rounds_replays_the_eager_result(pkg, dev):
    x, offsets, nA, strides, mask, input = CASES["quantised"]()
    X = tt(x[:, :, 0]).to(dev)

    def step(X):
        out = pkg.mutex_watershed(X, offsets, strides, rounds=48)
        return out.labels, out.counts, out.stats

    eager = [t.clone() for t in step(X)]
    g = pkg.graphed(step, X)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a, c) for a, c in zip(got, eager))
    assert int(eager[2][:, UNDECIDED].max()) == 0 and np.array_equal(eager[0].cpu().numpy(), reference("quantised")[0][:, 0])
    X.copy_(tt(np.ascontiguousarray(x[::-1, :, 0])))  # the input buffer refilled: the replay segments what it holds now
    got = [t.clone() for t in g.replay()]
    assert torch.equal(got[0], eager[0].flip(0)) and torch.equal(got[1], eager[1].flip(0))
    few = pkg.mutex_watershed(X, offsets, strides, rounds=2)  # rounds too small: said in stats, and a refinement
    assert int(few.stat("undecided").min()) > 0
    assert all(R.is_refinement(few.labels[b].cpu().numpy(), got[0][b].cpu().numpy()) for b in range(2))


def test_seg_mutex_on_a_leaf_image(pkg, dev):
    """the reference's call chain: embedding -> embedding2affs(activation='relu') -> seg_mutex(affs, offsets, strides), tensor and
    numpy forms, against the sequential definition on the same floats"""
    import __graft_entry__ as ge
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    leaves = synth.synth_nuclei(1, 64, 64, 9, 11, seed=31)[0]
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((int(leaves.max()) + 1, 16)).astype(np.float32)
    e = centres[leaves].transpose(2, 0, 1)[None] + 0.15 * rng.standard_normal((1, 16, 64, 64)).astype(np.float32)
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], neighbor=4)
    affs = pkg.embedding2affs(tt(e).to(dev), offsets, activation="relu")[0]
    a = affs.cpu().numpy()
    for strides, mask in (([5, 5], None), ([1, 1], leaves > 0)):
        ref = R.segment(a[None, :, None], off3(offsets), 2, [1] + strides, None if mask is None else mask[None, None], R.IN_AFFS)[0][0, 0]
        m = None if mask is None else tt(mask).to(dev)
        got = pkg.seg_mutex(affs, offsets, strides, mask=m)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref)
        gn = pkg.seg_mutex(a, offsets, strides, mask=mask)
        assert isinstance(gn, np.ndarray) and gn.dtype == np.uint64 and np.array_equal(gn, ref)
        ge_ = pkg.elf_mutex_watershed(1.0 - affs, offsets, strides, mask=m)  # the AC3/AC4 call site hands 1 - affs
        assert np.array_equal(ge_.cpu().numpy(), R.segment((np.float32(1) - a)[None, :, None], off3(offsets), 2, [1] + strides,
                                                          None if mask is None else mask[None, None], R.IN_ELF)[0][0, 0])
        print("leaf image, strides", strides, "clusters", int(got.max()), "leaves", int(leaves.max()))
        assert 2 <= int(got.max())
