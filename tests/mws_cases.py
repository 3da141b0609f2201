"""What test_gpu_mws.py, test_gpu_mws_rounds.py and test_mws_host.py share (a helper, no test of its own): the guard-banded C call of
pea_mws_segment, the seeded cases of test_gpu_mws.py with their reference, the comparison that every complete result goes through, and
the NAMED graphs of test_gpu_mws_rounds.py -- the shapes of graph that the round rule of include/pea_mws.h is weakest on.  A case is a
function that returns (x [B, K, Z, Y, X] float32, offsets, n_attractive, strides, mask or None, input); test_mws_host.py holds every
named graph to what its name promises on the reference alone, so that a GPU test cannot pass by its input degenerating."""
import ctypes
import functools

import numpy as np
import torch

import mws_reference as R
from arena import Arena

RESUME = 1
ROUNDS, UNDECIDED, MERGES, EXCLUSIONS = 0, 1, 2, 3
OFF2 = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-3, -3], [-9, 0], [0, -9], [3, -3]]
# K = 10, two attractive; (-1, 0, 0) has edges only where Z > 1 and (-3, -3, -3) only where Z > 3; the reach 27 leaves few rows
OFF10 = [[0, -1, 0], [0, 0, -1], [-1, 0, 0], [0, -3, 0], [0, 0, -3], [0, -9, 0], [0, 0, -9], [0, -27, 0], [0, 0, -27], [-3, -3, -3]]
# 3 attractive + 9 repulsive
OFF12 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9], [-1, -3, -3], [0, 3, -3], [-4, 0, 0]]


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def tt(a):
    return torch.tensor(np.asarray(a))


def off3(offsets):
    return [[0] * (3 - len(o)) + list(o) for o in offsets]


def st3(strides):
    return [1] * (3 - len(strides)) + list(strides)


def make_desc(pkg, x, offsets, n_attractive, strides, input, rounds, flags):
    d = pkg._lib.PeaMwsDesc()
    d.B, d.K, d.Z, d.Y, d.X = x.shape
    d.n_attractive, d.input, d.rounds, d.flags = n_attractive, input, rounds, flags
    for k, o in enumerate(off3(offsets)):
        d.offsets[k][:] = o
    d.strides[:] = st3(strides)
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


# ---- the named graphs ------------------------------------------------------------------------------------------------------------------
# Weights are small integers, or integers plus a fixed offset, or multiples of a power of two: their order is exact in float32.
def frozen(x, offsets, nA, strides, mask=None, input=R.IN_WEIGHTS):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x, offsets, nA, strides, mask, input


def rising_line(X=4100, K=1):
    """w[x] = x on the one attractive channel: every pixel's best edge is the one to its right, so ONE round hooks a single chain through
    every pixel.  K = 2 adds a repulsive channel of reach 150 that is all NaN."""
    x = np.full((1, K, 1, 1, X), np.nan, np.float32)
    x[0, 0, 0, 0] = np.arange(X)
    return frozen(x, [[0, 0, -1], [0, 0, -150]][:K], 1, (1, 1, 1))


def snake(Y=65, X=67):
    """the same chain laid boustrophedon through a 2D image: the horizontal edges of every row and one vertical edge per turn (the other
    vertical slots are NaN); an edge weighs the snake index of its later end"""
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    idx = yy * X + np.where(yy % 2 == 0, xx, X - 1 - xx)
    x = np.full((1, 2, 1, Y, X), np.nan, np.float32)
    x[0, 1, 0, :, 1:] = np.maximum(idx[:, 1:], idx[:, :-1])
    turn = np.where(yy % 2 == 1, xx == X - 1, xx == 0) & (yy > 0)
    x[0, 0, 0][turn] = idx[turn]
    return frozen(x, [[-1, 0], [0, -1]], 2, (1, 1))


def falling_line(X=300, reach=150):
    """w = -x on the attractive channel, 10 + x on a repulsive one of the given reach: the first round makes every repulsive edge an
    exclusion, so every cluster has one, and from then on only the mutual best -- the leftmost edge left -- merges: one edge a round"""
    x = np.zeros((1, 2, 1, 1, X), np.float32)
    x[0, 0, 0, 0] = -np.arange(X)
    x[0, 1, 0, 0] = 10 + np.arange(X)
    return frozen(x, [[0, 0, -1], [0, 0, -reach]], 1, (1, 1, 1))


def three_tempos():
    """three images that end after 1, 299 and a few rounds: the rising line, the falling line, uniform noise"""
    rng = np.random.default_rng(40)
    x = np.concatenate([rising_line(300, 2)[0], falling_line()[0], rng.random((1, 2, 1, 1, 300)).astype(np.float32)])
    return frozen(x, [[0, 0, -1], [0, 0, -150]], 1, (1, 1, 1))


FULLEST_OFFSETS = [[-1, 0], [0, -1], [-1, -1], [-1, 1], [-2, 0], [0, -2], [-2, -2], [-2, 2]]
FULLEST_CAPACITY = 4096  # the power of two >= 2 * 6 repulsive channels * 16 * 21 lattice points = 4032


def fullest_table(seed=41):
    """every repulsive weight above every attractive one, six repulsive channels on every pixel: the first round makes most of them
    exclusions at once"""
    rng = np.random.default_rng(seed)
    x = rng.random((1, 8, 1, 16, 21))
    x[:, 2:] += 2
    return frozen(x, FULLEST_OFFSETS, 2, (1, 1))


TWIN_OFFSETS = [[-1, 0], [0, -1], [0, 1], [-3, 0], [3, 0], [-3, 0], [0, 0]]


def twins(kind):
    """channels that name one pixel pair two or three times: (0, -1) / (0, 1) attract, (-3, 0) / (3, 0) / (-3, 0) again repel; and the
    zero offset, whose every edge joins a pixel with itself.  "quantised": multiples of 0.25, so the twins tie and the edge id decides"""
    rng = np.random.default_rng(42)
    x = rng.integers(0, 8, (1, 7, 1, 13, 21)) * 0.25 if kind == "quantised" else rng.random((1, 7, 1, 13, 21))
    return frozen(x, TWIN_OFFSETS, 3, (1, 1))


POSITIVE_OFFSETS = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 3, -3], [1, -2, 4], [-1, 4, 4]]


def positive_steps(scale=1, shift=0):
    """positive steps on every axis, strides (2, 3, 3), a random mask.  The noise is a multiple of 2^-20 in [0, 1), so 2 * w + 1 is exact"""
    rng = np.random.default_rng(43)
    w = rng.integers(0, 1 << 20, (1, 6, 5, 12, 20)) * 2.0 ** -20
    mask = (rng.random((1, 5, 12, 20)) < 0.8).astype(np.uint8)
    return frozen(np.float32(scale) * w.astype(np.float32) + np.float32(shift), POSITIVE_OFFSETS, 3, (2, 3, 3), mask)


FAR = [[0, 11], [0, -11], [9, 0], [-9, 0], [2 ** 30, 0], [-2 ** 30, 0], [0, 2 ** 30], [0, -2 ** 30], [2 ** 31 - 1, 2 ** 31 - 1], [-2 ** 31, -2 ** 31]]
K32_OFFSETS = OFF2 + [[1, 0], [0, 1]] + FAR[:4] + [[1, 1], [-1, -1], [2, -2]] + FAR[4:8] + [[-8, -10], [8, 10], [-2, 2], [4, 0]] + FAR[8:] + \
    [[0, 5], [-4, -5], [-8, 0], [0, -10], [3, 3]]


def k32_far():
    """9 x 11 with 32 channels: ten whose step reaches an extent (by one, by 2^30, by the ends of int32) lie among near ones; (-8, -10)
    and (8, 10) leave one slot inside.  One value in ten is a NaN, in the far channels too"""
    assert len(K32_OFFSETS) == 32
    rng = np.random.default_rng(44)
    x = rng.random((1, 32, 1, 9, 11)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = np.nan
    return frozen(x, K32_OFFSETS, 2, (2, 2))


BIG_OFFSETS = [[-1, 0], [0, -1], [-4, 0], [0, -4]]


def more_than_65536_pixels():
    """260 x 261 = 67860 pixels = 266 runs of 256: the labelling's scan of the runs' totals carries past its first 256.  The rows 8 ..
    267 of a map of 20-pixel blobs, so that the last row of blobs begins at row 252, past pixel 65536"""
    rng = np.random.default_rng(45)
    return frozen(noisy(rng, blobs(rng, 1, 1, 268, 261, BIG_OFFSETS, cell=20)[:, :, :, 8:]), BIG_OFFSETS, 2, (2, 2), None, R.IN_AFFS)


def more_than_256_images():
    """257 images of 3 x 5: the per-image kernels (k_mws_begin, k_mws_stats) need a second workgroup"""
    rng = np.random.default_rng(46)
    return frozen(rng.random((257, 3, 1, 3, 5)), [[-1, 0], [0, -1], [-2, -2]], 2, (1, 1))


def one_channel(sign=1):
    """one attractive channel along x whose weights are a permutation of -758 .. 758 (zero among them), or its negation: the reversed
    order.  Complete, both are the rows; after ONE round they are different partitions"""
    rng = np.random.default_rng(47)
    w = (rng.permutation(37 * 41) - 758).reshape(1, 1, 1, 37, 41)
    return frozen(sign * w, [[0, -1]], 1, (1, 1))


NAMED = {
    "rising line": rising_line,
    "snake": snake,
    "falling line": falling_line,
    "falling line, reach 2": functools.partial(falling_line, reach=2),
    "three tempos": three_tempos,
    "table at its fullest": fullest_table,
    "twins quantised": functools.partial(twins, "quantised"),
    "twins noise": functools.partial(twins, "noise"),
    "positive steps 3D": positive_steps,
    "K32 far": k32_far,
    "more than 65536 pixels": more_than_65536_pixels,
    "more than 256 images": more_than_256_images,
}


def graph(case, b=0):
    """the reference's graph of image b of a case"""
    x, offsets, nA, strides, mask, input = case
    return R.edges(x[b], off3(offsets), nA, st3(strides), None if mask is None else mask[b], input)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(labels, counts, missing, exclusive pairs, rounds) of a case of CASES or NAMED: computed once, shared, never written"""
    x, offsets, nA, strides, mask, input = (CASES[name] if name in CASES else NAMED[name])()
    return R.segment(x, off3(offsets), nA, st3(strides), mask, input, with_rounds=True)


def check(what, got, ref, mask):
    """a COMPLETE result (labels, counts, stats as device tensors) against segment(.., with_rounds=True): every integer that the header
    fixes"""
    labels, counts, stats = (t.cpu().numpy() for t in got)
    rl, rc, rm, rx, ru = ref
    print(what, "counts", counts.tolist(), "stats", stats.tolist())
    assert np.array_equal(stats[:, 4:8], rm), what            # missing by stride, mask, NaN, outside
    assert (stats[:, UNDECIDED] == 0).all(), what
    assert np.array_equal(counts, rc), what
    assert np.array_equal(labels.reshape(rl.shape), rl), what
    valid = np.full(rl.shape, True) if mask is None else np.asarray(mask).reshape(rl.shape) != 0
    # every merge takes one cluster away; the exclusions are the distinct exclusive cluster pairs of the sequential procedure; the
    # rounds are those of the round rule
    assert np.array_equal(stats[:, MERGES], valid.reshape(len(rc), -1).sum(1) - rc), what
    assert np.array_equal(stats[:, EXCLUSIONS], rx), what
    assert np.array_equal(stats[:, ROUNDS], ru), what
    assert ((labels.reshape(rl.shape) == 0) == ~valid).all(), what
