"""The cases of the merge tests (a plain helper, no test): name -> (images [B, Y, X], passes, max_id), and their restatement computed
once.  tests/test_merge_host.py checks on the CPU that every case holds what it is named for; tests/test_gpu_merge.py runs them."""
import functools

import numpy as np

import merge_reference as R


# ---- the cases: name -> (images [B, Y, X], passes, max_id) -----------------------------------------------------------------------------
def blank(Y=21, X=21):
    return np.zeros((Y, X), np.int64)


def chain_within_a_pass():
    """5, 7, 9 single pixels in a row, 11 a block, 20 a pixel whose crop reads the chain 5 -> 7 -> 9 -> 11 (three hops).  5: rank 0 is id 0
    and rank 1 the candidate itself (ties by id ascending) -> rank 2 = 7; 7, now two pixels, is served on its stale size 1 around the
    union's centroid -> 9; 9 ties with 11 at three pixels -> 11"""
    s = blank()
    s[10, 10], s[10, 11], s[10, 12], s[9, 9] = 5, 7, 9, 20
    s[10:14, 13:17] = 11
    return s


def chain_across_passes():
    """a pixel -> a block of 8 (pass 1) -> a block of 30 (pass 2) -> a block of 400 (pass 3): the aliases are compressed between passes"""
    s = blank(40, 40)
    s[20:40, 6:26] = 4   # 400
    s[14:20, 9:14] = 3   # 30
    s[10:14, 10:12] = 2  # 8
    s[9, 10] = 1
    return s


def edges():
    """21 x 21: candidates within window // 2 of the top and of the left edge (skipped), at the bottom right corner (clipped crop, merged),
    alone in the background (two distinct ids), and a block that is rank 0 of its own crop"""
    s = blank()
    s[0, 10], s[10, 0] = 1, 2               # r0 < 0; c0 < 0
    s[20, 20], s[19, 19], s[20, 18] = 3, 4, 5   # the crop is rows 18 .. 20, columns 18 .. 20
    s[10, 10] = 6                           # 0 and 6 only
    s[4:6, 14:16] = 7                       # window 3: 7 holds 4 of its crop's 9 pixels, 8 and 9 one each
    s[3, 13], s[3, 15] = 8, 9
    return s


def zero_is_small():
    """the background has three pixels: id 0 is a candidate like any other and takes the id that fills its window"""
    s = np.full((21, 23), 1, np.int64)
    s[:, 12:] = 2
    s[10, 10:13] = 0
    s[11, 11] = 3
    return s


def sparse_ids():
    s = blank(23, 37)
    s[2:12, 2:30] = 70000
    s[12:22, 5:36] = 65536
    s[11, 10], s[12, 20], s[5, 5], s[15, 15] = 40000, 300, 69999, 1
    return s


def out_of_range():
    s = R.random_image(np.random.default_rng(77), 23, 37)
    s[3, 3], s[20, 30], s[10, 10], s[10, 11] = -1, 5000, -2 ** 31, 2 ** 31 - 1
    return s


def rnd(seed, lo=21, hi=40):
    return R.random_image(np.random.default_rng(seed), lo, hi)


def fixed(seed, Y, X):
    rng = np.random.default_rng(seed)
    while True:
        s = R.random_image(rng, min(Y, X), max(Y, X))
        if s.shape == (Y, X):
            return s


def tied(Y, X):
    """a random image on which the tie rule decides (the reversed rule gives another image)"""
    for seed in range(1000):
        s = fixed(seed, Y, X)
        if not R.tie_free(s, R.CVPPP_MERGE_PASSES):
            return s
    raise AssertionError("no tied image found")


EIGHT = ((2, 1), (3, 3), (5, 5), (9, 4), (20, 7), (30, 11), (60, 15), (150, 21))
CASES = {
    "chain within a pass": (lambda: chain_within_a_pass()[None], ((5, 5),), None),
    "chain across passes": (lambda: chain_across_passes()[None], ((5, 5), (20, 11), (50, 11)), None),
    "edges": (lambda: edges()[None], ((5, 3),), None),
    "zero is small": (lambda: zero_is_small()[None], ((5, 5),), None),
    "sparse ids": (lambda: sparse_ids()[None], R.CVPPP_MERGE_PASSES, 70000),
    "out of range": (lambda: out_of_range()[None], R.BBBC_MERGE_PASSES, 400),
    "21 x 21 tied": (lambda: tied(21, 21)[None], R.CVPPP_MERGE_PASSES, None),
    "23 x 37 tied": (lambda: tied(23, 37)[None], R.BBBC_MERGE_PASSES, None),
    "windows 1 4 45": (lambda: fixed(5, 45, 50)[None], ((3, 1), (20, 4), (300, 45)), None),
    "eight passes": (lambda: fixed(6, 23, 37)[None], EIGHT, None),
    "one pass": (lambda: fixed(7, 23, 37)[None], ((20, 11),), None),
    "threshold 0": (lambda: fixed(8, 23, 37)[None], ((0, 5), (0, 21)), None),
    "batch of three": (lambda: np.stack([fixed(11, 30, 33), tied(30, 33), np.where(fixed(12, 30, 33) > 40, 0, fixed(12, 30, 33))]), R.CVPPP_MERGE_PASSES, None),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(images, passes, max_id, [Aliased per image]) of a case: computed once, shared, never written"""
    make, passes, max_id = CASES[name]
    segs = make()
    max_id = int(segs.max()) if max_id is None else max_id
    segs.setflags(write=False)
    return segs, passes, max_id, [R.aliased_passes(s, passes, max_id) for s in segs]
