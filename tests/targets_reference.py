"""Target generation and class-balance weights restated in plain numpy (what tests/test_gpu_targets.py holds pea_gen_targets and
pea_label_weights to, and what tests/test_targets_host.py holds to oracle.np_gen_targets / np_weight_binary_ratio, to
synth.affinity_targets / class_balance_weights, to the goldens gtgt_2d_*.npz and to hand-written expectations), and the tables of named
cases that both files use.

What include/pea.h promises, written down directly.  For labels [B, Z, Y, X] int32, offsets o_i = (dz, dy, dx) and flags:

    inside_i(p) = [p + o_i lies in the image]
    target_i(p) = inside_i(p) ? [label(p) == label(p + o_i)  (BOTH_FOREGROUND: and both > 0)] : [PADDING]
    mask_i(p)   = inside_i(p)
    count[b,i]  = number of p with target_i(p) != 0,  S = Z * Y * X
    wtab[b,i]   = (1, 1) if count is 0 or S; else with f = clip(float64(count) / float64(S), 0.05, 0.99):
                  f > 0.5: (1, float32(f / (1 - f)))   else: (float32((1 - f) / f), 1)          -- (weight of target 1, of target 0)
    weight_i(p) = target_i(p) ? wtab[b,i,0] : wtab[b,i,1]

PEA_TGT_MASK_INSIDE changes nothing here (it speaks to the labels-in training step).  The neighbour is gathered through index grids
(every coordinate of p + o_i, tested against the image, clipped for the gather), not through slices as utils/synth.py does it, and not
pixel by pixel as the oracle does: three statements of the same rule.

Case sizing (csrc/pea_targets.h, csrc/pea_fused_labels.h).  k_gen_targets walks 2048 consecutive pixels per workgroup, 8 per lane, four
channels per step; k_gen_weights 256 pixels per workgroup.  The count kernels take a 32 x 64 tile of one plane, four channels per step
on the direct route and five on the LDS route, which needs X % 4 == 0, a 16-byte aligned label image, oz == 0 and |oy|, |ox| <= 28.
GEOMETRIES holds the smallest images that reach each of those edges."""
import functools
import importlib

import numpy as np

PADDING, BOTH_FOREGROUND, MASK_INSIDE = 1, 2, 4
FLAG_COMBOS = (0, PADDING, BOTH_FOREGROUND, PADDING | BOTH_FOREGROUND)
INT_MAX = 2 ** 31 - 1
LDS_HALO = 28  # kCntHalo: the reach of the LDS route of the count kernels


def offsets3(offsets):
    return [tuple([0] * (3 - len(o)) + [int(v) for v in o]) for o in offsets]


def class_balance(count, S):
    """-> (weight of the target-1 voxels, weight of the target-0 voxels) as float32, for `count` target-1 voxels of S"""
    count, S = int(count), int(S)
    one = np.float32(1)
    if count == 0 or count == S:
        return one, one
    f = np.float64(count) / np.float64(S)
    f = np.clip(f, 0.05, 0.99)
    if f > 0.5:
        return one, np.float32(f / (1.0 - f))
    return np.float32((1.0 - f) / f), one


def targets_reference(labels, offsets, flags=0):
    """labels [B, Z, Y, X] int32 -> (target f32 [B,K,Z,Y,X], mask u8 [B,K,Z,Y,X], weight f32 [B,K,Z,Y,X], wtab f32 [B,K,2],
    count int64 [B,K])"""
    lab = np.asarray(labels)
    assert lab.dtype == np.int32 and lab.ndim == 4
    B, Z, Y, X = lab.shape
    offs = offsets3(offsets)
    K, S = len(offs), Z * Y * X
    z, y, x = np.meshgrid(np.arange(Z, dtype=np.int64), np.arange(Y, dtype=np.int64), np.arange(X, dtype=np.int64), indexing="ij")
    target = np.empty((B, K, Z, Y, X), np.float32)
    mask = np.empty((B, K, Z, Y, X), np.uint8)
    for i, (dz, dy, dx) in enumerate(offs):
        zz, yy, xx = z + dz, y + dy, x + dx
        inside = (zz >= 0) & (zz < Z) & (yy >= 0) & (yy < Y) & (xx >= 0) & (xx < X)
        nb = lab[:, np.clip(zz, 0, Z - 1), np.clip(yy, 0, Y - 1), np.clip(xx, 0, X - 1)]
        eq = lab == nb
        if flags & BOTH_FOREGROUND:
            eq = eq & (lab > 0) & (nb > 0)
        target[:, i] = np.where(inside[None], eq, bool(flags & PADDING))
        mask[:, i] = inside[None]
    count = (target != 0).reshape(B, K, S).sum(axis=2, dtype=np.int64)
    wtab = np.empty((B, K, 2), np.float32)
    for b in range(B):
        for i in range(K):
            wtab[b, i] = class_balance(count[b, i], S)
    sel = (slice(None), slice(None), None, None, None)
    weight = np.where(target != 0, wtab[..., 0][sel], wtab[..., 1][sel]).astype(np.float32)
    return target, mask, weight, wtab, count


def seg_to_aff_reference(seg, nhood=((-1, 0, 0), (0, -1, 0), (0, 0, -1)), pad="replicate"):
    """utils/targets.py seg_to_aff: both-foreground targets without padding; with three edges and pad='replicate' the first slice of
    channel c along axis c is (seg > 0) -- its three statements, in numpy"""
    t = targets_reference(seg, nhood, BOTH_FOREGROUND)[0]
    if len(nhood) == 3 and pad == "replicate":
        fg = (np.asarray(seg) > 0).astype(np.float32)
        t[:, 0, 0] = fg[:, 0]
        t[:, 1, :, 0] = fg[:, :, 0]
        t[:, 2, :, :, 0] = fg[:, :, :, 0]
    return t


# ---- the named cases ------------------------------------------------------------------------------------------------------------------------
def multi_offset(shifts, neighbor=4):
    """utils/affinity_ours.py multi_offset, restated (test_targets_host.py holds the two together)"""
    out = []
    for s in shifts:
        out += [[-s, 0], [0, -s]] + ([[-s, -s], [-s, s]] if neighbor == 8 else [])
    return out


GEOMETRIES = {  # name -> (B, Z, Y, X)
    "lds_37x100": (2, 1, 37, 100),   # X % 4 == 0: the LDS route; ragged tile on both axes; one whole run of 2048 pixels and a ragged one
    "direct_33x67": (2, 1, 33, 67),  # X % 4 != 0: the direct route
    "tiles_70x132": (1, 1, 70, 132),  # two whole tiles and a ragged one on each axis
    "tiny_3x5": (1, 1, 3, 5),
    "one_pixel": (1, 1, 1, 1),
    "vol_5x19x23": (2, 5, 19, 23),
    "vol_3x8x12": (1, 3, 8, 12),     # in-plane table, X % 4 == 0: the LDS route per plane of a volume
}


def _k32():
    """PEA_MAX_K offsets inside the LDS halo, both signs, no two alike"""
    out = [[-s, 0] for s in (1, 2, 3, 5, 9, 13, 27, 28)] + [[0, -s] for s in (1, 2, 3, 5, 9, 13, 27, 28)]
    out += [[s, 0] for s in (1, 4, 28)] + [[0, s] for s in (1, 4, 28)]
    out += [[-1, -1], [-1, 1], [1, -1], [1, 1], [-3, 7], [7, -3], [28, 28], [-28, -28], [28, -28], [-27, 28]]
    assert len(out) == 32 and len({tuple(o) for o in out}) == 32
    return out


TABLES_2D = {
    "nb4_k10": multi_offset([1, 3, 5, 9, 27], 4),
    "nb8_k12": multi_offset([1, 3, 9], 8),
    "k1": [[0, -1]],
    "k5": multi_offset([1, 3, 9], 4)[:5],       # one step of the LDS route, two of the direct route and of k_gen_targets
    "k6": multi_offset([1, 3, 9], 4),           # two steps of both
    "k32": _k32(),
    "far_halo": [[1, 0], [0, 1], [28, 0], [0, 28], [1, 28], [28, 1], [28, 28]],  # positive offsets: the far side of the halo
    "reach28": [[-28, 0], [0, -28], [28, 28], [0, -1]],   # the last table of the LDS route ...
    "reach29": [[-29, 0], [0, -28], [28, 28], [0, -1]],   # ... and the first that leaves it: one offset one pixel longer
}
# tables that reach past the image on every channel (|o| >= the dimension along an axis: every neighbour is outside)
PAST_3x5 = [[0, -5], [-3, 0], [3, 0], [0, 5], [7, 7], [-9, 2], [1, -6], [-28, 1], [0, 29]]
PAST_1x1 = [[0, -1], [-1, 0], [1, 1], [0, 27], [-29, 0]]
TABLES_3D = {
    # a step along z on several channels, one of them longer than Z = 5 in each direction, and diagonal steps
    "oz": [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [2, 3, -4], [-6, 0, 0], [1, -1, 1], [4, 0, 0], [7, 2, 0], [0, -9, 0], [-2, 0, 3], [0, 18, 22]],
    "norm5": [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9], [-4, 0, 0]],
    "inplane": [[0, -1, 0], [0, 0, -1], [0, -3, 0], [0, 0, -3], [0, 2, 5], [0, -7, 11], [0, 7, -11]],  # oz == 0 throughout
}


def _synth():
    import __graft_entry__ as ge
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


@functools.lru_cache(maxsize=None)
def label_image(geometry, seed=3, patches=True):
    """synth.synth_labels blobs (cells of 5 pixels, ids 0 .. 6) with patches rewritten to negative ids (two of them, each over several
    pixels), to 0, to 2^31 - 1 and to -2^31 + 1.  Never -2^31: include/pea.h reserves it.  Read-only: copy before changing it."""
    B, Z, Y, X = GEOMETRIES[geometry]
    lab = _synth().synth_labels(B, (Z, Y, X), seed, cell=5, n=6).astype(np.int32)
    if patches:
        lab[:, :, 1:8, 2:9] = -3
        lab[:, :, 4:8, 6:12] = -7
        lab[:, :, 10:15, 0:6] = 0
        lab[:, :, 12:20, 9:16] = INT_MAX
        lab[:, :, 16:22, 14:21] = -INT_MAX
        lab[:, Z // 2:, Y - 3:, X - 4:] = -3  # the far corner, from the middle plane on
    lab = np.ascontiguousarray(lab)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def expected(geometry, table, flags, seed=3):
    """the restatement's answer for a named image and table, computed once (read-only arrays)"""
    tables = dict(TABLES_2D, past_3x5=PAST_3x5, past_1x1=PAST_1x1, **TABLES_3D)
    out = targets_reference(label_image(geometry, seed), tables[table], flags)
    for a in out:
        a.setflags(write=False)
    return out


def table(name):
    return dict(TABLES_2D, past_3x5=PAST_3x5, past_1x1=PAST_1x1, **TABLES_3D)[name]


# (geometry, table) pairs every flag combination runs on
CASES = [
    ("lds_37x100", "nb4_k10"), ("lds_37x100", "nb8_k12"), ("lds_37x100", "k1"), ("lds_37x100", "k5"), ("lds_37x100", "k6"),
    ("lds_37x100", "k32"), ("lds_37x100", "far_halo"), ("lds_37x100", "reach28"), ("lds_37x100", "reach29"),
    ("direct_33x67", "nb4_k10"), ("direct_33x67", "nb8_k12"), ("direct_33x67", "k1"), ("direct_33x67", "k5"), ("direct_33x67", "k6"),
    ("direct_33x67", "k32"), ("direct_33x67", "far_halo"),
    ("tiles_70x132", "nb4_k10"), ("tiles_70x132", "k32"), ("tiles_70x132", "reach28"), ("tiles_70x132", "reach29"),
    ("tiny_3x5", "past_3x5"), ("tiny_3x5", "k1"), ("one_pixel", "past_1x1"),
    ("vol_5x19x23", "oz"), ("vol_5x19x23", "norm5"), ("vol_5x19x23", "inplane"),
    ("vol_3x8x12", "inplane"), ("vol_3x8x12", "oz"),
]


# ---- class balance on its branches ---------------------------------------------------------------------------------------------------------
BALANCE_Y = 5
W19 = np.float32(19.0)                     # (1 - 0.05) / 0.05 = 18.999999999999996 in float64: 19 as float32
W99 = np.float32(0.99 / (1.0 - 0.99))      # 98.99999999999991 in float64: 99 as float32
# (labels, X, flags) -> count, f and the hand-written (weight of target 1, weight of target 0) of channel 0, the table [(0, -1)].
# "distinct": all labels differ, PADDING: target 1 exactly in column 0, count = Y, f = 1 / X.
# "constant": one label, no padding: target 0 exactly in column 0, count = Y (X - 1), f = 1 - 1 / X.
BALANCE = [
    ("distinct", 2, PADDING, (1.0, 1.0)),     # f = 0.5: neither class is the minority
    ("distinct", 20, PADDING, (W19, 1.0)),    # f = 0.05 exactly: on the clip
    ("distinct", 21, PADDING, (W19, 1.0)),    # f < 0.05: clipped
    ("distinct", 24, PADDING, (W19, 1.0)),
    ("distinct", 8, PADDING, (7.0, 1.0)),     # f = 0.125, unclipped: (1 - f) / f = 7
    ("constant", 2, 0, (1.0, 1.0)),           # f = 0.5 from the other side
    ("constant", 8, 0, (1.0, 7.0)),           # f = 0.875: f / (1 - f) = 7
    ("constant", 100, 0, (1.0, W99)),         # f = 0.99 exactly
    ("constant", 128, 0, (1.0, W99)),         # f > 0.99: clipped
    ("distinct", 24, 0, (1.0, 1.0)),          # count = 0
    ("constant", 24, PADDING, (1.0, 1.0)),    # count = S
    ("distinct", 100, PADDING, (W19, 1.0)),   # f = 0.01
]


def balance_labels(kind, X, Y=BALANCE_Y):
    """[1, 1, Y, X] int32"""
    if kind == "distinct":
        return (np.arange(Y * X, dtype=np.int32) + 1).reshape(1, 1, Y, X)
    return np.full((1, 1, Y, X), 7, np.int32)


def balance_count(kind, X, flags, Y=BALANCE_Y):
    if kind == "distinct":
        return Y if flags & PADDING else 0
    return Y * X if flags & PADDING else Y * (X - 1)
