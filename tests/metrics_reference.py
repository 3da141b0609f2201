"""A numpy restatement of the semantics of include/pea_metrics.h (a plain helper, no GPU): the f32 steps exactly as the header
writes them -- division, relu, the products with the mask, the clip, 1 - u and 1 - t' each a rounded float32 -- then the logarithms,
the terms and every sum in float64, the counts as integers.

    table = metrics_reference(pred, target, mask, relu=.., weight_map=.., origin=.., clip=..)     # float64 [1 + C, 5]
    stored = finished_pred(pred, relu=.., weight_map=..)                                          # what PEA_MET_STORE leaves in pred
"""
import numpy as np

F = np.float32


def _as5(a):
    a = np.asarray(a)
    return a.reshape(a.shape[:2] + (1,) * (5 - a.ndim) + a.shape[2:])


def finished_pred(pred, relu=False, weight_map=None):
    """v of every element of pred (float32, pred's shape): x, x / weight_map, relu with NaN kept"""
    v = np.asarray(pred, dtype=F).copy()
    with np.errstate(all="ignore"):
        if weight_map is not None:
            v = (v / np.asarray(weight_map, dtype=F).reshape((1, 1) + v.shape[2:])).astype(F)
        if relu:
            v = np.where(v < 0, F(0), v).astype(F)  # (a NaN compares false and stays)
    return v


def metrics_reference(pred, target, mask=None, relu=False, weight_map=None, origin=(0, 0, 0), clip=(0.0, 1.0)):
    """-> float64 [1 + C, 5]: rows (whole map, channel 0, ..), columns (mse, bce, tp, fp, fn)"""
    pred, target = _as5(np.asarray(pred, dtype=F)), _as5(np.asarray(target, dtype=F))
    B, C = target.shape[:2]
    Z, Y, X = target.shape[2:]
    oz, oy, ox = [0] * (3 - len(origin)) + [int(o) for o in origin]
    wm = None if weight_map is None else np.asarray(weight_map, dtype=F).reshape(pred.shape[2:])
    v = finished_pred(pred, relu, wm)[:, :C, oz:oz + Z, oy:oy + Y, ox:ox + X]
    m = np.ones_like(target) if mask is None else _as5(np.asarray(mask)).astype(F)
    lo, hi = F(clip[0]), F(clip[1])
    with np.errstate(all="ignore"):
        a = (v * m).astype(F)
        t = (target * m).astype(F)
        cl = np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(F)  # the select form: NaN stays NaN
        u = (cl * m).astype(F)
        omu = (F(1) - u).astype(F)
        omt = (F(1) - t).astype(F)
        d = (a - t).astype(F)
        sq = d.astype(np.float64) ** 2
        l1 = np.log(u.astype(np.float64))
        l2 = np.log(omu.astype(np.float64))
        l1 = np.where(l1 < -100.0, -100.0, l1)  # (NaN stays)
        l2 = np.where(l2 < -100.0, -100.0, l2)
        bce = -(t.astype(np.float64) * l1 + omt.astype(np.float64) * l2)
    gb = t < F(1)
    pb = u <= F(0.5)  # (false for NaN)
    n = float(B * Z * Y * X)
    out = np.zeros((1 + C, 5), dtype=np.float64)
    tot = np.zeros(2, dtype=np.float64)
    for c in range(C):
        sums = (sq[:, c].sum(), bce[:, c].sum())
        tot += sums  # (in channel order, as the finish does)
        out[1 + c, 0] = sums[0] / n
        out[1 + c, 1] = sums[1] / n
        out[1 + c, 2] = int(np.count_nonzero(gb[:, c] & pb[:, c]))
        out[1 + c, 3] = int(np.count_nonzero(~gb[:, c] & pb[:, c]))
        out[1 + c, 4] = int(np.count_nonzero(gb[:, c] & ~pb[:, c]))
    out[0, :2] = tot / (C * n)
    out[0, 2:] = out[1:, 2:].sum(axis=0)
    return out


def f1(tp, fp, fn):
    """2 tp / (2 tp + fp + fn); 0.0 where the denominator is 0 (sklearn's zero_division default)"""
    den = 2 * tp + fp + fn
    return 2.0 * tp / den if den else 0.0
