"""A float64 numpy restatement of every column of pea_seg_scores (include/pea_segscore.h), from np.unique on combined keys: what the
GPU tests compare the kernels with, and what test_segscore_host.py holds to the reference's own numbers (tests/golden/gss_*.npz),
to sklearn's pair confusion matrix and to sklearn's entropies."""
import os

import numpy as np

COLUMNS = ("n_overflow", "n_bad", "best_dice", "best_dice_rev", "sbd", "diff_fg", "fgbg_dice", "voi_split", "voi_merge", "are",
           "are_precision", "are_recall", "sum_nij2", "sum_ai2", "sum_bj2", "n_prime", "n_pred_ids", "n_gt_ids", "n_pairs")
COL = {name: i for i, name in enumerate(COLUMNS)}
INTEGER_COLUMNS = ("n_overflow", "n_bad", "diff_fg", "sum_nij2", "sum_ai2", "sum_bj2", "n_prime", "n_pred_ids", "n_gt_ids", "n_pairs")
DICE_VOI_COLUMNS = ("best_dice", "best_dice_rev", "sbd", "fgbg_dice", "voi_split", "voi_merge")
ARE_COLUMNS = ("are", "are_precision", "are_recall")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ("gss_2d_leaves", "gss_2d_offset_min", "gss_3d_blocks", "gss_one_label")


def load_seg_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def contingency(pred, gt):
    """-> (pred ids, gt ids, counts) of the non-empty cells, sorted by (pred id, gt id); ids must be >= 0"""
    p, g = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    keys, counts = np.unique((p << 32) | g, return_counts=True)
    return (keys >> 32).astype(np.int64), (keys & 0xffffffff).astype(np.int64), counts.astype(np.int64)


def _xlog2x(n):
    n = n.astype(np.float64)
    return float(np.sum(n * np.log2(np.maximum(n, 1.0))))


def _best_dice(p, g, n, a, b, min_p, max_p, min_g):
    """a, b: dicts id -> pixel count"""
    if max_p == min_p:
        return 0.0
    best = {}
    for i, j, c in zip(p.tolist(), g.tolist(), n.tolist()):
        if i > min_p and j > min_g:
            d = 2.0 * c / (a[i] + b[j])
            if d > best.get(i, 0.0):
                best[i] = d
    return float(np.sum(np.array(sorted(best.values()), dtype=np.float64))) / float(max_p - min_p) if best else 0.0


def seg_reference_image(pred, gt):
    """one image -> float64 [19]"""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    out = np.full(len(COLUMNS), np.nan)
    n_bad = int((pred < 0).sum() + (gt < 0).sum())
    out[COL["n_overflow"]], out[COL["n_bad"]] = 0.0, float(n_bad)
    if n_bad:
        return out
    p, g, n = contingency(pred, gt)
    ids_p, a_n = np.unique(pred, return_counts=True)
    ids_g, b_n = np.unique(gt, return_counts=True)
    a, b = dict(zip(ids_p.tolist(), a_n.tolist())), dict(zip(ids_g.tolist(), b_n.tolist()))
    min_p, max_p, min_g, max_g = int(ids_p[0]), int(ids_p[-1]), int(ids_g[0]), int(ids_g[-1])
    bd = _best_dice(p, g, n, a, b, min_p, max_p, min_g)
    bdr = _best_dice(g, p, n, b, a, min_g, max_g, min_p)
    out[COL["best_dice"]], out[COL["best_dice_rev"]], out[COL["sbd"]] = bd, bdr, min(bd, bdr)
    out[COL["diff_fg"]] = float((max_p - min_p) - (max_g - min_g))
    fg_p, fg_g = int((pred != min_p).sum()), int((gt != min_g).sum())
    both = int(((pred != min_p) & (gt != min_g)).sum())
    out[COL["fgbg_dice"]] = 2.0 * both / (fg_p + fg_g) if fg_p + fg_g else 0.0
    # the pixels with gt != 0
    keep = g != 0
    pk, gk, nk = p[keep], g[keep], n[keep]
    n_prime = int(nk.sum())
    ap = np.bincount(np.unique(pk, return_inverse=True)[1], weights=nk).astype(np.int64) if len(pk) else np.zeros(0, np.int64)
    bp = np.bincount(np.unique(gk, return_inverse=True)[1], weights=nk).astype(np.int64) if len(gk) else np.zeros(0, np.int64)
    s_n2, s_a2, s_b2 = int(np.sum(nk * nk)), int(np.sum(ap * ap)), int(np.sum(bp * bp))
    if n_prime:
        out[COL["voi_split"]] = max(_xlog2x(bp) - _xlog2x(nk), 0.0) / n_prime
        out[COL["voi_merge"]] = max(_xlog2x(ap) - _xlog2x(nk), 0.0) / n_prime
    else:
        out[COL["voi_split"]] = out[COL["voi_merge"]] = 0.0
    P2, A2, B2 = float(s_n2 - n_prime), float(s_a2 - n_prime), float(s_b2 - n_prime)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[COL["are"]] = 1.0 - np.float64(P2) / np.float64(0.5 * A2 + 0.5 * B2)
        out[COL["are_precision"]] = np.float64(P2) / np.float64(A2)
        out[COL["are_recall"]] = np.float64(P2) / np.float64(B2)
    out[COL["sum_nij2"]], out[COL["sum_ai2"]], out[COL["sum_bj2"]], out[COL["n_prime"]] = s_n2, s_a2, s_b2, n_prime
    out[COL["n_pred_ids"]], out[COL["n_gt_ids"]], out[COL["n_pairs"]] = len(ids_p), len(ids_g), len(n)
    return out


def seg_reference(pred, gt):
    """pred, gt [B, ...] -> float64 [B, 19]"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    return np.stack([seg_reference_image(pred[b], gt[b]) for b in range(pred.shape[0])])
