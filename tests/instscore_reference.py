"""An integer / float64 numpy restatement of every column of pea_inst_scores (include/pea_instscore.h) and of its two match tables,
from the contingency table of np.unique on combined keys: what the GPU tests compare the kernels with, and what
test_instscore_host.py holds bit for bit to the reference's own numbers (tests/golden/gis_*.npz)."""
import os

import numpy as np

COLUMNS = ("n_overflow", "n_bad", "aji", "aji_inter", "aji_union", "dq", "sq", "pq", "tp", "fp", "fn", "sum_iou", "pixel_f1", "pix_tp",
           "pix_fp", "pix_fn", "n_pred_ids", "n_gt_ids")
COL = {name: i for i, name in enumerate(COLUMNS)}
INTEGER_COLUMNS = ("n_overflow", "n_bad", "aji_inter", "aji_union", "tp", "fp", "fn", "pix_tp", "pix_fp", "pix_fn", "n_pred_ids", "n_gt_ids")
EXACT_COLUMNS = ("aji", "dq", "pixel_f1")       # one f64 division of exact integers: bit for bit
FIXED_COLUMNS = ("sq", "pq", "sum_iou")         # through the fixed-point sum of the device: 2^-24 absolute
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ("gis_blocky", "gis_pred_doubled", "gis_gt_unmatched", "gis_equal_iou", "gis_runner_up", "gis_one_pred_id")


def load_inst_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def inst_reference_image(pred, gt, max_id=None, match_iou=0.5):
    """one image -> (float64 [18], aji_match int32 [max_id + 1], pq_match int32 [max_id + 1])"""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    if max_id is None:
        max_id = max(1, int(pred.max()), int(gt.max()))
    out = np.full(len(COLUMNS), np.nan)
    aji_match, pq_match = np.zeros(max_id + 1, np.int32), np.zeros(max_id + 1, np.int32)
    n_bad = int(((pred < 0) | (pred > max_id)).sum() + ((gt < 0) | (gt > max_id)).sum())
    out[COL["n_overflow"]], out[COL["n_bad"]] = 0.0, float(n_bad)
    if n_bad:
        return out, aji_match, pq_match
    keys, counts = np.unique((pred << 32) | gt, return_counts=True)
    n = {(int(k >> 32), int(k & 0xffffffff)): int(c) for k, c in zip(keys, counts)}
    a, b, rows = {}, {}, {}
    for (i, j), c in n.items():
        a[i] = a.get(i, 0) + c
        b[j] = b.get(j, 0) + c
        if i >= 1 and j >= 1:
            rows.setdefault(j, []).append(i)
    pred_ids, gt_ids = sorted(i for i in a if i >= 1), sorted(j for j in b if j >= 1)
    # AJI: the greedy walk in gt id order
    C = U = 0
    used = set()
    for j in gt_ids:
        best, winner, inter, union = -1.0, 1, 0, b[j] + (0 if 1 in used else a.get(1, 0))
        for i in sorted(rows.get(j, [])):
            if i in used:
                continue
            un = b[j] + a[i] - n[(i, j)]
            iou = np.float64(n[(i, j)]) / np.float64(un)
            if iou > best:  # ties: the lowest id, which comes first
                best, winner, inter, union = iou, i, n[(i, j)], un
        C += inter
        U += union
        used.add(winner)
        aji_match[j] = winner
    U += sum(a[i] for i in pred_ids if i not in used)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[COL["aji"]] = np.float64(C) / np.float64(U)
    out[COL["aji_inter"]], out[COL["aji_union"]] = C, U
    # PQ: the pairs in (gt id, pred id) order, which is the order of the reference's np.nonzero
    ious = []
    for j in gt_ids:
        for i in sorted(rows.get(j, [])):
            iou = np.float64(n[(i, j)]) / np.float64(a[i] + b[j] - n[(i, j)])
            if iou > match_iou:
                ious.append(iou)
                pq_match[j] = i
    tp = len(ious)
    fp, fn = len(pred_ids) - tp, len(gt_ids) - tp
    sum_iou = np.array(ious, dtype=np.float64).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        dq = np.float64(tp) / np.float64(tp + 0.5 * fp + 0.5 * fn)
    sq = sum_iou / (tp + 1.0e-6)
    out[COL["dq"]], out[COL["sq"]], out[COL["pq"]] = dq, sq, dq * sq
    out[COL["tp"]], out[COL["fp"]], out[COL["fn"]], out[COL["sum_iou"]] = tp, fp, fn, sum_iou
    ptp, pfp, pfn = int(((pred > 0) & (gt > 0)).sum()), int(((pred > 0) & (gt == 0)).sum()), int(((pred == 0) & (gt > 0)).sum())
    den = 2 * ptp + pfp + pfn
    out[COL["pixel_f1"]] = np.float64(2 * ptp) / np.float64(den) if den else 0.0
    out[COL["pix_tp"]], out[COL["pix_fp"]], out[COL["pix_fn"]] = ptp, pfp, pfn
    out[COL["n_pred_ids"]], out[COL["n_gt_ids"]] = len(pred_ids), len(gt_ids)
    return out, aji_match, pq_match


def inst_reference(pred, gt, max_id=None, match_iou=0.5):
    """pred, gt [B, ...] -> float64 [B, 18], aji_match int32 [B, max_id + 1], pq_match int32 [B, max_id + 1]"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if max_id is None:
        max_id = max(1, int(pred.max()), int(gt.max()))
    rows = [inst_reference_image(pred[b], gt[b], max_id, match_iou) for b in range(pred.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])


def pq_lists(pred, gt, pq_match):
    """the pairing lists of get_fast_pq from a row of pq_match -> paired_true, paired_pred, unpaired_true, unpaired_pred"""
    paired_true = np.nonzero(pq_match)[0]
    paired_pred = pq_match[paired_true]
    pt, pp = set(paired_true.tolist()), set(paired_pred.tolist())
    return (paired_true.astype(np.int64), paired_pred.astype(np.int64), [int(j) for j in np.unique(gt) if j > 0 and int(j) not in pt],
            [int(i) for i in np.unique(pred) if i > 0 and int(i) not in pp])
