#!/usr/bin/env python3
"""Generate tests/golden/gis_*.npz: the BBBC039V1 instance scores of the reference's utils/metrics_bbbc.py on small hand-sized label
images (include/pea_instscore.h says what they are).

Run on the development machine only, on the CPU (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity; the GPU box
has none):
    python tests/golden/make_golden_instscore.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the file is loaded where it lies):
    scripts_bbbc039v1/utils/metrics_bbbc.py    agg_jc_index (:11-61), pixel_f1 (:72-80), get_fast_pq (:120-213), remap_label (:216-244)
That module imports numexpr, which is not installed here, for the one expression "m&p" of agg_jc_index: a stand-in module of this
file's own is registered under that name, whose evaluate() evaluates the expression in the caller's frame.

Every image is 24 x 28; gt ids are consecutive from 1 (agg_jc_index walks range(1, max + 1)).
gis_blocky          a typical blocky pair: 6-pixel blocks of pred against 4-pixel blocks of gt, a quarter of the blocks background
gis_pred_doubled    the same with every pred id doubled: id 1 and every second id are absent.  get_fast_pq indexes its masks by id
                    and needs consecutive ones, so it sees remap_label(pred), as the reference's driver calls it, and the pred ids
                    of its lists are mapped back to the doubled ones here
gis_gt_unmatched    a gt instance that no prediction overlaps: it takes pred id 1
gis_equal_iou       a gt instance that two predictions overlap with equal IoU (0.5 each): the lower id wins
gis_runner_up       one prediction that is the best match of two gt instances: the second takes its runner-up
gis_one_pred_id     a pred with a single foreground id against the gt of gis_blocky
  each: pred, gt int32; aji = agg_jc_index(gt, pred), pixel_f1 = pixel_f1(gt, pred), dq / sq / pq and the int64 lists paired_true,
        paired_pred, unpaired_true, unpaired_pred = get_fast_pq(gt, pred, 0.5)

Arrays only.
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
SHAPE = (24, 28)


def numexpr_stand_in():
    mod = types.ModuleType("numexpr")

    def evaluate(expr):
        frame = sys._getframe(1)
        return eval(expr, frame.f_globals, frame.f_locals)

    mod.evaluate = evaluate
    return mod


def load(ref, name, path):
    sys.modules.setdefault("numexpr", numexpr_stand_in())
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def consecutive(lab):
    ids = np.unique(lab)
    new = np.zeros(int(ids.max()) + 1, np.int32)
    new[ids[ids > 0]] = np.arange(1, int((ids > 0).sum()) + 1)
    return new[lab].astype(np.int32)


def blocky(rng, block):
    coarse = rng.permutation(np.arange(1, 1 + ((SHAPE[0] + block - 1) // block) * ((SHAPE[1] + block - 1) // block)))
    coarse = coarse.reshape((SHAPE[0] + block - 1) // block, -1)
    coarse = np.where(rng.random(coarse.shape) < 0.25, 0, coarse)
    lab = np.repeat(np.repeat(coarse, block, axis=0), block, axis=1)[:SHAPE[0], :SHAPE[1]]
    return consecutive(np.ascontiguousarray(lab))


def boxes(spec):
    lab = np.zeros(SHAPE, np.int32)
    for idx, (y0, y1, x0, x1) in spec:
        lab[y0:y1, x0:x1] = idx
    return lab


def write(mb, name, pred, gt, pq_pred=None, back=None):
    """pq_pred: what get_fast_pq sees in place of pred; back: its pred ids -> the ids of pred"""
    pred, gt = np.ascontiguousarray(pred, np.int32), np.ascontiguousarray(gt, np.int32)
    assert pred.shape == gt.shape == SHAPE and np.array_equal(np.unique(gt[gt > 0]), np.arange(1, gt.max() + 1))
    aji = mb.agg_jc_index(gt, pred)
    f1 = mb.pixel_f1(gt, pred)
    (dq, sq, pq), lists = mb.get_fast_pq(gt, pred if pq_pred is None else pq_pred, match_iou=0.5)
    paired_true, paired_pred, unpaired_true, unpaired_pred = (np.asarray(v, np.int64).reshape(-1) for v in lists)
    if back is not None:
        paired_pred, unpaired_pred = back(paired_pred), back(unpaired_pred)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), pred=pred, gt=gt, aji=np.float64(aji), pixel_f1=np.float64(f1),
                        dq=np.float64(dq), sq=np.float64(sq), pq=np.float64(pq), paired_true=paired_true, paired_pred=paired_pred,
                        unpaired_true=unpaired_true, unpaired_pred=unpaired_pred)
    print(name, "aji", aji, "dq sq pq", dq, sq, pq, "f1", f1, "pairs", len(paired_true))


def main():
    mb = load(sys.argv[1], "ref_metrics_bbbc", "scripts_bbbc039v1/utils/metrics_bbbc.py")
    rng = np.random.default_rng(20240911)
    pred, gt = blocky(rng, 6), blocky(rng, 4)
    write(mb, "gis_blocky", pred, gt)
    doubled = 2 * pred
    remapped = mb.remap_label(doubled)
    assert np.array_equal(remapped, pred)
    write(mb, "gis_pred_doubled", doubled, gt, pq_pred=remapped, back=lambda ids: 2 * ids)
    # gt 3 lies where pred is background; pred 1 is taken by gt 1 before
    write(mb, "gis_gt_unmatched",
          boxes([(1, (0, 8, 0, 8)), (2, (0, 8, 10, 19)), (3, (16, 22, 20, 27))]),
          boxes([(1, (0, 8, 0, 9)), (2, (1, 8, 10, 18)), (3, (10, 15, 2, 9)), (4, (16, 22, 19, 26))]))
    # gt 2 is halved by pred 2 and pred 3: IoU 16 / 32 each
    write(mb, "gis_equal_iou",
          boxes([(1, (12, 20, 0, 10)), (2, (0, 4, 4, 8)), (3, (0, 4, 8, 12)), (4, (12, 18, 14, 24))]),
          boxes([(1, (12, 20, 1, 10)), (2, (0, 4, 4, 12)), (3, (13, 18, 14, 25))]))
    # pred 1 covers gt 1 and most of gt 2: gt 1 takes it (36 / 66), gt 2 is left with pred 2 (6 / 36) although pred 1 is better (30 / 72)
    write(mb, "gis_runner_up",
          boxes([(1, (0, 6, 0, 11)), (2, (0, 6, 11, 12)), (3, (10, 20, 5, 15))]),
          boxes([(1, (0, 6, 0, 6)), (2, (0, 6, 6, 12)), (3, (10, 20, 4, 15))]))
    write(mb, "gis_one_pred_id", np.where(pred > 0, 1, 0), gt)


if __name__ == "__main__":
    main()
