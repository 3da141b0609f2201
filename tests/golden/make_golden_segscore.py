#!/usr/bin/env python3
"""Generate tests/golden/gss_*.npz: the CVPPP segmentation scores of the reference's utils/evaluate.py on small seeded label images
(include/pea_segscore.h says what they are).

Run on the development machine only, on the CPU (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity; the GPU box
has none):
    python tests/golden/make_golden_segscore.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the file is loaded where it lies):
    scripts_cvppp/utils/evaluate.py    BestDice (:21-59), FGBGDice (:62-78), Dice (:81-99), SymmetricBestDice (:110-118)
DiffFGLabels (:4-18) calls np.int, which this numpy no longer has; its one line, (max - min) of the one image minus (max - min) of
the other, is restated here.  skimage is not installed, so adapted_rand_error and variation_of_information have no fixture: the
header's formulas are their contract, and tests/test_segscore_host.py holds them to sklearn.

gss_2d_leaves      40 x 52, blocky ids 0 .. 8 against 0 .. 7 (0 about a quarter of the blocks)
gss_2d_offset_min  the same images with every id doubled and moved up by 3 (pred) and 5 (gt): the lowest label is not 0 and every
                   second integer between min and max is absent
gss_3d_blocks      a 4 x 12 x 14 volume
gss_one_label      a pred that holds one label only (max == min: BestDice is 0) against the gt of gss_2d_leaves
  each: pred, gt int32; best_dice = BestDice(pred, gt), best_dice_rev = BestDice(gt, pred), sbd = SymmetricBestDice(pred, gt),
        fgbg_dice = FGBGDice(pred, gt), diff_fg (the restated line), and dice_ij float64 [n, 3] = rows (i, j, Dice(pred, gt, i, j)) for a
        few label pairs, absent labels among them

Arrays only.
"""
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))


def load(ref, name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blocky(rng, spatial, block, n_ids):
    coarse = rng.integers(1, n_ids, tuple((s + block - 1) // block for s in spatial))
    coarse = np.where(rng.random(coarse.shape) < 0.25, 0, coarse)
    lab = coarse
    for ax in range(len(spatial)):
        lab = np.repeat(lab, block, axis=ax)
    return np.ascontiguousarray(lab[tuple(slice(0, s) for s in spatial)].astype(np.int32))


def write(ev, name, pred, gt):
    lo_p, hi_p, lo_g, hi_g = int(pred.min()), int(pred.max()), int(gt.min()), int(gt.max())
    pairs = [(lo_p, lo_g), (hi_p, hi_g), (lo_p + 1, lo_g + 1), (hi_p, lo_g + 1), (hi_p + 1, hi_g), (lo_p + 2, hi_g + 3)]
    dice = np.array([(i, j, ev.Dice(pred, gt, i, j)) for i, j in pairs], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), pred=pred, gt=gt,
                        best_dice=np.float64(ev.BestDice(pred, gt)), best_dice_rev=np.float64(ev.BestDice(gt, pred)),
                        sbd=np.float64(ev.SymmetricBestDice(pred, gt)), fgbg_dice=np.float64(ev.FGBGDice(pred, gt)),
                        diff_fg=np.int64((hi_p - lo_p) - (hi_g - lo_g)), dice_ij=dice)
    print(name, "sbd", ev.SymmetricBestDice(pred, gt), "fgbg", ev.FGBGDice(pred, gt))


def main():
    ev = load(sys.argv[1], "ref_evaluate", "scripts_cvppp/utils/evaluate.py")
    rng = np.random.default_rng(20240607)
    pred, gt = blocky(rng, (40, 52), 8, 9), blocky(rng, (40, 52), 6, 8)
    write(ev, "gss_2d_leaves", pred, gt)
    write(ev, "gss_2d_offset_min", 2 * pred + 3, 2 * gt + 5)
    write(ev, "gss_3d_blocks", blocky(rng, (4, 12, 14), 4, 7), blocky(rng, (4, 12, 14), 3, 6))
    write(ev, "gss_one_label", np.full_like(pred, 2), gt)


if __name__ == "__main__":
    main()
