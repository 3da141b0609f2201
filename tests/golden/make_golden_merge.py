#!/usr/bin/env python3
"""Generate tests/golden/gmerge_chains.npz and gmerge_passes.npz: label images before and after the reference's merge_small_object,
merge_func and relabel (include/pea_merge.h says what they are).

Run on the development machine only, on the CPU (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity; the GPU box
has none):
    python tests/golden/make_golden_merge.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the files are loaded where they lie):
    scripts_cvppp/utils/postprocessing.py       merge_small_object (:8-33), merge_func (:35-40)
    scripts_bbbc039v1/utils/postprocessing.py   merge_small_object (:9-34), merge_func (:36-41)
    scripts_cvppp/utils/seg_waterz.py           relabel (:5-19)
Those modules import cv2, h5py, PIL, skimage, waterz, mahotas and utils.show for functions that are not called here: whichever of
them is not installed gets an empty stand-in module of this file's own under its name.

The images are tests/merge_reference.py's random_image: 21 to 69 pixels a side, blocks, random specks and holes, cast to uint16 as the
validation loops do before merge_func.  CONDITION FOR A FIXTURE: a seed is kept only if the restatement with ties ranked the other way
round (id descending instead of ascending) gives the same image in every pass -- then the order that the reference's unstable
np.argsort gave to equal counts cannot have mattered, on this or any other CPU.  The maker checks that, checks that the stable
restatement equals the reference's output, and records tie_free = 1 with every case.

gmerge_chains.npz   n = 8 full merge_func chains: kind_k (0 = CVPPP, 1 = BBBC039V1), seg_k, out_k = merge_func(seg_k),
                    relabel_k = relabel(out_k)
gmerge_passes.npz   n = 16 single passes: pass_k = (threshold, window) -- the settings of both loops in turn --, seg_k,
                    out_k = merge_small_object(seg_k, threshold, window), relabel_k = relabel(out_k)
  each also: n, tie_free (int32 [n], all 1).  Images are int32.

Arrays only.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import merge_reference as R  # noqa: E402


def stand_ins():
    for name in ("cv2", "h5py", "PIL", "PIL.Image", "skimage", "waterz", "mahotas", "utils", "utils.show"):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["utils.show"], "draw_fragments_2d"):
        sys.modules["utils.show"].draw_fragments_2d = None
    if not hasattr(sys.modules["PIL"], "Image"):
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]


def load(ref, name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    stand_ins()
    warnings.simplefilter("ignore")
    post = (load(ref, "ref_post_cvppp", "scripts_cvppp/utils/postprocessing.py"), load(ref, "ref_post_bbbc", "scripts_bbbc039v1/utils/postprocessing.py"))
    relabel = load(ref, "ref_seg_waterz", "scripts_cvppp/utils/seg_waterz.py").relabel
    settings = (R.CVPPP_MERGE_PASSES, R.BBBC_MERGE_PASSES)

    chains, seed = {}, 0
    for k in range(8):
        kind = k % 2
        while True:
            seed += 1
            seg = R.random_image(np.random.default_rng(1000 + seed)).astype(np.uint16)
            if R.tie_free(seg, settings[kind]):
                break
        out = post[kind].merge_func(seg.copy())
        assert np.array_equal(out, R.chain(seg, settings[kind])), ("chain", seed)
        chains.update({"kind_%d" % k: np.int32(kind), "seg_%d" % k: seg.astype(np.int32), "out_%d" % k: out.astype(np.int32),
                       "relabel_%d" % k: relabel(out.copy()).astype(np.int32)})
    chains.update(n=np.int32(8), tie_free=np.ones(8, np.int32))
    np.savez_compressed(os.path.join(OUT, "gmerge_chains.npz"), **chains)

    singles = {}
    order = [(kind, p) for p in range(4) for kind in (0, 1)] * 2
    for k, (kind, p) in enumerate(order):
        t, w = settings[kind][p]
        while True:
            seed += 1
            seg = R.random_image(np.random.default_rng(1000 + seed)).astype(np.uint16)
            if R.tie_free(seg, ((t, w),)):
                break
        out = post[kind].merge_small_object(seg.copy(), threshold=t, window=w)
        assert np.array_equal(out, R.literal(seg, t, w)), ("pass", seed)
        singles.update({"pass_%d" % k: np.array([t, w], np.int32), "seg_%d" % k: seg.astype(np.int32), "out_%d" % k: out.astype(np.int32),
                        "relabel_%d" % k: relabel(out.copy()).astype(np.int32)})
    singles.update(n=np.int32(len(order)), tie_free=np.ones(len(order), np.int32))
    np.savez_compressed(os.path.join(OUT, "gmerge_passes.npz"), **singles)
    print("wrote gmerge_chains.npz (8 chains) and gmerge_passes.npz (%d passes); %d seeds tried" % (len(order), seed))


if __name__ == "__main__":
    main(sys.argv[1])
