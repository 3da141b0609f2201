#!/usr/bin/env python3
"""Generate tests/golden/gflip_rules_3d.npz: the reference's 3D convert_consistency_flip, run as it is, on all sixteen rule
combinations.

Run in the build container only (needs /root/reference; the GPU box has neither):
    python tests/golden/make_golden_flip3d.py

What is imported from the reference (nothing is copied; the file is loaded where it lies):
    scripts_ac3ac4/utils/consistency_aug.py     convert_consistency_flip (:217-228) over simple_augment_reverse_torch (:58-77):
                                                FOUR rules per sample, (z-flip, x-flip, y-flip, xy-transpose)
The module imports cv2 at its top for functions this script does not call; where cv2 is not installed an empty module of that name
stands in for it.

The fixture is data only: gt [16, 2, 3, 6, 6] float32 with distinct values (every element its own flat index, so a misplaced
element cannot hide), rules [16, 4] float32 (what the data loader hands the training loop) and out = the reference's result.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def load(name, path):
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    ref = load("ref_consistency_3d", "scripts_ac3ac4/utils/consistency_aug.py")
    rules = np.array([[(i >> 3) & 1, (i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(16)], np.float32)
    shape = (16, 2, 3, 6, 6)
    gt = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
    out = ref.convert_consistency_flip(torch.from_numpy(gt), torch.from_numpy(rules)).numpy()
    assert len(np.unique(gt)) == gt.size and out.shape == gt.shape
    path = os.path.join(OUT, "gflip_rules_3d.npz")
    np.savez_compressed(path, gt=gt, rules=rules, out=np.ascontiguousarray(out))
    print("wrote", path, os.path.getsize(path), "bytes")
