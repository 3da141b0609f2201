#!/usr/bin/env python3
"""Generate tests/golden/gdisc_*.npz: the discriminative (pull / push) instance loss, from the reference's own code on small seeded
inputs (include/pea_disc.h says what it is).

Run on the development machine only, on the CPU (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity; the GPU box
has none):
    python tests/golden/make_golden_disc.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the file is loaded where it lies):
    scripts_ac3ac4/loss/loss_discriminative.py    discriminative_loss (:6-60)
The 3D copy indexes embedding[b][:, mask] and never looks at the spatial rank, so it takes the 2D fixture as it is; its `background`
flag stands for the two 2D copies (scripts_cvppp keeps id 0 = background=True, scripts_bbbc039v1 drops it = background=False), which
import torchvision at module level and are not loaded.  The function is run in float32 and, on the same inputs, in float64.

gdisc_2d_b3_37x53    B = 3, D = 16, S = 37 * 53 (odd); image 2 is all 0; two one-pixel ids with bit-equal vectors in image 0 (their means
                     coincide: a pair at distance exactly 0); background=False
gdisc_2d_b3_37x53_bg the same e and labels with background=True (a file of its own: both gradients in one exceed the size limit of a
                     committed file)
gdisc_3d_b2_5x20x24  B = 2, D = 16, a 5 x 20 x 24 volume, background=True
gdisc_d5             B = 1, D = 5, one id only (C_b = 1: no dist term), background=False
  each: e16 float16 [B, D, *spatial] -- the float32 embedding e ~ N(0, 1) the reference ran on is drawn on the float16 grid, so the
        half-size array holds it exactly (e = e16.astype(float32)) --, labels int32 [B, *spatial] (blocky, about 12 ids), background
        (bool), loss / loss64 = the reference's loss in float32 / float64, de64 = its float64 gradient, de_ulp int32 = the float32
        gradient as the distance of its bit pattern from that of float32(de64) (small integers, which compress; tests/disc_reference.py
        load_disc_golden puts e and de back together), params = the parameter names of discriminative_loss, defaults = their default
        values (delta_v, delta_d, alpha, beta, gama)

Arrays and names only.
"""
import importlib.util
import inspect
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))


def load(ref, name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blocky(rng, B, spatial, block, n_ids):
    """instance-like label images: blocks of one id drawn from 0 .. n_ids - 1 (0 about a quarter of the blocks)"""
    coarse_shape = tuple((s + block - 1) // block for s in spatial)
    coarse = rng.integers(1, n_ids, (B,) + coarse_shape)
    coarse = np.where(rng.random(coarse.shape) < 0.25, 0, coarse)
    lab = coarse
    for ax in range(len(spatial)):
        lab = np.repeat(lab, block, axis=1 + ax)
    return np.ascontiguousarray(lab[(slice(None),) + tuple(slice(0, s) for s in spatial)].astype(np.int32))


def run(fn, e, labels, background, dtype):
    x = torch.from_numpy(e).to(dtype).requires_grad_(True)
    loss = fn(x, torch.from_numpy(labels).long(), background=background)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())
    return loss.detach().numpy(), x.grad.numpy()


def grid16(rng, shape):
    """N(0, 1) on the float16 grid, as float32"""
    return rng.standard_normal(shape).astype(np.float16).astype(np.float32)


def store(fn, name, e, labels, background):
    sig = inspect.signature(fn)
    e16 = e.astype(np.float16)
    assert np.array_equal(e16.astype(np.float32), e)
    l32, g32 = run(fn, e, labels, background, torch.float32)
    l64, g64 = run(fn, e, labels, background, torch.float64)
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    ulp = g32.view(np.int32).astype(np.int64) - g64.astype(np.float32).view(np.int32).astype(np.int64)
    same_sign = np.signbit(g32) == np.signbit(g64.astype(np.float32))
    assert same_sign.all() and np.abs(ulp).max() < 2 ** 31
    print("%s background=%s: loss %.9g (float64 %.17g), float32 against float64 %.3g relative, gradient up to %d ulp apart" %
          (name, background, l32, l64, abs(float(l32) - float(l64)) / abs(float(l64)), np.abs(ulp).max()))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, e16=e16, labels=labels, background=np.array(background), loss=np.float32(l32), loss64=np.float64(l64),
                        de64=g64, de_ulp=ulp.astype(np.int32), params=np.array(list(sig.parameters)),
                        defaults=np.array([float(sig.parameters[k].default) for k in ("delta_v", "delta_d", "alpha", "beta", "gama")]))
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    fn = load(sys.argv[1], "ref_loss_disc", "scripts_ac3ac4/loss/loss_discriminative.py").discriminative_loss

    rng = np.random.default_rng(61)
    e = grid16(rng, (3, 16, 37, 53))
    labels = blocky(rng, 3, (37, 53), 9, 12)
    labels[2] = 0
    labels[0, 3, 4], labels[0, 30, 50] = 12, 13           # two one-pixel ids ..
    e[0, :, 30, 50] = e[0, :, 3, 4]                       # .. with bit-equal vectors
    assert len(np.unique(labels[0])) >= 8 and (labels[0] == 0).any() and (labels[1] == 0).any()
    store(fn, "gdisc_2d_b3_37x53", e, labels, False)
    store(fn, "gdisc_2d_b3_37x53_bg", e, labels, True)

    rng = np.random.default_rng(62)
    e = grid16(rng, (2, 16, 5, 20, 24))
    labels = blocky(rng, 2, (5, 20, 24), 6, 12)
    assert (labels == 0).any()
    store(fn, "gdisc_3d_b2_5x20x24", e, labels, True)

    rng = np.random.default_rng(63)
    e = grid16(rng, (1, 5, 21, 19))
    labels = np.zeros((1, 21, 19), np.int32)
    labels[0, 4:15, 3:12] = 7
    store(fn, "gdisc_d5", e, labels, False)


if __name__ == "__main__":
    main()
