#!/usr/bin/env python3
"""Generate tests/golden/gdist_*.npz: the distance-form affinities of a raw embedding, from the reference's own code on small seeded
inputs (include/pea_dist.h says what they are).

Run on the development machine only, on the CPU (it needs a checkout of the reference, weih527/Pixel-Embedded-Affinity; the GPU box
has none):
    python tests/golden/make_golden_dist.py /path/to/Pixel-Embedded-Affinity

What is imported from the reference (nothing is copied; the files are loaded where they lie):
    scripts_ac3ac4/utils/emb2affs.py          embeddings_to_affinities (:63-75, torch, replicate border), invert_offsets,
                                              segmentation_to_affinities (:78-95)
    scripts_ac3ac4/utils/embeddings_ours.py   embeddings_to_affinities (:58-98, numpy, scipy.ndimage.shift: zero vector outside)
The second imports skimage.segmentation.slic at module level for a function that is not run here; where skimage is not installed an
empty stand-in module is registered for that one name.

The embedding is "per-label mean + noise" over blocky labels (make_golden_disc.py's blocky: blocks of 4, 12 ids), drawn on the float16
grid, so that the pairs fall into every regime of the transform -- dead zone (d <= delta_v), slope, saturation (d >= 2 delta_d) and
d == 0; one pair of bit-equal neighbouring vectors is planted in the interior.

gdist_2d_b2_d5_37x53     B = 2, D = 5 (a runtime width), 37 x 53 (odd), K = 8 with both signs, a diagonal, a repeated offset, [0, 0] and
                         reaches of 9 and 27
gdist_2d_k1              the same embedding, K = 1
gdist_3d_b2_5x20x24      B = 2, D = 16, a 5 x 20 x 24 volume, K = 10 with [1, -2, 3], a repeated offset, [0, 0, 0], a reach of 9 (beyond Z = 5)
                         and of 27 (beyond X = 24): whole axes clamp.  In parts, each within the size limit of a committed file:
                         ..._map64 (affs64), ..._de64_b0 / _b1 (de64 per batch item), ..._np (the numpy form)
gdist_3d_reach_3x7x9     B = 1, D = 16, a 3 x 7 x 9 volume, K = 32, every offset with a reach beyond an extent

Torch form (delta = 1.5), each fixture: e16 float16 [B, D, *spatial] (e = e16.astype(float32), exact), labels int32 [B, *spatial],
offsets, delta, affs64 = the map of the float64 run, affs_ulp int32 = the float32 run's map as the distance of its bit pattern from
float32(affs64), g16 float16 = a dense upstream gradient of order 1, de64 = the float64 gradient of sum(affs * g), seg_affs uint8 =
segmentation_to_affinities(labels[:, None], offsets).
Numpy form on e[0] (one volume): np_dv05 / np_dv0 = the float32 map with delta_v = 0.5 / 0.0 (delta_d = 1.5), np_dv05_inv_ulp /
np_dv0_inv_ulp = the invert=True map as bit distance from float32(1) - map.
Names: params_emb2affs, params_seg2affs, params_invert, params_ours = the parameter names; defaults_ours = (delta_v, delta_d, invert),
offsets_ours = the default offsets, default_delta.  tests/dist_reference.py load_dist_golden puts the parts back together.

Arrays and names only.
"""
import importlib.util
import inspect
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_disc import blocky, load  # noqa: E402


def embedding(rng, B, D, spatial, mean_scale, noise):
    labels = blocky(rng, B, spatial, 4, 12)
    means = mean_scale * rng.standard_normal((B, 12, D))
    e = np.stack([np.moveaxis(means[b][labels[b]], -1, 0) for b in range(B)])
    e = e + noise * rng.standard_normal(e.shape)
    return e.astype(np.float16).astype(np.float32), labels


def ulp_from(a32, ref32):
    assert a32.dtype == np.float32 and ref32.dtype == np.float32
    assert (np.signbit(a32) == np.signbit(ref32)).all()
    u = a32.view(np.int32).astype(np.int64) - ref32.view(np.int32).astype(np.int64)
    assert np.abs(u).max() < 2 ** 31
    return u.astype(np.int32)


def regimes(d, dv, dd):
    n = d.size
    return {"dead": (d <= dv).sum() / n, "sloped": ((d > dv) & (d < 2 * dd)).sum() / n, "saturated": (d >= 2 * dd).sum() / n,
            "zero": (d == 0).sum() / n, "near": (np.abs(d - dv) < 1e-4).sum() / n}


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20, path


def store(t_mod, n_mod, name, e, labels, offsets, rng, split=False):
    delta = 1.5
    fn = t_mod.embeddings_to_affinities
    e16 = e.astype(np.float16)
    assert np.array_equal(e16.astype(np.float32), e)
    K = len(offsets)
    g = rng.standard_normal((e.shape[0], K) + e.shape[2:]).astype(np.float16)
    a32 = fn(torch.from_numpy(e), offsets, delta).numpy()
    x = torch.from_numpy(e).double().requires_grad_(True)
    a64 = fn(x, offsets, delta)
    (a64 * torch.from_numpy(g.astype(np.float64))).sum().backward()
    a64, de64 = a64.detach().numpy(), x.grad.numpy()
    assert a32.dtype == np.float32 and a64.dtype == np.float64 and de64.dtype == np.float64 and np.isfinite(de64).all()
    d64 = 2 * delta * (1 - np.sqrt(np.clip(a64, 0, None)))
    print(name, "torch form: float32 against float64 %.3g" % np.abs(a32 - a64).max(), {k: "%.4f" % v for k, v in regimes(d64, 0.5, delta).items()})
    seg = torch.from_numpy(labels[:, None].astype(np.int64))
    seg_affs = t_mod.segmentation_to_affinities(seg, offsets).numpy()
    assert set(np.unique(seg_affs)) <= {0.0, 1.0}
    out = dict(e16=e16, labels=labels, offsets=np.array(offsets, np.int32), delta=np.float64(delta),
               affs_ulp=ulp_from(a32, a64.astype(np.float32)), g16=g, seg_affs=seg_affs.astype(np.uint8))
    nps = {}
    for key, dv in (("np_dv05", 0.5), ("np_dv0", 0.0)):
        m = n_mod.embeddings_to_affinities(e[0], offsets, delta_v=dv, delta_d=delta)
        mi = n_mod.embeddings_to_affinities(e[0], offsets, delta_v=dv, delta_d=delta, invert=True)
        assert m.dtype == np.float32 and mi.dtype == np.float32 and m.shape == (K,) + e.shape[2:]
        nps[key], nps[key + "_inv_ulp"] = m, ulp_from(mi, np.float32(1) - m)
    sig_t, sig_n = inspect.signature(fn), inspect.signature(n_mod.embeddings_to_affinities)
    out.update(params_emb2affs=np.array(list(sig_t.parameters)), default_delta=np.float64(sig_t.parameters["delta"].default),
               params_seg2affs=np.array(list(inspect.signature(t_mod.segmentation_to_affinities).parameters)),
               params_invert=np.array(list(inspect.signature(t_mod.invert_offsets).parameters)),
               params_ours=np.array(list(sig_n.parameters)),
               defaults_ours=np.array([float(sig_n.parameters[k].default) for k in ("delta_v", "delta_d", "invert")]),
               offsets_ours=np.array(sig_n.parameters["offsets"].default, np.int32))
    if not split:
        save(name, affs64=a64, de64=de64, **nps, **out)
        return
    save(name, **out)
    save(name + "_map64", affs64=a64)
    for b in range(e.shape[0]):
        save(name + "_de64_b%d" % b, de64=de64[b])
    save(name + "_np", **nps)


def plant(e, src, dst):
    """e[0, :, dst] = e[0, :, src]: a pair at distance exactly 0 away from every border"""
    e[(0, slice(None)) + tuple(dst)] = e[(0, slice(None)) + tuple(src)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    try:
        import skimage.segmentation  # noqa: F401
    except ImportError:
        sk, seg = types.ModuleType("skimage"), types.ModuleType("skimage.segmentation")
        seg.slic = None
        sk.segmentation = seg
        sys.modules["skimage"], sys.modules["skimage.segmentation"] = sk, seg
    t_mod = load(ref, "ref_emb2affs", "scripts_ac3ac4/utils/emb2affs.py")
    n_mod = load(ref, "ref_embeddings_ours", "scripts_ac3ac4/utils/embeddings_ours.py")

    rng = np.random.default_rng(71)
    e, labels = embedding(rng, 2, 5, (37, 53), 0.8, 0.1)
    plant(e, (17, 22), (17, 21))  # the pair of offset [0, -1] at (17, 22)
    offs2 = [[-1, 0], [0, -1], [0, -1], [2, -3], [0, 0], [0, 9], [-27, 0], [5, 5]]
    store(t_mod, n_mod, "gdist_2d_b2_d5_37x53", e, labels, offs2, rng)
    store(t_mod, n_mod, "gdist_2d_k1", e, labels, [[0, -1]], rng)

    rng = np.random.default_rng(72)
    e, labels = embedding(rng, 2, 16, (5, 20, 24), 0.45, 0.06)
    plant(e, (2, 10, 12), (2, 10, 11))
    offs3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, -1], [1, -2, 3], [0, 0, 0], [-9, 0, 0], [0, 0, 27], [0, 9, 0], [0, -3, 3]]
    store(t_mod, n_mod, "gdist_3d_b2_5x20x24", e, labels, offs3, rng, split=True)

    rng = np.random.default_rng(73)
    e, labels = embedding(rng, 1, 16, (3, 7, 9), 0.45, 0.06)
    plant(e, (1, 3, 4), (1, 3, 3))
    base = [[3, 0, 0], [0, 7, 0], [0, 0, 9], [-3, 0, 0], [0, -7, 0], [0, 0, -9], [27, 1, -1], [1, -9, 2], [-1, 2, 27], [3, 7, 9],
            [-4, -8, -10], [5, -7, 9], [0, 0, -9], [-3, 1, 1], [2, -1, 11], [1, 1, -12]]
    offs_r = base + [[-v for v in o] for o in base]
    assert len(offs_r) == 32 and all(abs(o[0]) >= 3 or abs(o[1]) >= 7 or abs(o[2]) >= 9 for o in offs_r)
    store(t_mod, n_mod, "gdist_3d_reach_3x7x9", e, labels, offs_r, rng)


if __name__ == "__main__":
    main()
