"""The float64 restatement of the distance-form affinities (include/pea_dist.h), forward and vjp, both borders -- what the GPU tests
compare the kernels with -- and the loader of the gdist_* fixtures (tests/golden/make_golden_dist.py).  A helper module, no tests here.

  d = |e(p) - e(p + o)|, h = d <= delta_v ? 0 : d, u = (2 delta_d - h) / (2 delta_d), a = max(u, 0)^2 (invert: 1 - a)
  border "replicate": the index p + o is clamped into the volume; "zero": outside the volume the neighbour is the zero vector
  da / dd = -u / delta_d where u > 0 and d > delta_v, else 0; the direction (e(p) - e(q)) / d, 0 where d == 0; invert flips the sign
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _neighbours(spatial, off, border):
    """-> (flat index of p + o per voxel [S], inside [S] bool); the index is the clamped one also where `inside` is False"""
    axes = []
    inside = np.ones(spatial, bool)
    for ax, (n, o) in enumerate(zip(spatial, off)):
        raw = np.arange(n, dtype=np.int64) + int(o)
        shape = [1] * len(spatial)
        shape[ax] = n
        axes.append(np.clip(raw, 0, n - 1).reshape(shape))
        inside &= ((raw >= 0) & (raw < n)).reshape(shape)
    q = np.ravel_multi_index(np.broadcast_arrays(*axes), spatial)
    return q.reshape(-1), (inside.reshape(-1) if border == "zero" else np.ones(q.size, bool))


def _pairs(e, offsets, delta_v, delta_d, border):
    """per offset: (q, inside, diff [B, D, S], d [B, S], u [B, S]) in float64"""
    assert border in ("replicate", "zero")
    B, D = e.shape[:2]
    spatial = tuple(e.shape[2:])
    x = np.asarray(e, np.float64).reshape(B, D, -1)
    for off in offsets:
        assert len(off) == len(spatial)
        q, inside = _neighbours(spatial, off, border)
        diff = x - np.where(inside, x[:, :, q], 0.0)
        d = np.sqrt((diff * diff).sum(1))
        h = np.where(d <= delta_v, 0.0, d)
        yield q, inside, diff, d, (2 * delta_d - h) / (2 * delta_d)


def dist_reference(e, offsets, delta_v=0.0, delta_d=1.5, border="replicate", invert=False):
    """-> (affs float64 [B, K, *spatial], d float64 of the same shape)"""
    affs, ds = [], []
    for _, _, _, d, u in _pairs(e, offsets, delta_v, delta_d, border):
        a = np.where(u < 0, 0.0, u) ** 2
        affs.append(1 - a if invert else a)
        ds.append(d)
    shape = (e.shape[0], len(offsets)) + tuple(e.shape[2:])
    return np.stack(affs, 1).reshape(shape), np.stack(ds, 1).reshape(shape)


def dist_vjp_reference(e, offsets, g, delta_v=0.0, delta_d=1.5, border="replicate", invert=False, dscale=1.0):
    """-> de float64 = dscale * d sum(affs * g) / d e, for an arbitrary g [B, K, *spatial]"""
    B, D = e.shape[:2]
    gf = np.asarray(g, np.float64).reshape(B, len(offsets), -1)
    de = np.zeros((B, D, gf.shape[2]))
    for i, (q, inside, diff, d, u) in enumerate(_pairs(e, offsets, delta_v, delta_d, border)):
        slope = np.where((u > 0) & (d > delta_v), -u / delta_d, 0.0) * (-1.0 if invert else 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(d > 0, gf[:, i] * slope / d, 0.0)
        c = coef[:, None] * diff
        de += c
        np.subtract.at(de, (slice(None), slice(None), q[inside]), c[:, :, inside])
    return (float(dscale) * de).reshape(e.shape)


def bits_plus(ref32, ulp):
    """the float32 array `ulp` bit patterns away from ref32 (how the fixtures store a float32 result beside its float64 twin)"""
    return (np.ascontiguousarray(ref32, np.float32).view(np.int32) + ulp).view(np.float32)


def load_dist_golden(name):
    """a gdist_* fixture with its parts merged and its compact arrays expanded:
    e float32, labels, offsets (list of lists), delta, affs64, affs (the reference's float32 map), g float32, de64, seg_affs,
    np_dv05 / np_dv0 and np_dv05_inv / np_dv0_inv (the numpy form on e[0]), and the names (params_*, defaults_ours, offsets_ours,
    default_delta)"""
    g = {}
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g.update({k: z[k] for k in z.files})
    parts = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, name + "_*.npz"))):
        with np.load(path) as z:
            parts[os.path.basename(path)[len(name) + 1:-4]] = {k: z[k] for k in z.files}
    if parts:
        g["affs64"] = parts["map64"]["affs64"]
        g["de64"] = np.stack([parts["de64_b%d" % b]["de64"] for b in range(g["e16"].shape[0])])
        g.update(parts["np"])
    g["e"] = g.pop("e16").astype(np.float32)
    g["g"] = g.pop("g16").astype(np.float32)
    g["affs"] = bits_plus(g["affs64"].astype(np.float32), g.pop("affs_ulp"))
    for key in ("np_dv05", "np_dv0"):
        g[key + "_inv"] = bits_plus(np.float32(1) - g[key], g.pop(key + "_inv_ulp"))
    g["offsets"] = [[int(v) for v in o] for o in g["offsets"]]
    g["delta"] = float(g["delta"])
    return g
