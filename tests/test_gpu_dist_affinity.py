"""GPU: the distance-form affinities of the raw embedding (include/pea_dist.h, csrc/pea_k_dist.hip) through the C ABI, through
pea.distance_affinities and through the two mirrors of the reference (utils/emb2affs.py, utils/embeddings_ours.py):

  * the mirrors reproduce the reference's own float32 maps, and the emb2affs mirror under autograd its float64 gradient (tests/golden/gdist_*);
  * the map and the vjp against the float64 restatement (tests/dist_reference.py) in every kernel family: D = 16 and 32 (specialised),
    D = 5 and 64 (padded widths), f32 / f16 / bf16 storage, both borders, 2D and 3D.  Tolerances are the project's (tests/test_gpu_act_loss.py):
    affs 1e-5 absolute, de 1e-4 of its largest magnitude in f32 and 8e-3 with 16-bit storage.  Where delta_v > 0 the map jumps at d == delta_v
    by design: pairs whose float64 d lies within 1e-4 of delta_v are left out of the map's comparison (and the upstream gradient is zero
    there), and the share left out must stay below 0.1 %.  The dead zone, the slope and the saturation must each hold 2 % of the compared
    pairs; pairs with d == 0 are compared: a == 1 exactly and no contribution to de;
  * the vjp contract: an arbitrary dense g without a forward before it, dscale NULL and a device scalar, g == 0 -> de == +0;
  * the invert flag and non-finite vectors; element-aligned pointers in a guard-banded arena, two runs, a captured run;
  * strided / expanded / permuted views through the Python entry points; the stitcher.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import layouts
from arena import Arena
from dist_reference import _neighbours, dist_reference, dist_vjp_reference, load_dist_golden

pytestmark = pytest.mark.gpu
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TOL_AFFS = 1e-5
TOL_DE = {"f32": 1e-4, "f16": 8e-3, "bf16": 8e-3}
EDGE = 1e-4  # |d - delta_v| below which a pair is left out
REPLICATE, ZERO_VECTOR, INVERT = 2, 3, 1
BORDER = {"replicate": REPLICATE, "zero": ZERO_VECTOR}
GOLDENS = ("gdist_2d_b2_d5_37x53", "gdist_2d_k1", "gdist_3d_b2_5x20x24", "gdist_3d_reach_3x7x9")
OFFS2 = [[-1, 0], [0, -1], [0, -1], [2, -3], [0, 0], [0, 9], [-27, 0], [5, 5]]
OFFS3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, -1], [1, -2, 3], [0, 0, 0], [-9, 0, 0], [0, 0, 27], [0, 9, 0], [0, -3, 3]]
GEOM = {"2d": ((37, 53), OFFS2), "3d": ((5, 20, 24), OFFS3)}
DV, DD = 0.5, 1.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the cached embeddings are read-only)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def embedding(D, spatial, seed, B=2):
    """per-label mean + noise over blocky labels (blocks of 4, 12 ids), the recipe of tests/golden/make_golden_dist.py scaled with the
    width (means 2.1 / sqrt(D): at D = 64 the distances between two means concentrate, and 1.8 leaves under 1 % of the pairs
    saturated); one bit-equal pair of x neighbours in the interior.  float32 on the float16 grid."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 12, (B,) + tuple((s + 3) // 4 for s in spatial))
    labels = coarse
    for ax in range(len(spatial)):
        labels = np.repeat(labels, 4, axis=1 + ax)
    labels = labels[(slice(None),) + tuple(slice(0, s) for s in spatial)]
    means = 2.1 / np.sqrt(D) * rng.standard_normal((B, 12, D))
    e = np.stack([np.moveaxis(means[b][labels[b]], -1, 0) for b in range(B)])
    e = (e + 0.24 / np.sqrt(D) * rng.standard_normal(e.shape)).astype(np.float16).astype(np.float32)
    mid = tuple(s // 2 for s in spatial)
    e[(0, slice(None)) + mid[:-1] + (mid[-1] - 1,)] = e[(0, slice(None)) + mid]
    e.setflags(write=False)
    return e


def desc_of(pkg, E, offs, dv, dd, border, invert=False):
    d = pkg._lib.PeaDistDesc()
    d.B, d.D, d.K = E.shape[0], E.shape[1], len(offs)
    sp = list(E.shape[2:])
    d.dims[:] = [1] * (3 - len(sp)) + sp
    for i, o in enumerate(offs):
        d.offsets[i][:] = [0] * (3 - len(o)) + list(o)
    d.dtype = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[E.dtype]
    d.border, d.flags, d.delta_v, d.delta_d = BORDER[border], (INVERT if invert else 0), dv, dd
    return d


def c_fwd(pkg, E, offs, dv=DV, dd=DD, border="replicate", invert=False, affs=None):
    d = desc_of(pkg, E, offs, dv, dd, border, invert)
    if affs is None:
        affs = torch.full((E.shape[0], len(offs)) + tuple(E.shape[2:]), -7.0, dtype=torch.float32, device=E.device)
    pkg._lib.check(pkg._lib.lib().pea_dist_affinity(ctypes.byref(d), vp(E), vp(affs), None), "pea_dist_affinity")
    return affs


def c_vjp(pkg, E, offs, g, dv=DV, dd=DD, border="replicate", invert=False, dscale=None, de=None):
    """the vjp alone: no forward is run before it"""
    d = desc_of(pkg, E, offs, dv, dd, border, invert)
    if de is None:
        de = torch.full_like(E, -7.0)
    pkg._lib.check(pkg._lib.lib().pea_dist_affinity_vjp(ctypes.byref(d), vp(E), vp(g), vp(dscale), vp(de), None), "pea_dist_affinity_vjp")
    return de


@functools.lru_cache(maxsize=None)
def reference(D, geom, dt, border, seed=5):
    """-> (e in the storage type's values as float32, affs64, d64, keep, g float32 (zero where not keep), de64 for g)"""
    spatial, offs = GEOM[geom]
    e = torch.from_numpy(embedding(D, spatial, seed + D).copy()).to(TDT[dt]).float().numpy()
    a, d = dist_reference(e, offs, DV, DD, border)
    keep = np.abs(d - DV) >= EDGE
    g = np.random.default_rng(seed + 100).standard_normal(a.shape).astype(np.float32) * keep
    de = dist_vjp_reference(e, offs, g, DV, DD, border)
    return e, a, d, keep, g, de


# ---- the mirrors against the reference's own numbers -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_mirrors_reproduce_the_goldens(pkg, dev, name):
    g = load_dist_golden(name)
    offs, delta = g["offsets"], g["delta"]
    E = cu(g["e"], dev).requires_grad_(True)
    affs = pkg.emb2affs.embeddings_to_affinities(E, offs, delta)
    assert affs.dtype == torch.float32 and affs.shape == g["affs"].shape
    err = np.abs(affs.detach().cpu().numpy() - g["affs"]).max()
    (affs * cu(g["g"], dev)).sum().backward()
    top = np.abs(g["de64"]).max()
    err_g = np.abs(E.grad.cpu().numpy() - g["de64"]).max() / top
    print(name, "emb2affs mirror: |affs - reference f32| %.3g, |de - reference f64| / max %.3g" % (err, err_g))
    assert err <= TOL_AFFS and err_g <= TOL_DE["f32"]
    assert same_bits(affs.detach(), pkg.emb2affs.embeddings_to_affinities(E.detach(), offs)) or delta != 1.5
    _, d64 = dist_reference(g["e"][:1], offs, 0.5, delta, "zero")
    for key, dv in (("np_dv05", 0.5), ("np_dv0", 0.0)):
        keep = np.abs(d64[0] - dv) >= EDGE if dv > 0 else np.ones(d64[0].shape, bool)
        for inv in (False, True):
            ref = g[key + ("_inv" if inv else "")]
            out = pkg.embeddings_ours.embeddings_to_affinities(E.detach()[0], offs, delta_v=dv, delta_d=delta, invert=inv)
            assert isinstance(out, torch.Tensor) and out.device == E.device and out.dtype == torch.float32 and out.shape == ref.shape
            err = np.abs(out.cpu().numpy() - ref)[keep].max()
            print(name, key, "invert" if inv else "", "embeddings_ours mirror: |affs - reference f32| %.3g, %.4f %% left out" % (err, 100 * (1 - keep.mean())))
            assert err <= TOL_AFFS and 1 - keep.mean() < 1e-3
            out_np = pkg.embeddings_ours.embeddings_to_affinities(g["e"][0], offs, delta_v=dv, delta_d=delta, invert=inv)
            assert isinstance(out_np, np.ndarray) and out_np.dtype == np.float32 and np.array_equal(out_np.view(np.int32), out.cpu().numpy().view(np.int32))
    if len(offs[0]) == 3:
        default = pkg.embeddings_ours.embeddings_to_affinities(E.detach()[0])
        explicit = pkg.embeddings_ours.embeddings_to_affinities(E.detach()[0], [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], 0.5, 1.5, False)
        assert same_bits(default, explicit)
    seg = cu(g["labels"][:, None].astype(np.int64), dev)
    out = pkg.emb2affs.segmentation_to_affinities(seg, offs)
    assert out.device == seg.device and np.array_equal(out.cpu().numpy(), g["seg_affs"].astype(np.float32))


# ---- map and vjp against float64, every family ---------------------------------------------------------------------------------------
FAMILIES = [(5, "2d"), (16, "2d"), (16, "3d"), (32, "3d"), (64, "2d")]


@pytest.mark.parametrize("border", ["replicate", "zero"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("D,geom", FAMILIES)
def test_map_and_vjp_against_float64(pkg, dev, D, geom, dt, border):
    offs = GEOM[geom][1]
    e, a64, d64, keep, g, de64 = reference(D, geom, dt, border)
    E = cu(e, dev).to(TDT[dt])
    assert np.array_equal(E.float().cpu().numpy(), e)
    G = cu(g, dev)
    de = c_vjp(pkg, E, offs, G, border=border)  # first: the caller has run no forward
    affs = c_fwd(pkg, E, offs, border=border).cpu().numpy()
    n = keep.sum()
    share = {"left out": 1 - keep.mean(), "dead": (d64 <= DV)[keep].sum() / n, "sloped": ((d64 > DV) & (d64 < 2 * DD))[keep].sum() / n,
             "saturated": (d64 >= 2 * DD)[keep].sum() / n, "d == 0": (d64 == 0).mean()}
    err = np.abs(affs - a64)[keep].max()
    top = np.abs(de64).max()
    err_g = np.abs(de.float().cpu().numpy() - de64).max() / top
    print("D %d %s %s %s: |affs - f64| %.3g, |de - f64| / max %.3g (max %.3g);" % (D, geom, dt, border, err, err_g, top),
          ", ".join("%s %.4f %%" % (k, 100 * v) for k, v in share.items()))
    assert share["left out"] < 1e-3
    assert min(share["dead"], share["sloped"], share["saturated"]) >= 0.02
    assert np.isfinite(affs).all() and err <= TOL_AFFS
    assert top > 0.1 and err_g <= TOL_DE[dt]
    zero = d64 == 0
    assert zero.mean() > 0.01 and (affs[zero] == 1.0).all()
    # a device scalar scales the same sum; with the invert flag the map is 1 - a and the vjp changes sign, bit for bit
    sc = torch.tensor(-2.5, dtype=torch.float32, device=dev)
    de_s = c_vjp(pkg, E, offs, G, border=border, dscale=sc)
    assert np.abs(de_s.float().cpu().numpy() + 2.5 * de64).max() <= TOL_DE[dt] * 2.5 * top
    a_t = torch.from_numpy(affs).to(dev)
    assert same_bits(c_fwd(pkg, E, offs, border=border, invert=True), 1.0 - a_t)
    assert same_bits(c_vjp(pkg, E, offs, G, border=border, invert=True), -de)
    # g == 0: de == +0 everywhere
    dz = c_vjp(pkg, E, offs, torch.zeros_like(G), border=border)
    assert not dz.view(torch.int16 if dz.element_size() == 2 else torch.int32).any()


@pytest.mark.parametrize("border", ["replicate", "zero"])
def test_every_reach_beyond_an_extent(pkg, dev, border):
    """K = 32 on a 3 x 7 x 9 volume, every offset leaving it along some axis: whole axes clamp, pre-images are slabs"""
    g = load_dist_golden("gdist_3d_reach_3x7x9")
    e, offs = g["e"], g["offsets"]
    assert len(offs) == 32
    a64, d64 = dist_reference(e, offs, DV, DD, border)
    keep = np.abs(d64 - DV) >= EDGE
    gg = g["g"] * keep
    de64 = dist_vjp_reference(e, offs, gg, DV, DD, border)
    E, G = cu(e, dev), cu(gg.astype(np.float32), dev)
    de = c_vjp(pkg, E, offs, G, border=border).cpu().numpy()
    affs = c_fwd(pkg, E, offs, border=border).cpu().numpy()
    err, err_g = np.abs(affs - a64)[keep].max(), np.abs(de - de64).max() / np.abs(de64).max()
    print(border, "|affs - f64| %.3g, |de - f64| / max %.3g, left out %.4f %%" % (err, err_g, 100 * (1 - keep.mean())))
    assert err <= TOL_AFFS and err_g <= TOL_DE["f32"] and 1 - keep.mean() < 1e-3
    # a component that already leaves the extent may grow to the ends of int32 (p + o no longer fits): nothing changes
    ext, big = (3, 7, 9), (2 ** 31 - 1, -2 ** 31)
    far = [[(big[0] if v > 0 else big[1]) if abs(v) >= n else v for v, n in zip(o, ext)] for o in offs]
    assert far != offs
    assert same_bits(c_fwd(pkg, E, far, border=border), torch.from_numpy(affs).to(dev))
    assert same_bits(c_vjp(pkg, E, far, G, border=border), torch.from_numpy(de).to(dev))


def test_only_the_zero_offset(pkg, dev):
    """every pair is the voxel with itself: d == 0, a == 1 exactly, de == +0 whatever g holds"""
    e = embedding(16, (5, 20, 24), 21)
    E = cu(e, dev)
    G = torch.randn((2, 2, 5, 20, 24), device=dev)
    for border in ("replicate", "zero"):
        assert (c_fwd(pkg, E, [[0, 0, 0], [0, 0, 0]], border=border) == 1.0).all()
        assert not c_vjp(pkg, E, [[0, 0, 0], [0, 0, 0]], G, border=border).view(torch.int32).any()
    # under REPLICATE an offset that clamps a whole axis onto one slice pairs that slice with itself
    a = c_fwd(pkg, E, [[-9, 0, 0]], border="replicate")
    assert (a[:, :, 0] == 1.0).all() and not (a[:, :, 1:] == 1.0).all()


# ---- non-finite vectors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ["replicate", "zero"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_vector_marks_exactly_its_pairs(pkg, dev, value, border):
    spatial, offs = GEOM["3d"]
    e = embedding(16, spatial, 31).copy()
    clean = c_fwd(pkg, cu(e, dev), offs, border=border)
    assert torch.isfinite(clean).all()
    for b, voxel in ((0, (2, 9, 11)), (1, (0, 0, 23)), (1, (4, 19, 0))):  # the interior, two corners
        bad = e.copy()
        bad[(b, slice(None)) + voxel] = value
        v = np.ravel_multi_index(voxel, spatial)
        touched = np.zeros((2, len(offs), int(np.prod(spatial))), bool)
        for i, o in enumerate(offs):
            q, inside = _neighbours(spatial, o, border)
            touched[b, i] = (np.arange(q.size) == v) | ((q == v) & inside)
        touched = torch.from_numpy(touched.reshape(clean.shape)).to(dev)
        out = c_fwd(pkg, cu(bad, dev), offs, border=border)
        assert torch.equal(torch.isnan(out), touched), (value, voxel)
        assert same_bits(torch.where(touched, clean, out), clean)  # every other element: the bits of the finite run
        assert 0 < int(touched.sum()) < 400


# ---- placement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,geom", [("f32", 16, "3d"), ("f16", 5, "2d"), ("bf16", 32, "3d"), ("f16", 64, "2d")])
def test_element_aligned_pointers_in_a_guarded_arena_and_two_runs(pkg, dev, dt, D, geom):
    offs = GEOM[geom][1]
    e, _, _, _, g, _ = reference(D, geom, dt, "replicate")
    tdt = TDT[dt]
    item = torch.empty((), dtype=tdt).element_size()
    E, G = cu(e, dev).to(tdt), cu(g, dev)
    for border in ("replicate", "zero"):
        a0, d0 = c_fwd(pkg, E, offs, border=border), c_vjp(pkg, E, offs, G, border=border)
        a1 = c_fwd(pkg, E, offs, border=border, affs=torch.full_like(a0, 3.0))
        d1 = c_vjp(pkg, E, offs, G, border=border, de=torch.full_like(d0, 3.0))
        assert same_bits(a0, a1) and same_bits(d0, d1)  # two runs, from another pattern: every element is written
        for skew in (1, 3):  # odd element offsets: 16-bit tensors at a 2-byte boundary, nothing 16-byte aligned
            ar = Arena(8 << 20, dev)
            Es = ar.fill(ar.carve(E.shape, tdt, item * skew, name="e"), E)
            Gs = ar.fill(ar.carve(G.shape, torch.float32, 4 * skew, name="g"), G)
            As = ar.carve(a0.shape, torch.float32, 4 * (4 - skew), name="affs")
            Ds = ar.carve(E.shape, tdt, item * skew, name="de")
            assert Es.data_ptr() % 16 == item * skew == Ds.data_ptr() % 16 and As.data_ptr() % 16 == 4 * (4 - skew)
            c_vjp(pkg, Es, offs, Gs, border=border, de=Ds)
            c_fwd(pkg, Es, offs, border=border, affs=As)
            ar.check(written=[As, Ds], untouched=[Es, Gs])
            assert same_bits(As, a0) and same_bits(Ds, d0), (border, skew)


def test_graphed_step_replays_the_eager_bits(pkg, dev):
    spatial, offs = GEOM["3d"]
    E = cu(embedding(16, spatial, 41), dev).requires_grad_(True)
    Gup = torch.randn((2, len(offs)) + spatial, device=dev)

    def step(E, Gup):
        E.grad = None
        affs = pkg.distance_affinities(E, offs, DV, DD, "replicate")
        inv = pkg.distance_affinities(E, offs, 0.0, DD, "zero", True)
        torch.autograd.backward([affs, inv], [Gup, Gup])
        return affs, inv, E.grad

    eager = [o.detach().clone() for o in step(E, Gup)]
    gr = pkg.graphed(step, E, Gup)
    first = [o.detach().clone() for o in gr.replay()]
    assert all(same_bits(a, b) for a, b in zip(first, eager))
    with torch.no_grad():
        E.mul_(0.75)
        Gup.neg_()
    second = [o.detach().clone() for o in gr.replay()]
    again = [o.detach().clone() for o in step(E, Gup)]
    assert all(same_bits(a, b) for a, b in zip(second, again)) and not same_bits(second[0], first[0])
    de = c_vjp(pkg, E.detach(), offs, Gup) + c_vjp(pkg, E.detach(), offs, Gup, dv=0.0, border="zero", invert=True)
    assert torch.allclose(again[2], de, rtol=1e-5, atol=1e-6)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["L5", "L6", "L1b"])
@pytest.mark.parametrize("shape,offs", [((2, 5, 19, 23), OFFS2[:5]), ((2, 16, 4, 9, 11), OFFS3[:6])])
def test_views_give_the_bits_of_their_dense_clones(pkg, dev, layout, shape, offs):
    """a [::2] batch crop, channels_last and a batch expanded from one item (tests/layouts.py)"""
    view, _ = layouts.make(layout, shape, torch.float32, 77, dev)
    assert tuple(view.shape) == shape and not view.is_contiguous()
    twin = layouts.dense(view)
    up = torch.randn((shape[0], len(offs)) + shape[2:], device=dev)

    def run(fn, x):
        x = x.detach().requires_grad_(True)
        out = fn(x)
        (grad,) = torch.autograd.grad(out, x, up)
        return out.detach(), grad

    calls = {
        "distance_affinities": lambda x: pkg.distance_affinities(x, offs, 0.5, 3.0, "zero", True),
        "emb2affs": lambda x: pkg.emb2affs.embeddings_to_affinities(x, offs, delta=3.0),
    }
    for name, fn in calls.items():
        (a_v, g_v), (a_d, g_d) = run(fn, view), run(fn, twin)
        assert same_bits(a_v, a_d) and same_bits(g_v, g_d), name
        assert 0.02 < float(((a_d > 0) & (a_d < 1)).float().mean()), name  # not a constant map
    ours = lambda x: pkg.embeddings_ours.embeddings_to_affinities(x, offs, delta_v=0.5, delta_d=3.0)
    item = view[1]
    assert same_bits(ours(item), ours(twin[1]))
    assert same_bits(ours(item), pkg.distance_affinities(twin[1:2], offs, 0.5, 3.0, "zero")[0])
    half = view.to(torch.bfloat16)
    assert same_bits(calls["emb2affs"](half), calls["emb2affs"](layouts.dense(half)))


# ---- the stitcher ------------------------------------------------------------------------------------------------------------------------
def test_stitcher_adds_the_distance_affinities_of_two_overlapping_windows(pkg, dev):
    offs = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, -3, 3]]
    out_size, vol = (4, 12, 16), (6, 20, 24)
    e = cu(embedding(16, out_size, 51), dev)
    pos = [(0, 0, 0), (2, 6, 8)]
    for border, invert in (("replicate", False), ("zero", True)):
        a = pkg.VolumeStitcher(len(offs), vol, out_size, dev)
        a.add_distance_embedding(e, pos, offs, 0.5, 1.5, border, invert)
        b = pkg.VolumeStitcher(len(offs), vol, out_size, dev)
        maps = pkg.distance_affinities(e, offs, 0.5, 1.5, border, invert)
        for i in range(2):
            b.add_vol(maps[i], pos[i])
        assert same_bits(a.out_affs, b.out_affs) and same_bits(a.weight_map, b.weight_map)
        assert float(a.out_affs.abs().sum()) > 0 and float(a.weight_map[0, 3, 8, 10]) > 0 and float(a.weight_map[0, 5, 17, 23]) > 0
    with pytest.raises(ValueError, match="offsets"):
        a.add_distance_embedding(e, pos, offs[:3], 0.5, 1.5, "zero")
    with pytest.raises(ValueError, match="embedding must be"):
        a.add_distance_embedding(e[:, :, :3], pos, offs, 0.5, 1.5, "zero")
