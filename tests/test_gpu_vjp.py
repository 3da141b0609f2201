"""GPU (-m gpu): every backward family as the vector-Jacobian product include/pea.h promises -- an ARBITRARY upstream gradient g.

"g is either what pea_affinity_fwd wrote or any upstream gradient d(criterion) / d(affs)" (pea_affinity_bwd), "pea_inv_norm computes the
plane alone, for callers that hold e but did not run the forward: the vjp of a foreign criterion" (pea_affinity_bwd_ex).  Every other
GPU test that reaches a fast backward family hands it the g the library's own forward just wrote: exactly 0 on every pair CROP_ZERO
removes and where the mask is 0, smooth (it follows a - t), about 1e-6 in size.  A kernel that multiplies g_i(p) into a pending sum
without asking whether the pair (p, p + o_i) exists is bit-correct on that g and wrong for a caller's criterion whose gradient is
non-zero on a cropped pair -- |pred - t|^3 has one wherever pred = 0 != t, on every cropped border slice of the 3D losses.

Here the caller never runs a training forward.  Through the C ABI:

    1 / norm plane(s)   pea_inv_norm (twice with a second operand, into [2, B, Z, Y, X]) where mode 1 (2) of pea_cross_supported says 1
    raw map             pea_affinity_infer with no activation flag, where mode 3 (4) says the backward reads it
    g                   vjp_reference.make_g: dense, random sign, 2^-j (0.5 + u) with j in 0 .. 8, no 1 / N; under CROP_ZERO 64.0 on
                        every pair that does not exist, and a second array with -3.0 there
    dloss               the device scalar 0.625, and once per family NULL

and each case is held to tests/vjp_reference.py::vjp (float64 autograd on the device; tests/test_vjp_reference_host.py validates it):

    1. check_grad with the standing tolerances of tests/cross_stencils.py: 1e-4 of max for f32, 8e-3 for 16-bit storage
    2. CROP_ZERO: the launch with the other poison gives a BIT-identical gradient -- no tolerance; any read of a non-existing pair's g fails
    3. a rerun is bit-identical
    4. the worst relative error is printed ("vjp-ratio <family> ...")

Before a case runs pea_cross_supported modes 0 .. 5 must equal the table of tests/cross_stencils.py (EXPECT), the switches are set
with monkeypatch.setenv (tests/conftest.py makes the library re-read them): that is how a case knows which family it holds.  Outputs are
pre-filled with NaN.

    test_xdma_d16_self     k_bwd_xdma, D = 16 (mode 1, not 3)         pos, asym, two_sw32, dup, unsorted; two_sw64 at X = 96 and 43 x 96; tall
    test_xdma_pf           k_bwd_xdma_pf, D = 32 / 64 (modes 1, 3)    with the inference map, and with affs = NULL (then exactly bwd_ex)
    test_role_a_d16        k_bwd_xdma<OTHER> (mode 2)                 with and without PEA_FLAG_ACCUMULATE_DE (bit-equal to write + add)
    test_xdma_pfo          k_bwd_xdma_pfo (mode 4)                    D = 32 / 64 with the second operand's inference map
    test_h16               16-bit self and detached (modes 1, 3, 4)   f16 D = 32, bf16 D = 64; small also under PEA_H16_HW=1
    test_pair              pea_affinity_bwd_dual_ex (mode 5)          g and g_cross of different seeds, dloss 0.625 and 1.5
    test_volume            k_bwd_xdma<ZP> and k_bwd_zm                PEA_ZMARCH=2 alone and with PEA_ZSEG=2 / 3 (three / two segments at Z = 6)
    test_box               k_bwd_box, k_bwd_boxm                      PEA_BOXM=0 / PEA_ZMARCH=2 on the CROP volumes
    test_tiled_direct      pea_affinity_bwd (no plane)                37 x 50 (X % 4 != 0), D = 16, and 3 x 20 x 24 at D = 5; three borders;
                                                                      self, detached, both gradients; again under PEA_FORCE_DIRECT=1
    test_multi             k_bwd_multi (pea_multi_supported)          two 2D CIRCULAR scales + one 3D CROP_ZERO, f32 and bf16
    test_python_*          the AffinityMap node                       norm5 with |pred - t|^3, affs.sum(), affs[:, :2].mean(), bf16

The one combination the library declines: the runtime-D backward (D = 5) has no REPLICATE form, pea_affinity_bwd returns
PEA_E_UNSUPPORTED before anything is launched (affinity_op.AffinityMap raises for it) -- asserted as such, de left untouched.
test_python_norm5_cube_criterion runs at 2 x 16 x 6 x 28 x 32: the norm5 table steps 27 along y and x and an offset must be smaller
than the dimension it steps along (pea_desc_validate), so Y = 24 cannot hold it.

Result of the GPU run (MI355X): 116 cases, none failed -- every family ran where pea_cross_supported / its switch said it would, met the
float64 vjp inside the standing tolerances, and under CROP_ZERO gave bit-identical gradients for the two poisons; the inference map
serves as `affs` wherever the backward reads it; no library code was changed (include/pea.h: two comments).  Worst error over the
regular pixels, relative to their max, per family:

    k_bwd_xdma D = 16 2.2e-7   k_bwd_xdma_pf 2.7e-7 (affs NULL 2.7e-7)   k_bwd_xdma<OTHER> 2.2e-7   k_bwd_xdma_pfo 3.0e-7   <DUAL> 1.3e-7
    k_bwd_xdma<ZP> 2.0e-7      k_bwd_zm 2.0e-7 (all three segmentations)  k_bwd_box 2.3e-7           k_bwd_boxm 1.4e-7
    tiled 2.5e-7               direct 2.2e-7                              k_bwd_multi f32 2.0e-7, bf16 2.6e-3
    16-bit self f16 3.2e-4 (PEA_H16_HW=1 the same), bf16 2.5e-3           16-bit detached f16 3.6e-4, bf16 3.1e-3
    AffinityMap: norm5 2.3e-7, affs.sum() 1.7e-7, affs[:, :2].mean() 1.7e-7, bf16 2.0e-3

That the test can fail was checked on scratch copies of csrc/pea_tiled.h (k_bwd_tiled), the tiled cases run against each:
  - role A loads g_i(p) whether or not (p, p + o_i) exists, nothing else changed: all 18 cases still pass.  The kernel is protected twice:
    the neighbour vector of a pair that does not exist is staged / loaded as zeros as well, so g * 0 adds nothing.  That is the "read
    without effect" include/pea.h now allows for finite g (and why a non-finite g stays unspecified);
  - the same with the neighbour clamped into the image instead of zeroed (a kernel that never asks whether the pair exists): the three
    tiled CROP_ZERO cases fail BOTH checks -- ~24 900 of 59 200 gradient elements change with the poison, error 3.3 (self) and 782
    (detached, both) of max -- and the CIRCULAR, REPLICATE and direct cases pass.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from cross_stencils import DLOSS, DTYPES, ENV, EXPECT, FAMILIES, FLAG_ACCUMULATE, STENCILS, P, check_grad, fill_desc, make_inputs, relmax
from f64_reference import BORDER_CROP_ZERO, inv_norm_plane
from test_gpu_cross_stencils import _device_is_healthy, dev, expect, launched, nan, op, sync, synth  # noqa: F401  (fixtures; the autouse one too)
from vjp_reference import gone_mask, make_g, vjp

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -3
EPS = 1e-12
_CACHE = {}


# ---- inputs, G and the float64 vjp: computed once per case, shared by its switch variants ---------------------------------------------------
def family_inputs(synth, dev, family, stencil, border, other=False):
    key = ("I", family.replace("_march", ""), stencil, border, other)
    if key not in _CACHE:
        seed = 7 * sorted(STENCILS).index(stencil) + 3 * sorted(FAMILIES).index(key[1]) + border
        I = make_inputs(synth, dev, family, stencil, seed, other=other)
        I["seed"] = seed
        _CACHE[key] = I
    return _CACHE[key]


def shape_inputs(synth, dev, name, B, D, dims, o3, seed, dt="f32", other=False):
    """the dict of make_inputs (without targets) for a shape that is no entry of cross_stencils.FAMILIES"""
    key = ("S", name, other)
    if key not in _CACHE:
        Z, Y, X = dims
        S = Z * Y * X
        e = synth.synth_embedding((B, D, S), 100 + seed).reshape(B, D, Z, Y, X)
        e[:, :, 0, 0, 0] = 0.0
        e[:, :, Z - 1, Y - 1, X - 1] = 0.0
        e[-1, 0, Z - 1, Y - 1, X - 1] = 1e-14
        tdt = DTYPES[dt][0]
        I = dict(E=torch.from_numpy(e).to(dev).to(tdt), O=None, K=len(o3), o3=[list(o) for o in o3], B=B, dims=tuple(dims), D=D, tdt=tdt,
                 f32=dt == "f32", seed=seed)
        if other:
            eo = synth.synth_embedding((B, D, S), 500 + seed).reshape(B, D, Z, Y, X)
            eo[0, :, 0, 0, 0] = 0.0
            eo[0, :, Z - 1, Y - 1, X - 1] = 0.0
            I["O"] = torch.from_numpy(eo).to(dev).to(tdt)
        _CACHE[key] = I
    return _CACHE[key]


def upstream(I, border, salt=0):
    """(G, G_alt, float64 vjp for dloss = DLOSS with both gradients where there is a second operand)"""
    key = ("g", border, salt)
    if key not in I:
        G, G_alt = make_g(I, border, I["seed"] + 31 * salt)
        I[key] = (G, G_alt, vjp(I["E"], I["O"], G, I["o3"], EPS, border, DLOSS, other_grad=I["O"] is not None))
    return I[key]


def desc_for(pkg, I, border, norm=None, flags=0):
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2 if I["dims"][0] == 1 else 3, I["B"], I["D"], I["K"]
    d.dims[:] = list(I["dims"])
    d.border, d.dtype, d.norm, d.eps, d.flags = border, {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[I["tdt"]], (
        (1 if border == 1 else 0) if norm is None else norm), EPS, flags
    for i, o in enumerate(I["o3"]):
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    assert pkg._lib.lib().pea_desc_validate(ctypes.byref(d)) == 0
    return d


def regular_ratio(got, want, emb):
    """the error over the regular pixels, relative to their max (what check_grad asserts last)"""
    reg = (emb.double().pow(2).sum(1, keepdim=True).sqrt() >= EPS).expand_as(want)
    zero = torch.zeros_like(want)
    return relmax(torch.where(reg, got.double(), zero), torch.where(reg, want, zero))


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(v), b.view(v))


# ---- the caller's protocol ------------------------------------------------------------------------------------------------------------------
def protocol(pkg, op, dev, I, d, exp, what, raw_map=True):
    """what a vjp caller that follows pea_cross_supported prepares, with no training forward: -> (inv, raw)"""
    L, E, O = pkg._lib.lib(), I["E"], I["O"]
    plane = (I["B"],) + I["dims"]
    inv = raw = None
    if O is None and exp[1] == "1":
        inv = nan(plane, dev)
        assert launched(L.pea_inv_norm(ctypes.byref(d), P(E), P(inv), op._stream())) == 0, what
        want = inv_norm_plane(E, EPS)
    elif O is not None and exp[2] == "1":
        inv = nan((2,) + plane, dev)
        assert launched(L.pea_inv_norm(ctypes.byref(d), P(E), P(inv[0]), op._stream())) == 0, what
        assert launched(L.pea_inv_norm(ctypes.byref(d), P(O), P(inv[1]), op._stream())) == 0, what
        want = torch.stack([inv_norm_plane(E, EPS), inv_norm_plane(O, EPS)])
    if inv is not None:
        sync()
        assert torch.allclose(inv.double(), want, rtol=1e-5, atol=0.0), "%s: pea_inv_norm" % what
        if raw_map and exp[3 if O is None else 4] == "1":
            raw = nan((I["B"], I["K"]) + I["dims"], dev)
            assert launched(L.pea_affinity_infer(ctypes.byref(d), P(E), P(O), P(raw), op._stream())) == 0, what
            sync()
            assert bool(torch.isfinite(raw).all()), "%s: inference map not written" % what
    return inv, raw


def launch(pkg, op, dev, I, d, G, inv, raw, dl, want_other=False, want_de=True, base=None, plain=False):
    """one backward call -> (rc, de, de_other); plain: pea_affinity_bwd (no plane, no map)"""
    L, E, O = pkg._lib.lib(), I["E"], I["O"]
    de = nan(E.shape, dev, I["tdt"]) if want_de else None
    if base is not None:
        de.copy_(base)
    deo = nan(E.shape, dev, I["tdt"]) if want_other else None
    if plain:
        rc = L.pea_affinity_bwd(ctypes.byref(d), P(E), P(O), P(G), P(dl), P(de), P(deo), op._stream())
    else:
        rc = L.pea_affinity_bwd_ex2(ctypes.byref(d), P(E), P(O), P(G), P(inv), P(raw), P(dl), P(de), P(deo), op._stream())
    launched(rc)
    sync()
    return rc, de, deo


def hold(pkg, op, dev, I, d, border, fam, what, inv=None, raw=None, want_other=False, plain=False, null_dloss=False):
    """checks 1 - 4 of the header on one case -> de"""
    G, G_alt, ref = upstream(I, border)
    dl = torch.full((1,), DLOSS, device=dev)
    run = lambda g, s=dl: launch(pkg, op, dev, I, d, g, inv, raw, s, want_other=want_other, plain=plain)  # noqa: E731
    rc, de, deo = run(G)
    assert rc == 0, "%s: backward rc %d" % (what, rc)
    bad = []
    if border == BORDER_CROP_ZERO:
        assert G_alt is not None and bool(gone_mask(I, border).flatten(1).any(1).all()), "%s: an offset crops nothing" % what
        _, de_p, deo_p = run(G_alt)
        if not (bits_equal(de, de_p) and bits_equal(deo, deo_p)):
            n = int((de.double() != de_p.double()).sum()) + (0 if deo is None else int((deo.double() != deo_p.double()).sum()))
            bad.append("POISON: the g of a pair that does not exist changed %d gradient elements" % n)
    _, de_r, deo_r = run(G)
    if not (bits_equal(de, de_r) and bits_equal(deo, deo_r)):
        bad.append("a rerun is not bit-identical")
    pairs = [(de, ref["de"], I["E"], "de")] + ([(deo, ref["de_other"], I["O"], "de_other")] if want_other else [])
    for got, want, emb, name in pairs:
        print("vjp-ratio %s | %s %s | %.3g" % (fam, what, name, regular_ratio(got, want, emb)))
        try:
            check_grad(got, want, emb, I["f32"], "%s %s" % (what, name))
        except AssertionError as ex:
            bad.append("TOLERANCE: %s" % ex)
    if null_dloss:  # dloss = NULL is 1
        rc, de_1, _ = run(G, None)
        assert rc == 0, "%s: backward rc %d with dloss NULL" % (what, rc)
        try:
            check_grad(de_1, ref["de"] / DLOSS, I["E"], I["f32"], "%s dloss NULL" % what)
        except AssertionError as ex:
            bad.append("TOLERANCE: %s" % ex)
    assert not bad, "%s: %s" % (what, "; ".join(bad))
    return de


def _ids(params):
    return [pytest.param(*p, id="-".join(str(v) for v in p)) for p in params]


def _b(border):
    return "crop" if border else "circ"


# ---- k_bwd_xdma, D = 16, self ---------------------------------------------------------------------------------------------------------------
D16 = ([("f32_16", s) for s in ("pos", "asym", "two_sw32", "dup", "unsorted")] + [("f32_16_x96", "two_sw64"), ("f32_16_min", "two_sw64"),
                                                                                  ("f32_16_tall", "tall")])


@pytest.mark.parametrize("family,stencil,border", _ids([(f, s, b) for f, s in D16 for b in (0, 1)]))
def test_xdma_d16_self(pkg, op, dev, synth, family, stencil, border):
    what = "%s %s %s" % (family, stencil, _b(border))
    I = family_inputs(synth, dev, family, stencil, border)
    d = fill_desc(pkg, family, stencil, border)
    exp = expect(pkg, family, stencil, d)
    assert exp[1] == "1" and exp[3] == "0", what   # the cross backward that keeps G: no raw map is read
    inv, raw = protocol(pkg, op, dev, I, d, exp, what)
    assert inv is not None and raw is None
    hold(pkg, op, dev, I, d, border, "k_bwd_xdma D=16", what, inv=inv, null_dloss=(stencil == "pos"))


# ---- k_bwd_xdma_pf, D = 32 / 64: the raw map of pea_affinity_infer --------------------------------------------------------------------------
PF = [("f32_32", "pos"), ("f32_32", "two_sw32"), ("f32_64", "pos4"), ("f32_64", "asym")]


@pytest.mark.parametrize("family,stencil,border", _ids([(f, s, b) for f, s in PF for b in (0, 1)]))
def test_xdma_pf(pkg, op, dev, synth, family, stencil, border):
    what = "%s %s %s" % (family, stencil, _b(border))
    I = family_inputs(synth, dev, family, stencil, border)
    d = fill_desc(pkg, family, stencil, border)
    exp = expect(pkg, family, stencil, d)
    assert exp[1] == "1" and exp[3] == "1", what   # projection-first: <ehat, G> = sum g a from the map
    inv, raw = protocol(pkg, op, dev, I, d, exp, what)
    assert inv is not None and raw is not None
    hold(pkg, op, dev, I, d, border, "k_bwd_xdma_pf", what + " map", inv=inv, raw=raw, null_dloss=(stencil == "pos"))
    hold(pkg, op, dev, I, d, border, "k_bwd_xdma D>16 (affs NULL)", what + " affs=NULL", inv=inv, raw=None)


# ---- role A with a detached second operand, D = 16 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stencil,border,accumulate", _ids([(s, b, a) for s in ("pos", "two_sw32") for b in (0, 1) for a in (0, 1)]))
def test_role_a_d16(pkg, op, dev, synth, stencil, border, accumulate):
    family = "f32_16"
    what = "%s %s %s detached%s" % (family, stencil, _b(border), " +=" if accumulate else "")
    I = family_inputs(synth, dev, family, stencil, border, other=True)
    d = fill_desc(pkg, family, stencil, border)
    exp = expect(pkg, family, stencil, d)
    assert exp[2] == "1" and exp[4] == "0", what
    inv, raw = protocol(pkg, op, dev, I, d, exp, what)
    assert inv is not None and inv.shape[0] == 2 and raw is None
    de = hold(pkg, op, dev, I, d, border, "k_bwd_xdma<OTHER> D=16", what, inv=inv, null_dloss=(stencil == "pos" and not accumulate))
    if accumulate:
        # de += : bit-equal to the plain result + the pre-fill, added in f32 ("bit-equal to write + add")
        da = fill_desc(pkg, family, stencil, border, flags=FLAG_ACCUMULATE)
        G, G_alt, _ = upstream(I, border)
        idx = np.arange(I["E"].numel(), dtype=np.uint64)
        base = torch.from_numpy((synth.hash_uniform(idx, 977) - 0.5).astype(np.float32)).to(dev).view(I["E"].shape)
        dl = torch.full((1,), DLOSS, device=dev)
        for g in (G, G_alt):
            if g is None:
                continue
            rc, acc, _ = launch(pkg, op, dev, I, da, g, inv, None, dl, base=base)
            assert rc == 0, "%s: rc %d" % (what, rc)
            assert bits_equal(acc, de + base), "%s: accumulate is not write + add" % what


# ---- k_bwd_xdma_pfo: role A at D = 32 / 64 with the cross loss' raw map -----------------------------------------------------------------------
@pytest.mark.parametrize("family,stencil,border", _ids([(f, s, b) for f, s in (("f32_32", "pos"), ("f32_64", "pos4")) for b in (0, 1)]))
def test_xdma_pfo(pkg, op, dev, synth, family, stencil, border):
    what = "%s %s %s detached" % (family, stencil, _b(border))
    I = family_inputs(synth, dev, family, stencil, border, other=True)
    d = fill_desc(pkg, family, stencil, border)
    exp = expect(pkg, family, stencil, d)
    assert exp[2] == "1" and exp[4] == "1", what
    inv, raw = protocol(pkg, op, dev, I, d, exp, what)
    assert inv is not None and raw is not None
    hold(pkg, op, dev, I, d, border, "k_bwd_xdma_pfo", what, inv=inv, raw=raw, null_dloss=(border == 0))


# ---- 16-bit storage: self (k_bwd_xdma_h / _hqs) and detached ----------------------------------------------------------------------------------
H16 = [("f16_32", "small"), ("f16_32", "pos"), ("f16_32", "two_sw32"), ("bf16_64", "small"), ("bf16_64", "pos4"), ("bf16_64", "two_sw32")]


def _h16_params():
    out = [(f, s, b, o, "-") for f, s in H16 for b in (0, 1) for o in (0, 1)]
    out += [("f16_32", "small", b, 0, "1") for b in (0, 1)]   # the LDS-DMA form where the default runs producer / consumer waves
    return _ids(out)


@pytest.mark.parametrize("family,stencil,border,other,hw", _h16_params())
def test_h16(pkg, op, dev, synth, monkeypatch, family, stencil, border, other, hw):
    if hw != "-":
        monkeypatch.setenv("PEA_H16_HW", hw)
    what = "%s %s %s%s hw %s" % (family, stencil, _b(border), " detached" if other else "", hw)
    I = family_inputs(synth, dev, family, stencil, border, other=bool(other))
    d = fill_desc(pkg, family, stencil, border)
    exp = expect(pkg, family, stencil, d)
    assert (exp[2] == "1" and exp[4] == "1") if other else (exp[1] == "1" and exp[3] == "1"), what
    inv, raw = protocol(pkg, op, dev, I, d, exp, what)
    assert inv is not None and raw is not None
    fam = "16-bit detached" if other else ("k_bwd_xdma_h (PEA_H16_HW=1)" if hw == "1" else "16-bit self (h / hqs)")
    hold(pkg, op, dev, I, d, border, fam, what, inv=inv, raw=raw, null_dloss=(stencil == "small" and border == 0 and hw == "-"))


# ---- the pair backward: one launch ----------------------------------------------------------------------------------------------------------
def test_pair(pkg, op, dev, synth):
    family, stencil, border, what = "f32_16", "pos", 0, "pair f32_16 pos circ"
    L = pkg._lib.lib()
    I = family_inputs(synth, dev, family, stencil, border, other=True)
    d = fill_desc(pkg, family, stencil, border)
    exp = expect(pkg, family, stencil, d)
    assert exp[1] == "1" and exp[2] == "1" and exp[5] == "1", what
    inv, _ = protocol(pkg, op, dev, I, d, exp, what)
    Gx, _, ref_x = upstream(I, border)
    G0, _ = make_g(I, border, I["seed"] + 1000)
    ref_0 = vjp(I["E"], None, G0, I["o3"], EPS, border, DLOSS)
    want = ref_0["de"] + ref_x["de"] * (1.5 / DLOSS)
    dl0, dlx = torch.full((1,), DLOSS, device=dev), torch.full((1,), 1.5, device=dev)
    out = []
    for _ in range(2):
        de = nan(I["E"].shape, dev)
        rc = launched(L.pea_affinity_bwd_dual_ex(ctypes.byref(d), P(I["E"]), P(I["O"]), P(G0), P(Gx), P(inv[0]), P(inv[1]), P(dl0), P(dlx),
                                                 P(de), op._stream()))
        sync()
        assert rc == 0, "%s: rc %d" % (what, rc)
        out.append(de)
    assert bits_equal(out[0], out[1]), "%s: a rerun is not bit-identical" % what
    print("vjp-ratio k_bwd_xdma<DUAL> | %s | %.3g" % (what, relmax(out[0], want)))
    check_grad(out[0], want, I["E"], True, what)


# ---- 3D: tile per plane (ZP) and the z-march -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,stencil,zseg", _ids([("v3", "z_mixed", "-"), ("v3", "z_neg_inplane_pos", "-"), ("v3_march", "z_neg_inplane_pos", "-"),
                                                      ("v3_march", "z_neg_inplane_pos", "2"), ("v3_march", "z_neg_inplane_pos", "3")]))
def test_volume(pkg, op, dev, synth, monkeypatch, family, stencil, zseg):
    """PEA_ZSEG=2 / 3 at Z = 6: three / two segments per tile column, so warm-up and drain of the march see planes that carry poison"""
    if family in ENV:
        monkeypatch.setenv(*ENV[family])
    if zseg != "-":
        monkeypatch.setenv("PEA_ZSEG", zseg)
    what = "%s %s zseg %s" % (family, stencil, zseg)
    I = family_inputs(synth, dev, family, stencil, 1)
    d = fill_desc(pkg, family, stencil, 1)
    exp = expect(pkg, family, stencil, d)
    march = family == "v3_march"
    assert exp[1] == "1" and exp[3] == ("1" if march else "0"), what
    inv, raw = protocol(pkg, op, dev, I, d, exp, what)
    assert inv is not None and (raw is not None) == march
    hold(pkg, op, dev, I, d, 1, "k_bwd_zm" if march else "k_bwd_xdma<ZP>", what, inv=inv, raw=raw, null_dloss=(zseg == "-" and stencil != "z_mixed"))


# ---- the unit-box kernels --------------------------------------------------------------------------------------------------------------------
_N26 = [[dz, dy, dx] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
BOX = {  # the shapes of tests/test_gpu_parity.py::test_unit_box_stencils_vs_oracle: (B, dims, offsets, border, norm)
    "n26_crop": (2, (5, 37, 72), _N26, 1, 1),
    "n26_circular": (1, (4, 33, 68), _N26, 0, 2),
    "subset_3d": (2, (3, 20, 40), [[-1, 0, 0], [0, -1, 1], [1, 1, -1], [0, 0, -1], [-1, -1, -1], [1, 0, 1], [0, 1, 0]], 1, 1),
    "diag_2d_mask": (3, (1, 50, 100), [[0, -1, -1], [0, -1, 1], [0, 1, 1], [0, 0, -1], [0, -1, 0]], 0, 0),
}


@pytest.mark.parametrize("case,kernel", _ids([("n26_crop", "box"), ("n26_crop", "boxm"), ("subset_3d", "box"), ("subset_3d", "boxm"),
                                              ("n26_circular", "box"), ("diag_2d_mask", "box")]))
def test_box(pkg, op, dev, synth, monkeypatch, case, kernel):
    """k_bwd_box (PEA_BOXM=0 on the CROP volumes: nothing marches) and k_bwd_boxm (PEA_ZMARCH=2: the march on a volume this small; CROP_ZERO,
    Z >= 3), csrc/pea_k_box.hip::box_bwd"""
    B, dims, o3, border, norm = BOX[case]
    if border:
        monkeypatch.setenv(*(("PEA_BOXM", "0") if kernel == "box" else ("PEA_ZMARCH", "2")))
    assert kernel == "box" or (border == 1 and dims[0] >= 3)
    what = "%s %s" % (case, kernel)
    I = shape_inputs(synth, dev, case, B, 16, dims, o3, 60 + len(o3))
    d = desc_for(pkg, I, border, norm=norm)
    got = "".join(str(int(pkg._lib.lib().pea_cross_supported(ctypes.byref(d), m))) for m in range(6))
    assert got[:2] == "11" and got[3] == "0", "%s: pea_cross_supported %s" % (what, got)   # the box family, no map read
    inv, raw = protocol(pkg, op, dev, I, d, got, what)
    assert inv is not None and raw is None
    hold(pkg, op, dev, I, d, border, "k_bwd_" + kernel, what, inv=inv, null_dloss=(case == "subset_3d"))


# ---- tiled / direct: pea_affinity_bwd, no plane ---------------------------------------------------------------------------------------------
_S2 = [[0, -2, -3], [0, 5, 1], [0, 0, -11], [0, 7, 0]]
TILED = {"d16_37x50": (2, 16, (1, 37, 50), _S2), "d5_3x20x24": (2, 5, (3, 20, 24), _S2 + [[-1, 2, -3]])}


@pytest.mark.parametrize("shape,border,mode,direct", _ids([(s, b, m, f) for s in TILED for b in (0, 1, 2) for m in ("self", "detached", "both")
                                                           for f in (0, 1)]))
def test_tiled_direct(pkg, op, dev, synth, monkeypatch, shape, border, mode, direct):
    """no 1 / norm plane: the tiled kernels (pea_tiled.h) or, under PEA_FORCE_DIRECT=1 and at a runtime D, the direct ones (pea_direct.h).
    REPLICATE: every pair exists, no poison; the role-B pre-image loop sees a dense g"""
    if direct:
        monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
    B, D, dims, o3 = TILED[shape]
    what = "%s border %d %s%s" % (shape, border, mode, " direct" if direct else "")
    I = shape_inputs(synth, dev, shape, B, D, dims, o3, 11 + D, other=(mode != "self"))
    d = desc_for(pkg, I, border, norm=(2 if border == 2 else None))
    fam = "direct" if (direct or D == 5) else "tiled"
    if border == 2 and D == 5:  # the one refusal: the runtime-D backward has no REPLICATE form (affinity_op.AffinityMap raises for it)
        G, _, _ = upstream(I, border)
        rc, de, _ = launch(pkg, op, dev, I, d, G, None, None, None, want_other=(mode == "both"), plain=True)
        assert rc == E_UNSUPPORTED and bool(torch.isnan(de).all()), "%s: rc %d" % (what, rc)
        return
    hold(pkg, op, dev, I, d, border, fam, what, want_other=(mode == "both"), plain=True, null_dloss=(border == 1 and mode == "self"))


# ---- k_bwd_multi -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_multi(pkg, op, dev, synth, dt):
    """one table of three entries, built as tests/test_gpu_multi.py::_run_table builds its own: two 2D CIRCULAR scales and one 3D CROP_ZERO,
    each with its own G and its own dloss; every de_j against its own vjp, the CROP entry against the other poison"""
    L, mo = pkg._lib.lib(), pkg.multi_offset
    lift = lambda offs: [[0] * (3 - len(o)) + list(o) for o in offs]  # noqa: E731
    cfg = [(2, 16, (1, 37, 70), lift(mo([1, 3, 5, 9], 4)), 0, 0.625), (1, 32, (1, 19, 33), lift(mo([1, 3], 8)), 0, 1.75),
           (2, 16, (4, 16, 24), [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], 1, 0.5)]
    n = len(cfg)
    ents = []
    for j, (B, D, dims, o3, border, dloss) in enumerate(cfg):
        I = shape_inputs(synth, dev, "multi%d_%s" % (j, dt), B, D, dims, o3, 90 + j, dt=dt)
        G, G_alt = make_g(I, border, 70 + j)
        ents.append(dict(I=I, d=desc_for(pkg, I, border), G=G, G_alt=G_alt, border=border, dloss=dloss,
                         dl=torch.full((1,), dloss, device=dev), ref=vjp(I["E"], None, G, o3, EPS, border, dloss)))
    arr = (ctypes.POINTER(pkg._lib.PeaDesc) * n)(*[ctypes.pointer(x["d"]) for x in ents])
    assert L.pea_multi_supported(arr, n) == 1

    def run(alt):
        bt, des = (pkg._lib.PeaMultiBwd * n)(), []
        for j, x in enumerate(ents):
            g = x["G_alt"] if (alt and x["G_alt"] is not None) else x["G"]
            de = nan(x["I"]["E"].shape, dev, x["I"]["tdt"])
            b = bt[j]
            b.desc, b.e, b.g, b.dloss, b.de = ctypes.pointer(x["d"]), x["I"]["E"].data_ptr(), g.data_ptr(), x["dl"].data_ptr(), de.data_ptr()
            des.append(de)
        rc = launched(L.pea_affinity_bwd_multi(bt, n, op._stream()))
        sync()
        assert rc == 0, "pea_affinity_bwd_multi rc %d" % rc
        return des

    first, again, poisoned = run(False), run(False), run(True)
    for j, x in enumerate(ents):
        what = "multi %s entry %d" % (dt, j)
        assert bits_equal(first[j], again[j]), "%s: a rerun is not bit-identical" % what
        assert bits_equal(first[j], poisoned[j]), "%s: POISON: the g of a pair that does not exist reached de" % what
        print("vjp-ratio k_bwd_multi %s | %s | %.3g" % (dt, what, regular_ratio(first[j], x["ref"]["de"], x["I"]["E"])))
        check_grad(first[j], x["ref"]["de"], x["I"]["E"], dt == "f32", what)


# ---- through Python: the AffinityMap node ----------------------------------------------------------------------------------------------------
def _tw(synth, dev, shape, seed):
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    t = (synth.hash_uniform(idx, seed) < 0.6).astype(np.float32).reshape(shape)
    w = (0.5 + synth.hash_uniform(idx, seed + 1)).astype(np.float32).reshape(shape)
    return torch.from_numpy(t).to(dev), torch.from_numpy(w).to(dev)


def _cube(pred, tgt, wt):
    return torch.sum(wt * torch.abs(pred - tgt) ** 3) / pred.shape[0]


def _upstream_of(loss_fn, affs64):
    """d loss_fn(affs) / d affs in float64"""
    with torch.enable_grad():
        a = affs64.detach().clone().requires_grad_(True)
        loss_fn(a).backward()
    return a.grad


def test_python_norm5_cube_criterion(pkg, op, dev, synth):
    """embedding_loss_norm5 (3D, CROP_ZERO) with the foreign criterion sum(w |pred - t|^3) / B: once as the loss module applies it (per
    channel, on the cropped slice) and once on the WHOLE map through AffinityMap -- there d_affs is non-zero on the zero border slices
    (pred = 0 != t): the caller the vjp contract was written for"""
    m3 = importlib.import_module(ge.PKG_NAME + ".loss.loss_embedding_mse_3d")
    spec = m3._spec(m3.NORM5_SHIFTS, 1, 3)
    o3 = [list(o) for o in spec.offsets]
    I = shape_inputs(synth, dev, "py_norm5", 2, 16, (6, 28, 32), o3, 77)
    E = I["E"]
    t, w = _tw(synth, dev, (2, len(o3), 6, 28, 32), 780)
    affs64 = vjp(E, None, torch.zeros_like(t), o3, EPS, 1, 1.0)["affs"]

    def module_loss(a):  # loss_embedding_mse_3d._foreign
        loss = 0
        for i, s in enumerate(m3.NORM5_SHIFTS):
            ax = 2 + i % 3
            k = a.shape[ax] - s
            loss = loss + _cube(a[:, i:i + 1].narrow(ax, s, k), t.double()[:, i:i + 1].narrow(ax, s, k), w.double()[:, i:i + 1].narrow(ax, s, k))
        return loss

    et = E.clone().requires_grad_(True)
    loss, affs = pkg.embedding_loss_norm5(et, t, w, _cube)
    (loss * DLOSS).backward()
    sync()
    assert float((affs.double() - affs64).abs().max()) < 1e-5
    assert abs(float(loss.detach()) - float(module_loss(affs64))) <= 1e-5 * abs(float(module_loss(affs64)))
    check_grad(et.grad, vjp(E, None, _upstream_of(module_loss, affs64), o3, EPS, 1, DLOSS)["de"], E, True, "norm5, cube criterion")

    whole = lambda a: _cube(a, t.to(a.dtype), w.to(a.dtype))  # noqa: E731
    G = _upstream_of(whole, affs64)
    gone = gone_mask(I, 1).unsqueeze(0).expand_as(G)
    assert bool(G[gone].any()), "the whole-map criterion has a gradient on the cropped pairs"
    et = E.clone().requires_grad_(True)
    (whole(op.AffinityMap.apply(et, None, spec)) * DLOSS).backward()
    sync()
    check_grad(et.grad, vjp(E, None, G, o3, EPS, 1, DLOSS)["de"], E, True, "norm5 map, cube criterion on the whole map")


@pytest.mark.parametrize("form", ["sum", "mean_of_two"])
def test_python_2d_autograd_gradients(pkg, op, dev, synth, form):
    """affs.sum().backward(): autograd hands over an expanded, stride-0 gradient; affs[:, :2].mean().backward(): whole zero channels"""
    o3 = _S2
    I = shape_inputs(synth, dev, "py_2d", 2, 16, (1, 37, 50), o3, 27)
    E = I["E"][:, :, 0]
    spec = op.AffinitySpec(2, [o[1:] for o in o3], None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX, EPS)
    fn = (lambda a: a.sum()) if form == "sum" else (lambda a: a[:, :2].mean())
    et = E.clone().requires_grad_(True)
    affs = op.AffinityMap.apply(et, None, spec)
    fn(affs).backward()
    sync()
    affs64 = vjp(I["E"], None, torch.zeros((2, 4, 1, 37, 50), device=dev), o3, EPS, 0, 1.0)["affs"]
    G = _upstream_of(fn, affs64)
    assert form == "sum" or not bool(G[:, 2:].any())
    check_grad(et.grad.unsqueeze(2), vjp(I["E"], None, G, o3, EPS, 0, 1.0)["de"], I["E"], True, "2D map, %s" % form)


def test_python_bf16_foreign_criterion(pkg, op, dev, synth):
    """a bf16 embedding through a foreign criterion: e.grad is bf16 and within the 16-bit tolerance of the vjp on the embedding as rounded"""
    offsets = pkg.multi_offset([1, 3, 9], 8)
    o3 = [[0] + list(o) for o in offsets]
    I = shape_inputs(synth, dev, "py_bf16", 2, 16, (1, 30, 44), o3, 37, dt="bf16")
    E = I["E"][:, :, 0]
    K = len(o3)
    t, w = _tw(synth, dev, (2, K, 30, 44), 880)
    m = torch.from_numpy((synth.hash_uniform(np.arange(t.numel(), dtype=np.uint64), 882) < 0.9).astype(np.uint8).reshape(t.shape)).to(dev)
    et = E.clone().requires_grad_(True)
    loss, affs, _ = pkg.embedding_loss(et, t, w, m, _cube, offsets)
    (loss * DLOSS).backward()
    sync()
    assert et.grad.dtype == torch.bfloat16
    affs64 = vjp(I["E"], None, torch.zeros((2, K, 1, 30, 44), device=dev), o3, EPS, 0, 1.0)["affs"]

    def module_loss(a):  # loss_embedding_mse._foreign_criterion
        a = a[:, :, 0]
        return sum(_cube(a[:, i] * m[:, i].double(), t[:, i].double() * m[:, i].double(), w[:, i].double()) for i in range(K))

    assert float((affs.double() - affs64[:, :, 0]).abs().max()) < 1e-5
    check_grad(et.grad.unsqueeze(2), vjp(I["E"], None, _upstream_of(module_loss, affs64), o3, EPS, 0, DLOSS)["de"], I["E"], False, "bf16, cube criterion")
