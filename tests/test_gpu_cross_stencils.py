"""GPU (-m gpu): the LDS-DMA cross kernels on every axis-aligned stencil plan_xdma accepts, not only the reference's tables.

Every other GPU test that reaches csrc/pea_xdma.h, pea_xdma_pf.h, pea_xdma_dual.h, pea_xdma_h16.h, pea_xdma_hq.h, the in-plane part of
pea_zmarch.h or the labels-in forward builds its stencil with multi_offset(shifts, 4) or axis_offsets_3d: negative offsets, y and x
alternating, ascending, no repeats.  The kernels have code of their own for what the sign decides -- which strip a neighbour column
lands in (split, SW = 32 / 64, the xm / fm masks), the one-sided halos of the forward and of the role-A backward (hy0 / hy1), the g index
of the role-B slots (xgo, ygo, zgo), the spare slots that repeat slot 0 -- and a caller whose convention is +shift gets all of it on
its first call.  An error there is a plausible-looking affinity map, not a crash.

Every case is held to tests/f64_reference.py::cosine_loss, evaluated in float64 on the device (16-bit storage: on the embedding
already rounded to the storage type), with the suite's standing tolerances -- nothing new is measured:

    affs 1e-5 absolute, loss and every L_i 1e-5 relative, gradient 1e-4 of its max       (tests/test_gpu_parity.py)
    gradient 8e-3 of its max for 16-bit storage                                          (tests/test_gpu_alignment.py)

Each case has its own targets, weights and u8 mask per channel, distinct lambda_i, dloss = 0.625 and zero-norm pixels at (0, 0) and at
(Y-1, X-1), so that the eps branch is read through both strips (16-bit storage: the gradient AT those pixels, G / eps, does not fit
the storage type and is left out of the comparison; their neighbours' is in it).  Outputs are pre-filled with NaN: every element must be
written.  Before a case runs, pea_cross_supported(desc, 0 .. 5) must equal the table of tests/cross_stencils.py (EXPECT, pinned on the
host by tests/test_cross_stencils_host.py), and the caller's protocol follows it: the 1 / norm plane(s) are handed over where mode 1
(mode 2) says 1, the raw map where mode 3 (mode 4) does.  A refused case is still held to the reference: the next family serves it.

Stencils (tests/cross_stencils.py; (dy, dx), B = 2, 50 x 100 unless said otherwise: ragged 16 x 32 tiles on both axes):

    pos        +s along y and x, s in 1, 3, 5, 9, 27 (K = 10)     right strip only (split = 32), down halo only
    pos4       the same with s in 1, 3, 9, 27                      what the D = 64 backward holds (eight slots per axis)
    asym       y: +1, +3, +9; x: -1, -3, -27                       down halo with the left strip
    two_sw32   x: -1, +3, -9, +16; y: +1, -5, +9                   both strips, SW = 32, split = 16, reach exactly 16
    small      two_sw32 without the 16                             reach <= 9 both ways: the producer / consumer f16 backward
    two_sw64   x: -27, +17, +1; y: -27, +27                        both strips, SW = 64; the forward's 51-unit plane, filled; X = 100 and 96
    reach32    x: +32, -32; y: -1                                  reach == TW
    reach33    x: +33; y: -1                                       refused everywhere
    x_only     x: -1, -3, -5, -9, -27                              all ten x slots, no y slot: role A refuses
    y_only     y: +1, +3, +5, +9, +27                              the same on y
    six_on_x   x: -1, -2, -3, -5, -9, -11; y: -1, -3               forward accepted, self backward refused: two families in one step
    dup        (0,-3), (-3,0), (0,-3), (-9,0), (0,+3)              a repeated offset: the two maps bit-identical; +3 / -3 share a slot pair
    unsorted   the shipped ten reversed, x before y                slot 0 is the longest reach
    tall       y: +35, -35; x: +1 (52 x 100)                       the tallest halo the 51-unit planes hold (the shipped tables stop at 27)
    tall36     y: +36, -36; x: +1                                  one row more: refused everywhere
    z_mixed, z_neg_inplane_pos, z5                                 3D (2, 6, 48, 96), CROP_ZERO: see test_volume

pos, unsorted and two_sw64 also run at 43 x 96, the smallest image the +-27 self backward accepts, and pos at 43 x 64, the smallest the
one-sided forward accepts (there the self backward, two-sided through role B, is refused).

Families, and the modes of pea_cross_supported each asserts (all six, against EXPECT; the ones that decide its kernels are named):

    test_f32_d16_self       every stencil, both borders; train forward, backward, inference          modes 0, 1
    test_f32_wide_self      D = 32 / 64, every stencil, both borders; the backward with the raw map  modes 0, 1, 3
    test_h16_self           f16 D = 32, bf16 D = 64, X = 104, every stencil, both borders; small, pos, two_sw32 and dup also with
                            PEA_H16_HW=1 (the LDS-DMA form where the default runs producer / consumer waves) and =0   modes 0, 1, 3
    test_detached           D = 16 with and without PEA_FLAG_ACCUMULATE_DE; D = 32 / 64, f16, bf16 with the raw map   modes 2, 4
    test_planes_and_raw_map_handed_over_unasked   every refused backward once more with the planes and the raw map handed over
    test_pair               pea_affinity_fwd_dual_ex + pea_affinity_bwd_dual_ex against the two calls   mode 5 (and 1, 2)
    test_labels_two_launch  embedding_loss_from_labels with the scratch against the targets path     pea_labels_scratch_bytes
    test_volume             the three 3D stencils; z_neg_inplane_pos under PEA_ZMARCH=2               modes 0, 1, 3

Result of the GPU run (MI355X): 414 cases, none found wrong -- every accepted stencil ran on the family the table names and met the
float64 reference inside the standing tolerances, every refused one was served by the next family; no library code was changed.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from cross_stencils import (AFFS_ATOL, DLOSS, E_UNSUPPORTED, ENV, EXPECT, FAMILIES, FLAG_ACCUMULATE, LABELS_TWO_LAUNCH, STENCILS, P,
                            check_affs, check_cropped_exact, check_grad, check_loss, fill_desc, make_inputs, reference, relmax, supported)
from f64_reference import BORDER_CROP_ZERO, cosine_loss, shifted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(ge.PKG_NAME + ".affinity_op")


def sync():
    """sync(); a device error ends the whole run -- nothing more is started on a GPU that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:
        pytest.exit("device error, run ended: %s" % ex, returncode=3)


def launched(rc):
    """the return code of a call; a positive one is a hipError_t: the run ends there"""
    if rc > 0:
        pytest.exit("hipError %d from the library, run ended" % rc, returncode=3)
    return rc


@pytest.fixture(autouse=True)
def _device_is_healthy(dev):
    """a device error -- wherever in a test it surfaced -- ends the run before the next test launches anything"""
    sync()
    yield
    sync()


_CACHE = {}


def inputs(synth, dev, family, stencil, border, other=False):
    """inputs and float64 reference(s) of a case, computed once (the switch variants and the accumulate variant share them)"""
    key = (family.replace("_march", ""), stencil, border, other)
    if key not in _CACHE:
        seed = 7 * sorted(STENCILS).index(stencil) + 3 * sorted(FAMILIES).index(key[0]) + border
        I = make_inputs(synth, dev, family, stencil, seed, other=other)
        I["ref"] = reference(I, border, I["O"])
        _CACHE[key] = I
    return _CACHE[key]


def nan(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


def states(pkg, op, dev, d, n=1):
    L = pkg._lib.lib()
    sb = int(L.pea_workspace_bytes(ctypes.byref(d)))
    st = torch.empty(n * sb // 4, dtype=torch.int32, device=dev)
    assert L.pea_workspace_init(P(st), n * sb, op._stream()) == 0
    return st, sb


def expect(pkg, family, stencil, d):
    exp = EXPECT[family][stencil]
    got = supported(pkg, d)
    assert got == exp, "%s %s: pea_cross_supported modes 0..5 = %s, the table says %s" % (family, stencil, got, exp)
    return exp


def loss_step(pkg, op, dev, I, d, exp, border, what, accumulate=False, hand_all=False):
    """pea_affinity_fwd_ex + pea_affinity_bwd_ex2 as a caller that follows pea_cross_supported makes them, held to I["ref"];
    -> (affs, g).  With a second operand (I["O"]): the role-A backward, de only.  hand_all: the caller that never asks -- the
    1 / norm plane(s) and the raw map always come along ("same result either way", include/pea.h)"""
    L = pkg._lib.lib()
    B, K, dims, other = I["B"], I["K"], I["dims"], I["O"]
    kshape, plane = (B, K) + dims, (B,) + dims
    affs, g, lv = nan(kshape, dev), nan(kshape, dev), nan((1 + K,), dev)
    inv = None
    if other is None and (hand_all or exp[1] == "1"):
        inv = nan(plane, dev)
    elif other is not None and (hand_all or exp[2] == "1"):
        inv = nan((2,) + plane, dev)
    st, sb = states(pkg, op, dev, d)
    rc = launched(L.pea_affinity_fwd_ex(ctypes.byref(d), P(I["E"]), P(other), P(I["T"]), P(I["W"]), P(I["M"]), P(affs), P(g), P(inv), P(lv),
                                        P(st), sb, op._stream()))
    assert rc == 0, "%s: forward rc %d" % (what, rc)
    raw = affs if (inv is not None and (hand_all or exp[3 if other is None else 4] == "1")) else None
    dl = torch.full((1,), DLOSS, device=dev)
    ref = I["ref"]
    base = None
    de = nan(I["E"].shape, dev, I["tdt"])
    if accumulate:
        gen = torch.Generator().manual_seed(5)
        base = ((torch.rand(I["E"].shape, generator=gen) - 0.5) * 1e-3).to(dev)
        de.copy_(base)
    rc = launched(L.pea_affinity_bwd_ex2(ctypes.byref(d), P(I["E"]), P(other), P(g), P(inv), P(raw), P(dl), P(de), None, op._stream()))
    sync()
    check_affs(affs, ref["affs"], what)
    check_loss(lv, ref, what)
    if inv is not None:
        assert bool(torch.isfinite(inv).all()), "%s: 1 / norm plane not written" % what
    if accumulate and exp[2] == "0":
        # only the role-A cross kernel accumulates (include/pea.h): a stencil it refuses is refused, and de is left alone
        assert rc == E_UNSUPPORTED, "%s: backward rc %d" % (what, rc)
        assert torch.equal(de, base), "%s: a declined accumulate touched de" % what
    else:
        assert rc == 0, "%s: backward rc %d" % (what, rc)
        want = ref["de"] if base is None else ref["de"] + base.double()
        check_grad(de, want, I["E"], I["f32"], what)
    if border:
        check_cropped_exact(I, affs, g, what)
    return affs, g


def infer(pkg, op, dev, I, d, affs, what):
    """pea_affinity_infer on the same descriptor: the reference's map, and the training map"""
    out = nan(affs.shape, dev)
    rc = launched(pkg._lib.lib().pea_affinity_infer(ctypes.byref(d), P(I["E"]), P(I["O"]), P(out), op._stream()))
    sync()
    assert rc == 0, "%s: inference rc %d" % (what, rc)
    check_affs(out, I["ref"]["affs"], what + " (inference)")
    err = float((out - affs).abs().max())
    assert err < AFFS_ATOL, "%s: inference and training maps differ by %.3g" % (what, err)
    return out


def pairs(family, borders=(0, 1)):
    return [pytest.param(s, b, id="%s-%s" % (s, "crop" if b else "circ")) for s in EXPECT[family] for b in borders]


# ---- f32, D = 16: the only family that must run every stencil -------------------------------------------------------------------------
F32_16 = ("f32_16", "f32_16_x96", "f32_16_min", "f32_16_min64", "f32_16_tall")


@pytest.mark.parametrize("family,stencil,border", [pytest.param(f, *p.values, id="%s-%s" % (f, p.id)) for f in F32_16 for p in pairs(f)])
def test_f32_d16_self(pkg, op, dev, synth, family, stencil, border):
    what = "%s %s border %d" % (family, stencil, border)
    I = inputs(synth, dev, family, stencil, border)
    d = fill_desc(pkg, family, stencil, border, lam=I["lam"])
    exp = expect(pkg, family, stencil, d)
    affs, _ = loss_step(pkg, op, dev, I, d, exp, border, what)
    out = infer(pkg, op, dev, I, d, affs, what)
    if stencil == "dup":  # the repeated offset: one map twice, whatever target / weight / lambda its two channels carry
        assert torch.equal(affs[:, 0], affs[:, 2]) and torch.equal(out[:, 0], out[:, 2]), what


# ---- f32, D = 32 / 64: the backward with the raw map (mode 3) ----------------------------------------------------------------------------
@pytest.mark.parametrize("family,stencil,border", [pytest.param(f, *p.values, id="%s-%s" % (f, p.id)) for f in ("f32_32", "f32_64")
                                                   for p in pairs(f)])
def test_f32_wide_self(pkg, op, dev, synth, family, stencil, border):
    what = "%s %s border %d" % (family, stencil, border)
    I = inputs(synth, dev, family, stencil, border)
    d = fill_desc(pkg, family, stencil, border, lam=I["lam"])
    exp = expect(pkg, family, stencil, d)
    assert exp[3] == exp[1]  # at D > 16 the self backward of the cross family is the projection-first kernel: it reads the raw map
    affs, _ = loss_step(pkg, op, dev, I, d, exp, border, what)
    infer(pkg, op, dev, I, d, affs, what)


# ---- 16-bit storage: f16 at D = 32, bf16 at D = 64, X = 104 ------------------------------------------------------------------------------
def _h16_params():
    out = [pytest.param(f, *p.values, None, id="%s-%s" % (f, p.id)) for f in ("f16_32", "bf16_64") for p in pairs(f)]
    # the LDS-DMA form of the f16 backward where the default (PEA_H16_HW=2) takes producer / consumer waves, and the f32 working buffer
    for s in ("small", "pos", "two_sw32", "dup"):
        for hw in ("1", "0"):
            out.append(pytest.param("f16_32", s, 0, hw, id="f16_32-%s-circ-hw%s" % (s, hw)))
    out.append(pytest.param("f16_32", "small", 1, "1", id="f16_32-small-crop-hw1"))
    return out


@pytest.mark.parametrize("family,stencil,border,hw", _h16_params())
def test_h16_self(pkg, op, dev, synth, monkeypatch, family, stencil, border, hw):
    if hw is not None:
        monkeypatch.setenv("PEA_H16_HW", hw)
    what = "%s %s border %d hw %s" % (family, stencil, border, hw)
    I = inputs(synth, dev, family, stencil, border)
    d = fill_desc(pkg, family, stencil, border, lam=I["lam"])
    exp = EXPECT[family][stencil]
    if hw == "0":  # (the second operand's 16-bit kernels need the 16-bit working buffer: modes 2 and 4 turn 0, nothing else moves)
        exp = exp[:2] + "0" + exp[3] + "0" + exp[5]
        assert supported(pkg, d) == exp, what
    else:
        exp = expect(pkg, family, stencil, d)
    affs, _ = loss_step(pkg, op, dev, I, d, exp, border, what)
    infer(pkg, op, dev, I, d, affs, what)


# ---- the detached second operand: role A only --------------------------------------------------------------------------------------------
def _detached_params():
    out = []
    for p in pairs("f32_16"):
        out.append(pytest.param("f32_16", *p.values, False, id="f32_16-%s" % p.id))
        out.append(pytest.param("f32_16", *p.values, True, id="f32_16-%s-acc" % p.id))
    # the smallest images and the tallest halo; the projection-first role-A backwards (mode 4), f32 and 16-bit
    for f in ("f32_16_min", "f32_16_min64", "f32_16_tall", "f32_32", "f32_64", "f16_32", "bf16_64"):
        out += [pytest.param(f, *p.values, False, id="%s-%s" % (f, p.id)) for p in pairs(f)]
    return out


@pytest.mark.parametrize("family,stencil,border,accumulate", _detached_params())
def test_detached(pkg, op, dev, synth, family, stencil, border, accumulate):
    what = "%s %s border %d detached%s" % (family, stencil, border, " +=" if accumulate else "")
    I = inputs(synth, dev, family, stencil, border, other=True)
    d = fill_desc(pkg, family, stencil, border, flags=FLAG_ACCUMULATE if accumulate else 0, lam=I["lam"])
    exp = expect(pkg, family, stencil, d)
    loss_step(pkg, op, dev, I, d, exp, border, what, accumulate=accumulate)


# ---- the caller that never asks ------------------------------------------------------------------------------------------------------
def _unasked_params():
    """every (family, stencil) whose self backward or role-A backward pea_cross_supported refuses: with the plane(s) and the raw map
    handed over all the same, the launchers decide alone.  Some then run a cross kernel the query does not promise -- at D = 64 the
    projection-first backward has ten slots per axis where the plain one has eight -- and that kernel is held to the reference too."""
    out = []
    for f in ("f32_16", "f32_32", "f32_64", "f16_32", "bf16_64"):
        for s, exp in EXPECT[f].items():
            for other in (False, True):
                if exp[2 if other else 1] == "0":
                    out += [pytest.param(f, s, b, other, id="%s-%s-%s%s" % (f, s, "crop" if b else "circ", "-detached" if other else ""))
                            for b in (0, 1)]
    return out


@pytest.mark.parametrize("family,stencil,border,other", _unasked_params())
def test_planes_and_raw_map_handed_over_unasked(pkg, op, dev, synth, family, stencil, border, other):
    what = "%s %s border %d unasked%s" % (family, stencil, border, " detached" if other else "")
    I = inputs(synth, dev, family, stencil, border, other=other)
    d = fill_desc(pkg, family, stencil, border, lam=I["lam"])
    exp = expect(pkg, family, stencil, d)
    loss_step(pkg, op, dev, I, d, exp, border, what, hand_all=True)


# ---- the pair: one forward launch, one backward launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("stencil,border", pairs("f32_16"))
def test_pair(pkg, op, dev, synth, stencil, border):
    """pea_affinity_fwd_dual_ex: every output BIT-identical to the two pea_affinity_fwd_ex calls it replaces (include/pea.h), which are
    held to the float64 reference; pea_affinity_bwd_dual_ex against dl * de(self) + dl_cross * de(cross) of the reference"""
    family, what = "f32_16", "pair %s border %d" % (stencil, border)
    L = pkg._lib.lib()
    I = inputs(synth, dev, family, stencil, border, other=True)
    if "ref_self" not in I:
        I["lam_self"] = [1.0 + 0.25 * (i % 3) for i in range(I["K"])]
        I["ref_self"] = reference(I, border, None, I["lam_self"])
    d0 = fill_desc(pkg, family, stencil, border, lam=I["lam_self"])
    dx = fill_desc(pkg, family, stencil, border, lam=I["lam"])
    exp = expect(pkg, family, stencil, d0)
    B, K, dims = I["B"], I["K"], I["dims"]
    kshape, plane = (B, K) + dims, (B,) + dims
    E, O, T, W, M = I["E"], I["O"], I["T"], I["W"], I["M"]
    st, sb = states(pkg, op, dev, d0, 2)
    ws0, ws1 = P(st), ctypes.c_void_p(st.data_ptr() + sb)
    s = op._stream()
    # the two calls
    affs, g0, gx = nan(kshape, dev), nan(kshape, dev), nan(kshape, dev)
    inv0, inv2, l0, lx = nan(plane, dev), nan((2,) + plane, dev), nan((1 + K,), dev), nan((1 + K,), dev)
    assert launched(L.pea_affinity_fwd_ex(ctypes.byref(d0), P(E), None, P(T), P(W), P(M), P(affs), P(g0), P(inv0), P(l0), ws0, sb, s)) == 0
    assert launched(L.pea_affinity_fwd_ex(ctypes.byref(dx), P(E), P(O), P(T), P(W), P(M), None, P(gx), P(inv2), P(lx), ws1, sb, s)) == 0
    sync()
    check_affs(affs, I["ref_self"]["affs"], what + " (self)")
    check_loss(l0, I["ref_self"], what + " (self)")
    check_loss(lx, I["ref"], what + " (cross)")
    # the one launch
    affs_d, g0_d, gx_d = nan(kshape, dev), nan(kshape, dev), nan(kshape, dev)
    inv0_d, invo_d, l0_d, lx_d = nan(plane, dev), nan(plane, dev), nan((1 + K,), dev), nan((1 + K,), dev)
    rc = launched(L.pea_affinity_fwd_dual_ex(ctypes.byref(d0), ctypes.byref(dx), P(E), P(O), P(T), P(W), P(M), P(affs_d), P(g0_d), P(gx_d),
                                             P(inv0_d), P(invo_d), P(l0_d), P(lx_d), ws0, ws1, sb, s))
    sync()
    if exp[5] == "1":
        assert rc == 0, "%s: rc %d" % (what, rc)
        for name, a, b in (("affs", affs_d, affs), ("g", g0_d, g0), ("g_cross", gx_d, gx), ("inv", inv0_d, inv0), ("inv_own_of_pair", inv0_d, inv2[0]),
                           ("inv_other", invo_d, inv2[1]), ("loss", l0_d, l0), ("loss_cross", lx_d, lx)):
            assert torch.equal(a, b), "%s: %s differs from the two calls" % (what, name)
    else:
        assert rc == E_UNSUPPORTED, "%s: rc %d" % (what, rc)
        assert bool(torch.isnan(affs_d).all()) and bool(torch.isnan(gx_d).all()), "%s: a declined call wrote an output" % what
    if border:
        check_cropped_exact(I, affs, g0, what + " (self)")
        check_cropped_exact(I, affs, gx, what + " (cross g)")
    # the backward: one launch where the self backward AND the role-A backward take the stencil (CIRCULAR only), else the two calls
    dl0, dlx = torch.full((1,), 0.6, device=dev), torch.full((1,), 1.7, device=dev)
    want = I["ref_self"]["de"] * (0.6 / DLOSS) + I["ref"]["de"] * (1.7 / DLOSS)
    de = nan(E.shape, dev)
    rc = launched(L.pea_affinity_bwd_dual_ex(ctypes.byref(d0), P(E), P(O), P(g0), P(gx), P(inv0), P(inv2[1]), P(dl0), P(dlx), P(de), s))
    sync()
    if border == 0 and exp[1] == "1" and exp[2] == "1":
        assert rc == 0, "%s: backward rc %d" % (what, rc)
        check_grad(de, want, E, True, what)
    else:
        assert rc == E_UNSUPPORTED, "%s: backward rc %d" % (what, rc)
        assert bool(torch.isnan(de).all()), "%s: a declined backward wrote de" % what
        de2 = nan(E.shape, dev)
        assert launched(L.pea_affinity_bwd_ex(ctypes.byref(d0), P(E), None, P(g0), P(inv0), P(dl0), P(de), None, s)) == 0
        assert launched(L.pea_affinity_bwd_ex(ctypes.byref(dx), P(E), P(O), P(gx), P(inv2), P(dlx), P(de2), None, s)) == 0
        sync()
        check_grad(de.double() + de2.double(), want, E, True, what + " (two calls)")


# ---- the labels-in two-launch form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stencil", list(EXPECT["f32_16"]))
def test_labels_two_launch(pkg, op, dev, synth, monkeypatch, stencil):
    """embedding_loss_from_labels with the scratch (k_fwd_xdma<.., LAB> + the cross backward where pea_labels_scratch_bytes > 0) against
    gen_targets + embedding_loss on the same stencil (the pattern and the bounds of test_labels_step_matches_targets_path), the targets
    against their restatement, and both paths against the float64 reference"""
    monkeypatch.setattr(pkg.affinity_op, "LABELS_TWO_LAUNCH_MIN_PX", 0)
    family, what = "f32_16", "labels %s" % stencil
    D, _, (Z, Y, X), B = FAMILIES[family]
    offsets = STENCILS[stencil]
    K = len(offsets)
    d = fill_desc(pkg, family, stencil, 0, lam=[1.0] * K)
    expect(pkg, family, stencil, d)
    sb = pkg._lib.lib().pea_labels_scratch_bytes(ctypes.byref(d))
    assert (sb > 0) == (stencil in LABELS_TWO_LAUNCH), "%s: pea_labels_scratch_bytes %d" % (what, sb)
    lab = torch.from_numpy(synth.synth_labels(B, (1, Y, X), 91, cell=11)[:, 0].astype(np.int32)).to(dev)
    I = inputs(synth, dev, family, stencil, 0)
    E = I["E"][:, :, 0]
    t, m, w = pkg.gen_targets(lab, offsets, padding=True)
    for i, o in enumerate(I["o3"]):  # target = [label(p) == label(p + o)], 1 outside (padding); mask = [p + o inside]
        nb, ok = shifted(lab[:, None, None].double(), o, BORDER_CROP_ZERO)
        ok = ok.expand(B, 1, Y, X)[:, 0]
        assert torch.equal(t[:, i], torch.where(ok, (lab.double() == nb[:, 0, 0]).float(), torch.ones_like(t[:, i]))), "%s: target %d" % (what, i)
        assert torch.equal(m[:, i].bool(), ok), "%s: mask %d" % (what, i)
    v5 = lambda a: a.view(B, K, 1, Y, X)  # noqa: E731
    ref = cosine_loss(I["E"], None, v5(t), v5(w), v5(m), I["o3"], [1.0] * K, 1e-12, 0, 0, dloss=0.5)
    crit = pkg.WeightedMSE()

    def run(labels_in):
        et = E.clone().requires_grad_(True)
        if labels_in:
            loss, affs, parts = pkg.embedding_loss_from_labels(et, lab, crit, offsets)
        else:
            loss, affs, parts = pkg.embedding_loss(et, t, w, m, crit, offsets)
        (loss * 0.5).backward()
        sync()
        return loss, affs, et.grad, torch.tensor(list(parts), dtype=torch.float64, device=dev)

    res = [run(False), run(True)]
    for (loss, affs, grad, parts), name in zip(res, ("targets path", "labels-in")):
        check_affs(affs, ref["affs"], "%s, %s" % (what, name))
        check_loss(torch.cat([loss.detach().view(1).double(), parts]), ref, "%s, %s" % (what, name))
        check_grad(grad.view(I["E"].shape), ref["de"], I["E"], True, "%s, %s" % (what, name))
    (l0, a0, g0, p0), (l1, a1, g1, p1) = res
    assert abs(l1.item() - l0.item()) <= 2e-6 * abs(l0.item())
    assert float((a1 - a0).abs().max()) < 2e-6
    reg = (I["E"][:, :, 0].double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(g0)
    assert relmax(torch.where(reg, g1, torch.zeros_like(g1)), torch.where(reg, g0, torch.zeros_like(g0))) < 1e-5
    assert bool(((p1 - p0).abs() <= 2e-6 * p0.abs()).all())


# ---- 3D: (2, 6, 48, 96), D = 16, CROP_ZERO ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,stencil", [("v3", "z_mixed"), ("v3", "z_neg_inplane_pos"), ("v3_march", "z_neg_inplane_pos"), ("v3", "z5"),
                                            ("v3_march", "z_mixed")])
def test_volume(pkg, op, dev, synth, monkeypatch, family, stencil):
    """z_mixed: a positive z step -- the z-march declines (mode 3 stays 0 even under PEA_ZMARCH=2), the tile-per-plane cross kernels
    take it.  z_neg_inplane_pos: the z steps the march takes with every in-plane offset positive; under PEA_ZMARCH=2 the march itself
    runs with right strips and down halos (modes 1 and 3), without the switch the cross kernels do.  z5: five z steps, refused in every
    mode, served by the next family."""
    if family in ENV:
        monkeypatch.setenv(*ENV[family])
    what = "%s %s" % (family, stencil)
    I = inputs(synth, dev, family, stencil, 1)
    d = fill_desc(pkg, family, stencil, 1, lam=I["lam"])
    exp = expect(pkg, family, stencil, d)
    affs, _ = loss_step(pkg, op, dev, I, d, exp, 1, what)
    infer(pkg, op, dev, I, d, affs, what)
