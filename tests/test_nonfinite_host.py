"""CPU: where a non-finite embedding pixel may show -- footprint(), the index arithmetic of include/pea.h's "Non-finite embeddings"
paragraph -- held against the float64 restatement (tests/f64_reference.py) and against the reference's own modules
(tests/golden/gnf_2d.npz); and the argument check of pea_fill_border_relu.  tests/test_gpu_nonfinite.py holds every kernel family to
footprint().

One pixel q of sample 0 carries a NaN or an inf in one channel, in `e` or in the second operand.  With nb_i(p) the neighbour of p
under the border mode (wrapped, clamped, or none):

    F        = the existing pairs (p, i) that contain q:  p == q (q as the first operand) or nb_i(p) == q (as the second);
               a self loss reads one tensor in both roles, so both count
    affs, g  NaN exactly on F
    de       NaN at q (its own projection reads e(q)) when q lies in `e`, at every p with a pair (p, i) in F (role A reads g_i(p)) and,
             for a self loss, at every nb_i(p) of a pair in F (role B)
    de_other NaN at q when q lies in the second operand, and at every nb_i(p) of a pair in F
    L_i      NaN iff F has a pair of offset i
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from f64_reference import BORDER_CIRCULAR, BORDER_CROP_ZERO, BORDER_REPLICATE, cosine_loss

NAN, INF = float("nan"), float("inf")


def _axis(n, o, border):
    """-> (neighbour coordinate of c = 0 .. n-1, the neighbour exists) along one axis"""
    c = np.arange(n) + int(o)
    if border == BORDER_CIRCULAR:
        return c % n, np.ones(n, bool)
    inside = (c >= 0) & (c < n)
    return np.clip(c, 0, n - 1), (inside if border == BORDER_CROP_ZERO else np.ones(n, bool))


def footprint(q, operand, border, dims, offsets, other_mode):
    """q = (z, y, x) of sample 0; operand "e" or "other" (the tensor q lies in; "other" needs a second operand); other_mode None
    (self loss), "detached" or "both".  -> dict of bool tensors for SAMPLE 0 (the other samples are untouched): affs, g [K,Z,Y,X],
    de, de_other [Z,Y,X] (None where the call has no such output), loss [K]"""
    assert operand in ("e", "other") and other_mode in (None, "detached", "both") and (operand == "e" or other_mode)
    Z, Y, X = dims
    K = len(offsets)
    pairs = np.zeros((K, Z, Y, X), bool)
    de, de_o = np.zeros((Z, Y, X), bool), np.zeros((Z, Y, X), bool)
    first = operand == "e"                          # q is read as the first operand of a pair
    second = operand == "other" or other_mode is None  # ... as the second
    for i, o in enumerate(offsets):
        ax = [_axis(n, v, border) for n, v in zip(dims, o)]
        role_b = np.zeros((Z, Y, X), bool)  # the second-operand pixels nb_i(p) of the pairs of this offset in F
        if first and all(ok[c] for (_, ok), c in zip(ax, q)):  # the pair (q, i)
            pairs[(i,) + tuple(q)] = True
            role_b[tuple(idx[c] for (idx, _), c in zip(ax, q))] = True
        if second:  # the pairs (p, i) with nb_i(p) == q: per axis, the coordinates that the border mode maps onto q's
            pre = [ok & (idx == c) for (idx, ok), c in zip(ax, q)]
            hit = pre[0][:, None, None] & pre[1][None, :, None] & pre[2][None, None, :]
            pairs[i] |= hit
            if hit.any():
                role_b[tuple(q)] = True
        de |= pairs[i]
        if other_mode is None:
            de |= role_b
        else:
            de_o |= role_b
    if operand == "e":
        de[tuple(q)] = True
    else:
        de_o[tuple(q)] = True
    t = torch.from_numpy
    return dict(affs=t(pairs), g=t(pairs), de=t(de), de_other=t(de_o) if other_mode == "both" else None,
                loss=t(pairs.reshape(K, -1).any(1)))


# ---- against the float64 restatement ------------------------------------------------------------------------------------------------
OFFS_2D = [[0, -1, 0], [0, 0, -1], [0, -3, 3], [0, 2, 0], [0, 0, -9], [0, 5, 9], [0, 0, 0]]
OFFS_3D = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 2, -2], [-2, 0, 0], [2, -5, 9], [0, 0, 11], [3, 0, 0], [1, 1, 1]]
# (0, 0, -9) / (0, 0, 11) / (3, 0, 0): a reach of at least the extent minus one, and beyond it -- CROP_ZERO has no pair there,
# REPLICATE folds every pixel onto the border; CIRCULAR wraps (torch.roll takes any shift; the library itself wants |o| < extent)


def _inputs(dims, K, seed, second):
    g = torch.Generator().manual_seed(seed)
    B, D = 2, 3
    E = torch.randn((B, D) + dims, generator=g, dtype=torch.float64)
    O = torch.randn((B, D) + dims, generator=g, dtype=torch.float64) if second else None
    T = torch.randint(0, 2, (B, K) + dims, generator=g).double()
    W = torch.rand((B, K) + dims, generator=g, dtype=torch.float64) + 0.5
    M = torch.randint(0, 2, (B, K) + dims, generator=g).double()  # zeros among them: 0 * NaN must stay NaN
    return E, O, T, W, M


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["interior", "corner"])
@pytest.mark.parametrize("other_mode,operand", [(None, "e"), ("detached", "e"), ("detached", "other"), ("both", "e"), ("both", "other")])
@pytest.mark.parametrize("border", [BORDER_CIRCULAR, BORDER_CROP_ZERO, BORDER_REPLICATE], ids=["circular", "crop", "replicate"])
@pytest.mark.parametrize("dims", [(1, 6, 10), (3, 6, 10)], ids=["2d", "3d"])
def test_footprint_is_where_the_float64_restatement_is_nan(dims, border, other_mode, operand, where, value):
    offsets = OFFS_2D if dims[0] == 1 else OFFS_3D
    K = len(offsets)
    E, O, T, W, M = _inputs(dims, K, 5 + dims[0], other_mode is not None)
    q = (0, 0, 0) if where == "corner" else (dims[0] // 2, 3, 7)
    clean = cosine_loss(E, O, T, W, M, offsets, [1.0] * K, 1e-12, border, 2, other_grad=other_mode == "both")
    P = (O if operand == "other" else E).clone()
    P[(0, 1) + q] = value
    args = (E, P) if operand == "other" else (P, O)
    out = cosine_loss(*args, T, W, M, offsets, [1.0] * K, 1e-12, border, 2, other_grad=other_mode == "both")
    F = footprint(q, operand, border, dims, offsets, other_mode)
    assert F["affs"].any() and not bool(F["affs"].all())

    def only(t, mask, ref, what):
        full = torch.zeros(t.shape, dtype=torch.bool)
        full[0] = mask if mask.dim() == t.dim() - 1 else mask.unsqueeze(0).expand(t.shape[1:])
        assert torch.equal(torch.isnan(t), full), what
        assert torch.equal(t[~full], ref[~full]), what + ": a value outside the footprint changed"
        assert not bool(torch.isinf(t).any()), what

    only(out["affs"], F["affs"], clean["affs"], "affs")
    only(out["de"], F["de"], clean["de"], "de")
    if other_mode == "both":
        only(out["de_other"], F["de_other"], clean["de_other"], "de_other")
    assert torch.equal(torch.isnan(out["parts"]), F["loss"]) and bool(torch.isnan(out["loss"]))
    assert torch.equal(out["parts"][~F["loss"]], clean["parts"][~F["loss"]])
    if border == BORDER_CROP_ZERO:  # the cropped positions: exactly 0, also where the clamped index reads q
        for i, o in enumerate(offsets):
            ax = [_axis(n, v, border)[1] for n, v in zip(dims, o)]
            gone = ~torch.from_numpy(ax[0][:, None, None] & ax[1][None, :, None] & ax[2][None, None, :])
            assert not bool(out["affs"][:, i][:, gone].any())


def test_footprint_by_hand():
    """one row of five pixels, offset -1 along x, q = 0 (the left end)"""
    dims, offs, q = (1, 1, 5), [[0, 0, -1]], (0, 0, 0)
    row = lambda F, k: F[k].flatten().tolist()  # noqa: E731
    F = footprint(q, "e", BORDER_CIRCULAR, dims, offs, None)  # pairs (0, 4) and (1, 0)
    assert row(F, "affs") == [True, True, False, False, False] and row(F, "de") == [True, True, False, False, True]
    F = footprint(q, "e", BORDER_CROP_ZERO, dims, offs, None)  # the pair of pixel 0 does not exist
    assert row(F, "affs") == [False, True, False, False, False] and row(F, "de") == [True, True, False, False, False]
    F = footprint(q, "e", BORDER_REPLICATE, dims, offs, None)  # (0, 0) and (1, 0)
    assert row(F, "affs") == [True, True, False, False, False] and row(F, "de") == [True, True, False, False, False]
    F = footprint(q, "other", BORDER_REPLICATE, dims, [[0, 0, -7]], "both")  # every pixel is folded onto 0
    assert row(F, "affs") == [True] * 5 and row(F, "de") == [True] * 5 and row(F, "de_other") == [True, False, False, False, False]
    F = footprint(q, "e", BORDER_CROP_ZERO, dims, [[0, 0, -7]], "both")  # no pair at all: only q's own projection
    assert not F["affs"].any() and row(F, "de") == [True, False, False, False, False] and not F["de_other"].any() and not F["loss"].any()


# ---- against the reference's own modules -----------------------------------------------------------------------------------------------
RUNS = [(m, v) for m in ("loss_embedding_mse", "loss_embedding", "loss_embedding_exp") for v in ("nan", "inf")]


@pytest.mark.parametrize("module,value", RUNS)
def test_footprint_is_where_the_reference_modules_are_nan(module, value):
    """tests/golden/gnf_2d.npz (tests/golden/make_golden_actloss.py): embedding_loss of the reference's raw-cosine module and of its two
    clamp modules on an embedding with one NaN / one +inf channel value.  Their map is NaN exactly on the footprint -- torch.clamp keeps
    NaN -- and their loss is NaN; the raw module's gradient is NaN exactly on the de footprint, the clamp modules' at least at q"""
    g = load_golden("gnf_2d")
    q = tuple(int(v) for v in g["q_" + value])
    offsets = [[0] + [int(v) for v in o] for o in g["offsets"]]
    dims = (1,) + tuple(g["e"].shape[2:])
    F = footprint(q, "e", BORDER_CIRCULAR, dims, offsets, None)
    affs, grad = torch.from_numpy(g["affs_%s_%s" % (module, value)]), torch.from_numpy(g["grad_%s_%s" % (module, value)])
    clean = torch.from_numpy(g["affs_%s_clean" % module])
    want = torch.zeros(affs.shape, dtype=torch.bool)
    want[0] = F["affs"][:, 0]
    assert torch.equal(torch.isnan(affs), want)
    assert torch.equal(affs[~want], clean[~want])
    assert np.isnan(float(g["loss_%s_%s" % (module, value)])) and np.isfinite(float(g["loss_%s_clean" % module]))
    gn = torch.isnan(grad).all(1) if module == "loss_embedding_mse" else None
    assert bool(torch.isnan(grad[(0, slice(None)) + q[1:]]).all())
    if gn is not None:
        wd = torch.zeros(gn.shape, dtype=torch.bool)
        wd[0] = F["de"][0]
        assert torch.equal(gn, wd) and torch.equal(torch.isnan(grad).any(1), wd)


# ---- pea_fill_border_relu: the source slices must exist ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


@pytest.mark.parametrize("K,Z,Y,X,shift", [(1, 3, 8, 8, 2), (1, 1, 8, 8, 1), (2, 4, 3, 8, 2), (2, 8, 1, 8, 1), (3, 4, 4, 3, 2), (12, 8, 8, 5, 3),
                                          (3, 3, 8, 8, 2), (3, 8, 3, 8, 2)])
def test_fill_border_relu_refuses_missing_source_slices(lib, K, Z, Y, X, shift):
    """PEA_E_DESC before anything is launched (the pointer is never read: no GPU here) when slices [shift, 2 * shift) of an axis that a
    channel fills do not exist -- K = 1 and K = 2 used to go unchecked and read the next channel or past the tensor"""
    p = ctypes.c_void_p(0x1000)
    for relu in (0, 1):
        assert lib.pea_fill_border_relu(p, 1, K, Z, Y, X, shift, relu, None) == -2
