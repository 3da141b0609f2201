"""The axis-aligned stencils of tests/test_cross_stencils_host.py and tests/test_gpu_cross_stencils.py, the shapes they run at and what
pea_cross_supported answers for each; a helper module (no tests here).

plan_xdma (csrc/pea_xdma.h) takes any stencil whose offsets have exactly one non-zero component: either sign, any order, repeats, one
axis or two.  The tables of the reference (multi_offset(shifts, 4), axis_offsets_3d) are negative, alternate y and x, ascend and never
repeat; the ones below are everything else.  Offsets are (dy, dx) in 2D and (dz, dy, dx) in 3D; the neighbour of p is p + o.

EXPECT[family][stencil] is a string of six characters: pea_cross_supported(desc, mode) for mode 0 .. 5.  It was derived by hand from
plan_xdma, fwd_self, bwd_self, bwd_hq and xdma_cross_supported (csrc/pea_k_xdma*.hip) with these plane sizes (256-byte units): a 16 x 32
tile with halo rows hy0 above / hy1 below and strip rows of SW pixels takes (hy0 + hy1 + 16) * 128 + SW * 64 bytes per plane, SW = 64
only where a stencil reaches BOTH ways along x by more than 16; the forward's halos are one-sided (rows up, rows down as the offsets
say), the self backward's are two-sided (both roles).

    forward, f32                   51 units (13056 bytes); at most 10 in-plane offsets (+ 4 along z in 3D, 52 / 32 units there)
    forward, 16-bit; the pair;     30 units (7680 bytes): every one-sided stencil fits, and every two-sided one but +-27 rows with
    the labels-in forward; the     64-pixel strips (two_sw64: 13056 bytes)
    second operand at D = 32 / 64
    self backward, f32 / 16-bit    51 / 52 units; two slots per offset: at most 5 offsets per axis at D = 16 / 32, 4 at D = 64 and
                                   in 3D (the instantiation walks 8 slots), 4 along z
    role-A backward                one slot per offset; refuses a stencil with no offset on one of the two in-plane axes (its spare
                                   slots repeat slot 0 of the axis, and there is none)
    reach                          32 (= TW) is taken, 33 is refused by every plan
"""
import ctypes

import numpy as np
import torch

from f64_reference import BORDER_CROP_ZERO, cosine_loss, shifted

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL, GRAD_RTOL_16 = 1e-5, 1e-5, 1e-4, 8e-3  # tests/test_gpu_parity.py, tests/test_gpu_alignment.py
E_UNSUPPORTED = -3
FLAG_ACCUMULATE = 16
DLOSS = 0.625
DTYPES = {"f32": (torch.float32, 0), "f16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}


def _yx(pairs):
    return [[int(a), int(b)] for a, b in pairs]


SHIPPED = _yx([(-s, 0) if k == 0 else (0, -s) for s in (1, 3, 5, 9, 27) for k in (0, 1)])  # multi_offset([1, 3, 5, 9, 27], 4)

STENCILS = {
    # right strip only (split = 32), down halo only: the mirror of the shipped stencil
    "pos": _yx([(s, 0) if k == 0 else (0, s) for s in (1, 3, 5, 9, 27) for k in (0, 1)]),
    # the same with four offsets per axis: what the D = 64 backward holds
    "pos4": _yx([(s, 0) if k == 0 else (0, s) for s in (1, 3, 9, 27) for k in (0, 1)]),
    # down halo with the left strip
    "asym": _yx([(1, 0), (0, -1), (3, 0), (0, -3), (9, 0), (0, -27)]),
    # both strips, SW = 32, split = 16, reach exactly 16
    "two_sw32": _yx([(0, -1), (1, 0), (0, 3), (-5, 0), (0, -9), (9, 0), (0, 16)]),
    # two_sw32 without the 16: reach <= 9 both ways (the producer / consumer f16 backward's planes)
    "small": _yx([(0, -1), (1, 0), (0, 3), (-5, 0), (0, -9), (9, 0)]),
    # both strips, SW = 64, reach 17 and 27; the forward needs the 51-unit plane and fills it
    "two_sw64": _yx([(0, -27), (-27, 0), (0, 17), (27, 0), (0, 1)]),
    "reach32": _yx([(0, 32), (-1, 0), (0, -32)]),      # reach == TW
    "reach33": _yx([(0, 33), (-1, 0)]),                 # one more: refused by every plan
    "x_only": _yx([(0, -s) for s in (1, 3, 5, 9, 27)]),   # all ten x slots, no y slot
    "y_only": _yx([(s, 0) for s in (1, 3, 5, 9, 27)]),
    # six offsets on x: the forward takes eight offsets, the self backward has five slot pairs per axis
    "six_on_x": _yx([(0, -1), (-1, 0), (0, -2), (-3, 0), (0, -3), (0, -5), (0, -9), (0, -11)]),
    # a repeated offset (channels 0 and 2) with its own target / weight / lambda; +3 and -3 share a slot pair in the backward
    "dup": _yx([(0, -3), (-3, 0), (0, -3), (-9, 0), (0, 3)]),
    # the shipped ten reversed, x before y: slot 0 is the longest reach (the spare slots repeat it)
    "unsorted": [list(o) for o in reversed(SHIPPED)],
    # the tallest halo the 51-unit planes hold (35 rows both ways: (70 + 16) * 128 + 32 * 64 = 13056 bytes); the shipped tables stop at 27
    "tall": _yx([(35, 0), (0, 1), (-35, 0)]),
    "tall36": _yx([(36, 0), (0, 1), (-36, 0)]),        # one row more: 13312 bytes, refused
    # 3D: z either way (the z-march declines a positive z step)
    "z_mixed": [[1, 0, 0], [0, 1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, 9], [3, 0, 0], [-4, 0, 0]],
    # 3D: the z steps the march takes, in-plane offsets all positive (right strips, down halos inside the march)
    "z_neg_inplane_pos": [[-1, 0, 0], [0, 1, 0], [0, 0, 1], [-2, 0, 0], [0, 3, 0], [0, 0, 3], [-3, 0, 0], [0, 9, 0], [0, 0, 9], [-4, 0, 0],
                          [0, 27, 0], [0, 0, 27]],
    "z5": [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [-3, 0, 0], [-4, 0, 0], [-5, 0, 0]],   # five z steps: one too many
}

PLANE = ["pos", "asym", "two_sw32", "two_sw64", "reach32", "reach33", "x_only", "y_only", "six_on_x", "dup", "unsorted"]  # the issue's table

# family -> (D, storage, (Z, Y, X), B); 2D families run both borders (CIRCULAR / NORM_BX and CROP_ZERO / NORM_CROPPED)
FAMILIES = {
    "f32_16": (16, "f32", (1, 50, 100), 2),
    "f32_16_x96": (16, "f32", (1, 50, 96), 2),     # the narrowest image 64-pixel strips accept (X >= TW + SW)
    "f32_16_min": (16, "f32", (1, 43, 96), 2),     # the smallest image the +-27 self backward accepts (Y >= TH + 27, X >= TW + 64)
    "f32_16_min64": (16, "f32", (1, 43, 64), 2),   # the smallest the one-sided forward accepts (X >= TW + 32): the backward is refused
    "f32_16_tall": (16, "f32", (1, 52, 100), 2),   # Y >= TH + 35
    "f32_32": (32, "f32", (1, 50, 100), 2),
    "f32_64": (64, "f32", (1, 50, 100), 2),
    "f16_32": (32, "f16", (1, 50, 104), 2),        # 16-bit storage: X % 8 == 0
    "bf16_64": (64, "bf16", (1, 50, 104), 2),
    "v3": (16, "f32", (6, 48, 96), 2),             # CROP_ZERO only
    "v3_march": (16, "f32", (6, 48, 96), 2),       # the same under PEA_ZMARCH=2
}
ENV = {"v3_march": ("PEA_ZMARCH", "2")}

_ALL16 = "111001"   # D = 16, f32: forward, self backward, second operand; no raw map is read; the pair fuses
_ALLW = "111110"    # D = 32 / 64 and 16-bit storage: the backwards read the raw map (modes 3, 4); no pair
EXPECT = {
    "f32_16": {"pos": _ALL16, "asym": _ALL16, "two_sw32": _ALL16, "small": _ALL16, "reach32": _ALL16, "dup": _ALL16, "unsorted": _ALL16,
               "two_sw64": "111000",                # the pair's forward has 30-unit planes only
               "reach33": "000000",
               "x_only": "110001", "y_only": "110001",   # role A refuses; the pair's FORWARD fuses (its backward then declines)
               "six_on_x": "101001"},
    "f32_16_x96": {"two_sw64": "111000"},
    "f32_16_min": {"pos": _ALL16, "unsorted": _ALL16, "two_sw64": "111000"},
    "f32_16_min64": {"pos": "101001"},              # role B makes +27 two-sided: 64-pixel strips, X >= 96
    "f32_16_tall": {"tall": "111000", "tall36": "000000"},   # (the pair's 30-unit planes stop at 27 rows)
    "f32_32": {"pos": _ALLW, "asym": _ALLW, "two_sw32": _ALLW, "reach32": _ALLW, "dup": _ALLW, "unsorted": _ALLW,
               "two_sw64": "110100",                # the second operand's forward at D > 16 has 30-unit planes only
               "reach33": "000000", "x_only": "110100", "y_only": "110100", "six_on_x": "101010"},
    "f32_64": {"pos4": _ALLW, "asym": _ALLW, "two_sw32": _ALLW, "reach32": _ALLW, "dup": _ALLW,
               "pos": "101010", "unsorted": "101010",    # five offsets per axis: ten slots, the D = 64 backward walks eight
               "two_sw64": "110100", "reach33": "000000", "x_only": "100000", "y_only": "100000", "six_on_x": "101010"},
    "f16_32": {"pos": _ALLW, "asym": _ALLW, "two_sw32": _ALLW, "small": _ALLW, "reach32": _ALLW, "dup": _ALLW, "unsorted": _ALLW,
               "two_sw64": "010100",                # 16-bit forwards: 30-unit planes; the backward's 52 units hold it
               "reach33": "000000", "x_only": "110100", "y_only": "110100", "six_on_x": "101010"},
    "bf16_64": {"pos4": _ALLW, "asym": _ALLW, "two_sw32": _ALLW, "small": _ALLW, "reach32": _ALLW, "dup": _ALLW,
                "pos": "101010", "unsorted": "101010", "two_sw64": "010100", "reach33": "000000", "x_only": "100000", "y_only": "100000",
                "six_on_x": "101010"},
    # 3D, D = 16: the tile-per-plane cross kernels; mode 3 only where the z-march backward runs
    "v3": {"z_mixed": "111000", "z_neg_inplane_pos": "111000", "z5": "000000"},
    "v3_march": {"z_mixed": "111000", "z_neg_inplane_pos": "111100", "z5": "000000"},
}
# the 2D, f32, D = 16 stencils whose labels-in step runs as two launches on the cross kernels (pea_labels_scratch_bytes > 0: the
# 30-unit labels-in forward AND the self backward take them)
LABELS_TWO_LAUNCH = {"pos", "asym", "two_sw32", "small", "reach32", "x_only", "y_only", "dup", "unsorted"}


def offsets3(name):
    return [[0] * (3 - len(o)) + list(o) for o in STENCILS[name]]


def lambdas(K):
    return [1.0 + 0.125 * ((3 * i + 1) % 7) for i in range(K)]   # any seven neighbouring channels differ (dup: 1.125 and 1.0)


def fill_desc(pkg, family, stencil, border, flags=0, lam=None):
    """the PeaDesc of (family, stencil) with the border and its normaliser (CIRCULAR / NORM_BX or CROP_ZERO / NORM_CROPPED)"""
    D, dt, dims, B = FAMILIES[family]
    o3 = offsets3(stencil)
    lam = lam or lambdas(len(o3))
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2 if dims[0] == 1 else 3, B, D, len(o3)
    d.dims[:] = list(dims)
    d.border, d.dtype, d.norm, d.eps, d.flags = border, DTYPES[dt][1], (1 if border else 0), 1e-12, flags
    for i, o in enumerate(o3):
        d.offsets[i][:] = o
        d.lam[i] = lam[i]
    assert pkg._lib.lib().pea_desc_validate(ctypes.byref(d)) == 0
    return d


def supported(pkg, d):
    """pea_cross_supported(d, 0 .. 5) as the six-character string of EXPECT"""
    L = pkg._lib.lib()
    return "".join(str(int(L.pea_cross_supported(ctypes.byref(d), mode))) for mode in range(6))


# ---- inputs and the float64 reference (GPU file) -------------------------------------------------------------------------------------
def make_inputs(synth, dev, family, stencil, seed, other=False):
    """device tensors [B, *, Z, Y, X]: the embedding with zero-norm pixels at (0, 0) and (Y-1, X-1) of the first / last plane (the eps
    branch, read through both strips), per-channel targets, weights and u8 masks (hash-seeded as tests/test_gpu_cross.py::_inputs)"""
    D, dt, (Z, Y, X), B = FAMILIES[family]
    K, S = len(STENCILS[stencil]), Z * Y * X
    e = synth.synth_embedding((B, D, S), 100 + seed).reshape(B, D, Z, Y, X)
    e[:, :, 0, 0, 0] = 0.0
    e[:, :, Z - 1, Y - 1, X - 1] = 0.0
    e[-1, 0, Z - 1, Y - 1, X - 1] = 1e-14    # a norm below eps that is not zero (its 1 / norm is stored negated, too)
    idx = np.arange(B * K * S, dtype=np.uint64)
    t = (synth.hash_uniform(idx, 200 + seed) < 0.6).astype(np.float32).reshape(B, K, Z, Y, X)
    w = (0.5 + synth.hash_uniform(idx, 300 + seed)).astype(np.float32).reshape(B, K, Z, Y, X)
    m = (synth.hash_uniform(idx, 400 + seed) < 0.9).astype(np.uint8).reshape(B, K, Z, Y, X)
    tdt = DTYPES[dt][0]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    I = dict(E=cu(e).to(tdt), T=cu(t), W=cu(w), M=cu(m), O=None, K=K, o3=offsets3(stencil), lam=lambdas(K), B=B, dims=(Z, Y, X), D=D,
             tdt=tdt, f32=dt == "f32")
    if other:
        eo = synth.synth_embedding((B, D, S), 500 + seed).reshape(B, D, Z, Y, X)
        eo[0, :, 0, 0, 0] = 0.0
        eo[0, :, Z - 1, Y - 1, X - 1] = 0.0
        I["O"] = cu(eo).to(tdt)
    return I


def reference(I, border, other=None, lam=None, dloss=DLOSS):
    """tests/f64_reference.py::cosine_loss in float64 on the device, from the embedding as stored (16-bit: already rounded)"""
    return cosine_loss(I["E"], other, I["T"], I["W"], I["M"], I["o3"], lam or I["lam"], 1e-12, border, 1 if border else 0, dloss=dloss)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def relmax(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_affs(affs, ref_affs, what):
    err = float((affs.double() - ref_affs.view(affs.shape)).abs().max())
    print("%s: affs max err %.3g" % (what, err))
    assert err < AFFS_ATOL, "%s: affs max err %.3g" % (what, err)


def check_loss(lv, ref, what):
    lv = lv.double()
    assert bool(torch.isfinite(lv).all()), what
    print("%s: loss %.9g ref %.9g" % (what, float(lv[0]), float(ref["loss"])))
    assert abs(float(lv[0]) - float(ref["loss"])) <= LOSS_RTOL * abs(float(ref["loss"])), "%s: loss %.9g ref %.9g" % (
        what, float(lv[0]), float(ref["loss"]))
    parts = ref["parts"]
    bad = (lv[1:] - parts).abs() > LOSS_RTOL * parts.abs() + 1e-30
    assert not bool(bad.any()), "%s: per-offset losses %s ref %s" % (what, lv[1:].tolist(), parts.tolist())


def check_grad(de, ref_de, E, f32, what):
    """the gradient against the reference, relative to its max; then once more over the REGULAR pixels alone: a pixel on the clamp branch
    carries G / eps, 1e12 times a regular gradient, and would hide every other pixel behind it.  16-bit storage: the regular pixels only
    (G / eps overflows an f16, and is rounded to 8 bits in a bf16 whose max it then sets)"""
    tol = GRAD_RTOL if f32 else GRAD_RTOL_16
    ref_de = ref_de.view(de.shape)
    if f32:
        assert bool(torch.isfinite(de).all()), what
        r = relmax(de, ref_de)
        print("%s: gradient rel err %.3g" % (what, r))
        assert r < tol, "%s: gradient rel err %.3g" % (what, r)
    reg = (E.double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(ref_de)
    zero = torch.zeros_like(ref_de)
    got = torch.where(reg, de.double(), zero)
    assert bool(torch.isfinite(got).all()), what
    r = relmax(got, torch.where(reg, ref_de, zero))
    print("%s: regular gradient rel err %.3g" % (what, r))
    assert r < tol, "%s: regular gradient rel err %.3g" % (what, r)


def check_cropped_exact(I, affs, g, what):
    """CROP_ZERO: affs and g are EXACTLY 0 where p + o leaves the image (c16_crop of tests/test_gpu_alignment.py)"""
    for i, o in enumerate(I["o3"]):
        _, ok = shifted(I["E"][:, :1], o, BORDER_CROP_ZERO)
        gone = (~ok).expand(I["B"], *I["dims"])
        assert bool(gone.any()), "%s: offset %d crops nothing" % (what, i)
        assert not bool(affs[:, i][gone].any()), "%s: affs of a cropped neighbour, offset %d" % (what, i)
        if g is not None:
            assert not bool(g[:, i][gone].any()), "%s: g of a cropped neighbour, offset %d" % (what, i)
