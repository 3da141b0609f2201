"""GPU (-m gpu): element-aligned pointers and ragged batch strides in every kernel family, through the C ABI.

include/pea.h promises that any pointer aligned to its element size and any non-negative batch stride of target / weight / mask is
served with the same results; 16-byte alignment and strides that are multiples of four elements only select the faster kernels.  The
predicates that make a fast kernel step aside (misaligned(p, 16), (tbs | wbs | mbs) & 3, (B * S) % 4) are driven here to "no" ONE
POINTER AT A TIME: with every pointer skewed at once the first check that says no would hide every missing one.

Every tensor of a call lives in a guard-banded arena (tests/arena.py): after the calls the guards and stride gaps still hold the
pattern, the inputs are bit-unchanged and every owned output element was written.  The numbers are held to a float64 restatement
of the loss (tests/f64_reference.py, computed once per case; for 16-bit storage from the embedding already rounded to the storage
type) with the suite's standing tolerances -- nothing new is measured:

    affs 1e-5 absolute, loss and every L_i 1e-5 relative, gradient 1e-4 of its max      (tests/test_gpu_parity.py)
    gradient 8e-3 of its max for 16-bit storage (the stored gradient is rounded once)   (tests/test_gpu_bf16.py, test_gpu_mask_f32.py)
    the 1 / norm plane 1e-6 relative                                                     (test_inv_norm_plane_and_ex_entry_points)

PEA_FLAG_LOSS_ACT is never set: no clamp edge, no term dropped.  The state block is read back after every call: zero except for the
magic word (pea_workspace_init's "zero between calls").

Cases (B = 2, 48 x 96, multi_offset([1,3,5,9,27], 4), CIRCULAR, NORM_BX unless said otherwise); the aligned control of each asserts
pea_cross_supported(desc, mode) == 1 in the modes listed, which is what makes the skewed variants real refusals:

    c16            D=16 f32 self                                                modes 0, 1
    c16_crop       the same, CROP_ZERO / NORM_CROPPED; cropped affs and g exactly 0    0, 1
    c16_fmask      c16 with a fractional f32 mask                                0, 1
    c32            D=32 f32 self, the backward with the raw map                  0, 1, 3
    c64            D=64 f32, offsets[:8], the backward with the raw map          0, 1, 3
    h32_f16        D=32 f16                                                      0, 1
    h64_bf16       D=64 bf16, offsets[:8]                                        0, 1
    ema16          D=16, detached second operand (role-A backward)               2
    ema16_acc      the same backward with PEA_FLAG_ACCUMULATE_DE                 2
    ema32          D=32, detached second operand, the backward with the raw map  4
    ema16_both     D=16, second operand with de and de_other (tiled roles 1, 2)
    pair16         pea_affinity_fwd_dual_ex + pea_affinity_bwd_dual_ex           5
    diag16(_fmask) D=16, multi_offset([1,3,9], 8): k_fwd_tiled_v / tiled backward
    diag64         D=64, the diagonal stencil: chunked forward
    zm5            3D (2, 6, 48, 96) D=16 norm5 CROP_ZERO, PEA_ZMARCH=2          1, 3
    zm5_cross      the same without the switch (tile-per-plane cross kernels)    0, 1
    n26            3D (1, 7, 40, 72), 26-neighbourhood, CROP_ZERO                0, 1
    rep6           3D (1, 4, 40, 72) REPLICATE, a norm6-like table, NORM_FULL
    infer16, infer32_f16   pea_affinity_infer with PEA_FLAG_RELU_AFFS
    lab16          pea_label_weights, then pea_affinity_fwd_bwd_labels_ex with scratch (pea_labels_scratch_bytes > 0) and without
    multi4         the four ragged entries of tests/test_gpu_multi.py through pea_affinity_fwd_multi / _bwd_multi

The launchers' predicates against the widest access their kernels make to each pointer (read from the source before the first run of
this file; "elem" = a load / store of one element, which the entry point's PEA_E_ALIGN check already guarantees):

    launcher (file)                          pointer: widest access -> check
    fwd_self, xdma_fwd_other (k_xdma)        e / e_other staged: 16 B LDS-DMA -> 16;  own e at D=16: dword -> 4;  own e at D>16: DMA -> 16
                                             target, weight: dwordx4 -> 16;  affs, g_out: quad stores -> 16;  u8 mask: one dword per
                                             quad -> 4;  f32 mask: dwordx4 -> 16;  inv_norm_out: dword stores -> 4;  strides & 3
    xdma_fwd_dual (k_xdma)                   as fwd_self for e, ema, target, weight, mask, affs, g_out, g_cross_out;  both planes dword -> 4
    fwd_labels (k_xdma)                      e: DMA -> 16;  labels: DMA -> 16;  affs, g (scratch): quads -> 16;  wtab: dword -> elem
    bwd_self, xdma_bwd_other, xdma_bwd_dual  x / e_other / ema and the 1 / norm planes: DMA -> 16 (second plane: (B*S) % 4);
                                             g, g_cross, own e, own 1 / norm, dloss: dword loads -> elem;  de: dword stores -> elem
    xdma_pf_bwd_self / _other (k_xdma_pf)    x, e_other, own e (own tiles), planes: DMA -> 16;  g, affs: dword -> 4;  de: dword -> 4
    xdma_h_* (k_xdma_h, k_xdma_hq)           e, e_other: DMA / dwordx4 -> 16;  planes: DMA -> 16;  target, weight, affs, g_out as
                                             fwd_self;  g, affs (backward): dword -> 4;  de: 16-bit stores -> 2
    zmarch_fwd / _bwd (k_zmarch)             e, planes: DMA -> 16;  target, weight, affs, g_out: quads -> 16;  g, affs (backward):
                                             4-byte DMA -> 4;  de: dword -> 4
    box_fwd / box_bwd (k_box, boxm)          e, planes: DMA -> 16;  target, weight, affs, g_out: quads -> 16;  g: dword -> 4;  de: dword -> 4
    try_fwd_v (k_tiled)                      e: elem loads -> none needed;  target, weight: dwordx4 -> 16;  affs, g_out: quads -> 16;
                                             u8 mask -> 4, f32 mask -> 16;  strides and S & 3
    try_fwd_tiled, try_fwd_chunked,          every access is one element (bl_emb / bl32 / bl8, bs_emb / bs32): no check needed, none made
    try_bwd_tiled, direct, multi
    label_weights (k_labels)                 labels: int4 quads -> 16 and X % 4, else the per-element count kernel;  wtab: elem
    labels_step (k_labels)                   every access is one element: no check needed, none made
    pea_affinity_fwd_ex / _fwd_dual_ex       f32 mask: dword / dwordx4 loads -> 4 WAS MISSING (PEA_E_ALIGN now; tests/test_align_host.py)

Every predicate but the last was found sufficient; the GPU run confirms the table (nothing faulted, nothing was declined that the table
does not list, no guard byte changed).  The one-launch pair declines a skew of e, ema, target, weight, mask, affs, g_out or
g_cross_out and ragged strides (forward), of e, ema or either plane (backward); PEA_FLAG_ACCUMULATE_DE declines a skew of e_other or of
the planes.  Every other family hands a skewed call to the next one and returns 0.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from arena import PATTERN, PATTERN16, Arena
from f64_reference import BORDER_CROP_ZERO, cosine_loss, inv_norm_plane, shifted

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL, GRAD_RTOL_16, INV_RTOL = 1e-5, 1e-5, 1e-4, 8e-3, 1e-6
MAGIC = 0x50454133
E_UNSUPPORTED = -3
FLAG_RELU, FLAG_ACCUMULATE, FLAG_MASK_F32 = 1, 16, 32
TGT_PADDING, TGT_MASK_INSIDE = 1, 4
DLOSS = 0.625
DTYPES = {"f32": (torch.float32, 0), "f16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}


def mo(shifts, nb):
    out = []
    for s in shifts:
        out += [[-s, 0], [0, -s]] + ([[-s, -s], [-s, s]] if nb == 8 else [])
    return out


def _norm5():
    out = []
    for i, s in enumerate([1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27]):
        o = [0, 0, 0]
        o[i % 3] = -s
        out.append(o)
    return out


OFFS = {
    "cross": mo([1, 3, 5, 9, 27], 4), "cross8": mo([1, 3, 5, 9, 27], 4)[:8], "diag": mo([1, 3, 9], 8), "norm5": _norm5(),
    "n26": [[dz, dy, dx] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)],
    # norm6-like (embedding_loss_norm6 takes any table): axis steps, a diagonal in the plane, one across planes, a long y step
    "rep6": [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [0, -3, 3], [1, 2, -2], [0, 9, 0]],
}


def case(D=16, B=2, dims=(1, 48, 96), offs="cross", border=0, norm=0, dtype="f32", mask="u8", other=None, raw=False, modes=(),
         accumulate=False, env=None, crop_exact=False, data=None, seed=0):
    return dict(D=D, B=B, dims=dims, offs=offs, border=border, norm=norm, dtype=dtype, mask=mask, other=other, raw=raw, modes=modes,
                accumulate=accumulate, env=env, crop_exact=crop_exact, data=data, seed=seed)


V3 = dict(dims=(6, 48, 96), offs="norm5", border=1, norm=1, mask=None)
CASES = {
    "c16": case(modes=(0, 1), seed=1),
    "c16_crop": case(border=1, norm=1, modes=(0, 1), crop_exact=True, seed=2),
    "c16_fmask": case(mask="f32", modes=(0, 1), seed=3),
    "c32": case(D=32, raw=True, modes=(0, 1, 3), seed=4),
    "c64": case(D=64, offs="cross8", raw=True, modes=(0, 1, 3), seed=5),
    "h32_f16": case(D=32, dtype="f16", raw=True, modes=(0, 1), seed=6),
    "h64_bf16": case(D=64, offs="cross8", dtype="bf16", raw=True, modes=(0, 1), seed=7),
    "ema16": case(other="detached", modes=(2,), seed=8),
    "ema16_acc": case(other="detached", modes=(2,), accumulate=True, data="ema16", seed=8),
    "ema32": case(D=32, other="detached", raw=True, modes=(4,), seed=9),
    "ema16_both": case(other="both", seed=10),
    "diag16": case(offs="diag", seed=11),
    "diag16_fmask": case(offs="diag", mask="f32", seed=12),
    "diag64": case(D=64, offs="diag", seed=13),
    "zm5": case(modes=(1, 3), env=("PEA_ZMARCH", "2"), raw=True, seed=14, **V3),
    "zm5_cross": case(modes=(0, 1), data="zm5", seed=14, **V3),
    "n26": case(B=1, dims=(7, 40, 72), offs="n26", border=1, norm=1, mask=None, modes=(0, 1), seed=15),
    "rep6": case(B=1, dims=(4, 40, 72), offs="rep6", border=2, norm=2, mask=None, seed=16),
}
PAIR = case(other="detached", modes=(5,), seed=20)
INFER = {"infer16": case(seed=21), "infer32_f16": case(D=32, dtype="f16", seed=22)}
LAB = case(seed=23)

EMB = ("e", "e_other", "ema", "de", "de_other")  # pointers of the embedding's storage type


# ---- variants -----------------------------------------------------------------------------------------------------------------
def elem(c, ptr):
    if ptr in EMB:
        return 4 if c["dtype"] == "f32" else 2
    if ptr == "mask":
        return 4 if c["mask"] == "f32" else 1
    return 4


def variants(c, fwd, bwd, stride=True):
    """aligned, one variant per pointer of each call (16-bit embedding pointers once more by 8 bytes), all, and -- for the calls that
    take target / weight / mask -- stride"""
    out = ["aligned"]
    for side, ptrs in (("f", fwd), ("b", bwd)):
        for p in ptrs:
            out.append("%s:%s" % (side, p))
            if p in EMB and c["dtype"] != "f32":
                out.append("%s:%s+8" % (side, p))
    out.append("all")
    if stride:
        out.append("stride")
    return out


def skews(c, variant):
    """-> sk(side, ptr): the byte skew of that pointer in this variant"""
    def sk(side, ptr):
        if variant == "all":
            return elem(c, ptr)
        if variant == "%s:%s" % (side, ptr):
            return elem(c, ptr)
        if variant == "%s:%s+8" % (side, ptr):
            return 8
        return 0
    return sk


def loss_ptrs(c):
    fwd = ["e"] + (["e_other"] if c["other"] else []) + ["target", "weight"] + (["mask"] if c["mask"] else []) + \
        ["affs", "g_out", "inv_norm_out"]
    bwd = ["e"] + (["e_other"] if c["other"] else []) + ["g", "inv_norm"] + (["affs"] if c["raw"] else []) + ["de"] + \
        (["de_other"] if c["other"] == "both" else [])
    return fwd, bwd


def loss_params():
    out = []
    for name, c in CASES.items():
        fwd, bwd = loss_ptrs(c)
        if c["accumulate"]:
            fwd = []  # the flag is a backward flag: the forward variants are ema16's
        for v in variants(c, fwd, bwd):
            if v == "stride" and c["accumulate"]:
                continue
            out.append(pytest.param(name, v, id="%s-%s" % (name, v)))
    return out


# ---- fixtures, inputs, references (once per case) --------------------------------------------------------------------------------
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


_CACHE = {}


def offsets3(c):
    return [[0] * (3 - len(o)) + list(o) for o in OFFS[c["offs"]]]


def frac_mask(shape, seed):
    """U(0, 1) with exact 0, 0.5, 1 and 1.5 sprinkled in (the reference multiplies by mask.float(): any value counts)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape, generator=g)
    pick = torch.randint(0, 8, shape, generator=g)
    for v, k in ((0.0, 0), (0.5, 1), (1.0, 2), (1.5, 3)):
        m = torch.where(pick == k, torch.full_like(m, v), m)
    return m


def make_inputs(synth, dev, c, lam=None, lam_other=None):
    """device tensors (5D) of a case and its float64 reference(s)"""
    B, D, (Z, Y, X), seed = c["B"], c["D"], c["dims"], 900 + c["seed"]
    o3 = offsets3(c)
    K = len(o3)
    if Z == 1:
        e, t, w, m8 = synth.synth_inputs_2d(B, D, Y, X, OFFS[c["offs"]], seed)
    else:
        e, t, w = synth.synth_inputs_3d(B, D, Z, Y, X, o3, seed)
        m8 = None
    tdt = DTYPES[c["dtype"]][0]
    E = torch.from_numpy(np.ascontiguousarray(e)).view(B, D, Z, Y, X)
    if tdt == torch.float32:
        # pixels on the clamp branch of F.normalize: zero norm, and a norm of 1e-14 < eps (their 1 / norm is stored negated)
        for b in range(B):
            E[b, :, 0, 0, 0] = 0.0
            E[b, :, Z - 1, Y // 2, X // 2] = 0.0
            E[b, 0, Z - 1, Y // 2, X // 2] = 1e-14
    I = dict(E=E.to(tdt).to(dev), O=None, K=K, o3=o3,
             T=torch.from_numpy(np.ascontiguousarray(t)).view(B, K, Z, Y, X).to(dev),
             W=torch.from_numpy(np.ascontiguousarray(w)).view(B, K, Z, Y, X).to(dev), M=None)
    if c["mask"] == "u8":
        I["M"] = torch.from_numpy(np.ascontiguousarray(m8)).view(B, K, Z, Y, X).to(dev)
    elif c["mask"] == "f32":
        I["M"] = frac_mask((B, K, Z, Y, X), seed + 1).to(dev)
    if c["other"]:
        I["O"] = torch.from_numpy(synth.synth_embedding((B, D, Z, Y, X), seed + 2)).float().to(tdt).to(dev)
    I["lam"] = lam or [1.0 + 0.125 * (i % 3) for i in range(K)]
    return I


def reference(I, c, other, lam, other_grad=False):
    return cosine_loss(I["E"], other, I["T"], I["W"], I["M"], I["o3"], lam, 1e-12, c["border"], c["norm"], dloss=DLOSS,
                       other_grad=other_grad)


def loss_inputs(synth, dev, name):
    c = CASES[name]
    key = c["data"] or name
    if key not in _CACHE:
        I = make_inputs(synth, dev, c)
        I["ref"] = reference(I, c, I["O"], I["lam"], other_grad=c["other"] == "both")
        I["inv"] = inv_norm_plane(I["E"], 1e-12)
        I["inv_other"] = None if I["O"] is None else inv_norm_plane(I["O"], 1e-12)
        _CACHE[key] = I
    return _CACHE[key]


# ---- the descriptor and the calls ------------------------------------------------------------------------------------------------
def make_desc(pkg, c, o3, lam, flags=0, strides=(0, 0, 0), B=None, dims=None, D=None):
    d = pkg._lib.PeaDesc()
    dims = dims or c["dims"]
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2 if dims[0] == 1 else 3, B or c["B"], D or c["D"], len(o3)
    d.dims[:] = list(dims)
    d.border, d.dtype, d.norm, d.eps = c["border"], DTYPES[c["dtype"]][1], c["norm"], 1e-12
    d.flags = flags | (FLAG_MASK_F32 if c["mask"] == "f32" else 0)
    for i, o in enumerate(o3):
        d.offsets[i][:] = o
        d.lam[i] = lam[i]
    d.target_bstride, d.weight_bstride, d.mask_bstride = strides
    assert pkg._lib.lib().pea_desc_validate(ctypes.byref(d)) == 0
    return d


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


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


class Run(object):
    """the arena of one variant: inputs (filled, must stay bit-unchanged), outputs (every element must be written)"""

    def __init__(self, pkg, dev, nbytes):
        self.A, self.dev, self.pkg = Arena(nbytes, dev), dev, pkg
        self.inputs, self.written, self.scratch = [], [], []

    def inp(self, name, src, skew=0, extra=0):
        if src is None:
            return None
        if extra:
            v = self.A.carve_batch_strided(src.shape, src.dtype, extra, skew_bytes=skew, name=name)
        else:
            v = self.A.carve(src.shape, src.dtype, skew_bytes=skew, name=name)
        self.A.fill(v, src)
        self.inputs.append(v)
        return v

    def out(self, name, shape, dtype=torch.float32, skew=0):
        v = self.A.carve(tuple(shape), dtype, skew_bytes=skew, name=name)
        self.written.append(v)
        return v

    def check(self):
        sync()
        self.A.check(written=self.written, untouched=self.inputs, scratch=self.scratch)


def new_state(R, pkg, op, d, name="state", n=1):
    """n state blocks back to back, initialised; -> (int32 view, bytes of one)"""
    L = pkg._lib.lib()
    sb = int(L.pea_workspace_bytes(ctypes.byref(d)))
    assert sb % 8 == 0 and sb > 0
    st = R.out(name, (n * sb // 4,), torch.int32)
    assert L.pea_workspace_init(P(st), n * sb, op._stream()) == 0
    return st, sb


def assert_state_clean(st, sb, what=""):
    s = st.view(-1, sb // 4)
    assert bool((s[:, 0] == MAGIC).all()), "state block lost its magic word " + what
    assert not bool(s[:, 1:].any()), "state block is not zero between calls " + what


def holds_pattern(v):
    """every element of an arena view still holds the fill pattern"""
    if v.element_size() == 2:
        return bool((v.view(torch.int16) == PATTERN16).all())
    return bool((v.view(torch.int32) == PATTERN).all())


def relmax(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_affs(affs, ref_affs, what):
    err = float((affs.double() - ref_affs.view(affs.shape)).abs().max())
    assert err < AFFS_ATOL, "%s: affs max err %.3g" % (what, err)


def check_loss(lv, ref, lam, what):
    lv = lv.double()
    assert bool(torch.isfinite(lv).all()), what
    assert abs(float(lv[0]) - float(ref["loss"])) <= LOSS_RTOL * abs(float(ref["loss"])), "%s: loss %.9g ref %.9g" % (
        what, float(lv[0]), float(ref["loss"]))
    parts = ref["parts"]
    assert bool(((lv[1:] - parts).abs() <= LOSS_RTOL * parts.abs() + 1e-30).all()), "%s: per-offset losses" % what


def check_grad(de, ref_de, E, c, what):
    tol = GRAD_RTOL if c["dtype"] == "f32" else GRAD_RTOL_16
    assert bool(torch.isfinite(de.float()).all()), what
    r = relmax(de, ref_de.view(de.shape))
    assert r < tol, "%s: gradient rel err %.3g" % (what, r)
    # the pixels on the clamp branch carry G / eps, 1e12 times a regular gradient: the same bound against the largest REGULAR gradient
    reg = (E.double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(ref_de).reshape(de.shape)
    zero = torch.zeros_like(ref_de).view(de.shape)
    r = relmax(torch.where(reg, de.double(), zero), torch.where(reg, ref_de.view(de.shape), zero))
    assert r < tol, "%s: regular gradient rel err %.3g" % (what, r)


def check_inv(inv, ref_inv, what):
    ref_inv = ref_inv.view(inv.shape)
    bad = (inv.double() - ref_inv).abs() > INV_RTOL * ref_inv.abs()
    assert not bool(bad.any()), "%s: 1 / norm plane (%d off)" % (what, int(bad.sum()))


def arena_bytes(c, K, copies_e=8, copies_k=9):
    S = c["dims"][0] * c["dims"][1] * c["dims"][2]
    return c["B"] * S * 4 * (copies_e * c["D"] + copies_k * K + 16) + (1 << 20)


def ragged(c, variant, K):
    """target / weight / mask batch strides K*S + 1, + 2, + 3 in the stride variant -> (extras, descriptor strides)"""
    if variant != "stride":
        return (0, 0, 0), (0, 0, 0)
    KS = K * c["dims"][0] * c["dims"][1] * c["dims"][2]
    return (1, 2, 3), (KS + 1, KS + 2, KS + 3 if c["mask"] else 0)


# ---- the loss cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", loss_params())
def test_loss_case(pkg, op, dev, synth, monkeypatch, name, variant):
    c = CASES[name]
    I = loss_inputs(synth, dev, name)
    if c["env"]:
        monkeypatch.setenv(*c["env"])
    L = pkg._lib.lib()
    sk, K, B, dims = skews(c, variant), I["K"], c["B"], c["dims"]
    extras, strides = ragged(c, variant, K)
    d = make_desc(pkg, c, I["o3"], I["lam"], FLAG_ACCUMULATE if c["accumulate"] else 0, strides)
    if variant == "aligned":
        for mode in c["modes"]:
            assert L.pea_cross_supported(ctypes.byref(d), mode) == 1, "%s is not in the fast set of mode %d" % (name, mode)
    R = Run(pkg, dev, arena_bytes(c, K))
    kshape, tdt = (B, K) + tuple(dims), DTYPES[c["dtype"]][0]
    # forward
    e_f = R.inp("e", I["E"], sk("f", "e"))
    o_f = R.inp("e_other", I["O"], sk("f", "e_other"))
    t = R.inp("target", I["T"], sk("f", "target"), extras[0])
    w = R.inp("weight", I["W"], sk("f", "weight"), extras[1])
    m = R.inp("mask", I["M"], sk("f", "mask"), extras[2])
    dl = R.inp("dloss", torch.tensor([DLOSS], dtype=torch.float32))
    affs = R.out("affs", kshape, skew=sk("f", "affs"))
    g = R.out("g_out", kshape, skew=sk("f", "g_out"))
    inv = R.out("inv_norm_out", ((2 if c["other"] else 1), B) + tuple(dims), skew=sk("f", "inv_norm_out"))
    lv = R.out("loss_out", (1 + K,))
    st, sb = new_state(R, pkg, op, d)
    rc = launched(L.pea_affinity_fwd_ex(ctypes.byref(d), P(e_f), P(o_f), P(t), P(w), P(m), P(affs), P(g), P(inv), P(lv), P(st), sb, op._stream()))
    assert rc == 0, "forward rc %d" % rc
    # backward: the forward's buffers where the two calls' skews agree, a copy at the backward's address where they do not

    def again(label, buf, fkey, bkey, src=None):
        if buf is None or sk("f", fkey) == sk("b", bkey):
            return buf
        return R.inp(label + " (backward)", buf if src is None else src, sk("b", bkey))

    e_b = again("e", e_f, "e", "e", I["E"])
    o_b = again("e_other", o_f, "e_other", "e_other", I["O"])
    g_b = again("g", g, "g_out", "g")
    inv_b = again("inv_norm", inv, "inv_norm_out", "inv_norm")
    affs_b = again("affs", affs, "affs", "affs") if c["raw"] else None
    de = R.out("de", I["E"].shape, tdt, sk("b", "de"))
    de_o = R.out("de_other", I["E"].shape, tdt, sk("b", "de_other")) if c["other"] == "both" else None
    base = None
    if c["accumulate"]:
        # (a plain copy, not arena.fill: the arena still expects the pattern there, so de counts as written after either outcome)
        gen = torch.Generator().manual_seed(5)
        base = ((torch.rand(I["E"].shape, generator=gen) - 0.5) * 1e-3).to(dev)
        de.copy_(base)
    rc = launched(L.pea_affinity_bwd_ex2(ctypes.byref(d), P(e_b), P(o_b), P(g_b), P(inv_b), P(affs_b), P(dl), P(de), P(de_o), op._stream()))
    sync()
    what = "%s-%s" % (name, variant)
    ref = I["ref"]
    if c["accumulate"] and (sk("b", "e_other") or sk("b", "inv_norm")):
        # the role-A cross kernel stages e_other and the 1 / norm planes by 16-byte DMA: it declines, and nothing else accumulates
        assert rc == E_UNSUPPORTED, "%s: rc %d" % (what, rc)
        assert torch.equal(de.view(torch.int32), base.view(torch.int32)), "%s: a declined accumulate touched de" % what
    else:
        assert rc == 0, "%s: backward rc %d" % (what, rc)
        want = ref["de"] if base is None else ref["de"] + base.double()
        check_grad(de, want, I["E"], c, what)
        if de_o is not None:
            check_grad(de_o, ref["de_other"], I["O"], c, what + " de_other")
    check_affs(affs, ref["affs"], what)
    check_loss(lv, ref, I["lam"], what)
    check_inv(inv[0], I["inv"], what)
    if c["other"]:
        check_inv(inv[1], I["inv_other"], what + " (second operand)")
    if c["crop_exact"]:
        for i, o in enumerate(I["o3"]):
            _, ok = shifted(I["E"][:, :1], o, BORDER_CROP_ZERO)
            gone = (~ok).expand(B, *dims)
            assert gone.any() and not bool(affs[:, i][gone].any()) and not bool(g[:, i][gone].any()), "%s: cropped border, offset %d" % (what, i)
    assert_state_clean(st, sb, what)
    R.check()


# ---- the pair -----------------------------------------------------------------------------------------------------------------------
PAIR_FWD = ["e", "ema", "target", "weight", "mask", "affs", "g_out", "g_cross_out", "inv_norm_out", "inv_norm_other_out"]
PAIR_BWD = ["e", "ema", "g", "g_cross", "inv_norm", "inv_norm_other", "de"]
# what the one-launch kernels move in quads / by 16-byte DMA: a skew there is declined (csrc/pea_k_xdma.hip, xdma_fwd_dual / xdma_bwd_dual)
PAIR_FWD_DECLINES = {"f:e", "f:ema", "f:target", "f:weight", "f:mask", "f:affs", "f:g_out", "f:g_cross_out", "all", "stride"}
PAIR_BWD_DECLINES = {"b:e", "b:ema", "b:inv_norm", "b:inv_norm_other", "all"}


def pair_inputs(synth, dev):
    if "pair16" not in _CACHE:
        I = make_inputs(synth, dev, PAIR)
        K = I["K"]
        I["lam_cross"] = [0.7 if i < 2 else 1.0 for i in range(K)]
        I["ref"] = reference(I, PAIR, None, I["lam"])
        I["ref_cross"] = reference(I, PAIR, I["O"], I["lam_cross"])
        I["inv"], I["inv_other"] = inv_norm_plane(I["E"], 1e-12), inv_norm_plane(I["O"], 1e-12)
        _CACHE["pair16"] = I
    return _CACHE["pair16"]


@pytest.mark.parametrize("variant", variants(PAIR, PAIR_FWD, PAIR_BWD))
def test_pair16(pkg, op, dev, synth, variant):
    c, I = PAIR, pair_inputs(synth, dev)
    L = pkg._lib.lib()
    sk, K, B, dims = skews(c, variant), I["K"], c["B"], c["dims"]
    extras, strides = ragged(c, variant, K)
    d = make_desc(pkg, c, I["o3"], I["lam"], 0, strides)
    dc = make_desc(pkg, c, I["o3"], I["lam_cross"], 0, strides)
    if variant == "aligned":
        assert L.pea_cross_supported(ctypes.byref(d), 5) == 1
    R = Run(pkg, dev, arena_bytes(c, K, 8, 12))
    kshape, plane = (B, K) + tuple(dims), (B,) + tuple(dims)
    e_f = R.inp("e", I["E"], sk("f", "e"))
    o_f = R.inp("ema", I["O"], sk("f", "ema"))
    t = R.inp("target", I["T"], sk("f", "target"), extras[0])
    w = R.inp("weight", I["W"], sk("f", "weight"), extras[1])
    m = R.inp("mask", I["M"], sk("f", "mask"), extras[2])
    dl = R.inp("dloss", torch.tensor([DLOSS], dtype=torch.float32))
    affs = R.out("affs", kshape, skew=sk("f", "affs"))
    g = R.out("g_out", kshape, skew=sk("f", "g_out"))
    gx = R.out("g_cross_out", kshape, skew=sk("f", "g_cross_out"))
    inv = R.out("inv_norm_out", plane, skew=sk("f", "inv_norm_out"))
    lv, lvx = R.out("loss_out", (1 + K,)), R.out("loss_cross_out", (1 + K,))
    st, sb = new_state(R, pkg, op, d, "states", 2)
    ws, wsx = P(st), ctypes.c_void_p(st.data_ptr() + sb)
    what = "pair16-" + variant
    if variant in PAIR_FWD_DECLINES:
        # refused "before anything is launched": the outputs still hold the pattern, the states are as initialised; then the two
        # calls the header prescribes, on the same blocks (the cross call writes both planes: {own, other})
        inv2 = R.out("inv_norm pair", (2,) + plane, skew=sk("f", "inv_norm_other_out"))
        rc = launched(L.pea_affinity_fwd_dual_ex(ctypes.byref(d), ctypes.byref(dc), P(e_f), P(o_f), P(t), P(w), P(m), P(affs), P(g), P(gx), P(inv),
                                        P(inv2[1]), P(lv), P(lvx), ws, wsx, sb, op._stream()))
        sync()
        assert rc == E_UNSUPPORTED, "%s: rc %d" % (what, rc)
        for v in (affs, g, gx, inv, inv2, lv, lvx):
            assert holds_pattern(v), "%s: a declined call wrote an output" % what
        assert_state_clean(st, sb, what + " (declined)")
        assert L.pea_affinity_fwd_ex(ctypes.byref(d), P(e_f), None, P(t), P(w), P(m), P(affs), P(g), P(inv), P(lv), ws, sb, op._stream()) == 0
        assert L.pea_affinity_fwd_ex(ctypes.byref(dc), P(e_f), P(o_f), P(t), P(w), P(m), None, P(gx), P(inv2), P(lvx), wsx, sb,
                                     op._stream()) == 0
        inv_o = inv2[1]
        check_inv(inv2[0], I["inv"], what + " (cross call, own plane)")
    else:
        inv_o = R.out("inv_norm_other_out", plane, skew=sk("f", "inv_norm_other_out"))
        rc = launched(L.pea_affinity_fwd_dual_ex(ctypes.byref(d), ctypes.byref(dc), P(e_f), P(o_f), P(t), P(w), P(m), P(affs), P(g), P(gx), P(inv),
                                        P(inv_o), P(lv), P(lvx), ws, wsx, sb, op._stream()))
        assert rc == 0, "%s: rc %d" % (what, rc)
    sync()
    check_affs(affs, I["ref"]["affs"], what)
    check_loss(lv, I["ref"], I["lam"], what)
    check_loss(lvx, I["ref_cross"], I["lam_cross"], what + " (cross)")
    check_inv(inv, I["inv"], what)
    check_inv(inv_o, I["inv_other"], what + " (ema)")
    assert_state_clean(st, sb, what)

    # backward
    def again(label, buf, fkey, bkey, src=None):
        if sk("f", fkey) == sk("b", bkey):
            return buf
        return R.inp(label + " (backward)", buf if src is None else src, sk("b", bkey))

    e_b, o_b = again("e", e_f, "e", "e", I["E"]), again("ema", o_f, "ema", "ema", I["O"])
    g_b, gx_b = again("g", g, "g_out", "g"), again("g_cross", gx, "g_cross_out", "g_cross")
    inv_b = again("inv_norm", inv, "inv_norm_out", "inv_norm")
    if variant in PAIR_FWD_DECLINES:  # (there the plane is the second half of the pair the cross call wrote)
        invo_b = R.inp("inv_norm_other (backward)", inv_o, sk("b", "inv_norm_other"))
    else:
        invo_b = again("inv_norm_other", inv_o, "inv_norm_other_out", "inv_norm_other")
    de = R.out("de", I["E"].shape, torch.float32, sk("b", "de"))
    rc = launched(L.pea_affinity_bwd_dual_ex(ctypes.byref(d), P(e_b), P(o_b), P(g_b), P(gx_b), P(inv_b), P(invo_b), P(dl), P(dl), P(de), op._stream()))
    sync()
    want = I["ref"]["de"] + I["ref_cross"]["de"]
    if variant in PAIR_BWD_DECLINES:
        assert rc == E_UNSUPPORTED, "%s: backward rc %d" % (what, rc)
        assert holds_pattern(de), "%s: a declined backward wrote de" % what
        # two pea_affinity_bwd_ex calls and an add, as the header says
        de2 = R.out("de (cross)", I["E"].shape, torch.float32, sk("b", "de"))
        inv_pair = R.inp("inv_norm pair (backward)", torch.stack([inv_b, invo_b]), sk("b", "inv_norm"))
        assert L.pea_affinity_bwd_ex(ctypes.byref(d), P(e_b), None, P(g_b), P(inv_b), P(dl), P(de), None, op._stream()) == 0
        assert L.pea_affinity_bwd_ex(ctypes.byref(dc), P(e_b), P(o_b), P(gx_b), P(inv_pair), P(dl), P(de2), None, op._stream()) == 0
        sync()
        check_grad(de.double() + de2.double(), want, I["E"], c, what + " (two calls)")
    else:
        assert rc == 0, "%s: backward rc %d" % (what, rc)
        check_grad(de, want, I["E"], c, what)
    R.check()


# ---- inference --------------------------------------------------------------------------------------------------------------------
def infer_params():
    return [pytest.param(n, v, id="%s-%s" % (n, v)) for n, c in INFER.items() for v in variants(c, ["e", "affs"], [], stride=False)]


@pytest.mark.parametrize("name,variant", infer_params())
def test_infer(pkg, op, dev, synth, name, variant):
    c = INFER[name]
    if name not in _CACHE:
        I = make_inputs(synth, dev, c)
        zero = torch.zeros_like(I["T"])
        I["ref"] = cosine_loss(I["E"], None, zero, zero, None, I["o3"], I["lam"], 1e-12, c["border"], c["norm"])
        _CACHE[name] = I
    I = _CACHE[name]
    sk, K = skews(c, variant), I["K"]
    d = make_desc(pkg, dict(c, mask=None), I["o3"], I["lam"], FLAG_RELU)
    R = Run(pkg, dev, arena_bytes(c, K, 2, 2))
    e = R.inp("e", I["E"], sk("f", "e"))
    affs = R.out("affs", (c["B"], K) + tuple(c["dims"]), skew=sk("f", "affs"))
    rc = launched(pkg._lib.lib().pea_affinity_infer(ctypes.byref(d), P(e), None, P(affs), op._stream()))
    sync()
    assert rc == 0
    check_affs(affs, I["ref"]["affs"].clamp_min(0.0), "%s-%s" % (name, variant))
    assert not bool((affs < 0).any())
    R.check()


# ---- the labels-in step ---------------------------------------------------------------------------------------------------------------
LAB_PTRS = ["e", "labels", "wtab", "affs", "de"]


def label_weights(pkg, op, d, lab, wtab, counts):
    L = pkg._lib.lib()
    return launched(L.pea_label_weights(ctypes.byref(d), P(lab), TGT_PADDING | TGT_MASK_INSIDE, P(wtab), P(counts), counts.numel() * 4,
                                        op._stream()))


def lab_inputs(pkg, op, synth, dev):
    if "lab16" not in _CACHE:
        c = LAB
        I = make_inputs(synth, dev, c)
        B, K, (Z, Y, X) = c["B"], I["K"], c["dims"]
        lab = torch.from_numpy(synth.synth_labels(B, (Z, Y, X), 923).astype(np.int32)).to(dev)
        # the class-balance table of these labels, from the library on plain (16-byte aligned) tensors: every variant must reproduce it
        # bit for bit (the counts are integers whichever kernel takes them)
        d = make_desc(pkg, dict(c, mask=None), I["o3"], I["lam"])
        I["counts_bytes"] = max(4, int(pkg._lib.lib().pea_targets_workspace_bytes(ctypes.byref(d))))
        wtab = torch.full((B, K, 2), float("nan"), dtype=torch.float32, device=dev)
        assert label_weights(pkg, op, d, lab, wtab, torch.empty(I["counts_bytes"] // 4, dtype=torch.int32, device=dev)) == 0
        sync()
        assert bool(torch.isfinite(wtab).all()) and bool((wtab > 0).all())
        T, M = [], []
        for o in I["o3"]:
            nb, ok = shifted(lab[:, None].double(), o, BORDER_CROP_ZERO)  # label(p + o); ok: the neighbour is inside
            ok = ok.expand(B, Z, Y, X)
            T.append(torch.where(ok, (lab.double() == nb[:, 0]).double(), torch.ones_like(nb[:, 0])))  # PEA_TGT_PADDING: 1 outside
            M.append(ok.to(torch.uint8))                                                              # PEA_TGT_MASK_INSIDE
        I["T"], I["M"] = torch.stack(T, 1).float(), torch.stack(M, 1)
        I["W"] = torch.where(I["T"] == 1, wtab[:, :, 0].view(B, K, 1, 1, 1), wtab[:, :, 1].view(B, K, 1, 1, 1)).expand_as(I["T"]).contiguous()
        I["labels"], I["wtab"] = lab, wtab
        I["ref"] = reference(I, c, None, I["lam"])
        _CACHE["lab16"] = I
    return _CACHE["lab16"]


@pytest.mark.parametrize("form", ["scratch", "one_launch"])
@pytest.mark.parametrize("variant", variants(LAB, LAB_PTRS, [], stride=False))
def test_lab16(pkg, op, dev, synth, variant, form):
    c, I = LAB, lab_inputs(pkg, op, synth, dev)
    L = pkg._lib.lib()
    sk, K = skews(c, variant), I["K"]
    d = make_desc(pkg, dict(c, mask=None), I["o3"], I["lam"])
    R = Run(pkg, dev, arena_bytes(c, K, 4, 6))
    e = R.inp("e", I["E"], sk("f", "e"))
    lab = R.inp("labels", I["labels"], sk("f", "labels"))
    wtab = R.out("wtab", I["wtab"].shape, skew=sk("f", "wtab"))
    counts = R.A.carve((I["counts_bytes"] // 4,), torch.int32, name="counts")
    R.scratch.append(counts)
    assert label_weights(pkg, op, d, lab, wtab, counts) == 0
    dl = R.inp("dloss", torch.tensor([DLOSS], dtype=torch.float32))
    affs = R.out("affs", (c["B"], K) + tuple(c["dims"]), skew=sk("f", "affs"))
    de = R.out("de", I["E"].shape, torch.float32, sk("f", "de"))
    lv = R.out("loss_out", (1 + K,))
    st, sb = new_state(R, pkg, op, d)
    scratch, nsc = None, 0
    if form == "scratch":
        nsc = int(L.pea_labels_scratch_bytes(ctypes.byref(d)))
        assert nsc > 0 and nsc % 16 == 0, "lab16 is not in the two-launch set"
        scratch = R.A.carve((nsc // 4,), torch.float32, name="scratch")
        R.scratch.append(scratch)
    rc = launched(L.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), P(e), None, P(lab), P(wtab), TGT_PADDING | TGT_MASK_INSIDE, P(affs), P(lv), P(dl),
                                          P(de), P(st), sb, P(scratch), nsc, op._stream()))
    sync()
    what = "lab16-%s-%s" % (form, variant)
    assert rc == 0, "%s: rc %d" % (what, rc)
    check_affs(affs, I["ref"]["affs"], what)
    check_loss(lv, I["ref"], I["lam"], what)
    check_grad(de, I["ref"]["de"], I["E"], c, what)
    assert torch.equal(wtab.view(torch.int32), I["wtab"].view(torch.int32)), "%s: the weight table differs from the aligned call's" % what
    assert_state_clean(st, sb, what)
    R.check()


# ---- four self losses per launch ------------------------------------------------------------------------------------------------------
MULTI = [  # (B, D, H, W, offsets, mask kind, affs wanted, dloss, lambda): the table of tests/test_gpu_multi.py
    (3, 16, 37, 70, mo([1, 3, 5, 9], 4), "f32", True, 0.625, None),
    (1, 16, 19, 33, mo([1, 3, 5], 4), "u8", False, None, None),
    (2, 32, 17, 40, mo([1, 3], 8), None, True, 1.75, [2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0]),
    (2, 16, 5, 6, mo([1], 4), "u8", True, None, None),
]


def multi_variants():
    out = ["aligned"]
    for j, (_, _, _, _, _, mk, want_affs, _, _) in enumerate(MULTI):
        for p in ["e", "target", "weight"] + (["mask"] if mk else []) + (["affs"] if want_affs else []) + ["g_out"]:
            out.append("f:%s@%d" % (p, j))
        for p in ("e", "g", "de"):
            out.append("b:%s@%d" % (p, j))
    return out + ["all", "stride"]


def multi_inputs(synth, dev):
    if "multi4" not in _CACHE:
        ents = []
        for j, (B, D, H, W, offs, mk, want_affs, dloss, lam) in enumerate(MULTI):
            c = case(D=D, B=B, dims=(1, H, W), mask=mk, seed=40 + j)
            OFFS["multi%d" % j] = offs
            c["offs"] = "multi%d" % j
            I = make_inputs(synth, dev, c, lam=lam or [1.0] * len(offs))
            I["ref"] = cosine_loss(I["E"], None, I["T"], I["W"], I["M"], I["o3"], I["lam"], 1e-12, 0, 0, dloss=dloss)
            I["c"], I["dloss"], I["want_affs"] = c, dloss, want_affs
            ents.append(I)
        _CACHE["multi4"] = ents
    return _CACHE["multi4"]


@pytest.mark.parametrize("variant", multi_variants())
def test_multi4(pkg, op, dev, synth, variant):
    ents = multi_inputs(synth, dev)
    L, n = pkg._lib.lib(), len(ents)

    def sk(side, ptr, j, c):
        if variant == "all" or variant == "%s:%s@%d" % (side, ptr, j):
            return elem(c, ptr)
        return 0

    total = sum(arena_bytes(I["c"], I["K"], 3, 6) for I in ents)
    R = Run(pkg, dev, total)
    ft, bt = (pkg._lib.PeaMultiFwd * n)(), (pkg._lib.PeaMultiBwd * n)()
    descs, outs = [], []
    for j, I in enumerate(ents):
        c, K = I["c"], I["K"]
        extras, strides = ragged(c, variant, K)
        d = make_desc(pkg, c, I["o3"], I["lam"], 0, strides)
        descs.append(d)
        tag = "@%d" % j
        e_f = R.inp("e" + tag, I["E"], sk("f", "e", j, c))
        t = R.inp("target" + tag, I["T"], sk("f", "target", j, c), extras[0])
        w = R.inp("weight" + tag, I["W"], sk("f", "weight", j, c), extras[1])
        m = R.inp("mask" + tag, I["M"], sk("f", "mask", j, c), extras[2])
        kshape = (c["B"], K) + tuple(c["dims"])
        affs = R.out("affs" + tag, kshape, skew=sk("f", "affs", j, c)) if I["want_affs"] else None
        g = R.out("g_out" + tag, kshape, skew=sk("f", "g_out", j, c))
        lv = R.out("loss_out" + tag, (1 + K,))
        dl = None if I["dloss"] is None else R.inp("dloss" + tag, torch.tensor([I["dloss"]], dtype=torch.float32))
        a = ft[j]
        a.desc, a.e, a.target, a.weight = ctypes.pointer(d), e_f.data_ptr(), t.data_ptr(), w.data_ptr()
        a.mask = None if m is None else m.data_ptr()
        a.affs = None if affs is None else affs.data_ptr()
        a.g_out, a.loss_out = g.data_ptr(), lv.data_ptr()
        outs.append(dict(e_f=e_f, affs=affs, g=g, lv=lv, dl=dl))
    arr = (ctypes.POINTER(pkg._lib.PeaDesc) * n)(*[ctypes.pointer(x) for x in descs])
    assert L.pea_multi_supported(arr, n) == 1
    st, sb = new_state(R, pkg, op, descs[0], "states", n)
    rc = launched(L.pea_affinity_fwd_multi(ft, n, P(st), n * sb, op._stream()))
    assert rc == 0, "forward rc %d" % rc
    for j, I in enumerate(ents):
        c, o = I["c"], outs[j]
        tag = "@%d" % j
        e_b = o["e_f"] if sk("f", "e", j, c) == sk("b", "e", j, c) else R.inp("e (backward)" + tag, I["E"], sk("b", "e", j, c))
        g_b = o["g"] if sk("f", "g_out", j, c) == sk("b", "g", j, c) else R.inp("g (backward)" + tag, o["g"], sk("b", "g", j, c))
        o["de"] = R.out("de" + tag, I["E"].shape, torch.float32, sk("b", "de", j, c))
        b = bt[j]
        b.desc, b.e, b.g, b.de = ctypes.pointer(descs[j]), e_b.data_ptr(), g_b.data_ptr(), o["de"].data_ptr()
        b.dloss = None if o["dl"] is None else o["dl"].data_ptr()
    rc = launched(L.pea_affinity_bwd_multi(bt, n, op._stream()))
    sync()
    assert rc == 0, "backward rc %d" % rc
    for j, I in enumerate(ents):
        o, what = outs[j], "multi4-%s entry %d" % (variant, j)
        if o["affs"] is not None:
            check_affs(o["affs"], I["ref"]["affs"], what)
        check_loss(o["lv"], I["ref"], I["lam"], what)
        check_grad(o["de"], I["ref"]["de"], I["E"], I["c"], what)
    assert_state_clean(st, sb, "multi4-" + variant)
    R.check()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def off_by_one(src):
    """a contiguous view of `src`'s data at storage offset 1 of a flat buffer: element-aligned, never 16-byte aligned"""
    flat = torch.empty(src.numel() + 1, dtype=src.dtype, device=src.device)
    v = flat[1:].view(src.shape)
    v.copy_(src)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("D,dtype", [(16, "f32"), (32, "bf16")])
def test_python_layer_on_views_at_storage_offset_1(pkg, dev, synth, D, dtype):
    """embedding_loss and ema_embedding_loss on e, ema, target, weight and mask that are contiguous but not 16-byte aligned: no copy is
    made (the library gets these very pointers), same reference, same tolerances"""
    c = case(D=D, dtype=dtype, other="detached", seed=30 + D)
    I = make_inputs(synth, dev, c)
    lam_x = [0.7 if i < 2 else 1.0 for i in range(I["K"])]
    ref = cosine_loss(I["E"], None, I["T"], I["W"], I["M"], I["o3"], [1.0] * I["K"], 1e-12, 0, 0)
    refx = cosine_loss(I["E"], I["O"], I["T"], I["W"], I["M"], I["o3"], lam_x, 1e-12, 0, 0)
    sq = lambda v: v.view(v.shape[:2] + v.shape[3:])  # noqa: E731  (the 2D API takes [B, C, H, W])
    T, W, M, O = [off_by_one(sq(I[k])) for k in ("T", "W", "M", "O")]
    crit = pkg.WeightedMSE()
    for second, r in ((None, ref), (O, refx)):
        x = off_by_one(sq(I["E"])).detach().requires_grad_(True)
        assert x.is_contiguous() and x.data_ptr() % 16 != 0
        if second is None:
            loss, affs, _ = pkg.embedding_loss(x, T, W, M, crit, OFFS["cross"])
        else:
            loss, affs = pkg.ema_embedding_loss(x, second, T, W, M, crit, OFFS["cross"], affs0_weight=0.7)
        loss.backward()
        sync()
        what = "python layer D=%d %s %s" % (D, dtype, "self" if second is None else "ema")
        assert abs(loss.item() - float(r["loss"])) <= LOSS_RTOL * abs(float(r["loss"])), what
        check_affs(affs, r["affs"], what)
        check_grad(x.grad.view(I["E"].shape), r["de"], I["E"], c, what)
