"""GPU (-m gpu): the batched deep-supervision losses on f16 / bf16 embeddings (include/pea_multi.h, include/pea_multi_labels.h on
16-bit storage; csrc/pea_k_multi.hip, csrc/pea_k_multi_labels.hip instantiated per storage type).  Every test runs for both types.

  1. the C ABI on the ragged table of tests/test_gpu_multi.py (and its one / two entry prefixes), the embeddings rounded to the
     storage type, against the C oracle on the exact upcast;
  2. the same arithmetic: the f32 calls on the upcast against the 16-bit calls -- affs, g, loss bit-equal, de = round(de32);
  3. four CROP_ZERO norm1 entries in 3D, the cropped border slices exactly 0;
  4. the labels-in form on the table of tests/test_gpu_multi_labels.py against pea_gen_targets + the oracle; wtab NULL = given;
  5. e / de that are 2-byte but not 4-byte aligned, odd S, guard elements around de;
  6. one NaN channel: de is NaN exactly where a formula reads it, never inf, the other entries keep their bits;
  7. bit-reproducibility, and the state blocks left ready for a single f32 call;
  8. the public functions, the sections with batched=True and pea.graphed on 16-bit leaves.

Inputs: the synth inputs of the two f32 test files with their zero-norm pixels; the pixel of norm 1e-14 (below eps = 1e-12) survives
the rounding to bf16, in f16 it rounds to the zero vector, which is that type's clamp-branch case.

Bounds.  AFFS_ATOL and LOSS_RTOL are those of tests/test_gpu_bf16.py, and so is the rule for de (one_ulp_rule below, for either
16-bit type): within one storage ulp of the f32 gradient rounded to the storage type; where |g32| is below 2^-16 of the largest
element the f32 reordering bound 2^-20 * max|g32| is accepted instead.  The clamp-branch pixels carry G / eps, 1e12 times a regular
gradient (inf in f16), so over a whole tensor that holds one every regular element falls under the carve-out: the regular pixels are
therefore ALSO held, on their own, to  |de16 - ref| <= rtol * max|ref over regular pixels| + one storage ulp of |ref|  with the rtol
the f32 tests of the same comparison use (1e-4 against the float64-accumulating oracle, 1e-5 between two f32 kernels): the error of
the f32 evaluation plus one rounding.  g has no oracle output: it is 2 lambda_i / N_i * w m^2 (a - t), held to the oracle's map
through AFFS_ATOL scaled by that factor.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import test_gpu_multi as gm
import test_gpu_multi_labels as gl
from conftest import load_golden
from test_gpu_bf16 import AFFS_ATOL, LOSS_RTOL, _mono

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float16, id="f16"), pytest.param(torch.bfloat16, id="bf16")]
MANT = {torch.float16: 10, torch.bfloat16: 7}          # stored mantissa bits
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126}   # exponent of the smallest normal number
ORACLE_RTOL, KERNEL_RTOL = 1e-4, 1e-5                   # GRAD_RTOL of tests/test_gpu_multi.py: against the oracle / multi against single
FLAGS_2D, FLAGS_3D = gl.FLAGS_2D, gl.FLAGS_3D


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


FUSED = ("pea_affinity_fwd_multi", "pea_affinity_bwd_multi", "pea_affinity_fwd_bwd_labels_multi")


class Spy(object):
    """return codes of the three batched calls made while it is installed"""

    def __init__(self, pkg, monkeypatch):
        L = pkg._lib.lib()
        self.fwd, self.bwd, self.labels = [], [], []
        for name, log in zip(FUSED, (self.fwd, self.bwd, self.labels)):
            real = getattr(L, name)
            monkeypatch.setattr(L, name, lambda *a, _real=real, _log=log: (_log.append(_real(*a)), _log[-1])[1])


@pytest.fixture
def spy(pkg, monkeypatch):
    return Spy(pkg, monkeypatch)


cu = gm.cu


def rounded(e, tdt):
    """numpy f32 -> (the values rounded to the storage type as a CPU tensor, their exact upcast as numpy f32)"""
    x = torch.from_numpy(np.ascontiguousarray(e)).to(tdt)
    return x, x.float().numpy()


def ulp_of(ref, tdt):
    """the storage type's spacing at |ref| (f32 tensor)"""
    ex = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** MIN_EXP[tdt]))).clamp_min(MIN_EXP[tdt])
    return torch.exp2(ex - MANT[tdt])


def one_ulp_rule(g16, g32):
    """assert_within_one_ulp of tests/test_gpu_bf16.py for either 16-bit type -> the number of elements that are not bit-equal to
    g32 rounded to the storage type"""
    assert g16.dtype in MANT and g32.dtype == torch.float32 and g16.shape == g32.shape
    r = g32.to(g16.dtype)
    d = (_mono(g16) - _mono(r)).abs()
    gmax = float(g32.abs().max())
    small = g32.abs() < gmax * 2.0 ** -16
    if (~small).any():
        assert int(d[~small].max()) <= 1
    far = (d > 1) & ((g16.float() - g32).abs() > gmax * 2.0 ** -20)
    assert int(far.sum()) == 0, "%d elements beyond one %s ulp" % (int(far.sum()), g16.dtype)
    return int((g16.view(torch.int16) != r.view(torch.int16)).sum())


def regular_rule(g16, ref, e_up, rtol, what=""):
    """the regular pixels (|e| >= eps) on their own: |g16 - ref| <= rtol * max|ref| + one storage ulp of |ref| (module docstring)"""
    ref = ref.float()
    reg = (e_up.double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(ref)
    refr = torch.where(reg, ref, torch.zeros_like(ref))
    got = torch.where(reg, g16.float(), torch.zeros_like(ref))
    assert torch.isfinite(got).all(), what
    bound = rtol * float(refr.abs().max()) + ulp_of(refr, g16.dtype)
    excess = float(((got - refr).abs() - bound).max())
    print("%s regular pixels: max |diff| %.3g, max |ref| %.3g" % (what, float((got - refr).abs().max()), float(refr.abs().max())))
    assert excess <= 0, what


def check_de(de16, ref32, e_up, rtol, what=""):
    """the rule of tests/test_gpu_bf16.py over the whole tensor, then the regular pixels alone -> the count of one_ulp_rule"""
    ref32 = ref32.to(de16.device)
    n = one_ulp_rule(de16, ref32)
    regular_rule(de16, ref32, e_up.to(de16.device), rtol, what)
    return n


def expected_g(ent, o_affs):
    """g = 2 lambda_i / N_i * w m^2 (a - t) from the oracle's map (float64) and the factor in front of (a - t)"""
    d = ent["desc"]
    K = d.K
    dims = [d.dims[a] for a in range(3)]
    f = np.empty(K)
    for i in range(K):
        n = d.B * dims[2] if d.norm == 0 else d.B * np.prod([dims[a] - abs(d.offsets[i][a]) for a in range(3)])
        f[i] = 2.0 * d.lam[i] / n
    w = ent["ow"].astype(np.float64)
    if ent["om"] is not None:
        w = w * ent["om"].astype(np.float64)
    fac = f.reshape((1, K) + (1,) * (w.ndim - 2)) * w
    return fac * (o_affs.astype(np.float64) - ent["t"].astype(np.float64)), np.abs(fac)


# ----------------------------------------------------------------------------------------------------------------------------
# the tensor-form table: the configuration of tests/test_gpu_multi.py, the embedding rounded, the oracle on the upcast
# ----------------------------------------------------------------------------------------------------------------------------
_TABLES = {}


def tensor_table(pkg, orc, synth, tdt):
    key = ("tensor", tdt)
    if key in _TABLES:
        return _TABLES[key]
    mo = pkg.multi_offset
    cfg = [  # (B, D, H, W, offsets, mask kind, affs wanted, dloss, lambda): tests/test_gpu_multi.py
        (3, 16, 37, 70, mo([1, 3, 5, 9], 4), "f32", True, 0.625, None),
        (1, 16, 19, 33, mo([1, 3, 5], 4), "u8", False, None, None),
        (2, 32, 17, 40, mo([1, 3], 8), None, True, 1.75, [2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0]),
        (2, 16, 5, 6, mo([1], 4), "u8", True, None, None),
    ]
    out = []
    for j, (B, D, H, W, offsets, mkind, want_affs, dloss, lam) in enumerate(cfg):
        e, t, w, m8 = synth.synth_inputs_2d(B, D, H, W, offsets, 410 + j)
        e16, e = rounded(gm._degenerate_pixels(e), tdt)
        n = np.sqrt((e.astype(np.float64) ** 2).sum(1))
        assert (n == 0).sum() >= 3 * B and ((n > 0) & (n < 1e-12)).sum() == (B if tdt == torch.bfloat16 else 0)
        d = orc.desc_2d(e, offsets, lam)
        if mkind == "f32":  # (tests/test_gpu_multi.py: a fractional mask m is the weight w m^2 without a mask)
            m = gm._frac_mask(synth, t.shape, 77)
            ow, om = (w.astype(np.float64) * m.astype(np.float64) ** 2).astype(np.float32), None
        else:
            m = m8 if mkind == "u8" else None
            ow, om = w, m
        o_affs, o_loss = orc.c_fwd(d, e, None, t, ow, om)
        o_grad, _ = orc.c_bwd(d, e, None, t, ow, om, dloss=1.0 if dloss is None else dloss)
        out.append(dict(e16=e16, e=e, t=t, w=w, m=m, ow=ow, om=om, desc=d, offsets=offsets, lam=lam, want_affs=want_affs, dloss=dloss,
                        K=len(offsets), packed=j == 0, o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    _TABLES[key] = out
    return out


def device_entry(pkg, op, dev, ent, tdt, offset_view=False):
    """_device_entry of tests/test_gpu_multi.py with the embedding in tdt (None: the f32 upcast); offset_view: e starts one element
    into its buffer"""
    if tdt is None:
        E = cu(ent["e"], dev)
    elif offset_view:
        buf = torch.zeros(ent["e16"].numel() + 1, dtype=tdt, device=dev)
        E = buf[1:].view(ent["e16"].shape)
        E.copy_(ent["e16"])
        assert E.data_ptr() % 4 == 2 and E.is_contiguous()
    else:
        E = ent["e16"].to(dev)
    K = ent["K"]
    if ent.get("packed"):
        packed = torch.cat([cu(ent["t"], dev), cu(ent["w"], dev), cu(ent["m"], dev)], dim=1)
        T, Wt, M = packed[:, 0:K], packed[:, K:2 * K], packed[:, 2 * K:3 * K]
    else:
        T, Wt, M = cu(ent["t"], dev), cu(ent["w"], dev), cu(ent["m"], dev)
    kshape = op._affs_shape(E, K)
    T, ts = op._batch_strided(T, "target", torch.float32, kshape)
    Wt, ws = op._batch_strided(Wt, "weightmap", torch.float32, kshape)
    M, ms, mflag = op.mask_arg(M, kshape)
    d = op.make_desc(ent["spec"] if "spec" in ent else gm._spec2d(pkg, op, ent), E, ts, ws, ms, mflag)
    assert d.dtype == {None: 0, torch.float16: 1, torch.bfloat16: 2}[tdt]
    return dict(E=E, T=T, W=Wt, M=M, d=d, kshape=kshape,
                dl=None if ent["dloss"] is None else torch.tensor([ent["dloss"]], dtype=torch.float32, device=dev))


GUARD = 64  # elements on either side of an offset de


def run_table(pkg, op, dev, ents, tdt, fill=float("nan"), offset_view=False):
    """pea_affinity_fwd_multi + pea_affinity_bwd_multi through ctypes -> per entry (affs, g, loss_vec, de), the device entries, the
    workspace and (offset_view) the buffers that hold de between guard elements"""
    L = pkg._lib.lib()
    n = len(ents)
    dv = [device_entry(pkg, op, dev, ent, tdt, offset_view) for ent in ents]
    arr = (ctypes.POINTER(pkg._lib.PeaDesc) * n)(*[ctypes.pointer(x["d"]) for x in dv])
    assert L.pea_multi_supported(arr, n) == 1
    work, wsb = op.workspace(dev, dv[0]["d"], n)
    ft, bt = (pkg._lib.PeaMultiFwd * n)(), (pkg._lib.PeaMultiBwd * n)()
    outs, holders = [], []
    for j, x in enumerate(dv):
        affs = torch.full(x["kshape"], fill, dtype=torch.float32, device=dev) if ents[j]["want_affs"] else None
        g = torch.full(x["kshape"], fill, dtype=torch.float32, device=dev)
        lv = torch.full((1 + ents[j]["K"],), fill, dtype=torch.float32, device=dev)
        if offset_view:
            hold = torch.full((x["E"].numel() + 2 * GUARD + 1,), 7.0, dtype=x["E"].dtype, device=dev)
            de = hold[GUARD + 1:GUARD + 1 + x["E"].numel()].view(x["E"].shape)
            assert de.data_ptr() % 4 == 2
            holders.append(hold)
        else:
            de = torch.full_like(x["E"], fill)
        a, b = ft[j], bt[j]
        a.desc, a.e, a.target, a.weight = ctypes.pointer(x["d"]), x["E"].data_ptr(), x["T"].data_ptr(), x["W"].data_ptr()
        a.mask = None if x["M"] is None else x["M"].data_ptr()
        a.affs = None if affs is None else affs.data_ptr()
        a.g_out, a.loss_out = g.data_ptr(), lv.data_ptr()
        b.desc, b.e, b.g, b.de = ctypes.pointer(x["d"]), x["E"].data_ptr(), g.data_ptr(), de.data_ptr()
        b.dloss = None if x["dl"] is None else x["dl"].data_ptr()
        outs.append((affs, g, lv, de))
    rc = (L.pea_affinity_fwd_multi(ft, n, op._ptr(work), wsb, op._stream()), L.pea_affinity_bwd_multi(bt, n, op._stream()))
    torch.cuda.synchronize()
    assert rc == (0, 0), rc
    return outs, dv, work, holders


def check_against_oracle(j, ent, affs, g, lv, de, tdt):
    if affs is not None:
        assert np.abs(affs.cpu().numpy() - ent["o_affs"]).max() < AFFS_ATOL, j
    lv = lv.cpu().numpy().astype(np.float64)
    print("entry %d: loss %.9g oracle %.9g" % (j, lv[0], ent["o_loss"][0]))
    assert abs(lv[0] - ent["o_loss"][0]) <= LOSS_RTOL * abs(ent["o_loss"][0]), j
    assert np.all(np.abs(lv[1:] - ent["o_loss"][1:]) <= LOSS_RTOL * np.abs(ent["o_loss"][1:]) + 1e-30), j
    if g is not None:
        g_o, fac = expected_g(ent, ent["o_affs"])
        assert np.all(np.abs(g.cpu().numpy().astype(np.float64) - g_o) <= fac * AFFS_ATOL + 1e-6 * np.abs(g_o)), j
    assert de.dtype == tdt
    check_de(de, torch.from_numpy(ent["o_grad"]), torch.from_numpy(ent["e"]), ORACLE_RTOL, "entry %d de" % j)


# ----------------------------------------------------------------------------------------------------------------------------
# (1) the C ABI, tensor form
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 2, 1])
@pytest.mark.parametrize("tdt", DTYPES)
def test_c_abi_table_matches_oracle(pkg, op, dev, orc, synth, spy, tdt, n):
    table = tensor_table(pkg, orc, synth, tdt)
    outs, _, _, _ = run_table(pkg, op, dev, table[:n], tdt)
    assert spy.fwd == [0] and spy.bwd == [0]  # the fused launches ran
    for j, (affs, g, lv, de) in enumerate(outs):
        check_against_oracle(j, table[j], affs, g, lv, de, tdt)


# ----------------------------------------------------------------------------------------------------------------------------
# (2) the same arithmetic as the f32 instantiation
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", DTYPES)
def test_same_arithmetic_as_the_f32_calls_on_the_upcast(pkg, op, dev, orc, synth, tdt):
    table = tensor_table(pkg, orc, synth, tdt)
    o16, _, _, _ = run_table(pkg, op, dev, table, tdt)
    o32, _, _, _ = run_table(pkg, op, dev, table, None)
    differ = 0
    for j, ((a16, g16, l16, d16), (a32, g32, l32, d32)) in enumerate(zip(o16, o32)):
        assert (a16 is None and a32 is None) or torch.equal(a16, a32), j
        assert torch.equal(g16, g32) and torch.equal(l16, l32), j
        assert d32.dtype == torch.float32 and d16.dtype == tdt
        differ += one_ulp_rule(d16, d32)
    print("de16 != de32.to(%s) at %d elements of the table" % (tdt, differ))
    assert differ == 0  # one rounding of the f32 result and nothing else


# ----------------------------------------------------------------------------------------------------------------------------
# (3) 3D
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", DTYPES)
def test_c_abi_3d_norm1_table_matches_oracle(pkg, op, dev, orc, synth, tdt):
    Lm = pkg._lib
    cfg = [((5, 12, 20), 1, 0.5), ((4, 9, 11), 2, None), ((3, 6, 7), 1, 2.0), ((2, 4, 5), 1, None)]  # dims, shift, dloss
    ents = []
    for j, (dims, shift, dloss) in enumerate(cfg):
        shifts = [shift] * 3
        lam = [0.7, 1.0, 1.0]  # affs0_weight on loss0 (norm1)
        e, t, w = synth.synth_inputs_3d(2, 16, dims[0], dims[1], dims[2], orc.norm_offsets(shifts), 520 + j)
        e[:, :, 1, 1, 1] = 0.0
        e[:, :, 0, 0, 0] = 0.0
        e[:, 0, 0, 0, 0] = 1e-14
        e16, e = rounded(e, tdt)
        d = orc.desc_3d(e, shifts, lam)
        o_affs, o_loss = orc.c_fwd(d, e, None, t, w, None)
        o_grad, _ = orc.c_bwd(d, e, None, t, w, None, dloss=1.0 if dloss is None else dloss)
        spec = op.AffinitySpec(3, orc.norm_offsets(shifts), lam, Lm.BORDER_CROP_ZERO, Lm.NORM_CROPPED, 1e-12)
        ents.append(dict(e16=e16, e=e, t=t, w=w, m=None, ow=w, om=None, desc=d, K=3, want_affs=True, dloss=dloss, spec=spec, shift=shift,
                         o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    outs, _, _, _ = run_table(pkg, op, dev, ents, tdt, fill=7.0)
    for j, (affs, g, lv, de) in enumerate(outs):
        s = ents[j]["shift"]
        check_against_oracle(j, ents[j], affs, g, lv, de, tdt)
        affs, g = affs.cpu().numpy(), g.cpu().numpy()
        for x in (affs, g):  # the cropped border slices: exactly 0 in the map and in g (the buffers held 7.0)
            assert not x[:, 0, :s].any() and not x[:, 1, :, :s].any() and not x[:, 2, :, :, :s].any(), j
        assert g[:, 0, s:].any() and affs[:, 2, :, :, s:].any(), j


# ----------------------------------------------------------------------------------------------------------------------------
# (4) the labels-in form: the table of tests/test_gpu_multi_labels.py
# ----------------------------------------------------------------------------------------------------------------------------
def labels_table(pkg, orc, synth, dev, tdt):
    key = ("labels", tdt)
    if key in _TABLES:
        return _TABLES[key]
    mo = pkg.multi_offset
    shared = gl._plant(synth.synth_labels(3, (1, 74, 140), 901, cell=13)[:, 0])  # [3, 74, 140]: entries 0 and 1 sample it
    own2 = gl._plant(synth.synth_labels(2, (1, 17, 40), 902, cell=6)[:, 0])
    own3 = gl._plant(synth.synth_labels(2, (1, 5, 6), 903, cell=2)[:, 0])
    cfg = [  # (B, D, H, W, offsets, label image, step, affs wanted, dloss, lambda): tests/test_gpu_multi_labels.py
        (3, 16, 37, 70, mo([1, 3, 5, 9], 4), shared, (1, 2, 2), True, 0.625, None),
        (1, 16, 19, 33, mo([1, 3, 5], 4), shared, (1, 4, 4), False, None, None),
        (2, 32, 17, 40, mo([1, 3], 8), own2, (1, 1, 1), True, 1.75, [2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0]),
        (2, 16, 5, 6, [[-4, 0], [0, -5]], own3, (1, 1, 1), True, None, None),
    ]
    out = []
    for j, (B, D, H, W, offsets, lab, step, want_affs, dloss, lam) in enumerate(cfg):
        e16, e = rounded(gl._degenerate_pixels(synth.synth_embedding((B, D, H, W), 910 + j)), tdt)
        mat = gl._sample(lab[:B, None], (1, H, W), step)[:, 0]  # [B, H, W]: the label image this scale sees
        t, m, w = (x.cpu().numpy() for x in pkg.gen_targets(cu(mat.astype(np.int32), dev), offsets, padding=True))  # pea_gen_targets
        d = orc.desc_2d(e, offsets, lam)
        o_affs, o_loss = orc.c_fwd(d, e, None, t, w, m)
        o_grad, _ = orc.c_bwd(d, e, None, t, w, m, dloss=1.0 if dloss is None else dloss)
        out.append(dict(e16=e16, e=e, lab=lab, B=B, step=step, mat=mat, offsets=offsets, lam=lam, want_affs=want_affs, dloss=dloss,
                        K=len(offsets), w=w, t=t, m=m, ow=w, om=m, desc=d, o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    _TABLES[key] = out
    return out


def run_labels_table(pkg, op, dev, ents, flags, tdt, fill=float("nan"), wtabs=None, offset_view=False):
    """pea_affinity_fwd_bwd_labels_multi through ctypes -> per entry (affs, loss_vec, de), and the buffers that hold an offset de"""
    L = pkg._lib.lib()
    n = len(ents)
    cache, keep, outs, holders = {}, [], [], []
    tab = (pkg._lib.PeaMultiLabels * n)()
    first = None
    for j, ent in enumerate(ents):
        if offset_view:
            buf = torch.zeros(ent["e16"].numel() + 1, dtype=tdt, device=dev)
            E = buf[1:].view(ent["e16"].shape)
            E.copy_(ent["e16"])
            hold = torch.full((E.numel() + 2 * GUARD + 1,), 7.0, dtype=tdt, device=dev)
            de = hold[GUARD + 1:GUARD + 1 + E.numel()].view(E.shape)
            assert E.data_ptr() % 4 == 2 and de.data_ptr() % 4 == 2
            holders.append(hold)
        else:
            E = cu(ent["e"], dev) if tdt is None else ent["e16"].to(dev)  # (None: the f32 upcast)
            de = torch.full_like(E, fill)
        lab = cache.setdefault(id(ent["lab"]), cu(ent["lab"].astype(np.int32), dev))
        d = op.make_desc(ent["spec"] if "spec" in ent else gl._spec2d(pkg, op, ent), E)
        first = first or d
        kshape = op._affs_shape(E, ent["K"])
        affs = torch.full(kshape, fill, dtype=torch.float32, device=dev) if ent["want_affs"] else None
        lv = torch.full((1 + ent["K"],), fill, dtype=torch.float32, device=dev)
        dl = None if ent["dloss"] is None else torch.tensor([ent["dloss"]], dtype=torch.float32, device=dev)
        a = tab[j]
        a.desc, a.e, a.labels = ctypes.pointer(d), E.data_ptr(), lab.data_ptr()
        a.label_dims[:] = [1] * (4 - lab.dim()) + list(lab.shape[1:])
        a.label_step[:] = ent["step"]
        a.wtab = None if wtabs is None else wtabs[j].data_ptr()
        a.affs = None if affs is None else affs.data_ptr()
        a.loss_out, a.de = lv.data_ptr(), de.data_ptr()
        a.dloss = None if dl is None else dl.data_ptr()
        keep.append((E, d, dl))
        outs.append((affs, lv, de))
    assert L.pea_multi_labels_supported(tab, n, flags) == 1
    sb = L.pea_multi_labels_scratch_bytes(tab, n)
    scratch = torch.zeros((max(sb, 4),), dtype=torch.uint8, device=dev)
    work, wsb = op.workspace(dev, first, n)
    rc = L.pea_affinity_fwd_bwd_labels_multi(tab, n, flags, op._ptr(work), wsb, op._ptr(scratch), sb, op._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return outs, holders


@pytest.mark.parametrize("n", [4, 2, 1])
@pytest.mark.parametrize("tdt", DTYPES)
def test_labels_c_abi_table_matches_gen_targets_and_oracle(pkg, op, dev, orc, synth, spy, tdt, n):
    table = labels_table(pkg, orc, synth, dev, tdt)
    outs, _ = run_labels_table(pkg, op, dev, table[:n], FLAGS_2D, tdt)
    assert spy.labels == [0]
    for j, (affs, lv, de) in enumerate(outs):
        check_against_oracle(j, table[j], affs, None, lv, de, tdt)


@pytest.mark.parametrize("tdt", DTYPES)
def test_labels_table_computed_by_the_call_equals_a_given_one(pkg, op, dev, orc, synth, tdt):
    table = labels_table(pkg, orc, synth, dev, tdt)
    computed, _ = run_labels_table(pkg, op, dev, table, FLAGS_2D, tdt)
    tabs = gl._label_weight_tables(pkg, op, dev, table, FLAGS_2D)  # pea_label_weights on the materialised images (f32 descriptors)
    given, _ = run_labels_table(pkg, op, dev, table, FLAGS_2D, tdt, wtabs=tabs)
    for a, b in zip(computed, given):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)


# ----------------------------------------------------------------------------------------------------------------------------
# (5) 2-byte aligned, not 4-byte aligned
# ----------------------------------------------------------------------------------------------------------------------------
def _guards_untouched(holders):
    for hold in holders:
        assert (hold[:GUARD + 1] == 7.0).all() and (hold[-GUARD:] == 7.0).all()


@pytest.mark.parametrize("tdt", DTYPES)
def test_e_and_de_one_element_into_their_buffers(pkg, op, dev, orc, synth, tdt):
    """entries (1,16,19,33) and (2,16,5,6): S = 627 and 30, so every channel plane of the first starts at an odd element too"""
    table = tensor_table(pkg, orc, synth, tdt)
    ents = [table[1], table[3]]
    aligned, _, _, _ = run_table(pkg, op, dev, ents, tdt)
    shifted, _, _, holders = run_table(pkg, op, dev, ents, tdt, offset_view=True)
    _guards_untouched(holders)
    for a, b in zip(aligned, shifted):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    ltable = labels_table(pkg, orc, synth, dev, tdt)
    lents = [ltable[1], ltable[3]]
    aligned, _ = run_labels_table(pkg, op, dev, lents, FLAGS_2D, tdt)
    shifted, holders = run_labels_table(pkg, op, dev, lents, FLAGS_2D, tdt, offset_view=True)
    _guards_untouched(holders)
    for a, b in zip(aligned, shifted):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)


# ----------------------------------------------------------------------------------------------------------------------------
# (6) non-finite
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tensor", "labels"])
@pytest.mark.parametrize("tdt", DTYPES)
def test_one_nan_channel_spreads_exactly_where_it_is_read(pkg, op, dev, orc, synth, tdt, form):
    """entry 0, batch item 1, channel 3 of pixel (20, 40) (neither it nor a neighbour is a zero-norm pixel): de(r) reads e(r),
    e(r + o_i) and e(r - o_i) (circular), each through its norm, so de is NaN in all D channels at the pixel and at its 2K
    neighbours p -+ o_i, and nowhere else"""
    table = tensor_table(pkg, orc, synth, tdt) if form == "tensor" else labels_table(pkg, orc, synth, dev, tdt)
    run = (lambda ents: run_table(pkg, op, dev, ents, tdt)[0]) if form == "tensor" else \
          (lambda ents: run_labels_table(pkg, op, dev, ents, FLAGS_2D, tdt)[0])
    clean = run(table)
    b, c, y, x = 1, 3, 20, 40
    bad = dict(table[0])
    bad["e16"] = table[0]["e16"].clone()
    bad["e16"][b, c, y, x] = float("nan")
    dirty = run([bad] + table[1:])
    de = dirty[0][-1]
    H, W = de.shape[-2:]
    expect = torch.zeros(de.shape, dtype=torch.bool)
    expect[b, :, y, x] = True
    for oy, ox in table[0]["offsets"]:
        for s in (1, -1):
            expect[b, :, (y + s * oy) % H, (x + s * ox) % W] = True
    assert expect[b, 0].sum() == 1 + 2 * table[0]["K"]
    assert torch.equal(torch.isnan(de).cpu(), expect)
    assert not torch.isinf(de[expect.to(dev)]).any()  # no 16-bit store turned NaN into inf
    keep = ~expect.to(dev)
    assert torch.equal(de[keep], clean[0][-1][keep])
    for a, bb in zip(clean[1:], dirty[1:]):  # the other entries: bit-identical to the finite run
        for p, q in zip(a, bb):
            assert (p is None and q is None) or torch.equal(p, q)


# ----------------------------------------------------------------------------------------------------------------------------
# (7) reproducibility and state
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", DTYPES)
def test_reproducible_and_the_states_serve_a_single_f32_call(pkg, op, dev, orc, synth, tdt):
    table = tensor_table(pkg, orc, synth, tdt)
    first, _, work, _ = run_table(pkg, op, dev, table, tdt)
    second, _, work2, _ = run_table(pkg, op, dev, table, tdt)
    assert work.data_ptr() == work2.data_ptr()
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    lfirst, _ = run_labels_table(pkg, op, dev, labels_table(pkg, orc, synth, dev, tdt), FLAGS_2D, tdt)
    lsecond, _ = run_labels_table(pkg, op, dev, labels_table(pkg, orc, synth, dev, tdt), FLAGS_2D, tdt)
    for a, b in zip(lfirst, lsecond):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    # every state of the block, as the batched calls left it, serves a single f32 pea_affinity_fwd: its usual loss
    L = pkg._lib.lib()
    x = device_entry(pkg, op, dev, table[0], None)
    state = L.pea_workspace_bytes(ctypes.byref(x["d"]))

    def single(ws_ptr):
        lv = torch.empty(1 + table[0]["K"], dtype=torch.float32, device=dev)
        g = torch.empty(x["kshape"], dtype=torch.float32, device=dev)
        assert L.pea_affinity_fwd(ctypes.byref(x["d"]), op._ptr(x["E"]), None, op._ptr(x["T"]), op._ptr(x["W"]), op._ptr(x["M"]), None,
                                  op._ptr(g), op._ptr(lv), ctypes.c_void_p(ws_ptr), state, op._stream()) == 0
        torch.cuda.synchronize()
        return lv

    own, _ = op.workspace(dev, x["d"])
    usual = single(own.data_ptr())
    for i in range(4):
        assert torch.equal(single(work.data_ptr() + i * state), usual), i
    assert abs(float(usual[0]) - table[0]["o_loss"][0]) <= LOSS_RTOL * abs(table[0]["o_loss"][0])


# ----------------------------------------------------------------------------------------------------------------------------
# (8) the public layer
# ----------------------------------------------------------------------------------------------------------------------------
# powers of two: the multi and the single labels-in nodes both rescale a stored gradient in place, and two such chains may end two
# ulps apart; with these weights the comparison between them stays a comparison of one rounding each.  The second rounding itself
# is held to its bound by test_labels_multi_rescale_by_any_weight_stays_within_one_ulp.
WEIGHTS = [0.5, 1.0, 0.25, 2.0]


def _leaves(dev, table):
    return [ent["e16"].to(dev).requires_grad_(True) for ent in table]


def _compare_public(out, ref, xs, ys, tdt):
    for j, ((l, a, parts), (rl, ra, rparts)) in enumerate(zip(out, ref)):
        assert abs(l.item() - rl.item()) <= LOSS_RTOL * abs(rl.item()), j
        assert np.allclose(list(parts), list(rparts), rtol=LOSS_RTOL, atol=0), j
        assert a.shape == ra.shape and (a.numel() == 0 or float((a - ra).abs().max()) < AFFS_ATOL), j
        assert xs[j].grad.dtype == tdt and ys[j].grad.dtype == tdt
        check_de(xs[j].grad, ys[j].grad.float(), ys[j].detach().float(), KERNEL_RTOL, "entry %d grad" % j)


@pytest.mark.parametrize("tdt", DTYPES)
def test_embedding_loss_multi_equals_single_calls(pkg, dev, orc, synth, spy, tdt):
    table = tensor_table(pkg, orc, synth, tdt)
    crit = pkg.WeightedMSE()
    offs = [ent["offsets"] for ent in table]
    T, W, M = ([cu(ent[k], dev) for ent in table] for k in ("t", "w", "m"))
    xs, ys = _leaves(dev, table), _leaves(dev, table)
    out = pkg.embedding_loss_multi(xs, T, W, M, crit, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, WEIGHTS)).backward()
    assert spy.fwd == [0] and spy.bwd == [0]
    ref = [pkg.embedding_loss(y, t, w, m, crit, o) for y, t, w, m, o in zip(ys, T, W, M, offs)]
    sum(l * c for (l, _, _), c in zip(ref, WEIGHTS)).backward()
    assert spy.fwd == [0] and spy.bwd == [0]
    _compare_public(out, ref, xs, ys, tdt)


@pytest.mark.parametrize("tdt", DTYPES)
def test_embedding_loss_norm1_multi_equals_single_calls(pkg, dev, orc, synth, spy, tdt):
    crit = pkg.WeightedMSE()
    shapes = [(5, 12, 20), (4, 9, 11), (3, 6, 7), (2, 4, 5)]
    data = [synth.synth_inputs_3d(2, 16, z, y, x, orc.norm_offsets([1, 1, 1]), 620 + j) for j, (z, y, x) in enumerate(shapes)]
    xs = [cu(e, dev).to(tdt).requires_grad_(True) for e, _, _ in data]
    ys = [x.detach().clone().requires_grad_(True) for x in xs]
    T, W = [cu(t, dev) for _, t, _ in data], [cu(w, dev) for _, _, w in data]
    out = pkg.embedding_loss_norm1_multi(xs, T, W, crit, affs0_weight=0.7)
    sum(l * c for (l, _), c in zip(out, WEIGHTS)).backward()
    assert spy.fwd == [0] and spy.bwd == [0]
    ref = [pkg.embedding_loss_norm1(y, t, w, crit, affs0_weight=0.7) for y, t, w in zip(ys, T, W)]
    sum(l * c for (l, _), c in zip(ref, WEIGHTS)).backward()
    for j in range(4):
        assert abs(out[j][0].item() - ref[j][0].item()) <= LOSS_RTOL * abs(ref[j][0].item()), j
        assert float((out[j][1] - ref[j][1]).abs().max()) < AFFS_ATOL, j
        check_de(xs[j].grad, ys[j].grad.float(), ys[j].detach().float(), KERNEL_RTOL, "head %d grad" % j)


@pytest.mark.parametrize("tdt", DTYPES)
def test_embedding_loss_from_labels_multi_equals_single_calls(pkg, dev, orc, synth, spy, tdt):
    table = labels_table(pkg, orc, synth, dev, tdt)
    crit = pkg.WeightedMSE()
    offs = [ent["offsets"] for ent in table]
    labs = [cu(ent["mat"].astype(np.int32), dev) for ent in table]
    xs, ys = _leaves(dev, table), _leaves(dev, table)
    out = pkg.embedding_loss_from_labels_multi(xs, labs, crit, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, WEIGHTS)).backward()
    assert spy.labels == [0]
    ref = [pkg.embedding_loss_from_labels(y, lab, crit, o, need_affs=True) for y, lab, o in zip(ys, labs, offs)]
    sum(l * c for (l, _, _), c in zip(ref, WEIGHTS)).backward()
    assert spy.labels == [0]
    _compare_public(out, ref, xs, ys, tdt)


@pytest.mark.parametrize("tdt", DTYPES)
def test_labels_multi_rescale_by_any_weight_stays_within_one_ulp(pkg, dev, orc, synth, spy, tdt):
    """The labels-in node stores de for grad_output = 1 (one rounding) and rescales it in place in backward: a weight that is no power
    of two rounds a second time.  Against the same node on the f32 upcast (the same arithmetic, rounded never): s * round(de) lies
    less than one ulp from s * de, so the two roundings stay within one storage ulp of the f32 product rounded once."""
    table = labels_table(pkg, orc, synth, dev, tdt)
    crit = pkg.WeightedMSE()
    weights = [0.3, 1.0, 0.7, 1.9]
    offs = [ent["offsets"] for ent in table]
    labs = [cu(ent["mat"].astype(np.int32), dev) for ent in table]
    xs = _leaves(dev, table)
    ys = [x.detach().float().requires_grad_(True) for x in xs]
    for leaves in (xs, ys):
        out = pkg.embedding_loss_from_labels_multi(leaves, labs, crit, offs)
        sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.labels == [0, 0]
    for j, (x, y) in enumerate(zip(xs, ys)):
        assert x.grad.dtype == tdt and y.grad.dtype == torch.float32
        one_ulp_rule(x.grad, y.grad)
        reg = (y.detach().double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(y.grad)  # the regular pixels on their own
        n = one_ulp_rule(torch.where(reg, x.grad, torch.zeros_like(x.grad)), torch.where(reg, y.grad, torch.zeros_like(y.grad)))
        print("entry %d (weight %g): %d elements differ from the f32 product rounded once" % (j, weights[j], n))


@pytest.mark.parametrize("tdt", DTYPES)
def test_large_16_bit_table_runs_the_single_calls(pkg, op, dev, spy, tdt):
    """a 16-bit tensor-form table above affinity_op.MULTI16_MAX_TILES: nothing batched is launched (the single calls were measured
    to be faster there), the results are those of the single calls bit for bit; the same table in f32 is fused as before"""
    crit = pkg.WeightedMSE()
    offsets = pkg.multi_offset([1], 4)[:2]
    B = op.MULTI16_MAX_TILES // 289 + 1  # 272^2 = 289 tiles per batch item
    gen = torch.Generator(device=dev).manual_seed(7)
    e = torch.randn((B, 16, 272, 272), generator=gen, device=dev)
    t = (torch.rand((B, 2, 272, 272), generator=gen, device=dev) < 0.6).float()
    w = torch.rand((B, 2, 272, 272), generator=gen, device=dev) + 0.5

    def run(fn, x):
        x = x.detach().clone().requires_grad_(True)
        loss, affs, _ = fn(x)
        loss.backward()
        return loss.detach(), affs, x.grad

    multi = lambda x: pkg.embedding_loss_multi([x], [t], [w], [None], crit, [offsets], need_affs=True)[0]
    single = lambda x: pkg.embedding_loss(x, t, w, None, crit, offsets)
    out = run(multi, e.to(tdt))
    assert spy.fwd == [] and spy.bwd == []
    ref = run(single, e.to(tdt))
    assert out[2].dtype == tdt and all(torch.equal(a, b) for a, b in zip(out, ref))
    run(multi, e)
    assert spy.fwd == [0] and spy.bwd == [0]


def _cvppp_tensors(pkg, synth, dev, tdt, seed, offsets, nb_half, B=2, D=16, H=96, W=96):
    """the section inputs of tests/test_gpu_multi.py's graph test, the five embeddings and the EMA embedding in tdt"""
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, seed)
    ema = synth.synth_embedding((B, D, H, W), seed + 1)
    emds, downs = [], []
    for j in range(4):
        k = nb_half * (4 - j)
        ej, tj, wj, mj = synth.synth_inputs_2d(B, D, H >> (j + 1), W >> (j + 1), offsets[:k], seed + 2 + j)
        emds.append(ej)
        downs.append(np.concatenate([tj, wj, mj.astype(np.float32)], axis=1))
    return [cu(x, dev).to(tdt) for x in [e] + emds + [ema]] + [cu(t, dev), cu(w, dev), cu(m, dev)] + [cu(x, dev) for x in downs]


def _compare_sections(a, b, leaves, tdt):
    """(loss, pred, grads) of the batched and the unbatched section on the same 16-bit leaves"""
    assert abs(a[0] - b[0]) <= LOSS_RTOL * abs(b[0])
    assert float((a[1] - b[1]).abs().max()) < AFFS_ATOL
    for j, (x, y) in enumerate(zip(a[2], b[2])):
        assert x.dtype == tdt and y.dtype == tdt
        check_de(x, y.float(), leaves[j].detach().float(), KERNEL_RTOL, "leaf %d grad" % j)


@pytest.mark.parametrize("tdt", DTYPES)
def test_cvppp_loss_section_batched_equals_unbatched(pkg, dev, synth, spy, tdt):
    offsets, nb_half = pkg.multi_offset([1, 3, 5, 9, 27], 4), 2
    crit = pkg.WeightedMSE()
    bufs = _cvppp_tensors(pkg, synth, dev, tdt, 171, offsets, nb_half)

    def run(batched):
        leaves = [x.detach().clone().requires_grad_(True) for x in bufs[:5]]
        loss, pred, _ = pkg.cvppp_loss_section(leaves[0], leaves[1:], bufs[5], bufs[6], bufs[7], bufs[8], list(bufs[9:13]), crit, offsets,
                                               nb_half, batched=batched)
        loss.backward()
        return loss.item(), pred, [x.grad for x in leaves]

    ref = run(False)
    assert spy.fwd == [] and spy.bwd == []
    out = run(True)
    assert spy.fwd == [0] and spy.bwd == [0]  # the four 16-bit scales ran as one launch each way
    _compare_sections(out, ref, bufs[:5], tdt)


@pytest.mark.parametrize("tdt", DTYPES)
def test_ac3ac4_loss_section_batched_equals_unbatched(pkg, dev, spy, tdt):
    g = load_golden("gsection_ac3ac4_norm1")
    crit = pkg.WeightedMSE()
    embs = [cu(g["emb"], dev).to(tdt)] + [cu(g["emd%d" % j], dev).to(tdt) for j in range(1, 5)]
    ema, downs = cu(g["ema"], dev).to(tdt), [cu(g["down%d" % j], dev) for j in range(1, 5)]

    def run(batched):
        leaves = [x.detach().clone().requires_grad_(True) for x in embs]
        loss, pred = pkg.ac3ac4_loss_section(leaves[0], leaves[1:], ema, cu(g["target"], dev), cu(g["weight"], dev), downs, crit,
                                             embedding_mode=int(g["mode"]), affs0_weight=1, batched=batched)
        loss.backward()
        return loss.item(), pred, [x.grad for x in leaves]

    ref = run(False)
    assert spy.fwd == [] and spy.bwd == []
    out = run(True)
    assert spy.fwd == [0] and spy.bwd == [0]
    _compare_sections(out, ref, embs, tdt)


@pytest.mark.parametrize("tdt", DTYPES)
def test_graphed_batched_section_equals_eager(pkg, dev, synth, spy, tdt):
    """pea.graphed over a cvppp_loss_section(batched=True) step on 16-bit embeddings: the replay, also on refilled inputs, gives the
    eager step's total, map and gradients"""
    offsets, nb_half = pkg.multi_offset([1, 3, 5, 9, 27], 4), 2
    crit = pkg.WeightedMSE()

    def step(*bufs):
        leaves = list(bufs[:5])
        for x in leaves:
            x.grad = None
        loss, pred, _ = pkg.cvppp_loss_section(leaves[0], leaves[1:], bufs[5], bufs[6], bufs[7], bufs[8], list(bufs[9:13]), crit, offsets,
                                               nb_half, batched=True)
        pkg.backward(loss)
        return loss, pred, [x.grad for x in leaves]

    static = _cvppp_tensors(pkg, synth, dev, tdt, 171, offsets, nb_half)
    for x in static[:5]:
        x.requires_grad_(True)
    graph = pkg.graphed(step, *static)
    assert spy.fwd and set(spy.fwd) == {0} and set(spy.bwd) == {0}  # the capture enqueued the batched launches
    for seed in (171, 173):
        fresh = _cvppp_tensors(pkg, synth, dev, tdt, seed, offsets, nb_half)
        with torch.no_grad():
            for dst, src in zip(static, fresh):
                dst.copy_(src)
        loss, pred, grads = graph.replay()
        torch.cuda.synchronize()
        for x in fresh[:5]:
            x.requires_grad_(True)
        e_loss, e_pred, e_grads = step(*fresh)
        assert abs(loss.item() - e_loss.item()) <= 1e-6 * abs(e_loss.item()), seed
        assert torch.equal(pred, e_pred), seed
        for a, b in zip(grads, e_grads):
            assert a.dtype == tdt and torch.equal(a, b), seed
