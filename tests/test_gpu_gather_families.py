"""GPU (-m gpu): the gather-form kernel families carry each other's bits (csrc/pea_gather.h).

The direct kernels (csrc/pea_direct.h, taken under PEA_FORCE_DIRECT=1), the batched tensor form (csrc/pea_k_multi.hip) and the batched
labels-in form (csrc/pea_k_multi_labels.hip) compose the same per-pixel blocks, so on the same tensors

  1. affs, g and de of a single forced-direct self loss equal those of a one-entry pea_affinity_fwd_multi / pea_affinity_bwd_multi table;
  2. affs and de of pea_affinity_fwd_bwd_labels_multi equal those of the tensor-form table fed with pea_gen_targets' output for the
     same labels (class-balance table computed by the call, or given by pea_label_weights)

bit for bit (torch.equal).  The loss rows are compared at LOSS_RTOL of tests/test_gpu_parity.py: the families sum the per-tile loss
partials in different orders on purpose.  One pair is not bit-equal by construction, and was not before the blocks were shared: the
f16 `de` of k_bwd_direct against the batched kernels.  The two families store f16 through different policies on purpose, at every D,
so their values are equal or adjacent f16 numbers: every f16 case of (1) is held to that (f16_store_rule below), not to equality.

Shapes: the smallest at which these bodies can go wrong.  2D CIRCULAR, B = 2, D = 16 and 32, 19 x 23 (S = 437: two tiles per item,
the second ragged), offsets (0,-1), (-3,0), (2,5), (-18,22) -- the last wraps on both axes at |o| = dim - 1 --, storage f32 / f16 /
bf16, mask none / u8 / f32.  3D CROP_ZERO, B = 2, D = 16, 5 x 9 x 11 (S = 495), shifts 1, 1, 1 and a z step of -4; the cropped border
slices are exactly 0.  The labels form samples a 38 x 46 label image with step 2 and one of the embedding's own size with step 1.
Every embedding holds zero-norm pixels and one of norm 1e-14 (the clamp branch of F.normalize).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_multi as gm
import test_gpu_multi16 as m16
import test_gpu_multi_labels as gl
from test_gpu_parity import LOSS_RTOL

pytestmark = pytest.mark.gpu

dev, synth, op = m16.dev, m16.synth, m16.op  # module-scoped fixtures
cu = gm.cu

STORAGE = [pytest.param(None, id="f32"), pytest.param(torch.float16, id="f16"), pytest.param(torch.bfloat16, id="bf16")]
OFFS_2D = [[0, -1], [-3, 0], [2, 5], [-18, 22]]
OFFS_3D = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-4, 0, 0]]
LAM = [0.7, 1.0, 2.0, 1.0]
DIMS_2D, DIMS_3D = (19, 23), (5, 9, 11)


def spec_of(pkg, op, ndim, border=None, offsets=None):
    L = pkg._lib
    if ndim == 2:
        return op.AffinitySpec(2, offsets or OFFS_2D, LAM, L.BORDER_CIRCULAR if border is None else border, L.NORM_BX, 1e-12)
    return op.AffinitySpec(3, offsets or OFFS_3D, LAM, L.BORDER_CROP_ZERO if border is None else border, L.NORM_CROPPED, 1e-12)


def embedding(synth, shape, seed, tdt):
    """-> (the embedding in its storage type or None for f32, its exact f32 value): zero-norm pixels and one of norm 1e-14"""
    e = synth.synth_embedding(shape, seed)
    mid = tuple(n // 2 for n in shape[2:])
    e[(slice(None), slice(None)) + (0,) * len(mid)] = 0.0
    e[(slice(None), slice(None)) + tuple(n - 1 for n in shape[2:])] = 0.0
    e[(slice(None), slice(None)) + mid] = 0.0
    e[(slice(None), 0) + mid] = 1e-14
    return (None, e) if tdt is None else m16.rounded(e, tdt)


def entry_2d(pkg, op, synth, D, mkind, tdt):
    H, W = DIMS_2D
    _, t, w, m8 = synth.synth_inputs_2d(2, D, H, W, OFFS_2D, 1300 + D)
    e16, e = embedding(synth, (2, D, H, W), 1310 + D, tdt)
    m = {"none": None, "u8": m8, "f32": gm._frac_mask(synth, t.shape, 77)}[mkind]
    return dict(e16=e16, e=e, t=t, w=w, m=m, K=4, want_affs=True, dloss=0.625, spec=spec_of(pkg, op, 2))


def entry_3d(pkg, op, synth, tdt, border=None):
    Z, Y, X = DIMS_3D
    _, t, w = synth.synth_inputs_3d(2, 16, Z, Y, X, OFFS_3D, 1400)
    e16, e = embedding(synth, (2, 16, Z, Y, X), 1410, tdt)
    return dict(e16=e16, e=e, t=t, w=w, m=None, K=4, want_affs=True, dloss=1.75, spec=spec_of(pkg, op, 3, border))


def run_single(pkg, op, dev, ent, tdt, other=None, fill=float("nan")):
    """pea_affinity_fwd + pea_affinity_bwd through ctypes (the caller sets PEA_FORCE_DIRECT) -> (affs, g, loss_vec, de[, de_other])"""
    L = pkg._lib.lib()
    x = m16.device_entry(pkg, op, dev, ent, tdt)
    E, d = x["E"], x["d"]
    O = None if other is None else (cu(other, dev) if tdt is None else cu(other, dev).to(tdt))
    affs, g = (torch.full(x["kshape"], fill, dtype=torch.float32, device=dev) for _ in range(2))
    lv = torch.full((1 + ent["K"],), fill, dtype=torch.float32, device=dev)
    de = torch.full_like(E, fill)
    de_o = None if O is None else torch.full_like(E, fill)
    work, wsb = op.workspace(dev, d)
    rc = L.pea_affinity_fwd(ctypes.byref(d), op._ptr(E), op._ptr(O), op._ptr(x["T"]), op._ptr(x["W"]), op._ptr(x["M"]), op._ptr(affs),
                            op._ptr(g), op._ptr(lv), op._ptr(work), wsb, op._stream())
    assert rc == 0, rc
    rc = L.pea_affinity_bwd(ctypes.byref(d), op._ptr(E), op._ptr(O), op._ptr(g), op._ptr(x["dl"]), op._ptr(de), op._ptr(de_o), op._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return (affs, g, lv, de) + (() if O is None else (de_o,))


def same_loss(lv, ref):
    lv, ref = lv.double().cpu().numpy(), ref.double().cpu().numpy()
    print("loss rows", lv, ref)
    return np.all(np.abs(lv - ref) <= LOSS_RTOL * np.abs(ref) + 1e-30)


def assert_direct_equals_one_entry_table(pkg, op, dev, monkeypatch, ent, tdt, fill=float("nan")):
    (m_affs, m_g, m_lv, m_de), = m16.run_table(pkg, op, dev, [ent], tdt, fill=fill)[0]
    monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
    s_affs, s_g, s_lv, s_de = run_single(pkg, op, dev, ent, tdt, fill=fill)
    assert torch.isfinite(s_affs).all() and torch.isfinite(s_g).all() and s_g.abs().max() > 0
    assert torch.equal(s_affs, m_affs)
    assert torch.equal(s_g, m_g)
    assert same_loss(m_lv, s_lv)
    assert s_de.dtype == m_de.dtype and s_de.float().abs().max() > 0
    if tdt is torch.float16:  # two store policies: equal or adjacent f16 values
        f16_store_rule(s_de, m_de)
    else:
        assert torch.equal(s_de, m_de)
    return s_affs, s_g


F16_GRAD_RTOL = 2e-3  # tests/test_gpu_parity.py: "f16 rounding of the stored gradient"


def f16_store_rule(s_de, m_de):
    """The f16 `de` of k_bwd_direct against that of the batched kernels: equal or adjacent f16 values, by the two store policies
    (and so it was before the blocks were shared).  The f32 value in front of the store is the same; the store is not, on purpose
    (project_store<ROUNDED> of csrc/pea_gather.h): the batched kernels round the finished f32 product to f16, in k_bwd_direct the
    compiler fuses the last multiply into the conversion (v_fma_mixlo_f16, at every D), which rounds the exact product once.  That
    depends on the storage type alone: where a case happens to come out bit-equal, no value landed on a tie.  Both are roundings of numbers
    half an f32 ulp apart, so the results are equal or adjacent f16 values: held to that, and to the f16 gradient tolerance of
    tests/test_gpu_parity.py over the finite elements (a clamp-branch pixel carries G / eps: inf in f16).  On an MI355X 0 to 3 of the
    14 to 28 thousand elements of a case differ, each by one ulp."""
    assert s_de.dtype == torch.float16
    d = (m16._mono(s_de) - m16._mono(m_de)).abs()
    print("f16 de: %d of %d elements differ, by at most %d ulp" % (int((d > 0).sum()), d.numel(), int(d.max())))
    assert int(d.max()) <= 1
    fin = torch.isfinite(s_de) & torch.isfinite(m_de)
    s, m = s_de.float()[fin], m_de.float()[fin]
    assert float((s - m).abs().max()) <= F16_GRAD_RTOL * float(m.abs().max())


# ----------------------------------------------------------------------------------------------------------------------------
# (1) the direct kernels against a one-entry table of the batched tensor form
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mkind", ["none", "u8", "f32"])
@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("tdt", STORAGE)
def test_direct_self_loss_equals_one_entry_table_2d(pkg, op, dev, synth, monkeypatch, tdt, D, mkind):
    assert_direct_equals_one_entry_table(pkg, op, dev, monkeypatch, entry_2d(pkg, op, synth, D, mkind, tdt), tdt)


@pytest.mark.parametrize("tdt", STORAGE)
def test_direct_self_loss_equals_one_entry_table_3d_crop(pkg, op, dev, synth, monkeypatch, tdt):
    affs, g = assert_direct_equals_one_entry_table(pkg, op, dev, monkeypatch, entry_3d(pkg, op, synth, tdt), tdt, fill=7.0)
    for x in (affs, g):  # the cropped border slices: exactly 0 (the buffers held 7.0)
        assert not x[:, 0, :1].any() and not x[:, 1, :, :1].any() and not x[:, 2, :, :, :1].any() and not x[:, 3, :4].any()
        assert x[:, 0, 1:].any() and x[:, 3, 4:].any()


# ----------------------------------------------------------------------------------------------------------------------------
# (2) the labels-in form against the tensor form on pea_gen_targets' output
# ----------------------------------------------------------------------------------------------------------------------------
def labels_pair(pkg, op, synth, dev, case, D, tdt):
    """-> (entry of the labels-in table, entry of the tensor-form table on what pea_gen_targets makes of the same labels, flags)"""
    if case == "3d":
        dims, offsets, flags, step = DIMS_3D, OFFS_3D, gl.FLAGS_3D, (1, 1, 1)
        lab = synth.synth_labels(2, dims, 1500, cell=3)
        mat = lab
        kw = dict(padding=False, both_foreground=True, want_mask=False)
    else:
        dims, offsets, flags = DIMS_2D, OFFS_2D, gl.FLAGS_2D
        step = (1, 2, 2) if case == "2d_step2" else (1, 1, 1)
        lab = gl._plant(synth.synth_labels(2, (1, dims[0] * step[1], dims[1] * step[2]), 1501, cell=7)[:, 0])
        mat = gl._sample(lab[:, None], (1,) + dims, step)[:, 0]
        kw = dict(padding=True)
    t, m, w = (None if x is None else x.cpu().numpy() for x in pkg.gen_targets(cu(mat.astype(np.int32), dev), offsets, **kw))
    e16, e = embedding(synth, (2, D) + dims, 1510 + D, tdt)
    common = dict(e16=e16, e=e, K=4, B=2, want_affs=True, dloss=0.625, spec=spec_of(pkg, op, len(dims)))
    return dict(common, lab=lab, mat=mat, step=step), dict(common, t=t, w=w, m=m), flags


@pytest.mark.parametrize("given", [False, True], ids=["counted", "wtab"])
@pytest.mark.parametrize("case,D", [("2d_step2", 16), ("2d_step2", 32), ("2d_step1", 16), ("2d_step1", 32), ("3d", 16)])
@pytest.mark.parametrize("tdt", STORAGE)
def test_labels_form_equals_tensor_form_on_generated_targets(pkg, op, dev, synth, tdt, case, D, given):
    lab_ent, ten_ent, flags = labels_pair(pkg, op, synth, dev, case, D, tdt)
    wtabs = gl._label_weight_tables(pkg, op, dev, [lab_ent], flags) if given else None
    (l_affs, l_lv, l_de), = m16.run_labels_table(pkg, op, dev, [lab_ent], flags, tdt, wtabs=wtabs)[0]
    (t_affs, _, t_lv, t_de), = m16.run_table(pkg, op, dev, [ten_ent], tdt)[0]
    assert torch.isfinite(t_affs).all() and t_de.float().abs().max() > 0
    assert torch.equal(l_affs, t_affs)
    assert same_loss(l_lv, t_lv)
    assert l_de.dtype == t_de.dtype
    assert torch.equal(l_de, t_de)
