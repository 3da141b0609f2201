"""CPU: the binary cross-entropy form of the loss on the activated map (PEA_FLAG_LOSS_BCE) at the C ABI, and the criterion classes of
loss/loss.py; no compute calls here."""
import ctypes
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import golden_names, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELU, ONE_MINUS, HALF, CLAMP, MASK_F32, LOSS_ACT, LOSS_BCE = 1, 2, 4, 8, 32, 64, 128
OK, E_NULL, E_DESC, E_UNSUPPORTED = 0, -1, -2, -3
NORM5 = [1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _desc(pkg, D=16, H=544, W=544, offs=None, dtype=0, border=0, B=8, flags=0):
    d = pkg._lib.PeaDesc()
    offs = offs if offs is not None else pkg.multi_offset([1, 3, 5, 9, 27], 4)
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, B, D, len(offs)
    d.dims[:] = [1, H, W]
    d.border, d.dtype, d.norm, d.eps, d.flags = border, dtype, 2, 1e-6, flags
    for i, o in enumerate(offs):
        d.offsets[i][:] = [0] * (3 - len(o)) + list(o)
        d.lam[i] = 1.0
    return d


def _desc3d(pkg, flags=0):
    """the window of the fused 3D inference (tests/test_infer_stitch_host.py)"""
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 3, 1, 16, len(NORM5)
    d.dims[:] = [18, 160, 160]
    d.border, d.dtype, d.norm, d.eps, d.flags = 1, 0, 1, 1e-12, flags
    for i, s in enumerate(NORM5):
        o = [0, 0, 0]
        o[i % 3] = -s
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    return d


def test_flag_value(pkg):
    src = open(os.path.join(ROOT, "include", "pea.h")).read()
    m = re.search(r"#define\s+PEA_FLAG_LOSS_BCE\s+(\S+)", src)
    assert m and m.group(1) == "128u"
    assert pkg._lib.FLAG_LOSS_BCE == LOSS_BCE
    assert re.search(r"#define\s+PEA_ABI_VERSION\s+2\b", src) and pkg._lib.PEA_ABI_VERSION == 2  # (the flag does not bump the ABI)
    assert ctypes.sizeof(pkg._lib.PeaDesc) == 592  # PeaDesc is unchanged


@pytest.mark.parametrize("extra", [0, HALF, MASK_F32, HALF | MASK_F32])
def test_validate_accepts_bce_on_the_clamped_map(pkg, lib, extra):
    d = _desc(pkg, flags=LOSS_BCE | LOSS_ACT | CLAMP | extra)
    assert lib.pea_desc_validate(ctypes.byref(d)) == OK
    assert lib.pea_workspace_bytes(ctypes.byref(d)) > 0


@pytest.mark.parametrize("flags", [LOSS_BCE,                                  # alone (the parent commit ignored bit 128: this was PEA_OK)
                                   LOSS_BCE | CLAMP, LOSS_BCE | HALF | CLAMP,  # the activation bits without LOSS_ACT
                                   LOSS_BCE | LOSS_ACT | HALF,                 # LOSS_ACT without the clamp
                                   LOSS_BCE | LOSS_ACT,
                                   LOSS_BCE | LOSS_ACT | CLAMP | RELU, LOSS_BCE | LOSS_ACT | CLAMP | ONE_MINUS,
                                   LOSS_BCE | LOSS_ACT | HALF | CLAMP | RELU | ONE_MINUS, LOSS_BCE | MASK_F32])
def test_validate_refuses_every_other_combination(pkg, lib, flags):
    """PEA_E_DESC from pea_desc_validate and from every entry point"""
    d = _desc(pkg, flags=flags)
    n = None
    assert lib.pea_desc_validate(ctypes.byref(d)) == E_DESC
    assert lib.pea_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.pea_affinity_infer(ctypes.byref(d), n, n, n, n) == E_DESC
    assert lib.pea_affinity_fwd(ctypes.byref(d), n, n, n, n, n, n, n, n, n, ctypes.c_size_t(0), n) == E_DESC
    assert lib.pea_affinity_fwd_ex(ctypes.byref(d), n, n, n, n, n, n, n, n, n, n, ctypes.c_size_t(0), n) == E_DESC
    assert lib.pea_affinity_bwd(ctypes.byref(d), n, n, n, n, n, n, n) == E_DESC
    assert lib.pea_affinity_bwd_ex2(ctypes.byref(d), n, n, n, n, n, n, n, n, n) == E_DESC
    assert lib.pea_inv_norm(ctypes.byref(d), n, n, n) == E_DESC
    good = _desc(pkg)
    assert lib.pea_affinity_fwd_dual_ex(ctypes.byref(d), ctypes.byref(good), *([n] * 14), ctypes.c_size_t(0), n) == E_DESC
    assert lib.pea_affinity_fwd_dual_ex(ctypes.byref(good), ctypes.byref(d), *([n] * 14), ctypes.c_size_t(0), n) == E_DESC
    assert lib.pea_affinity_fwd_bwd_labels(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n) == E_DESC
    for mode in range(6):
        assert lib.pea_cross_supported(ctypes.byref(d), mode) == 0


@pytest.mark.parametrize("act", [CLAMP, HALF | CLAMP])
def test_entry_points_without_the_form_refuse_a_valid_bce_descriptor(pkg, lib, act):
    """they have no PEA_FLAG_LOSS_ACT form, so they refuse the criterion with it: PEA_E_UNSUPPORTED with every pointer NULL"""
    d, plain = _desc(pkg, flags=LOSS_BCE | LOSS_ACT | act), _desc(pkg, flags=act)
    n = None
    assert lib.pea_cross_supported(ctypes.byref(plain), 5) == 1 and lib.pea_cross_supported(ctypes.byref(d), 5) == 0
    for a, b in ((d, plain), (plain, d), (d, d)):
        assert lib.pea_affinity_fwd_dual_ex(ctypes.byref(a), ctypes.byref(b), *([n] * 14), ctypes.c_size_t(0), n) == E_UNSUPPORTED
        assert lib.pea_affinity_fwd_bwd_labels_dual(ctypes.byref(a), ctypes.byref(b), n, n, n, n, 0, n, n, n, n, n, n, n,
                                                    ctypes.c_size_t(0), n) == E_UNSUPPORTED
    assert lib.pea_affinity_fwd_bwd_labels(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n) == E_UNSUPPORTED
    assert lib.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n,
                                              ctypes.c_size_t(0), n) == E_UNSUPPORTED
    # the batched self losses
    PD = pkg._lib.PeaDesc
    small, small_bce = _desc(pkg, H=136, W=136, B=2), _desc(pkg, H=136, W=136, B=2, flags=LOSS_BCE | LOSS_ACT | act)
    table = lambda *ds: (ctypes.POINTER(PD) * len(ds))(*[ctypes.pointer(x) for x in ds])
    assert lib.pea_multi_supported(table(small), 1) == 1
    assert lib.pea_multi_supported(table(small_bce), 1) == 0
    assert lib.pea_multi_supported(table(small, small_bce), 2) == 0
    # the fused 3D window inference
    assert lib.pea_infer_stitch_supported(ctypes.byref(_desc3d(pkg)), 1) == 1
    assert lib.pea_infer_stitch_supported(ctypes.byref(_desc3d(pkg, flags=LOSS_BCE | LOSS_ACT | act)), 1) == 0
    # the tensor forward takes the descriptor as far as its pointer check; inference and backward ignore the bit
    assert lib.pea_affinity_fwd_ex(ctypes.byref(d), n, n, n, n, n, n, n, n, n, n, ctypes.c_size_t(0), n) == E_NULL
    assert lib.pea_affinity_infer(ctypes.byref(d), n, n, n, n) == E_NULL
    assert lib.pea_affinity_bwd(ctypes.byref(d), n, n, n, n, n, n, n) == E_NULL


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_support_questions_ignore_the_bit(pkg, lib, mode):
    """pea_cross_supported (which kernels, whether to allocate the 1 / norm planes) answers as for LOSS_ACT alone"""
    cv = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    for kw in (dict(D=16), dict(D=32), dict(D=64, offs=cv[:8]), dict(D=16, border=1), dict(D=16, offs=pkg.multi_offset([1, 3, 9], 8))):
        for act in (CLAMP, HALF | CLAMP):
            a = lib.pea_cross_supported(ctypes.byref(_desc(pkg, flags=act | LOSS_ACT, **kw)), mode)
            b = lib.pea_cross_supported(ctypes.byref(_desc(pkg, flags=act | LOSS_ACT | LOSS_BCE, **kw)), mode)
            assert a == b, (mode, kw, act)


# ---- the criterion classes ----------------------------------------------------------------------------------------------------------

def _pred_target_weight(seed=3):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(2, 5, 7, generator=g)
    pred[0, 0, 0], pred[0, 0, 1] = 0.0, 1.0  # the clamped logs
    target = (torch.rand(2, 5, 7, generator=g) < 0.5).float()
    weight = torch.rand(2, 5, 7, generator=g) * 3
    return pred, target, weight


def test_criteria_called_directly_equal_torch(pkg):
    pred, target, weight = _pred_target_weight()
    assert torch.equal(pkg.WeightedBCE()(pred, target, weight), F.binary_cross_entropy(pred, target, weight))
    assert torch.equal(pkg.WeightedBCE()(pred, target), F.binary_cross_entropy(pred, target))
    assert torch.equal(pkg.WeightedBCE(size_average=False, reduce=False)(pred, target, weight), F.binary_cross_entropy(pred, target, weight))
    assert torch.equal(pkg.BCELoss()(pred, target, weight), F.binary_cross_entropy(pred, target))   # the weight is ignored
    assert torch.equal(pkg.BCELoss()(pred, target), F.binary_cross_entropy(pred, target))
    assert torch.equal(pkg.MSELoss()(pred, target, weight), F.mse_loss(pred, target))
    assert torch.equal(pkg.MSELoss()(pred, target), F.mse_loss(pred, target))
    x = pred.clone().clamp(0.1, 0.9).requires_grad_(True)
    pkg.WeightedBCE()(x, target, weight).backward()
    y = x.detach().clone().requires_grad_(True)
    F.binary_cross_entropy(y, target, weight).backward()
    assert torch.equal(x.grad, y.grad)


def test_criterion_attributes(pkg):
    loss = importlib.import_module(pkg.__name__ + ".loss.loss")
    kinds = {"WeightedMSE": "wmse", "MSELoss": "mse", "BCELoss": "bce", "WeightedBCE": "wbce"}
    for name, kind in kinds.items():
        cls = getattr(loss, name)
        assert getattr(pkg, name) is cls and name in pkg.__all__
        assert cls.pea_criterion == kind and cls().pea_criterion == kind
        assert isinstance(cls(), torch.nn.Module)
    # only WeightedMSE is what the loss sections, head_embedding_loss and the multi / labels paths fuse
    assert loss.WeightedMSE.pea_fused is True
    for name in ("MSELoss", "BCELoss", "WeightedBCE"):
        assert not hasattr(getattr(loss, name), "pea_fused") and not hasattr(getattr(loss, name)(), "pea_fused")
    act = importlib.import_module(pkg.__name__ + ".loss._activated")
    assert [act.criterion_kind(getattr(loss, n)()) for n in kinds] == list(kinds.values())
    assert act.criterion_kind(lambda a, b, w: a) is None and act.criterion_kind(torch.nn.BCELoss()) is None


def test_weighted_mse_is_unchanged(pkg):
    pred, target, weight = _pred_target_weight(5)
    crit = pkg.WeightedMSE()
    n = pred.shape[0] * pred.shape[2]  # the reference's normaliser: B * prod(size()[2:])
    assert crit.norm_term(pred) == float(n)
    assert torch.equal(crit(pred, target, weight), torch.sum(weight * (pred - target) ** 2) / float(n))
    assert torch.equal(crit(pred, target), torch.sum((pred - target) ** 2) / float(n))
    assert list(crit.parameters()) == [] and list(pkg.WeightedBCE().parameters()) == []


def test_ones_weight_is_cached_per_device_and_shape(pkg):
    act = importlib.import_module(pkg.__name__ + ".loss._activated")
    a, b = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 6)
    wa = act.ones_weight(a)
    assert wa is act.ones_weight(torch.ones(2, 3, 4, 5)) and wa is not act.ones_weight(b)
    assert wa.shape == a.shape and wa.dtype == torch.float32 and bool((wa == 1).all())


@pytest.mark.parametrize("module", ["loss_embedding", "loss_embedding_exp", "loss_embedding_norm"])
def test_cpu_tensors_raise(pkg, module):
    """no CPU fallback for the new criteria either"""
    mod = getattr(pkg, module)
    offs = pkg.multi_offset([1, 3], 4)
    e = torch.randn(1, 16, 32, 32, requires_grad=True)
    t = torch.zeros(1, len(offs), 32, 32)
    for crit in (pkg.WeightedBCE(), pkg.BCELoss(), pkg.MSELoss()):
        with pytest.raises(RuntimeError):
            mod.embedding_loss(e, t, t + 1, t + 1, crit, offs)
    with pytest.raises(RuntimeError):
        pkg.embedding_loss(e, t, t + 1, t + 1, pkg.MSELoss(), offs)


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------

GBCE = golden_names("gbce_")


def test_fixtures_present():
    gs = [load_golden(n) for n in GBCE]
    assert len(gs) >= 10
    assert {str(g["criterion"]) for g in gs} == {"WeightedBCE", "BCELoss", "MSELoss"}
    assert {str(g["module"]) for g in gs} == {"loss_embedding", "loss_embedding_exp", "loss_embedding_norm", "loss_embedding_mse"}
    assert any("ema" in g for g in gs) and any(str(g["mode"]) == "l2" for g in gs) and any(g["mask"].dtype == "float32" for g in gs)
    assert any(float(g["affs0_weight"]) != 1 for g in gs)
    for g in gs:
        if str(g["module"]) == "loss_embedding_mse":
            assert str(g["criterion"]) == "MSELoss"   # BCE on the raw cosine is not meaningful
        if g["mask"].dtype == "float32":
            assert set(map(float, set(g["mask"].ravel().tolist()))) <= {0.0, 1.0}
