"""CPU: the loss on the activated map (PEA_FLAG_LOSS_ACT) at the C ABI and in the Python layer; no compute calls here."""
import ctypes
import importlib
import inspect
import os
import re

import pytest
import torch

from conftest import golden_names, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_ACT, HALF, CLAMP, RELU, ONE_MINUS, MASK_F32 = 64, 4, 8, 1, 2, 32
E_DESC, E_UNSUPPORTED, E_NULL = -2, -3, -1


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _desc(pkg, D=16, H=544, W=544, offs=None, dtype=0, border=0, B=8, flags=0):
    d = pkg._lib.PeaDesc()
    offs = offs if offs is not None else pkg.multi_offset([1, 3, 5, 9, 27], 4)
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, B, D, len(offs)
    d.dims[:] = [1, H, W]
    d.border, d.dtype, d.norm, d.eps, d.flags = border, dtype, 0, 1e-6, flags
    for i, o in enumerate(offs):
        d.offsets[i][:] = [0] * (3 - len(o)) + list(o)
        d.lam[i] = 1.0
    return d


def test_flag_value(pkg):
    src = open(os.path.join(ROOT, "include", "pea.h")).read()
    m = re.search(r"#define\s+PEA_FLAG_LOSS_ACT\s+(\S+)", src)
    assert m and m.group(1) == "64u"
    assert pkg._lib.FLAG_LOSS_ACT == LOSS_ACT
    assert re.search(r"#define\s+PEA_ABI_VERSION\s+2\b", src) and pkg._lib.PEA_ABI_VERSION == 2  # (the flag does not bump the ABI)
    for f in ("loss_embedding.py", "loss_embedding_exp.py", "loss_embedding_norm.py"):  # the header cites the three reference modules
        assert f in src


@pytest.mark.parametrize("act", [HALF, CLAMP, HALF | CLAMP])
def test_validate_accepts_the_valid_combinations(pkg, lib, act):
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, flags=LOSS_ACT | act))) == 0
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, flags=LOSS_ACT | act | MASK_F32))) == 0
    assert lib.pea_workspace_bytes(ctypes.byref(_desc(pkg, flags=LOSS_ACT | act))) > 0


@pytest.mark.parametrize("act", [0, RELU, ONE_MINUS, RELU | ONE_MINUS, HALF | RELU, CLAMP | ONE_MINUS, HALF | CLAMP | RELU, MASK_F32])
def test_validate_refuses_the_invalid_combinations(pkg, lib, act):
    """LOSS_ACT with no activation bit, or with RELU_AFFS / ONE_MINUS: PEA_E_DESC from pea_desc_validate and from every entry point"""
    d = _desc(pkg, flags=LOSS_ACT | act)
    n = None
    assert lib.pea_desc_validate(ctypes.byref(d)) == E_DESC
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, flags=act))) == 0  # (the same bits without the flag are fine)
    assert lib.pea_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.pea_affinity_infer(ctypes.byref(d), n, n, n, n) == E_DESC
    assert lib.pea_affinity_fwd(ctypes.byref(d), n, n, n, n, n, n, n, n, n, ctypes.c_size_t(0), n) == E_DESC
    assert lib.pea_affinity_fwd_ex(ctypes.byref(d), n, n, n, n, n, n, n, n, n, n, ctypes.c_size_t(0), n) == E_DESC
    assert lib.pea_affinity_bwd(ctypes.byref(d), n, n, n, n, n, n, n) == E_DESC
    assert lib.pea_affinity_bwd_ex2(ctypes.byref(d), n, n, n, n, n, n, n, n, n) == E_DESC
    assert lib.pea_inv_norm(ctypes.byref(d), n, n, n) == E_DESC
    for mode in range(6):
        assert lib.pea_cross_supported(ctypes.byref(d), mode) == 0


@pytest.mark.parametrize("act", [HALF, CLAMP, HALF | CLAMP])
def test_entry_points_without_the_form_decline_before_any_pointer(pkg, lib, act):
    """the one-launch pair and the three labels-in calls: PEA_E_UNSUPPORTED with every pointer NULL (nothing is looked at, nothing launched)"""
    d, plain = _desc(pkg, flags=LOSS_ACT | act), _desc(pkg, flags=act)
    n = None
    assert lib.pea_cross_supported(ctypes.byref(plain), 5) == 1  # the headline shape fuses the pair ...
    assert lib.pea_cross_supported(ctypes.byref(d), 5) == 0      # ... but not with the loss on the activated map
    for a, b in ((d, plain), (plain, d), (d, d)):
        assert lib.pea_affinity_fwd_dual_ex(ctypes.byref(a), ctypes.byref(b), *([n] * 14), ctypes.c_size_t(0), n) == E_UNSUPPORTED
        assert lib.pea_affinity_fwd_bwd_labels_dual(ctypes.byref(a), ctypes.byref(b), n, n, n, n, 0, n, n, n, n, n, n, n,
                                                    ctypes.c_size_t(0), n) == E_UNSUPPORTED
    assert lib.pea_affinity_fwd_bwd_labels(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n) == E_UNSUPPORTED
    assert lib.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n,
                                              ctypes.c_size_t(0), n) == E_UNSUPPORTED
    # without the flag the same calls get as far as the pointer check; with it the tensor forward does too
    assert lib.pea_affinity_fwd_bwd_labels(ctypes.byref(plain), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n) == E_NULL
    assert lib.pea_affinity_fwd_dual_ex(ctypes.byref(plain), ctypes.byref(plain), *([n] * 14), ctypes.c_size_t(0), n) == E_NULL
    assert lib.pea_affinity_fwd_ex(ctypes.byref(d), n, n, n, n, n, n, n, n, n, n, ctypes.c_size_t(0), n) == E_NULL


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_backward_questions_ignore_the_bit(pkg, lib, mode):
    """the backward kernels take g = d loss / d a(raw) whatever the loss was taken on: pea_cross_supported answers as for the same
    activation bits without the flag (the raw-map kernels stay off: the stored map is not raw)"""
    cv = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    for kw in (dict(D=16), dict(D=32), dict(D=64, offs=cv[:8]), dict(D=32, dtype=1), dict(D=32, dtype=2), dict(D=16, border=1),
               dict(D=16, offs=pkg.multi_offset([1, 3, 9], 8))):
        for act in (HALF, CLAMP, HALF | CLAMP):
            a = lib.pea_cross_supported(ctypes.byref(_desc(pkg, flags=act, **kw)), mode)
            b = lib.pea_cross_supported(ctypes.byref(_desc(pkg, flags=act | LOSS_ACT, **kw)), mode)
            assert a == b, (mode, kw, act)
            if mode in (3, 4):
                assert b == 0


GAL = golden_names("gal_")


def test_fixtures_present():
    assert len(GAL) >= 7 and {str(load_golden(n)["module"]) for n in GAL} == {"loss_embedding", "loss_embedding_exp", "loss_embedding_norm"}


@pytest.mark.parametrize("name", GAL)
def test_signatures_equal_the_reference(pkg, name):
    """names, order and defaults of the reference's functions, recorded by tests/golden/make_golden_actloss.py"""
    g = load_golden(name)
    mod = importlib.import_module(pkg.__name__ + ".loss." + str(g["module"]))
    assert getattr(pkg, str(g["module"])) is mod
    for f in ("embedding_loss", "embedding2affs", "ema_embedding_loss"):
        if "params_" + f not in g:
            assert not hasattr(mod, f), f  # (loss_embedding_exp has no EMA variant)
            continue
        sig = inspect.signature(getattr(mod, f))
        assert list(sig.parameters) == [str(x) for x in g["params_" + f]], f
        defaults = [repr(p.default) for p in sig.parameters.values() if p.default is not inspect.Parameter.empty]
        assert defaults == [str(x) for x in g["defaults_" + f]], f


def test_package_exports_do_not_shadow_the_mse_functions(pkg):
    mse = importlib.import_module(pkg.__name__ + ".loss.loss_embedding_mse")
    assert pkg.embedding_loss is mse.embedding_loss and pkg.ema_embedding_loss is mse.ema_embedding_loss
    assert pkg.embedding2affs is mse.embedding2affs
    assert pkg.embedding_loss_half_clamp is pkg.loss_embedding.embedding_loss
    assert pkg.ema_embedding_loss_half_clamp is pkg.loss_embedding.ema_embedding_loss
    assert pkg.embedding_loss_clamp is pkg.loss_embedding_exp.embedding_loss
    assert pkg.embedding_loss_normalized is pkg.loss_embedding_norm.embedding_loss
    assert pkg.ema_embedding_loss_normalized is pkg.loss_embedding_norm.ema_embedding_loss
    for n in ("embedding_loss_half_clamp", "embedding2affs_half_clamp", "embedding_loss_clamp", "embedding2affs_clamp",
              "embedding_loss_normalized", "embedding2affs_normalized"):
        assert n in pkg.__all__


def test_descriptor_carries_the_bit(pkg):
    """AffinitySpec.act takes the flag to desc.flags, the memo keys on it, and an invalid combination is a ValueError"""
    op = importlib.import_module(pkg.__name__ + ".affinity_op")
    L = pkg._lib
    offs = pkg.multi_offset([1, 3], 4)
    e = torch.empty(2, 16, 64, 64)
    plain = pkg.AffinitySpec(2, offs, None, L.BORDER_CIRCULAR, L.NORM_BX, 1e-6, False, HALF | CLAMP)
    fused = pkg.AffinitySpec(2, offs, None, L.BORDER_CIRCULAR, L.NORM_BX, 1e-6, False, HALF | CLAMP | L.FLAG_LOSS_ACT)
    d0, d1 = op.make_desc(plain, e), op.make_desc(fused, e)
    assert d0 is not d1 and d0.flags == HALF | CLAMP and d1.flags == HALF | CLAMP | LOSS_ACT
    assert op.make_desc(fused, e, mflag=L.FLAG_MASK_F32).flags == HALF | CLAMP | LOSS_ACT | MASK_F32
    assert op.activation_flags("clamp") == CLAMP
    with pytest.raises(ValueError):
        op.make_desc(pkg.AffinitySpec(2, offs, None, L.BORDER_CIRCULAR, L.NORM_BX, 1e-6, False, L.FLAG_LOSS_ACT), e)
    with pytest.raises(ValueError):
        op.make_desc(pkg.AffinitySpec(2, offs, None, L.BORDER_CIRCULAR, L.NORM_BX, 1e-6, True, CLAMP | L.FLAG_LOSS_ACT), e)


@pytest.mark.parametrize("module", ["loss_embedding", "loss_embedding_exp", "loss_embedding_norm"])
def test_cpu_tensors_raise(pkg, module):
    """no CPU fallback, for the fused criterion and for a foreign one alike"""
    mod = getattr(pkg, module)
    offs = pkg.multi_offset([1, 3], 4)
    e = torch.randn(1, 16, 32, 32, requires_grad=True)
    t = torch.zeros(1, len(offs), 32, 32)
    for crit in (pkg.WeightedMSE(), lambda a, b, w: ((a - b) ** 2 * w).mean()):
        with pytest.raises(RuntimeError):
            mod.embedding_loss(e, t, t + 1, t + 1, crit, offs)
        if hasattr(mod, "ema_embedding_loss"):
            with pytest.raises(RuntimeError):
                mod.ema_embedding_loss(e, e.detach(), t, t + 1, t + 1, crit, offs)
    with pytest.raises(RuntimeError):
        mod.embedding2affs(e.detach(), offs)
