"""CPU: f32 loss masks (PEA_FLAG_MASK_F32) at the C ABI and in the Python layer's descriptors; no compute calls here."""
import ctypes
import importlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_F32 = 32


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _desc(pkg, D=16, H=544, W=544, offs=None, dtype=0, border=0, B=8, flags=0):
    d = pkg._lib.PeaDesc()
    offs = offs if offs is not None else pkg.multi_offset([1, 3, 5, 9, 27], 4)
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, B, D, len(offs)
    d.dims[:] = [1, H, W]
    d.border, d.dtype, d.norm, d.eps, d.flags = border, dtype, 0, 1e-12, flags
    for i, o in enumerate(offs):
        d.offsets[i][:] = [0] * (3 - len(o)) + list(o)
        d.lam[i] = 1.0
    return d


def test_flag_value(pkg):
    src = open(os.path.join(ROOT, "include", "pea.h")).read()
    m = re.search(r"#define\s+PEA_FLAG_MASK_F32\s+(\S+)", src)
    assert m and m.group(1) == "32u"
    assert pkg._lib.FLAG_MASK_F32 == MASK_F32


def test_validate_accepts_the_bit(pkg, lib):
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, flags=MASK_F32))) == 0
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, flags=MASK_F32 | pkg._lib.FLAG_RELU_AFFS))) == 0


def _shapes(pkg):
    cv = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    bbbc = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    diag = pkg.multi_offset([1, 3, 9], 8)
    return [dict(D=16),                                                   # the headline shape
            dict(D=16, H=520, W=696, B=4, offs=bbbc),                     # BBBC039V1
            dict(D=32, dtype=1), dict(D=32, dtype=2),
            dict(D=64, dtype=1, offs=cv[:8]), dict(D=64, dtype=2, offs=cv[:8]),
            dict(D=32), dict(D=64, offs=cv[:8]),
            dict(D=16, border=1), dict(D=16, W=548),
            dict(D=16, offs=diag), dict(D=32, offs=diag), dict(D=64, offs=diag)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
def test_cross_supported_ignores_the_bit(pkg, lib, mode):
    """the backward never reads the mask and the forward has an f32-mask form of every fast kernel: same answer with and without"""
    for kw in _shapes(pkg):
        a = lib.pea_cross_supported(ctypes.byref(_desc(pkg, **kw)), mode)
        b = lib.pea_cross_supported(ctypes.byref(_desc(pkg, flags=MASK_F32, **kw)), mode)
        assert a == b, (mode, kw)
    assert lib.pea_cross_supported(ctypes.byref(_desc(pkg, flags=MASK_F32)), 5) == 1  # the headline pair stays one launch


def test_labels_entry_points_refuse_the_bit(pkg, lib):
    """the labels-in calls derive their own masks: the bit is a descriptor error, found before any pointer is looked at"""
    d = _desc(pkg, flags=MASK_F32)
    dc = _desc(pkg)
    n = None
    assert lib.pea_affinity_fwd_bwd_labels(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n) == -2
    assert lib.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n,
                                              ctypes.c_size_t(0), n) == -2
    assert lib.pea_affinity_fwd_bwd_labels_dual(ctypes.byref(d), ctypes.byref(dc), n, n, n, n, 0, n, n, n, n, n, n, n,
                                                ctypes.c_size_t(0), n) == -2
    assert lib.pea_affinity_fwd_bwd_labels_dual(ctypes.byref(dc), ctypes.byref(d), n, n, n, n, 0, n, n, n, n, n, n, n,
                                                ctypes.c_size_t(0), n) == -2
    # without the bit the same calls get as far as the pointer check
    assert lib.pea_affinity_fwd_bwd_labels(ctypes.byref(dc), n, n, n, n, 0, n, n, n, n, n, ctypes.c_size_t(0), n) == -1


def test_dual_refuses_mismatched_mask_types(pkg, lib):
    """the pair's two descriptors must agree outside the activation bits: one f32 mask, one u8, is PEA_E_DESC"""
    p = ctypes.c_void_p(0x10000)
    ptrs = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12)]
    rc = lib.pea_affinity_fwd_dual_ex(ctypes.byref(_desc(pkg, flags=MASK_F32)), ctypes.byref(_desc(pkg)), *ptrs[:3], p, p,
                                      *ptrs[3:11], ptrs[11], ctypes.c_size_t(1 << 20), None)
    assert rc == -2


def test_mask_arg_and_desc_key(pkg):
    """float masks keep f32 (no copy for a float32 slice), bool / uint8 keep the u8 path; the descriptor memo keys on the mask type"""
    op = importlib.import_module(pkg.__name__ + ".affinity_op")
    spec = pkg.AffinitySpec(2, pkg.multi_offset([1, 3], 4), None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    e = torch.empty(2, 16, 64, 64)
    d0 = op.make_desc(spec, e)
    d1 = op.make_desc(spec, e, mflag=pkg._lib.FLAG_MASK_F32)
    assert d0 is not d1 and d0.flags == 0 and d1.flags == MASK_F32
    assert op.make_desc(spec, e, mflag=pkg._lib.FLAG_MASK_F32) is d1
    assert op.mask_arg(None, (2, 4, 64, 64)) == (None, 0, 0)
    if torch.cuda.is_available():  # (_batch_strided insists on GPU tensors; the rest of this test runs on the CPU)
        packed = torch.rand(2, 12, 64, 64, device="cuda")
        m, ms, fl = op.mask_arg(packed[:, 8:12], (2, 4, 64, 64))
        assert fl == MASK_F32 and m.data_ptr() == packed[:, 8:12].data_ptr() and ms == 12 * 64 * 64
        m, ms, fl = op.mask_arg(packed[:, 8:12].half(), (2, 4, 64, 64))
        assert fl == MASK_F32 and m.dtype == torch.float32
        m, ms, fl = op.mask_arg(packed[:, 8:12] > 0.5, (2, 4, 64, 64))
        assert fl == 0 and m.dtype == torch.uint8
