"""CPU: bfloat16 embedding storage (PEA_BF16) at the C ABI and in the Python layer's descriptors; no compute calls here."""
import ctypes
import importlib

import pytest
import torch


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _desc(pkg, D=16, H=544, W=544, offs=None, dtype=2, border=0, B=8):
    d = pkg._lib.PeaDesc()
    offs = offs if offs is not None else pkg.multi_offset([1, 3, 5, 9, 27], 4)
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, B, D, len(offs)
    d.dims[:] = [1, H, W]
    d.border, d.dtype, d.norm, d.eps = border, dtype, 0, 1e-12
    for i, o in enumerate(offs):
        d.offsets[i][:] = [0] * (3 - len(o)) + list(o)
        d.lam[i] = 1.0
    return d


def test_bf16_dtype_code(pkg):
    assert (pkg._lib.F32, pkg._lib.F16, pkg._lib.BF16) == (0, 1, 2)
    assert pkg._lib.PEA_ABI_VERSION == 2


def test_validate_accepts_bf16(pkg, lib):
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, dtype=2))) == 0
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, dtype=3))) == -2
    assert lib.pea_desc_validate(ctypes.byref(_desc(pkg, dtype=-1))) == -2


def test_bf16_alignment_is_two_bytes(pkg, lib):
    """a bf16 tensor is 2-byte aligned, not 4: an odd address is refused, an even one that is not 4-aligned is not (it fails later, on
    the NULL affs, before anything is launched)"""
    d = _desc(pkg, dtype=2)
    assert lib.pea_affinity_infer(ctypes.byref(d), ctypes.c_void_p(0x1001), None, ctypes.c_void_p(0x2000), None) == -5
    assert lib.pea_affinity_infer(ctypes.byref(d), ctypes.c_void_p(0x1002), None, None, None) == -1
    assert lib.pea_inv_norm(ctypes.byref(d), ctypes.c_void_p(0x1001), ctypes.c_void_p(0x2000), None) == -5


def test_scale_inplace_accepts_bf16_dtype(pkg, lib):
    """the dtype check comes before any launch: bf16 passes it (n = 0 returns at once), dtype 3 does not"""
    p = ctypes.c_void_p(0x1000)
    assert lib.pea_scale_inplace(p, 2, ctypes.c_size_t(0), p, None) == 0
    assert lib.pea_scale_inplace(p, 3, ctypes.c_size_t(0), p, None) == -2
    bufs = (ctypes.c_void_p * 1)(0x1000)
    cnts = (ctypes.c_size_t * 1)(0)
    assert lib.pea_scale_inplace_multi(bufs, cnts, 1, 2, p, None) == 0
    assert lib.pea_scale_inplace_multi(bufs, cnts, 1, 3, p, None) == -2


@pytest.mark.parametrize("bwd", [0, 1])
def test_cross_supported_bf16_matches_f16(pkg, lib, bwd):
    cv = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    q = lambda d: lib.pea_cross_supported(ctypes.byref(d), bwd)
    shapes = [dict(D=16), dict(D=64, offs=cv[:8]), dict(D=16, W=548), dict(D=32, H=704, W=704, offs=pkg.multi_offset([1, 3, 5, 9, 11], 4)),
              dict(D=16, border=1), dict(D=8), dict(D=16, offs=pkg.multi_offset([1, 3, 9], 8))]
    for kw in shapes:
        assert q(_desc(pkg, dtype=2, **kw)) == q(_desc(pkg, dtype=1, **kw)), kw
    assert q(_desc(pkg, D=16, dtype=2)) == 1
    assert q(_desc(pkg, D=64, offs=cv[:8], dtype=2)) == 1
    assert q(_desc(pkg, D=16, W=548, dtype=2)) == 0


def test_cross_supported_bf16_cross_loss(pkg, lib):
    """the cross loss with a detached second operand (mode 2) runs on the 16-bit kernels in bf16 at D = 16 / 32 / 64"""
    cv = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    for D, offs in ((16, cv), (32, cv), (64, cv[:8])):
        assert lib.pea_cross_supported(ctypes.byref(_desc(pkg, D=D, offs=offs, dtype=2)), 2) == 1, D
    assert lib.pea_cross_supported(ctypes.byref(_desc(pkg, D=16, W=548, dtype=2)), 2) == 0


def test_make_desc_keys_on_the_dtype(pkg):
    """same-shaped f32 / f16 / bf16 tensors get three descriptors (the memo must not hand a bf16 tensor the f32 descriptor)"""
    op = importlib.import_module(pkg.__name__ + ".affinity_op")
    spec = pkg.AffinitySpec(2, pkg.multi_offset([1, 3], 4), None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    ds = [op.make_desc(spec, torch.empty(2, 16, 64, 64, dtype=dt)) for dt in (torch.float32, torch.float16, torch.bfloat16)]
    assert [d.dtype for d in ds] == [0, 1, 2]
    assert len({id(d) for d in ds}) == 3
    assert op.make_desc(spec, torch.empty(2, 16, 64, 64, dtype=torch.bfloat16)) is ds[2]

