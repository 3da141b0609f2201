"""CPU: PEA_E_ALIGN at the entry points that take a workspace -- each pointer argument in turn at an address that is not a multiple of its
element size must give -5.

Fake addresses, never dereferenced: every call here passes workspace = NULL, and the alignment check comes before the workspace check
in all six entry points, so a check that is missing ends in PEA_E_WORKSPACE (-4), never in a launch.  (The entry points without a
workspace argument -- the backward calls, pea_affinity_infer, pea_inv_norm -- would launch on a missed check: their checks are held by
the GPU suite and by test_abi.py / test_bf16_host.py.)
"""
import ctypes

import pytest

E_WORKSPACE, E_ALIGN = -4, -5
MASK_F32 = 32
BASE = 0x100000


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _desc(pkg, dtype=0, flags=0, D=16):
    d = pkg._lib.PeaDesc()
    offs = pkg.multi_offset([1, 3], 4)
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, 2, D, len(offs)
    d.dims[:] = [1, 48, 96]
    d.border, d.dtype, d.norm, d.eps, d.flags = 0, dtype, 0, 1e-12, flags
    for i, o in enumerate(offs):
        d.offsets[i][:] = [0] + list(o)
        d.lam[i] = 1.0
    return d


def _ptrs(names, skew=None, by=0):
    """distinct 256-byte aligned fake addresses, `skew` moved by `by` bytes"""
    return {n: BASE * (i + 1) + (by if n == skew else 0) for i, n in enumerate(names)}


# entry point -> (pointer arguments in call order with their element size: 'e' = the embedding's; the call)
def _fwd(lib, d, p):
    return lib.pea_affinity_fwd(ctypes.byref(d), p["e"], p["e_other"], p["target"], p["weight"], p["mask"], p["affs"], p["g_out"],
                                p["loss_out"], None, ctypes.c_size_t(1 << 20), None)


def _fwd_ex(lib, d, p):
    return lib.pea_affinity_fwd_ex(ctypes.byref(d), p["e"], p["e_other"], p["target"], p["weight"], p["mask"], p["affs"], p["g_out"],
                                   p["inv_norm_out"], p["loss_out"], None, ctypes.c_size_t(1 << 20), None)


def _fwd_dual(lib, d, p):
    return lib.pea_affinity_fwd_dual_ex(ctypes.byref(d), ctypes.byref(d), p["e"], p["ema"], p["target"], p["weight"], p["mask"], p["affs"],
                                        p["g_out"], p["g_cross_out"], p["inv_norm_out"], p["inv_norm_other_out"], p["loss_out"],
                                        p["loss_cross_out"], None, None, ctypes.c_size_t(1 << 20), None)


def _labels(lib, d, p):
    return lib.pea_affinity_fwd_bwd_labels(ctypes.byref(d), p["e"], p["e_other"], p["labels"], p["wtab"], 0, p["affs"], p["loss_out"],
                                           p["dloss"], p["de"], None, ctypes.c_size_t(1 << 20), None)


def _labels_ex(lib, d, p):
    return lib.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), p["e"], p["e_other"], p["labels"], p["wtab"], 0, p["affs"], p["loss_out"],
                                              p["dloss"], p["de"], None, ctypes.c_size_t(1 << 20), p["scratch"], ctypes.c_size_t(1 << 24),
                                              None)


def _labels_dual(lib, d, p):
    return lib.pea_affinity_fwd_bwd_labels_dual(ctypes.byref(d), ctypes.byref(d), p["e"], p["ema"], p["labels"], p["wtab"], 0, p["affs"],
                                                p["loss_out"], p["loss_cross_out"], p["dloss"], p["dloss_cross"], p["de"], None,
                                                ctypes.c_size_t(1 << 20), None)


E = "e"  # element size of the embedding storage
ENTRY = {
    "pea_affinity_fwd": (_fwd, dict(e=E, e_other=E, target=4, weight=4, mask=1, affs=4, g_out=4, loss_out=4)),
    "pea_affinity_fwd_ex": (_fwd_ex, dict(e=E, e_other=E, target=4, weight=4, mask=1, affs=4, g_out=4, inv_norm_out=4, loss_out=4)),
    "pea_affinity_fwd_dual_ex": (_fwd_dual, dict(e=E, ema=E, target=4, weight=4, mask=1, affs=4, g_out=4, g_cross_out=4, inv_norm_out=4,
                                                 inv_norm_other_out=4, loss_out=4, loss_cross_out=4)),
    "pea_affinity_fwd_bwd_labels": (_labels, dict(e=E, e_other=E, labels=4, wtab=4, affs=4, loss_out=4, dloss=4, de=E)),
    "pea_affinity_fwd_bwd_labels_ex": (_labels_ex, dict(e=E, e_other=E, labels=4, wtab=4, affs=4, loss_out=4, dloss=4, de=E, scratch=16)),
    "pea_affinity_fwd_bwd_labels_dual": (_labels_dual, dict(e=E, ema=E, labels=4, wtab=4, affs=4, loss_out=4, loss_cross_out=4, dloss=4,
                                                            dloss_cross=4, de=E)),
}
MASKED = ("pea_affinity_fwd", "pea_affinity_fwd_ex", "pea_affinity_fwd_dual_ex")


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_each_pointer_in_turn(pkg, lib, name, dtype):
    """aligned pointers get as far as the workspace check; one pointer off its element size is PEA_E_ALIGN"""
    call, args = ENTRY[name]
    es = 4 if dtype == 0 or name == "pea_affinity_fwd_dual_ex" else 2  # (the pair's forward checks its f32-only operands at 4 bytes)
    d = _desc(pkg, dtype=dtype)
    assert call(lib, d, _ptrs(args)) == E_WORKSPACE, name
    for arg, size in args.items():
        size = es if size == E else size
        if size == 1:
            continue  # a u8 mask has no misaligned address (the f32 mask: below)
        for by in sorted({size // 2, 1} - {0}):
            assert call(lib, d, _ptrs(args, arg, by)) == E_ALIGN, (name, arg, by)
        # a whole element further is aligned again: the check looks at the element size, not at 16 bytes
        assert call(lib, d, _ptrs(args, arg, size)) == E_WORKSPACE, (name, arg)


@pytest.mark.parametrize("name", MASKED)
def test_f32_mask_is_an_f32_pointer(pkg, lib, name):
    """PEA_FLAG_MASK_F32: the mask must be 4-byte aligned; without the flag the same odd address is a u8 pointer and passes"""
    call, args = ENTRY[name]
    for by in (1, 2, 3):
        assert call(lib, _desc(pkg, flags=MASK_F32), _ptrs(args, "mask", by)) == E_ALIGN, (name, by)
        assert call(lib, _desc(pkg), _ptrs(args, "mask", by)) == E_WORKSPACE, (name, by)
    assert call(lib, _desc(pkg, flags=MASK_F32), _ptrs(args, "mask", 4)) == E_WORKSPACE, name
    p = _ptrs(args)
    p["mask"] = None  # the flag is ignored where there is no mask
    assert call(lib, _desc(pkg, flags=MASK_F32), p) == E_WORKSPACE, name
