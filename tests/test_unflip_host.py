"""CPU: the un-flip of the EMA embedding (include/pea_flip.h: pea_consistency_unflip) -- the header and the library agree on the new
symbol and the three older headers keep theirs, every refusal of the call is reached before anything is launched and in the
header's order (dummy device pointers, no GPU), and the torch composition convert_consistency_flip takes for CPU tensors equals the
reference's 2D and 3D functions on every rule combination (goldens gflip_rules, gflip_rules_3d)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
U8, I32, I64, RF32 = 0, 1, 2, 3

# the symbol lists of the three older headers, as they were before pea_flip.h
PEA_H = ["pea_affinity_bwd", "pea_affinity_bwd_dual", "pea_affinity_bwd_dual_ex", "pea_affinity_bwd_ex", "pea_affinity_bwd_ex2",
         "pea_affinity_fwd", "pea_affinity_fwd_bwd_labels", "pea_affinity_fwd_bwd_labels_dual", "pea_affinity_fwd_bwd_labels_ex",
         "pea_affinity_fwd_dual_ex", "pea_affinity_fwd_ex", "pea_affinity_infer", "pea_cross_supported", "pea_desc_validate",
         "pea_fill_border_relu", "pea_gen_targets", "pea_head_bwd", "pea_head_fwd", "pea_head_workspace_bytes", "pea_inv_norm",
         "pea_label_weights", "pea_labels_scratch_bytes", "pea_reload_env", "pea_scale_inplace", "pea_scale_inplace_multi",
         "pea_stitch_add", "pea_stitch_finalize", "pea_strerror", "pea_targets_workspace_bytes", "pea_version", "pea_weighted_sum",
         "pea_workspace_bytes", "pea_workspace_init"]
PEA_INFER_H = ["pea_affinity_infer_stitch", "pea_infer_stitch_supported"]
PEA_MULTI_H = ["pea_affinity_bwd_multi", "pea_affinity_fwd_multi", "pea_multi_supported"]


def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_entry_point(pkg):
    assert declared_symbols("pea_flip.h") == sorted(pkg._lib.EXPORTS_FLIP) == ["pea_consistency_unflip"]
    src = open(os.path.join(ROOT, "include", "pea_flip.h")).read()
    assert '#include "pea.h"' in src
    for name, code in (("U8", 0), ("I32", 1), ("I64", 2), ("F32", 3)):
        assert re.search(r"#define\s+PEA_RULES_%s\s+%d\b" % (name, code), src), name
        assert getattr(pkg._lib, "RULES_" + name) == code


def test_library_exports_it_and_the_older_headers_are_unchanged(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in pkg._lib.EXPORTS_FLIP:
        assert hasattr(raw, name), name
    older = set(pkg._lib.EXPORTS) | set(pkg._lib.EXPORTS_INFER) | set(pkg._lib.EXPORTS_MULTI)
    assert not set(pkg._lib.EXPORTS_FLIP) & older
    assert declared_symbols("pea.h") == sorted(pkg._lib.EXPORTS) == PEA_H
    assert declared_symbols("pea_infer.h") == sorted(pkg._lib.EXPORTS_INFER) == PEA_INFER_H
    assert declared_symbols("pea_multi.h") == sorted(pkg._lib.EXPORTS_MULTI) == PEA_MULTI_H
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2


# ---- return codes ------------------------------------------------------------------------------------------------------------------
SRC, DST, RULES = 0x10000000, 0x20000000, 0x30000000


def call(lib, B=2, C=16, Z=1, Y=64, X=64, dtype=F32, src=SRC, dst=DST, rules=RULES, rdt=U8, nrules=3):
    """pea_consistency_unflip on dummy pointers: anything but an early return would fault"""
    vp = lambda a: ctypes.c_void_p(a) if a else None
    return lib.pea_consistency_unflip(B, C, Z, Y, X, dtype, vp(src), vp(dst), vp(rules), rdt, nrules, None)


def test_refusals_before_a_launch(lib):
    # PEA_E_DESC: a dimension below 1, an unknown dtype / rules dtype, nrules not 3 or 4
    for dim in ("B", "C", "Z", "Y", "X"):
        assert call(lib, **{dim: 0}) == E_DESC, dim
        assert call(lib, **{dim: -3}) == E_DESC, dim
    assert call(lib, dtype=3) == E_DESC and call(lib, dtype=-1) == E_DESC
    assert call(lib, rdt=4) == E_DESC and call(lib, rdt=-1) == E_DESC
    for n in (0, 2, 5, -3):
        assert call(lib, nrules=n) == E_DESC, n
    # PEA_E_NULL
    for ptr in ("src", "dst", "rules"):
        assert call(lib, **{ptr: 0}) == E_NULL, ptr
    # PEA_E_ALIGN: src / dst to the element size, rules to ITS element size
    assert call(lib, src=SRC + 2) == E_ALIGN and call(lib, dst=DST + 2) == E_ALIGN      # a 2-byte-aligned f32 pointer
    assert call(lib, src=SRC + 1) == E_ALIGN and call(lib, dst=DST + 3) == E_ALIGN
    for dt in (F16, BF16):
        assert call(lib, dtype=dt, src=SRC + 1) == E_ALIGN and call(lib, dtype=dt, dst=DST + 1) == E_ALIGN
    assert call(lib, rdt=I32, rules=RULES + 2) == E_ALIGN and call(lib, rdt=RF32, rules=RULES + 1) == E_ALIGN
    assert call(lib, rdt=I64, rules=RULES + 4) == E_ALIGN
    # PEA_E_DESC: the byte ranges of src and dst overlap -- in place, and by ONE element at either end
    n = 2 * 16 * 64 * 64
    assert call(lib, dst=SRC) == E_DESC
    assert call(lib, dst=SRC + 4 * (n - 1)) == E_DESC and call(lib, src=DST + 4 * (n - 1)) == E_DESC
    assert call(lib, dtype=BF16, dst=SRC + 2 * (n - 1)) == E_DESC and call(lib, dtype=F16, src=DST + 2 * (n - 1)) == E_DESC
    assert call(lib, Z=3, nrules=4, dst=SRC + 4 * (3 * n - 1)) == E_DESC
    # PEA_E_UNSUPPORTED: more tiles than one grid holds (2^31 - 1): 2^15 * 2^16 planes of one tile, or one plane of 2^31 tiles
    far = 1 << 60
    assert call(lib, B=1 << 15, C=1 << 16, Y=1, X=1, dst=far) == E_UNSUPPORTED
    assert call(lib, B=1, C=1, Y=1 << 21, X=1 << 22, dtype=BF16, dst=far) == E_UNSUPPORTED
    assert call(lib, B=1 << 10, C=1 << 10, Z=1 << 11, Y=65, X=1, nrules=4, dst=far) == E_UNSUPPORTED


def test_refusals_come_in_the_stated_order(lib):
    big = dict(B=1 << 15, C=1 << 16, Y=1, X=1)  # (unsupported when nothing else is wrong)
    assert call(lib, dst=1 << 60, **big) == E_UNSUPPORTED
    assert call(lib, dst=SRC, **big) == E_DESC                           # overlap before the tile count
    assert call(lib, dst=SRC + 2, **big) == E_ALIGN                      # alignment before overlap
    assert call(lib, src=SRC + 2, dst=0, **big) == E_NULL                # NULL before alignment
    assert call(lib, src=0, rdt=I32, rules=RULES + 2) == E_NULL
    assert call(lib, src=0, dst=0, rules=0, nrules=2) == E_DESC          # the descriptor before NULL
    assert call(lib, src=0, dtype=7) == E_DESC and call(lib, rules=0, X=0) == E_DESC
    assert call(lib, rules=RULES + 1, rdt=I32, dst=SRC) == E_ALIGN


# ---- the torch composition (CPU tensors) against the reference ------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", ["gflip_rules", "gflip_rules_3d"])
def test_cpu_composition_equals_the_reference(pkg, name):
    g = load_golden(name)
    n = 3 if name == "gflip_rules" else 4
    assert g["rules"].shape == (2 ** n, n) and len(np.unique(g["rules"], axis=0)) == 2 ** n  # every rule combination
    x = torch.from_numpy(g["gt"]).requires_grad_(True)
    for rules in (torch.from_numpy(g["rules"]), g["rules"].tolist(), g["rules"].astype(np.uint8), torch.from_numpy(g["rules"]).bool()):
        out = pkg.convert_consistency_flip(x, rules)
        assert not out.requires_grad and out.dtype == x.dtype and out.is_contiguous()
        assert np.array_equal(bits(out.numpy()), bits(g["out"]))
    out = pkg.convert_consistency_flip(x, None)
    assert not out.requires_grad and out.data_ptr() != x.data_ptr() and np.array_equal(bits(out.numpy()), bits(g["gt"]))


def test_three_rules_on_a_volume_apply_to_every_z_slice(pkg):
    g = load_golden("gflip_rules")
    rng = np.random.default_rng(5)
    vol = torch.from_numpy(rng.standard_normal((8, 2, 3, 6, 6)).astype(np.float32))
    rules = torch.from_numpy(g["rules"])
    out = pkg.convert_consistency_flip(vol, rules)
    assert out.shape == vol.shape
    for z in range(vol.shape[2]):
        assert torch.equal(out[:, :, z], pkg.convert_consistency_flip(vol[:, :, z].contiguous(), rules))
    # .. which is the four-rule form with the z-flip clear
    assert torch.equal(out, pkg.convert_consistency_flip(vol, torch.cat([torch.zeros(8, 1), rules], dim=1)))


def test_shapes_that_are_refused(pkg):
    img, vol = torch.zeros(4, 2, 6, 6), torch.zeros(4, 2, 3, 6, 6)
    with pytest.raises(ValueError):
        pkg.convert_consistency_flip(img, torch.zeros(4, 4))           # four rules need a volume
    with pytest.raises(ValueError):
        pkg.convert_consistency_flip(img, [[0, 1, 0, 1]] * 4)
    for t in (img, vol):
        with pytest.raises(ValueError):
            pkg.convert_consistency_flip(t, torch.zeros(4, 2))
        with pytest.raises(ValueError):
            pkg.convert_consistency_flip(t, torch.zeros(3, 3))         # batch mismatch
        with pytest.raises(ValueError):
            pkg.convert_consistency_flip(t, torch.zeros(5, 3))
        with pytest.raises(ValueError):
            pkg.convert_consistency_flip(t, torch.zeros(12))
    with pytest.raises(ValueError):
        pkg.convert_consistency_flip(vol, torch.zeros(3, 4))
    with pytest.raises(ValueError):
        pkg.convert_consistency_flip(torch.zeros(4, 6, 6), torch.zeros(4, 3))
    assert pkg.convert_consistency_flip(vol, torch.zeros(4, 4)).shape == vol.shape


def test_unflip_is_a_device_call(pkg):
    """no CPU fallback behind the public op"""
    assert "unflip" in pkg.__all__
    with pytest.raises(RuntimeError):
        pkg.unflip(torch.zeros(2, 2, 6, 6), torch.zeros(2, 3))
