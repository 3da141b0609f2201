"""CPU: the embedding head on 16-bit features (include/pea_head16.h: pea_head_supported_t, pea_head_fwd_t, pea_head_bwd_t) -- the header
and the library agree on the three new symbols while pea.h and the four other headers keep theirs, the support query answers as the
header documents over every type pair, every return code of the two calls is reached before anything is launched and in the documented
order (dummy device pointers, no GPU), and the Python layer hands over the right dtype codes (meta tensors carry the dtypes)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
PAIRS = [(28, 16), (32, 16), (36, 16), (48, 16), (64, 16), (80, 16), (128, 16), (256, 16), (32, 32), (64, 32), (128, 32), (256, 32)]
NEW = ["pea_head_bwd_t", "pea_head_fwd_t", "pea_head_supported_t"]
PEA_H = ["pea_affinity_bwd", "pea_affinity_bwd_dual", "pea_affinity_bwd_dual_ex", "pea_affinity_bwd_ex", "pea_affinity_bwd_ex2",
         "pea_affinity_fwd", "pea_affinity_fwd_bwd_labels", "pea_affinity_fwd_bwd_labels_dual", "pea_affinity_fwd_bwd_labels_ex",
         "pea_affinity_fwd_dual_ex", "pea_affinity_fwd_ex", "pea_affinity_infer", "pea_cross_supported", "pea_desc_validate",
         "pea_fill_border_relu", "pea_gen_targets", "pea_head_bwd", "pea_head_fwd", "pea_head_workspace_bytes", "pea_inv_norm",
         "pea_label_weights", "pea_labels_scratch_bytes", "pea_reload_env", "pea_scale_inplace", "pea_scale_inplace_multi",
         "pea_stitch_add", "pea_stitch_finalize", "pea_strerror", "pea_targets_workspace_bytes", "pea_version", "pea_weighted_sum",
         "pea_workspace_bytes", "pea_workspace_init"]
OTHERS = {"pea_multi.h": ["pea_affinity_bwd_multi", "pea_affinity_fwd_multi", "pea_multi_supported"],
          "pea_multi_labels.h": ["pea_affinity_fwd_bwd_labels_multi", "pea_multi_labels_scratch_bytes", "pea_multi_labels_supported"],
          "pea_infer.h": ["pea_affinity_infer_stitch", "pea_infer_stitch_supported"],
          "pea_flip.h": ["pea_consistency_unflip"]}


def header_text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def declared_symbols(header):
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", header_text(header))))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


P = lambda a: ctypes.c_void_p(a) if a else None
X, W, BIAS, E, DX, DW, DB, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


def fwd(lib, B=2, C=32, D=16, S=100, x=X, xt=BF16, w=W, bias=BIAS, e=E, et=BF16):
    """pea_head_fwd_t on dummy pointers: anything but an early return would fault"""
    return lib.pea_head_fwd_t(B, C, D, S, P(x), xt, P(w), P(bias), P(e), et, None)


def bwd(lib, B=2, C=32, D=16, S=100, x=X, xt=BF16, w=W, de=E, et=BF16, dx=DX, dw=DW, db=DB, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.pea_head_workspace_bytes(C, D)
    return lib.pea_head_bwd_t(B, C, D, S, P(x), xt, P(w), P(de), et, P(dx), P(dw), P(db), P(ws), ws_bytes, None)


def test_header_declares_exactly_the_three_entry_points(pkg):
    assert declared_symbols("pea_head16.h") == sorted(pkg._lib.EXPORTS_HEAD16) == NEW
    text = open(os.path.join(ROOT, "include", "pea_head16.h")).read()
    assert '#include "pea.h"' in text
    for cited in ("OutConv", "conv3dBlock", "PEA_E_UNSUPPORTED"):  # the reference lines it replaces; the refused pairs
        assert cited in text


def test_library_exports_them_and_the_older_headers_are_unchanged(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    older = (set(pkg._lib.EXPORTS) | set(pkg._lib.EXPORTS_INFER) | set(pkg._lib.EXPORTS_MULTI) | set(pkg._lib.EXPORTS_FLIP)
             | set(pkg._lib.EXPORTS_MULTI_LABELS))
    assert not set(NEW) & older
    assert declared_symbols("pea.h") == sorted(pkg._lib.EXPORTS) == PEA_H
    assert declared_symbols("pea_multi.h") == sorted(pkg._lib.EXPORTS_MULTI) == OTHERS["pea_multi.h"]
    assert declared_symbols("pea_multi_labels.h") == sorted(pkg._lib.EXPORTS_MULTI_LABELS) == OTHERS["pea_multi_labels.h"]
    assert declared_symbols("pea_infer.h") == sorted(pkg._lib.EXPORTS_INFER) == OTHERS["pea_infer.h"]
    assert declared_symbols("pea_flip.h") == sorted(pkg._lib.EXPORTS_FLIP) == OTHERS["pea_flip.h"]
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert re.search(r"#define\s+PEA_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "include", "pea.h")).read())


def test_supported_truth_table(pkg, lib):
    """9 type pairs x the 12 channel pairs of the f32 head, plus (33, 16) and (32, 64): served are f16 / bf16 features with the
    embedding in the same type or in f32; the Python restatement (no library) agrees everywhere"""
    tt = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
    served = {(F16, F16), (F16, F32), (BF16, BF16), (BF16, F32)}
    n = 0
    for xt in (F32, F16, BF16):
        for et in (F32, F16, BF16):
            for C, D in PAIRS + [(33, 16), (32, 64)]:
                want = int((xt, et) in served and (C, D) in PAIRS)
                assert lib.pea_head_supported_t(C, D, xt, et) == want, (C, D, xt, et)
                assert int(pkg.head16_supported(C, D, tt[xt], tt[et])) == want, (C, D, xt, et)
                n += want
    assert n == 4 * 12
    for C, D in PAIRS:
        assert pkg.model.head.head_supported(C, D)
    assert lib.pea_head_supported_t(32, 16, 3, 3) == 0 and lib.pea_head_supported_t(32, 16, BF16, -1) == 0
    assert lib.pea_head_supported_t(0, 16, BF16, BF16) == 0


def test_forward_return_codes_before_a_launch(lib):
    # PEA_E_DESC: sizes below 1, dtype codes outside 0..2
    for kw in (dict(B=0), dict(C=0), dict(D=0), dict(S=0), dict(xt=3), dict(xt=-1), dict(et=3), dict(et=-1)):
        assert fwd(lib, **kw) == E_DESC, kw
    # PEA_E_NULL: x, W, e (bias may be NULL: it is then not an error, the next check decides)
    for kw in (dict(x=None), dict(w=None), dict(e=None)):
        assert fwd(lib, **kw) == E_NULL, kw
    # PEA_E_ALIGN: element alignment -- odd addresses for 16-bit tensors, 2-byte-aligned ones for the f32 W / bias / e
    for kw in (dict(x=X + 1), dict(e=E + 1), dict(w=W + 2), dict(bias=BIAS + 2), dict(e=E + 2, et=F32), dict(w=W + 1)):
        assert fwd(lib, **kw) == E_ALIGN, kw
    # PEA_E_UNSUPPORTED: the five refused type pairs and other channel pairs
    for xt, et in ((F32, F32), (F32, F16), (F32, BF16), (F16, BF16), (BF16, F16)):
        assert fwd(lib, xt=xt, et=et, x=X, e=E) == E_UNSUPPORTED, (xt, et)
    assert fwd(lib, C=33) == E_UNSUPPORTED and fwd(lib, D=64) == E_UNSUPPORTED
    # the order: DESC, NULL, ALIGN, UNSUPPORTED
    assert fwd(lib, B=0, x=None, e=E + 1, C=33) == E_DESC
    assert fwd(lib, xt=3, x=None) == E_DESC
    assert fwd(lib, x=None, e=E + 1, C=33) == E_NULL
    assert fwd(lib, e=E + 1, C=33) == E_ALIGN
    assert fwd(lib, x=X + 2, e=E + 2, C=33) == E_UNSUPPORTED  # 2-byte aligned 16-bit tensors are aligned


def test_backward_return_codes_before_a_launch(lib):
    for kw in (dict(B=0), dict(C=0), dict(D=0), dict(S=0), dict(xt=3), dict(xt=-1), dict(et=3), dict(et=-1)):
        assert bwd(lib, **kw) == E_DESC, kw
    for kw in (dict(x=None), dict(w=None), dict(de=None), dict(dw=None)):
        assert bwd(lib, **kw) == E_NULL, kw
    for kw in (dict(x=X + 1), dict(de=E + 1), dict(dx=DX + 1), dict(w=W + 2), dict(dw=DW + 2), dict(db=DB + 2), dict(ws=WS + 2),
               dict(de=E + 2, et=F32), dict(dw=DW + 1)):
        assert bwd(lib, **kw) == E_ALIGN, kw
    for xt, et in ((F32, F32), (F32, F16), (F32, BF16), (F16, BF16), (BF16, F16)):
        assert bwd(lib, xt=xt, et=et) == E_UNSUPPORTED, (xt, et)
    assert bwd(lib, C=33) == E_UNSUPPORTED and bwd(lib, D=64) == E_UNSUPPORTED
    # PEA_E_WORKSPACE: missing, or 4 bytes short
    need = lib.pea_head_workspace_bytes(32, 16)
    assert need == 1024 * (16 * 32 + 16) * 4
    assert bwd(lib, ws=None) == E_WORKSPACE
    assert bwd(lib, ws_bytes=need - 4) == E_WORKSPACE
    assert bwd(lib, ws_bytes=0) == E_WORKSPACE
    for xt, et in ((F16, F16), (F16, F32), (BF16, BF16), (BF16, F32)):
        assert bwd(lib, xt=xt, et=et, ws_bytes=need - 4) == E_WORKSPACE, (xt, et)
    # the order: DESC, NULL, ALIGN, UNSUPPORTED, WORKSPACE
    assert bwd(lib, S=0, x=None, dw=DW + 2, C=33, ws=None) == E_DESC
    assert bwd(lib, x=None, dw=DW + 2, C=33, ws=None) == E_NULL
    assert bwd(lib, dw=DW + 2, C=33, ws=None) == E_ALIGN
    assert bwd(lib, C=33, ws=None) == E_UNSUPPORTED
    assert bwd(lib, xt=F32, et=F32, ws_bytes=0) == E_UNSUPPORTED
    assert bwd(lib, dx=None, db=None, ws=None) == E_WORKSPACE  # the optional outputs are optional


def test_python_layer_builds_the_dtype_codes(pkg):
    """host-only: meta tensors carry the dtypes"""
    head = pkg.model.head
    for dt, code in ((torch.float16, F16), (torch.bfloat16, BF16)):
        x = torch.empty(2, 32, 8, 8, device="meta", dtype=dt)
        assert head.head_dtype_codes(x.dtype) == (code, code)
        assert head.head_dtype_codes(x.dtype, torch.float32) == (code, F32)
        e = torch.empty(2, 16, 8, 8, device="meta", dtype=dt)
        spec = pkg.AffinitySpec(2, [[-1, 0], [0, -1]], None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
        assert pkg.affinity_op.make_desc(spec, e).dtype == code  # what HeadAffinityMSE hands the loss kernels
    assert head.head_dtype_codes(torch.float32) == (F32, F32)
    assert (pkg._lib.F32, pkg._lib.F16, pkg._lib.BF16) == (F32, F16, BF16)
    # the modules keep their constructors and parameter names and gain a plain attribute
    oc, h3 = pkg.OutConv(32, 16), pkg.head_conv3d_block(28, 16)
    assert oc.out_dtype is None and h3.out_dtype is None
    assert sorted(oc.state_dict()) == ["conv.bias", "conv.weight"] and sorted(h3.state_dict()) == ["0.bias", "0.weight"]
    assert list(inspect.signature(pkg.OutConv.__init__).parameters) == ["self", "in_ch", "out_ch"]
    assert list(inspect.signature(pkg.head_conv3d_block).parameters) == ["in_planes", "out_planes", "bias"]
    assert "head16_supported" in pkg.__all__ and pkg.head16_supported is head.head16_supported
    assert list(inspect.signature(pkg.head16_supported).parameters) == ["C", "D", "x_dtype", "e_dtype"]


def test_cpu_tensors_still_raise(pkg):
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError):
            pkg.OutConv(32, 16)(torch.zeros(1, 32, 8, 8, dtype=dt))
        with pytest.raises(RuntimeError):
            pkg.EmbeddingHead.apply(torch.zeros(1, 32, 8, 8, dtype=dt), torch.zeros(16, 32, 1, 1), None)
