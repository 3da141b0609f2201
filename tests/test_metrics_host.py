"""CPU: the validation pixel metrics (include/pea_metrics.h: pea_metrics_validate, pea_metrics_workspace_bytes, pea_affs_metrics) --
the header and the library agree on the three new symbols and every older header keeps its own, every refusal of the call is
reached before anything is launched and in the header's order (dummy device pointers, no GPU), the workspace is five loss states,
the Python entry points refuse CPU tensors, and the numpy restatement tests/metrics_reference.py -- what the GPU tests compare the
kernel with -- reproduces the reference's own numbers on both fixtures (gmetrics_2d: MSELoss / BCELoss of scripts_cvppp/loss/loss.py;
gmetrics_3d: scripts_ac3ac4/main.py:339-351 with sklearn's f1_score)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from metrics_reference import f1, finished_pred, metrics_reference

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
RELU, DIVIDE, STORE, MASK_F32 = 1, 2, 4, 8
NEW = ["pea_affs_metrics", "pea_metrics_validate", "pea_metrics_workspace_bytes"]
# the symbol counts of the older headers, as they were before pea_metrics.h
OLDER = {"pea.h": ("EXPORTS", 33), "pea_infer.h": ("EXPORTS_INFER", 2), "pea_multi.h": ("EXPORTS_MULTI", 3), "pea_flip.h": ("EXPORTS_FLIP", 1),
         "pea_multi_labels.h": ("EXPORTS_MULTI_LABELS", 3), "pea_head16.h": ("EXPORTS_HEAD16", 3)}


def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_entry_points(pkg):
    assert declared_symbols("pea_metrics.h") == sorted(pkg._lib.EXPORTS_METRICS) == NEW
    src = open(os.path.join(ROOT, "include", "pea_metrics.h")).read()
    assert '#include "pea.h"' in src
    assert re.search(r"#define\s+PEA_METRICS_COLS\s+5\b", src) and pkg._lib.METRICS_COLS == 5
    for name, code in (("RELU", 1), ("DIVIDE", 2), ("STORE", 4), ("MASK_F32", 8)):
        assert re.search(r"#define\s+PEA_MET_%s\s+%du\b" % (name, code), src), name
        assert getattr(pkg._lib, "MET_" + name) == code
    # the ctypes mirror has the header's layout: fifteen 4-byte fields, no padding
    assert ctypes.sizeof(pkg._lib.PeaMetricsDesc) == 15 * 4
    assert [f[0] for f in pkg._lib.PeaMetricsDesc._fields_] == ["B", "C", "CP", "dims", "pred_dims", "origin", "flags", "clip_lo", "clip_hi"]


def test_library_exports_them_and_the_older_headers_are_unchanged(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    older = set()
    for header, (tup, count) in OLDER.items():
        names = getattr(pkg._lib, tup)
        assert declared_symbols(header) == sorted(names) and len(names) == count, header
        older |= set(names)
    assert not set(NEW) & older
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    src = open(os.path.join(ROOT, "include", "pea.h")).read()
    assert re.search(r"#define\s+PEA_ABI_VERSION\s+2\b", src)


# ---- return codes ------------------------------------------------------------------------------------------------------------------
PRED, WMAP, TGT, MASK, OUT, WORK = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000


def desc(pkg, B=1, C=3, CP=12, dims=(4, 14, 16), pred_dims=(6, 20, 24), origin=(1, 3, 4), flags=0, clip=(0.0, 1.0)):
    d = pkg._lib.PeaMetricsDesc()
    d.B, d.C, d.CP = B, C, CP
    d.dims[:], d.pred_dims[:], d.origin[:] = dims, pred_dims, origin
    d.flags, d.clip_lo, d.clip_hi = flags, clip[0], clip[1]
    return d


def call(pkg, lib, d="default", pred=PRED, wmap=WMAP, target=TGT, mask=MASK, out=OUT, work=WORK, wbytes=None, **kw):
    """pea_affs_metrics on dummy pointers: anything but an early return would fault"""
    vp = lambda a: ctypes.c_void_p(a) if a else None
    if isinstance(d, str):
        d = desc(pkg, **kw)
    wbytes = lib.pea_metrics_workspace_bytes() if wbytes is None else wbytes
    return lib.pea_affs_metrics(None if d is None else ctypes.byref(d), vp(pred), vp(wmap), vp(target), vp(mask), vp(out), vp(work),
                                wbytes, None)


BIG = dict(B=1 << 6, C=32, CP=32, dims=(1 << 11, 1 << 11, 1 << 11), pred_dims=(1 << 11, 1 << 11, 1 << 11), origin=(0, 0, 0))  # 2^32 workgroups


def test_descriptor_refusals(pkg, lib):
    v = lambda **kw: lib.pea_metrics_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_metrics_validate(None) == E_NULL and call(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(flags=RELU | STORE | MASK_F32) == OK and v(flags=DIVIDE | STORE) == OK and v(clip=(1e-6, 0.999999)) == OK
    assert v(clip=(0.5, 0.5)) == OK and v(C=12) == OK and v(dims=(6, 20, 24), origin=(0, 0, 0)) == OK
    bad = [dict(B=0), dict(B=-1), dict(C=0), dict(CP=0), dict(dims=(0, 14, 16)), dict(dims=(4, 0, 16)), dict(dims=(4, 14, -2)),
           dict(pred_dims=(6, 20, 0)), dict(pred_dims=(0, 20, 24)),
           dict(C=13), dict(C=33, CP=40),                                        # C > CP, C > PEA_MAX_K
           dict(origin=(-1, 3, 4)), dict(origin=(1, 3, -4)),                     # a negative origin
           dict(origin=(3, 3, 4)), dict(origin=(1, 7, 4)), dict(origin=(1, 3, 9)), dict(dims=(4, 14, 21)),   # the region leaves pred
           dict(origin=(2 ** 31 - 1, 3, 4)),                                     # (no overflow in origin + dims)
           dict(flags=16), dict(flags=RELU | 256), dict(flags=1 << 31),          # unknown flag bits
           dict(flags=STORE), dict(flags=STORE | MASK_F32),                      # STORE with neither RELU nor DIVIDE
           dict(flags=DIVIDE, B=2), dict(flags=DIVIDE | STORE | RELU, B=3),      # DIVIDE with B != 1
           dict(clip=(0.6, 0.5)), dict(clip=(float("nan"), 1.0)), dict(clip=(0.0, float("nan")))]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert call(pkg, lib, **kw) == E_DESC, kw
    assert v(C=32, CP=32) == OK and v(flags=RELU, B=2) == OK


def test_pointer_refusals_before_a_launch(pkg, lib):
    # PEA_E_NULL: pred, target or out missing; the weight map only with DIVIDE; the mask may be missing
    for ptr in ("pred", "target", "out"):
        assert call(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    assert call(pkg, lib, wmap=0, flags=DIVIDE) == E_NULL and call(pkg, lib, wmap=0, flags=DIVIDE | STORE) == E_NULL
    # PEA_E_ALIGN: 4 bytes for pred, weight_map, target and an f32 mask; 8 for out and workspace
    for ptr, base in (("pred", PRED), ("target", TGT)):
        for skew in (1, 2, 3):
            assert call(pkg, lib, **{ptr: base + skew}) == E_ALIGN, (ptr, skew)
    assert call(pkg, lib, wmap=WMAP + 2, flags=DIVIDE) == E_ALIGN
    assert call(pkg, lib, mask=MASK + 1, flags=MASK_F32) == E_ALIGN and call(pkg, lib, mask=MASK + 2, flags=MASK_F32 | RELU) == E_ALIGN
    assert call(pkg, lib, out=OUT + 4) == E_ALIGN and call(pkg, lib, work=WORK + 4) == E_ALIGN and call(pkg, lib, out=OUT + 1) == E_ALIGN
    # PEA_E_WORKSPACE: missing or short
    need = lib.pea_metrics_workspace_bytes()
    assert call(pkg, lib, work=0) == E_WORKSPACE and call(pkg, lib, wbytes=need - 1) == E_WORKSPACE and call(pkg, lib, wbytes=0) == E_WORKSPACE
    assert call(pkg, lib, wbytes=need // 5) == E_WORKSPACE
    # PEA_E_UNSUPPORTED: more than 2^31 - 1 workgroups of 4096 elements
    assert call(pkg, lib, **BIG) == E_UNSUPPORTED
    assert call(pkg, lib, flags=RELU | STORE, **dict(BIG, C=1, B=1 << 11)) == E_UNSUPPORTED      # (a STORE walk counts all CP channels)
    assert call(pkg, lib, B=1, C=1, CP=1, dims=(1, 1, 1), pred_dims=(1 << 15, 1 << 15, 1 << 15), origin=(0, 0, 0), flags=RELU | STORE) == E_UNSUPPORTED
    assert call(pkg, lib, B=1, C=1, CP=1, dims=(2 ** 31 - 1,) * 3, pred_dims=(2 ** 31 - 1,) * 3, origin=(0, 0, 0)) == E_UNSUPPORTED


def test_refusals_come_in_the_stated_order(pkg, lib):
    assert call(pkg, lib, work=0, **BIG) == E_WORKSPACE                               # the workspace before the grid
    assert call(pkg, lib, work=0, out=OUT + 4, **BIG) == E_ALIGN                      # alignment before the workspace
    assert call(pkg, lib, wbytes=0, work=WORK + 4, **BIG) == E_ALIGN
    assert call(pkg, lib, pred=PRED + 2, target=0, work=0, **BIG) == E_NULL           # NULL before alignment
    assert call(pkg, lib, pred=PRED + 2, wmap=0, flags=DIVIDE, B=1) == E_NULL
    assert call(pkg, lib, pred=0, target=0, out=0, work=0, flags=STORE) == E_DESC     # the descriptor before NULL
    assert call(pkg, lib, pred=0, clip=(1.0, 0.0)) == E_DESC and call(pkg, lib, out=0, C=0) == E_DESC
    # what a flag does not ask for is not looked at: the weight map without DIVIDE, a u8 mask's alignment, a missing mask
    assert call(pkg, lib, wmap=0, work=0) == E_WORKSPACE and call(pkg, lib, wmap=WMAP + 2, work=0) == E_WORKSPACE
    assert call(pkg, lib, mask=MASK + 1, work=0) == E_WORKSPACE and call(pkg, lib, mask=0, flags=MASK_F32, work=0) == E_WORKSPACE


def test_workspace_is_five_loss_states(pkg, lib):
    AffinitySpec, make_desc = pkg.AffinitySpec, pkg.affinity_op.make_desc
    one = 0
    for shape, offs in (((1, 16, 8, 8), [(0, 0, 1)]), ((2, 4, 3, 5, 7), [(0, 1, 0), (1, 0, 0)])):
        spec = AffinitySpec(len(shape) - 2, offs, None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_FULL, 1e-12)
        d = make_desc(spec, torch.empty(shape, device="meta"))
        nb = lib.pea_workspace_bytes(ctypes.byref(d))
        assert nb > 0 and (one == 0 or nb == one)
        one = nb
    assert lib.pea_metrics_workspace_bytes() == 5 * one and one % 64 == 0


# ---- the Python entry points -------------------------------------------------------------------------------------------------------
def test_python_entry_points_are_device_calls(pkg):
    """no CPU fallback behind affinity_metrics and VolumeStitcher.finish"""
    assert "affinity_metrics" in pkg.__all__ and "AffinityMetrics" in pkg.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.affinity_metrics(torch.zeros(1, 2, 6, 6), torch.zeros(1, 2, 6, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.affinity_metrics(torch.zeros(1, 2, 3, 6, 6), torch.zeros(1, 2, 3, 6, 6), torch.ones(1, 2, 3, 6, 6), relu=True, store=True)
    st = pkg.VolumeStitcher.__new__(pkg.VolumeStitcher)  # (the constructor itself refuses a CPU device)
    st.C, st.shape = 12, (6, 20, 24)
    st.out_affs, st.weight_map = torch.zeros(12, 6, 20, 24), torch.ones(1, 6, 20, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.finish((1, 3, 4), torch.zeros(3, 4, 14, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.VolumeStitcher(12, (6, 20, 24), (4, 8, 8), "cpu")


def test_metrics_switch_of_the_validation_section_needs_a_target(pkg):
    import inspect
    sig = inspect.signature(pkg.cvppp_validation_section)
    assert sig.parameters["metrics"].default is False
    with pytest.raises(ValueError):
        pkg.cvppp_validation_section(None, None, None, None, None, None, None, None, None, test_mode=True, metrics=True)


def test_affinity_metrics_object_reads_its_table_lazily(pkg):
    tab = torch.tensor([[0.5, 2.0, 3, 1, 2], [0.25, 1.0, 3, 0, 1], [0.75, 3.0, 0, 1, 1], [0.0, 0.0, 0, 0, 0]], dtype=torch.float64)
    m = pkg.AffinityMetrics(tab)
    assert m._host is None and m.table is tab
    assert (m.mse, m.bce, m.tp, m.fp, m.fn) == (0.5, 2.0, 3, 1, 2) and m.f1 == 6.0 / 9.0
    pc = m.per_channel
    assert pc["mse"] == [0.25, 0.75, 0.0] and pc["tp"] == [3, 0, 0] and pc["fn"] == [1, 1, 0]
    assert pc["f1"] == [6.0 / 7.0, 0.0, 0.0]  # (0.0 where the denominator is 0)


# ---- the restatement against the reference's numbers -----------------------------------------------------------------------------------
def rel(a, b):
    return abs(a - b) / abs(b)


def test_restatement_reproduces_the_2d_fixture():
    """MSELoss / BCELoss sum in float32, the restatement in float64: 1e-6 relative"""
    g = load_golden("gmetrics_2d")
    assert g["pred"].shape == (1, 4, 24, 40) and g["pred"].min() < -0.25 and g["pred"].max() > 1.25
    tab = metrics_reference(g["pred"], g["target"], g["mask"], relu=True, clip=(0.0, 1.0))
    assert rel(tab[0, 0], float(g["mse"])) <= 1e-6 and rel(tab[0, 1], float(g["bce"])) <= 1e-6
    assert np.array_equal(finished_pred(g["pred"], relu=True).view(np.int32), g["relu"].view(np.int32))
    # a float mask is the same mask
    assert np.array_equal(tab, metrics_reference(g["pred"], g["target"], g["mask"].astype(np.float32), relu=True))
    assert np.array_equal(tab[0, 2:], tab[1:, 2:].sum(axis=0)) and tab[0, 2:].sum() <= g["pred"].size


def test_restatement_reproduces_the_3d_fixture():
    g = load_golden("gmetrics_3d")
    acc = g["acc_f16"].astype(np.float32)
    assert acc.shape == (12, 6, 20, 24) and g["gt"].shape == (3, 4, 14, 16) and tuple(g["padding"]) == (1, 3, 4)
    tab = metrics_reference(acc[None], g["gt"][None].astype(np.float32), None, weight_map=g["weight_map"], origin=tuple(g["padding"]),
                            clip=(np.float32(1e-6), np.float32(0.999999)))
    assert rel(tab[0, 0], float(g["mse"])) <= 1e-6 and rel(tab[0, 1], float(g["bce"])) <= 1e-6
    assert [int(v) for v in tab[0, 2:]] == [int(v) for v in g["counts"]]
    assert f1(*[int(v) for v in tab[0, 2:]]) == float(g["f1"])
    vz, vy, vx = g["padding"]
    fin = finished_pred(acc[None], weight_map=g["weight_map"])[0]
    assert np.array_equal(fin[:3, vz:-vz, vy:-vy, vx:-vx].view(np.int32), g["results"].view(np.int32))
