"""CPU: the instance scores of the BBBC039V1 validation loop (include/pea_instscore.h) -- the integer / float64 restatement
tests/instscore_reference.py, which the GPU tests compare the kernels with, gives the reference's own aji, dq, sq and pq on every
fixture (tests/golden/make_golden_instscore.py) BIT FOR BIT, its pairing lists, and sklearn's f1_score; the header and the library
agree on the four new symbols, the ctypes mirror has the header's layout, the descriptor refusals are those of the header and are
reached before anything is launched (dummy device pointers, no GPU), the workspace grows with B, the capacity and max_id, and the
Python layer refuses wrong shapes, dtypes and match_iou < 0.5 without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from instscore_reference import COL, COLUMNS, GOLDENS, inst_reference, inst_reference_image, load_inst_golden, pq_lists

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
NEW = ["pea_inst_scores", "pea_inst_validate", "pea_inst_workspace_bytes", "pea_inst_workspace_init"]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def bits(x):
    return np.float64(x).tobytes()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_goldens_bit_for_bit(name):
    from sklearn.metrics import f1_score
    g = load_inst_golden(name)
    pred, gt = g["pred"], g["gt"]
    assert pred.dtype == np.int32 and gt.dtype == np.int32 and pred.shape == gt.shape == (24, 28)
    assert np.array_equal(np.unique(gt[gt > 0]), np.arange(1, gt.max() + 1))  # gt ids consecutive from 1
    r, aji_match, pq_match = inst_reference_image(pred, gt)
    for col in ("aji", "dq", "sq", "pq", "pixel_f1"):
        print(name, col, r[COL[col]], float(g[col]))
        assert bits(r[COL[col]]) == bits(g[col]), col
    f1 = f1_score((gt > 0).reshape(-1), (pred > 0).reshape(-1))
    assert abs(r[COL["pixel_f1"]] - f1) <= 1e-15
    mine = pq_lists(pred, gt, pq_match)
    for got, key in zip(mine, ("paired_true", "paired_pred", "unpaired_true", "unpaired_pred")):
        assert np.array_equal(np.asarray(got, np.int64), g[key]), key
    assert r[COL["tp"]] == len(g["paired_true"]) and r[COL["fp"]] == len(g["unpaired_pred"]) and r[COL["fn"]] == len(g["unpaired_true"])
    assert r[COL["n_overflow"]] == 0 and r[COL["n_bad"]] == 0 and aji_match[0] == 0 and pq_match[0] == 0
    assert (aji_match[1:gt.max() + 1] > 0).all()  # every present gt id takes a prediction
    # what each fixture is there for
    if name == "gis_pred_doubled":
        base = load_inst_golden("gis_blocky")
        assert np.array_equal(pred, 2 * base["pred"]) and not (pred == 1).any() and (aji_match == 1).any()
        assert all(bits(g[c]) == bits(base[c]) for c in ("aji", "dq", "sq", "pq", "pixel_f1"))  # the numbering plays no part
        assert np.array_equal(g["paired_pred"], 2 * base["paired_pred"])
    if name == "gis_gt_unmatched":
        assert not (pred[gt == 3] > 0).any() and aji_match[3] == 1 and aji_match[1] == 1 and pq_match[3] == 0
    if name == "gis_equal_iou":
        assert sorted(np.unique(pred[gt == 2]).tolist()) == [2, 3] and (pred == 2).sum() == (pred == 3).sum() and aji_match[2] == 2
    if name == "gis_runner_up":
        n11, n12 = int(((pred == 1) & (gt == 1)).sum()), int(((pred == 1) & (gt == 2)).sum())
        n22 = int(((pred == 2) & (gt == 2)).sum())
        iou = lambda n, i, j: n / float((pred == i).sum() + (gt == j).sum() - n)
        assert iou(n12, 1, 2) > iou(n22, 2, 2) > 0 and n11 > 0 and aji_match[1] == 1 and aji_match[2] == 2
    if name == "gis_one_pred_id":
        assert np.unique(pred).tolist() == [0, 1] and r[COL["n_pred_ids"]] == 1 and r[COL["tp"]] == 0


def test_restatement_edge_cases():
    g = load_inst_golden("gis_blocky")
    pred, gt = g["pred"], g["gt"]
    zero = np.zeros_like(pred)
    r, am, _ = inst_reference_image(zero, gt)  # a pred without ids: aji 0, every gt id takes pred id 1
    assert r[COL["aji"]] == 0 and r[COL["aji_union"]] == (gt > 0).sum() and (am[1:gt.max() + 1] == 1).all()
    assert r[COL["dq"]] == 0 and r[COL["sq"]] == 0 and r[COL["pixel_f1"]] == 0
    r, am, pm = inst_reference_image(zero, zero)  # neither has ids
    assert np.isnan(r[COL["aji"]]) and np.isnan(r[COL["dq"]]) and np.isnan(r[COL["pq"]]) and r[COL["sq"]] == 0 and r[COL["pixel_f1"]] == 0
    assert not am.any() and not pm.any()
    r, am, pm = inst_reference_image(pred, pred)  # a perfect match
    assert r[COL["aji"]] == 1 and r[COL["dq"]] == 1 and r[COL["pixel_f1"]] == 1 and abs(r[COL["sq"]] - 1) < 1e-6
    assert np.array_equal(am[1:], np.arange(1, pred.max() + 1)) and np.array_equal(am, pm)
    gap = np.where(gt > 2, gt + 3, gt)  # gt ids 3 .. 5 absent: skipped
    r2, am2, _ = inst_reference_image(pred, gap)
    assert bits(r2[COL["aji"]]) == bits(g["aji"]) and not am2[3:6].any() and np.array_equal(am2[6:gt.max() + 4], inst_reference_image(pred, gt)[1][3:gt.max() + 1])
    bad = pred.copy()
    bad[0, :3] = (-1, 999, 40)  # 40 is an id at max_id = 40, 999 is not
    r, am, pm = inst_reference(np.stack([bad, pred]), np.stack([gt, gt]), max_id=40)
    assert r[0, 1] == 2 and r[0, 0] == 0 and np.isnan(r[0, 2:]).all() and not am[0].any() and not pm[0].any()
    assert bits(r[1, COL["aji"]]) == bits(g["aji"]) and am.shape == (2, 41)


# ---- exports and layout ----------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_instscore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_INSTSCORE) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src and lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert re.search(r"#define\s+PEA_INST_COLS\s+18\b", src) and pkg._lib.INST_COLS == 18 == len(COLUMNS)
    assert re.search(r"#define\s+PEA_INST_MIN_CAPACITY\s+64\b", src) and pkg._lib.INST_MIN_CAPACITY == 64
    assert re.search(r"#define\s+PEA_INST_MAX_ID\s+65535\b", src) and pkg._lib.INST_MAX_ID == 65535
    assert tuple(pkg._lib.INST_COLUMNS) == COLUMNS
    for i, name in enumerate(COLUMNS):
        assert re.search(r"#define\s+PEA_INST_%s\s+%d\b" % (name.upper(), i), src), name
    for phrase in ("ABSENT between 1 and the maximum is skipped", "a pred without any id > 0 gives aji = 0"):
        assert phrase in src, phrase  # the two inputs that the reference leaves undefined are stated


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaInstDesc
    names = ["B", "S", "capacity", "max_id", "match_iou", "flags"]
    assert [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == [0, 8, 16, 24, 32, 40] and ctypes.sizeof(D) == 48


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
PRED, GT, OUT, WORK, AJI, PQ = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000


def desc(pkg, B=2, S=6336, capacity=256, max_id=200, match_iou=0.5, flags=0):
    d = pkg._lib.PeaInstDesc()
    d.B, d.S, d.capacity, d.max_id, d.match_iou, d.flags = B, S, capacity, max_id, match_iou, flags
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def scores(pkg, lib, d="default", pred=PRED, gt=GT, out=OUT, aji=AJI, pq=PQ, work=WORK, wbytes=None, **kw):
    """pea_inst_scores on dummy pointers: anything but an early return would fault"""
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = 0 if d is None else lib.pea_inst_workspace_bytes(ctypes.byref(d))
    return lib.pea_inst_scores(None if d is None else ctypes.byref(d), vp(pred), vp(gt), vp(out), vp(aji), vp(pq), vp(work), wbytes, None)


def test_descriptor_refusals(pkg, lib):
    v = lambda **kw: lib.pea_inst_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_inst_validate(None) == E_NULL and scores(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(B=1, S=1, capacity=64, max_id=1) == OK and v(capacity=1 << 20, max_id=65535) == OK and v(S=2 ** 31 - 1) == OK
    assert v(match_iou=0.75) == OK and v(match_iou=1.0) == OK
    bad = [dict(capacity=0), dict(capacity=-64), dict(capacity=32), dict(capacity=63), dict(capacity=65), dict(capacity=96),
           dict(capacity=1 << 32), dict(B=0), dict(B=-1), dict(S=0), dict(S=-1), dict(flags=1), dict(flags=1 << 31), dict(max_id=0),
           dict(max_id=-1), dict(max_id=65536), dict(match_iou=-0.1), dict(match_iou=1.5), dict(match_iou=float("nan"))]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert scores(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_inst_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    for kw in (dict(match_iou=0.49), dict(match_iou=0.0), dict(S=2 ** 31), dict(S=2 ** 40)):
        assert v(**kw) == E_UNSUPPORTED and scores(pkg, lib, **kw) == E_UNSUPPORTED, kw
        assert lib.pea_inst_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    assert v(S=2 ** 31, capacity=100) == E_DESC and v(match_iou=0.49, max_id=0) == E_DESC  # PEA_E_UNSUPPORTED is checked last


def test_workspace_bytes_increase_strictly(pkg, lib):
    ws = lambda **kw: lib.pea_inst_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    for sizes in ([ws(capacity=1 << k) for k in range(6, 22)], [ws(B=b) for b in (1, 2, 3, 8, 33)],
                  [ws(max_id=m) for m in (1, 2, 3, 4, 63, 64, 255, 256, 257, 4095, 65534, 65535)],
                  [ws(max_id=m, capacity=64) for m in (1, 2, 3, 62, 63, 64, 65, 66, 1000, 65535)]):
        assert all(s > 0 and s % 8 == 0 for s in sizes) and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert ws(S=1) == ws(S=2 ** 31 - 1) and ws(match_iou=0.5) == ws(match_iou=0.9)  # neither plays a part
    assert lib.pea_inst_workspace_bytes(None) == 0


def test_workspace_bytes(pkg, lib):
    ws = lambda **kw: lib.pea_inst_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    al8 = lambda x: (x + 7) // 8 * 8
    # a header of 8 words, 32 words per image, 6 words per (image, slot) (a pair and a row entry), 2 words per (image, present gt id) with
    # room for min(max_id + 1, capacity) of them, and three int32 per (image, id) that are padded to 8 bytes TOGETHER.  max_id + 1 below,
    # at and above the capacity; odd B * (max_id + 1) among them
    cases = ((1, 64, 1), (1, 64, 2), (3, 64, 62), (3, 64, 63), (3, 64, 64), (5, 64, 200), (2, 256, 200), (7, 256, 255), (7, 256, 256),
             (1, 1024, 65534), (33, 1 << 14, 65535), (3, 1 << 21, 4))
    for B, cap, max_id in cases:
        M = max_id + 1
        assert ws(B=B, capacity=cap, max_id=max_id) == 8 * (8 + 32 * B + 6 * B * cap + 2 * B * min(M, cap)) + al8(12 * B * M), (B, cap, max_id)
    # 48 * (2^31 - 1) * 2^31 bytes are more than 2^64: the count does not fit
    assert ws(B=2 ** 31 - 1, capacity=2 ** 31) == 2 ** 64 - 1 and ws(B=2 ** 31 - 1, capacity=2 ** 31, max_id=65535) == 2 ** 64 - 1


def test_workspace_init_refusals(pkg, lib):
    f = lambda p, n: lib.pea_inst_workspace_init(vp(p), n, None)
    assert f(0, 4096) == E_NULL and f(WORK + 4, 4096) == E_ALIGN and f(WORK + 1, 4096) == E_ALIGN
    assert f(WORK, 0) == E_WORKSPACE and f(WORK, 56) == E_WORKSPACE and f(WORK, 4097) == E_WORKSPACE
    assert f(0, 0) == E_NULL and f(WORK + 4, 0) == E_ALIGN  # the order


def test_call_refusals_before_a_launch(pkg, lib):
    for ptr in ("pred", "gt", "out"):
        assert scores(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    for skew in (1, 2, 3):
        assert scores(pkg, lib, pred=PRED + skew) == E_ALIGN and scores(pkg, lib, gt=GT + skew) == E_ALIGN
        assert scores(pkg, lib, aji=AJI + skew) == E_ALIGN and scores(pkg, lib, pq=PQ + skew) == E_ALIGN
    assert scores(pkg, lib, out=OUT + 4) == E_ALIGN and scores(pkg, lib, work=WORK + 4) == E_ALIGN
    need = lib.pea_inst_workspace_bytes(ctypes.byref(desc(pkg)))
    assert scores(pkg, lib, work=0) == E_WORKSPACE and scores(pkg, lib, wbytes=need - 8) == E_WORKSPACE and scores(pkg, lib, wbytes=0) == E_WORKSPACE
    assert scores(pkg, lib, aji=0, pq=0, work=0) == E_WORKSPACE  # the match tables may be NULL: the next refusal is reached
    # the stated order: descriptor, NULL, alignment, workspace, grid
    assert scores(pkg, lib, pred=0, out=OUT + 4, work=0) == E_NULL and scores(pkg, lib, out=OUT + 4, work=0) == E_ALIGN
    assert scores(pkg, lib, pred=0, gt=0, out=0, work=0, capacity=100) == E_DESC
    big = dict(B=1 << 21, S=1 << 20, capacity=64, max_id=1)  # exactly 2^31 workgroups of 1024 pixels: one too many
    assert scores(pkg, lib, **big) == E_UNSUPPORTED and scores(pkg, lib, work=0, **big) == E_WORKSPACE


# ---- the Python entry points ---------------------------------------------------------------------------------------------------------------
def test_python_exports_and_signatures(pkg):
    for name in ("instance_scores", "InstanceScores", "metrics_bbbc", "agg_jc_index", "get_fast_pq", "pixel_f1", "remap_label"):
        assert name in pkg.INSTSCORE_EXPORTS and hasattr(pkg, name), name
    mb = pkg.metrics_bbbc
    assert mb.agg_jc_index is pkg.agg_jc_index and mb.BestDice is pkg.BestDice and mb.FGBGDice is pkg.FGBGDice
    assert list(inspect.signature(mb.agg_jc_index).parameters) == ["gt_ins", "pred"]
    assert list(inspect.signature(mb.pixel_f1).parameters) == ["gt_ins", "pred_ins"]
    sig = inspect.signature(mb.get_fast_pq)
    assert list(sig.parameters) == ["true", "pred", "match_iou"] and sig.parameters["match_iou"].default == 0.5
    sig = inspect.signature(mb.remap_label)
    assert list(sig.parameters) == ["pred", "by_size"] and sig.parameters["by_size"].default is False
    sig = inspect.signature(pkg.instance_scores)
    assert list(sig.parameters) == ["pred", "gt", "max_id", "capacity", "batched", "match_iou"]
    for name in ("max_id", "capacity", "batched", "match_iou"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["match_iou"].default == 0.5 and sig.parameters["max_id"].default is None
    for prop in ("aji", "dq", "sq", "pq", "pixel_f1", "tp", "fp", "fn", "n_bad", "n_overflow"):
        assert isinstance(getattr(pkg.InstanceScores, prop), property), prop
    assert callable(pkg.InstanceScores.aji_match) and callable(pkg.InstanceScores.pq_pairs)


def test_wrappers_refuse_without_a_gpu(pkg):
    a, b = np.zeros((4, 5), np.int32), np.zeros((4, 6), np.int32)
    with pytest.raises(NotImplementedError, match="Munkres"):
        pkg.instance_scores(a, a, match_iou=0.49)
    with pytest.raises(NotImplementedError, match="Munkres"):
        pkg.get_fast_pq(a, a, match_iou=0.3)
    with pytest.raises(ValueError, match="match_iou"):
        pkg.instance_scores(a, a, match_iou=1.5)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.instance_scores(a, b)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.agg_jc_index(a, b)
    with pytest.raises(ValueError, match="empty"):
        pkg.instance_scores(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
    for wrong in (np.zeros((4, 5), np.float32), torch.zeros(4, 5), np.zeros((4, 5), bool)):
        with pytest.raises(TypeError, match="integer ids"):
            pkg.instance_scores(wrong, a)
        with pytest.raises(TypeError, match="integer ids"):
            pkg.pixel_f1(a, wrong)
    with pytest.raises(TypeError):
        pkg.instance_scores([1, 2], [1, 2])
    for m in (0, -3, 65536):
        with pytest.raises(ValueError, match="max_id"):
            pkg.instance_scores(a, a, max_id=m)
    with pytest.raises(ValueError, match="outside int32"):
        pkg.instance_scores(np.full((4, 5), 2 ** 31, np.int64), a)


def test_default_max_id_and_remap_label(pkg):
    mod = __import__(pkg.__name__ + ".harness.instscore", fromlist=["x"])
    z = np.zeros((3, 4), np.uint16)
    big = z.copy()
    big[0, 0] = 300
    assert mod.default_max_id(z, z) == 1 and mod.default_max_id(big, z) == 300 and mod.default_max_id(z, torch.from_numpy(big.astype(np.int32))) == 300
    assert mod.default_max_id(np.full((2, 2), 70000, np.int32), z) == 65535  # ids above the ceiling are counted in n_bad by the kernel
    lab = np.array([[0, 7, 7, 7], [3, 3, 0, 9]], np.int32)
    assert pkg.remap_label(lab).tolist() == [[0, 2, 2, 2], [1, 1, 0, 3]] and pkg.remap_label(lab).dtype == np.int32
    assert pkg.remap_label(lab, by_size=True).tolist() == [[0, 1, 1, 1], [2, 2, 0, 3]]
    none = np.zeros((2, 2), np.int32)
    assert pkg.remap_label(none) is none
    for name in GOLDENS:  # the PQ numbers do not depend on the numbering
        g = load_inst_golden(name)
        shuffled = (g["pred"] * 7) % 101
        assert len(np.unique(shuffled)) == len(np.unique(g["pred"]))
        r = inst_reference_image(pkg.remap_label(shuffled), g["gt"])[0]
        assert all(bits(r[COL[c]]) == bits(g[c]) for c in ("dq", "pixel_f1")) and abs(r[COL["sq"]] - float(g["sq"])) < 1e-12
