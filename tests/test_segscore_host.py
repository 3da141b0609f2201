"""CPU: the segmentation scores (include/pea_segscore.h) -- the float64 restatement tests/segscore_reference.py, which the GPU tests
compare the kernels with, reproduces the reference's own numbers on every fixture (tests/golden/make_golden_segscore.py) to 1e-12,
its ARAND the value built from sklearn's pair confusion matrix and its VOI sklearn's entropy - mutual information; the header and the
library agree on the five new symbols, the ctypes mirror has the header's layout, the descriptor refusals are those of the header and
are reached before anything is launched (dummy device pointers, no GPU), the workspace grows with the capacity, and the Python layer
applies its dtype and range rules without a GPU."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from segscore_reference import ARE_COLUMNS, COL, COLUMNS, GOLDENS, contingency, load_seg_golden, seg_reference, seg_reference_image

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
NEW = ["pea_seg_scores", "pea_seg_table", "pea_seg_validate", "pea_seg_workspace_bytes", "pea_seg_workspace_init"]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_goldens(name):
    g = load_seg_golden(name)
    pred, gt = g["pred"], g["gt"]
    assert pred.dtype == np.int32 and gt.dtype == np.int32 and pred.shape == gt.shape
    r = seg_reference_image(pred, gt)
    for col in ("best_dice", "best_dice_rev", "sbd", "fgbg_dice"):
        print(name, col, r[COL[col]], float(g[col]))
        assert abs(r[COL[col]] - float(g[col])) <= 1e-12, col
    assert r[COL["diff_fg"]] == int(g["diff_fg"]) and r[COL["n_overflow"]] == 0 and r[COL["n_bad"]] == 0
    assert r[COL["sbd"]] == min(r[COL["best_dice"]], r[COL["best_dice_rev"]])
    # Dice(i, j) of the reference from the table: 2 n_ij / (a_i + b_j), 0 for absent labels
    p, q, n = contingency(pred, gt)
    for i, j, d in g["dice_ij"]:
        size = int(n[p == i].sum()) + int(n[q == j].sum())
        mine = 2.0 * int(n[(p == i) & (q == j)].sum()) / size if size else 0.0
        assert abs(mine - d) <= 1e-12, (i, j)
    assert (g["dice_ij"][:, 2] > 0).any() and (g["dice_ij"][:, 2] == 0).any()
    # what each fixture is there for
    if name == "gss_2d_offset_min":
        base = load_seg_golden("gss_2d_leaves")
        assert pred.min() == 3 and gt.min() == 5 and np.array_equal(pred, 2 * base["pred"] + 3)
        assert abs(2 * r[COL["best_dice"]] - float(base["best_dice"])) <= 1e-12  # the divisor max - min doubles, the sum stays
        assert r[COL["fgbg_dice"]] == float(base["fgbg_dice"])
    if name == "gss_one_label":
        assert pred.min() == pred.max() and r[COL["sbd"]] == 0 and r[COL["best_dice"]] == 0 and r[COL["n_pred_ids"]] == 1
    if name == "gss_3d_blocks":
        assert pred.ndim == 3


def _relabelled(name):
    g = load_seg_golden(name)
    return g["pred"].reshape(-1) + 1, g["gt"].reshape(-1) + 1  # no label 0: nothing is ignored


@pytest.mark.parametrize("name", GOLDENS)
def test_are_is_the_pair_confusion_matrix(name):
    from sklearn.metrics.cluster import pair_confusion_matrix
    pred, gt = _relabelled(name)
    r = seg_reference_image(pred, gt)
    C = pair_confusion_matrix(gt, pred).astype(np.float64)  # rows: pairs apart / together in gt; columns: in pred
    P2, A2, B2 = C[1, 1], C[0, 1] + C[1, 1], C[1, 0] + C[1, 1]  # together in both; together in pred; together in gt
    assert r[COL["n_prime"]] == pred.size
    assert r[COL["sum_nij2"]] - pred.size == P2 and r[COL["sum_ai2"]] - pred.size == A2 and r[COL["sum_bj2"]] - pred.size == B2
    assert math.isclose(r[COL["are"]], 1.0 - P2 / (0.5 * A2 + 0.5 * B2), rel_tol=1e-12)
    assert math.isclose(r[COL["are_precision"]], P2 / A2, rel_tol=1e-12) and math.isclose(r[COL["are_recall"]], P2 / B2, rel_tol=1e-12)


@pytest.mark.parametrize("name", GOLDENS)
def test_voi_is_entropy_minus_mutual_information(name):
    from sklearn.metrics import mutual_info_score
    from sklearn.metrics.cluster import entropy
    pred, gt = _relabelled(name)
    r = seg_reference_image(pred, gt)
    mi = mutual_info_score(gt, pred)
    split, merge = (entropy(pred) - mi) / math.log(2.0), (entropy(gt) - mi) / math.log(2.0)  # H(pred | gt), H(gt | pred) in bits
    print(name, r[COL["voi_split"]], split, r[COL["voi_merge"]], merge)
    assert abs(r[COL["voi_split"]] - split) <= 1e-10 and abs(r[COL["voi_merge"]] - merge) <= 1e-10


def test_restatement_ignores_gt_zero_and_counts_negative_labels():
    g = load_seg_golden("gss_2d_leaves")
    pred, gt = g["pred"].reshape(-1), g["gt"].reshape(-1)
    keep = gt != 0
    assert keep.any() and not keep.all()
    full, cut = seg_reference_image(pred, gt), seg_reference_image(pred[keep], gt[keep])
    for col in ARE_COLUMNS + ("voi_split", "voi_merge", "sum_nij2", "sum_ai2", "sum_bj2", "n_prime"):
        assert full[COL[col]] == cut[COL[col]], col
    zero = seg_reference_image(pred, np.zeros_like(gt))  # N' = 0
    assert zero[COL["n_prime"]] == 0 and zero[COL["voi_split"]] == 0 and zero[COL["voi_merge"]] == 0
    assert all(np.isnan(zero[COL[c]]) for c in ARE_COLUMNS) and zero[COL["sbd"]] == 0
    bad = pred.copy()
    bad[:3] = -1
    r = seg_reference(np.stack([bad, pred]), np.stack([gt, gt]))
    assert r[0, 1] == 3 and r[0, 0] == 0 and np.isnan(r[0, 2:]).all() and np.array_equal(r[1], full)


# ---- exports and layout ----------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_segscore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_SEGSCORE) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src and lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert re.search(r"#define\s+PEA_SEG_COLS\s+19\b", src) and pkg._lib.SEG_COLS == 19 == len(COLUMNS)
    assert re.search(r"#define\s+PEA_SEG_MIN_CAPACITY\s+64\b", src) and pkg._lib.SEG_MIN_CAPACITY == 64
    assert tuple(pkg._lib.SEG_COLUMNS) == COLUMNS
    for i, name in enumerate(COLUMNS):
        assert re.search(r"#define\s+PEA_SEG_%s\s+%d\b" % (name.upper(), i), src), name


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaSegDesc
    names = ["B", "S", "capacity", "flags"]
    assert [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == [0, 8, 16, 24] and ctypes.sizeof(D) == 32


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
PRED, GT, OUT, WORK, IDS, CNT, NOUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000


def desc(pkg, B=2, S=6336, capacity=256, flags=0):
    d = pkg._lib.PeaSegDesc()
    d.B, d.S, d.capacity, d.flags = B, S, capacity, flags
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def scores(pkg, lib, d="default", pred=PRED, gt=GT, out=OUT, work=WORK, wbytes=None, **kw):
    """pea_seg_scores on dummy pointers: anything but an early return would fault"""
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = 0 if d is None else lib.pea_seg_workspace_bytes(ctypes.byref(d))
    return lib.pea_seg_scores(None if d is None else ctypes.byref(d), vp(pred), vp(gt), vp(out), vp(work), wbytes, None)


def table(pkg, lib, d="default", b=0, pred=PRED, gt=GT, pi=IDS, gi=IDS + 0x1000, cnt=CNT, nout=NOUT, n_max=64, work=WORK, wbytes=None, **kw):
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = 0 if d is None else lib.pea_seg_workspace_bytes(ctypes.byref(d))
    return lib.pea_seg_table(None if d is None else ctypes.byref(d), vp(pred), vp(gt), b, vp(pi), vp(gi), vp(cnt), vp(nout), n_max, vp(work),
                             wbytes, None)


def test_descriptor_refusals(pkg, lib):
    v = lambda **kw: lib.pea_seg_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_seg_validate(None) == E_NULL and scores(pkg, lib, d=None) == E_NULL and table(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(B=1, S=1, capacity=64) == OK and v(capacity=1 << 20) == OK and v(S=2 ** 31 - 1) == OK
    bad = [dict(capacity=0), dict(capacity=-64), dict(capacity=32), dict(capacity=63), dict(capacity=65), dict(capacity=96), dict(capacity=255),
           dict(capacity=1 << 32), dict(B=0), dict(B=-1), dict(S=0), dict(S=-1), dict(flags=1), dict(flags=1 << 31)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert scores(pkg, lib, **kw) == E_DESC and table(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_seg_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    for S in (2 ** 31, 2 ** 40):
        assert v(S=S) == E_UNSUPPORTED and scores(pkg, lib, S=S) == E_UNSUPPORTED and table(pkg, lib, S=S) == E_UNSUPPORTED
        assert lib.pea_seg_workspace_bytes(ctypes.byref(desc(pkg, S=S))) == 0
    assert v(S=2 ** 31, capacity=100) == E_DESC  # PEA_E_UNSUPPORTED is checked last


def test_workspace_bytes_are_monotone_in_capacity(pkg, lib):
    ws = lambda **kw: lib.pea_seg_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    sizes = [ws(capacity=1 << k) for k in range(6, 22)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and all(a < b for a, b in zip(sizes, sizes[1:]))
    sizes = [ws(B=b) for b in (1, 2, 3, 8, 33)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert ws(S=1) == ws(S=2 ** 31 - 1)  # pixels play no part
    assert ws(B=2, capacity=256) == 8 * (8 + 32 * 2 + 10 * 2 * 256)  # a header, 32 words per image, 10 words per (image, slot)
    assert lib.pea_seg_workspace_bytes(None) == 0


def test_workspace_bytes(pkg, lib):
    ws = lambda **kw: lib.pea_seg_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    # a header of 8 words, 32 words per image, 10 words per (image, slot): the pair table (2) and the row and column tables (4 each)
    for B, cap in ((1, 64), (3, 64), (2, 256), (7, 1024), (33, 1 << 14), (1, 1 << 31), (2 ** 31 - 1, 64), (5, 1 << 21)):
        assert ws(B=B, capacity=cap) == 8 * (8 + 32 * B + 10 * B * cap), (B, cap)
    # 80 * (2^31 - 1) * 2^31 bytes are more than 2^64: the count does not fit
    assert ws(B=2 ** 31 - 1, capacity=2 ** 31) == 2 ** 64 - 1
    assert ws(B=2 ** 29, capacity=2 ** 31) == 2 ** 64 - 1 and ws(B=2 ** 26, capacity=2 ** 31) == 8 * (8 + 2 ** 31 + 10 * 2 ** 57)


def test_workspace_init_refusals(pkg, lib):
    f = lambda p, n: lib.pea_seg_workspace_init(vp(p), n, None)
    assert f(0, 4096) == E_NULL and f(WORK + 4, 4096) == E_ALIGN and f(WORK + 1, 4096) == E_ALIGN
    assert f(WORK, 0) == E_WORKSPACE and f(WORK, 56) == E_WORKSPACE and f(WORK, 4097) == E_WORKSPACE
    assert f(0, 0) == E_NULL and f(WORK + 4, 0) == E_ALIGN  # the order


def test_call_refusals_before_a_launch(pkg, lib):
    for ptr in ("pred", "gt", "out"):
        assert scores(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    for skew in (1, 2, 3):
        assert scores(pkg, lib, pred=PRED + skew) == E_ALIGN and scores(pkg, lib, gt=GT + skew) == E_ALIGN
    assert scores(pkg, lib, out=OUT + 4) == E_ALIGN and scores(pkg, lib, work=WORK + 4) == E_ALIGN
    need = lib.pea_seg_workspace_bytes(ctypes.byref(desc(pkg)))
    assert scores(pkg, lib, work=0) == E_WORKSPACE and scores(pkg, lib, wbytes=need - 8) == E_WORKSPACE and scores(pkg, lib, wbytes=0) == E_WORKSPACE
    # the stated order: descriptor, NULL, alignment, workspace, grid
    assert scores(pkg, lib, pred=0, out=OUT + 4, work=0) == E_NULL and scores(pkg, lib, out=OUT + 4, work=0) == E_ALIGN
    assert scores(pkg, lib, pred=0, gt=0, out=0, work=0, capacity=100) == E_DESC
    big = dict(B=1 << 21, S=1 << 20, capacity=64)  # exactly 2^31 workgroups of 1024 pixels: one too many
    assert scores(pkg, lib, **big) == E_UNSUPPORTED and scores(pkg, lib, work=0, **big) == E_WORKSPACE
    # pea_seg_table
    assert table(pkg, lib, b=-1) == E_DESC and table(pkg, lib, b=2) == E_DESC and table(pkg, lib, n_max=0) == E_DESC
    for ptr in ("pred", "gt", "pi", "gi", "cnt", "nout"):
        assert table(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    assert table(pkg, lib, pi=IDS + 2) == E_ALIGN and table(pkg, lib, cnt=CNT + 4) == E_ALIGN and table(pkg, lib, nout=NOUT + 4) == E_ALIGN
    assert table(pkg, lib, work=0) == E_WORKSPACE and table(pkg, lib, wbytes=need - 8) == E_WORKSPACE
    assert table(pkg, lib, b=5, pred=0) == E_DESC and table(pkg, lib, pred=0, cnt=CNT + 4) == E_NULL


# ---- the Python entry points ---------------------------------------------------------------------------------------------------------------
def test_python_exports_and_signatures(pkg):
    names = ("segmentation_scores", "SegmentationScores", "DiffFGLabels", "BestDice", "FGBGDice", "Dice", "AbsDiffFGLabels",
             "SymmetricBestDice", "adapted_rand_error", "variation_of_information")
    for name in names:
        assert name in pkg.SEGSCORE_EXPORTS and hasattr(pkg, name), name
    assert pkg.evaluate.SymmetricBestDice is pkg.SymmetricBestDice and pkg.seg_scores.adapted_rand_error is pkg.adapted_rand_error
    for name in ("DiffFGLabels", "BestDice", "FGBGDice", "AbsDiffFGLabels", "SymmetricBestDice"):
        assert list(inspect.signature(getattr(pkg, name)).parameters) == ["inLabel", "gtLabel"], name
    assert list(inspect.signature(pkg.Dice).parameters) == ["inLabel", "gtLabel", "i", "j"]
    sig = inspect.signature(pkg.adapted_rand_error)
    assert list(sig.parameters) == ["image_true", "image_test", "ignore_labels"] and sig.parameters["ignore_labels"].default == (0,)
    sig = inspect.signature(pkg.variation_of_information)
    assert list(sig.parameters) == ["image0", "image1", "ignore_labels"] and sig.parameters["ignore_labels"].default == (0,)
    sig = inspect.signature(pkg.segmentation_scores)
    assert sig.parameters["capacity"].default is None and sig.parameters["capacity"].kind is inspect.Parameter.KEYWORD_ONLY
    for prop in ("sbd", "best_dice", "best_dice_rev", "diff_fg", "abs_diff_fg", "fgbg_dice", "voi_split", "voi_merge", "voi", "are",
                 "are_precision", "are_recall", "n_overflow"):
        assert isinstance(getattr(pkg.SegmentationScores, prop), property), prop
    assert callable(pkg.SegmentationScores.contingency)


def test_shape_mismatch_returns_of_the_reference_and_ignore_labels(pkg):
    a, b = np.zeros((4, 5), np.int32), np.zeros((4, 6), np.int32)
    assert pkg.DiffFGLabels(a, b) == -1 and pkg.AbsDiffFGLabels(a, b) == 1
    assert pkg.BestDice(a, b) == 0 and pkg.FGBGDice(a, b) == 0 and pkg.Dice(a, b, 1, 1) == 0 and pkg.SymmetricBestDice(a, b) == 0
    for ig in ((1,), (0, 1), 2, (0, 0)):
        with pytest.raises(ValueError, match="ignore_labels"):
            pkg.adapted_rand_error(a, a, ignore_labels=ig)
        with pytest.raises(ValueError, match="ignore_labels"):
            pkg.variation_of_information(a, a, ignore_labels=ig)
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.adapted_rand_error(a, b)


def test_dtype_and_range_rules_without_a_gpu(pkg):
    mod = __import__(pkg.__name__ + ".harness.segscore", fromlist=["x"])
    to32 = mod.labels_int32
    for dt in (np.uint8, np.int16, np.uint16, np.int32, np.int64, np.uint64):
        x = np.array([[0, 7], [200, 3]]).astype(dt)
        t = to32(x)
        assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == [[0, 7], [200, 3]], dt
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
        t = to32(torch.tensor([[0, 7], [100, 3]], dtype=dt).t())  # a transposed view: what comes back is contiguous
        assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == [[0, 100], [7, 3]], dt
    assert to32(np.array([65535], np.uint16)).tolist() == [65535]  # widened, not reinterpreted
    assert to32(np.array([2 ** 31 - 1], np.int64)).tolist() == [2 ** 31 - 1]
    assert to32(np.array([-5], np.int64)).tolist() == [-5]  # negative ids reach the kernel, which counts them
    for big in (np.array([0, 2 ** 31], np.int64), np.array([2 ** 40], np.uint64), torch.tensor([2 ** 31]), torch.tensor([-2 ** 31 - 1])):
        with pytest.raises(ValueError, match="outside int32"):
            to32(big)
    for wrong in (np.zeros(3, np.float32), torch.zeros(3), torch.zeros(3, dtype=torch.bool), np.zeros(3, bool)):
        with pytest.raises(TypeError, match="integer ids"):
            to32(wrong)
    with pytest.raises(TypeError):
        pkg.segmentation_scores([1, 2], [1, 2])
    with pytest.raises(ValueError, match="differ in shape"):
        pkg.segmentation_scores(np.zeros((2, 3), np.int32), np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError, match="empty"):
        pkg.segmentation_scores(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
    with pytest.raises(TypeError, match="integer ids"):
        pkg.segmentation_scores(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32))
    # the default capacity: the power of two at or above S / 32 within [256, 32768]
    cap = mod.default_capacity
    assert [cap(s) for s in (1, 8192, 8193, 544 * 544, 1024 * 1024, 10 ** 8)] == [256, 256, 512, 16384, 32768, 32768]
