"""GPU: the instance scores of the BBBC039V1 validation loop (include/pea_instscore.h, csrc/pea_k_instscore.hip) through the C ABI,
through instance_scores and through the mirrors of utils/metrics_bbbc.py, against the reference's own numbers (tests/golden/gis_*.npz)
and the integer / float64 restatement tests/instscore_reference.py (which test_instscore_host.py holds to those numbers bit for bit).

Bars.  aji, dq and pixel_f1 are single f64 divisions of exact integers and every integer column is exact: compared on the bit patterns
(a NaN against a NaN).  sq, pq and sum_iou pass through the fixed-point sum with 32 fractional bits, each term truncated once and the
sum divided by at least the number of terms: 2^-24 absolute is the bar of test_gpu_segscore.py, with room to spare.  Everything called
bit-identical is compared on the bit patterns, NaNs included.  Every C call of this file runs in a guard-banded arena (arena.py):
pred and gt come back untouched, every element of out and of the two match tables is written, nothing else changes, and the
workspace is all zero but for its magic word afterwards."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from arena import Arena
from instscore_reference import (COL, COLUMNS, EXACT_COLUMNS, FIXED_COLUMNS, GOLDENS, INTEGER_COLUMNS, inst_reference, load_inst_golden,
                                 pq_lists)

pytestmark = pytest.mark.gpu
ABS_FIXED = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def is_clean(ws):
    words = ws.view(torch.int32)
    return int((words != 0).sum()) == 1 and int(words[0]) != 0


def raw(pkg, dev, pred, gt, capacity, max_id, match_iou=0.5, skew=(0, 0), tables=True):
    """pea_inst_scores on numpy [B, S] in an arena -> (out f64 [B, 18], aji_match, pq_match) on the device (None without tables)"""
    L = pkg._lib.lib()
    B, S = pred.shape
    d = pkg._lib.PeaInstDesc()
    d.B, d.S, d.capacity, d.max_id, d.match_iou, d.flags = B, S, capacity, max_id, match_iou, 0
    nb = L.pea_inst_workspace_bytes(ctypes.byref(d))
    assert nb > 0 and nb % 8 == 0
    ar = Arena(nb + 2 * (B * S * 4 + 256) + 2 * B * (max_id + 1) * 4 + (1 << 16), dev)
    P = ar.fill(ar.carve(pred.shape, torch.int32, skew[0], name="pred"), pred)
    G = ar.fill(ar.carve(gt.shape, torch.int32, skew[1], name="gt"), gt)
    out = ar.carve((B, len(COLUMNS)), torch.float64, 8, name="out")
    am = ar.carve((B, max_id + 1), torch.int32, 4, name="aji_match") if tables else None
    pm = ar.carve((B, max_id + 1), torch.int32, 12, name="pq_match") if tables else None
    ws = ar.carve((nb // 8,), torch.float64, name="workspace")
    assert P.data_ptr() % 16 == skew[0] and G.data_ptr() % 16 == skew[1]
    pkg._lib.check(L.pea_inst_workspace_init(vp(ws), nb, None), "pea_inst_workspace_init")
    for _ in range(2):  # the second call runs on the workspace as the first one left it
        pkg._lib.check(L.pea_inst_scores(ctypes.byref(d), vp(P), vp(G), vp(out), vp(am), vp(pm), vp(ws), nb, None), "pea_inst_scores")
        torch.cuda.synchronize()
        assert is_clean(ws), "the workspace is not clean after the call"
    ar.check(written=[out, ws] + ([am, pm] if tables else []), untouched=[P, G])
    return out.clone(), (am.clone() if tables else None), (pm.clone() if tables else None)


def close(what, got, ref):
    """device columns [B, 18] against the restatement's: the bars of the module docstring"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for b in range(ref.shape[0]):
        for name in COLUMNS:
            g, r = got[b, COL[name]], ref[b, COL[name]]
            print("%s image %d %-11s %.17g ref %.17g" % (what, b, name, g, r))
            if np.isnan(r):
                assert np.isnan(g), (what, b, name, g)
            elif name in INTEGER_COLUMNS or name in EXACT_COLUMNS:
                assert np.float64(g).tobytes() == np.float64(r).tobytes(), (what, b, name, g, r)
            else:
                assert name in FIXED_COLUMNS and abs(g - r) <= ABS_FIXED, (what, b, name, g, r)


def check(what, pkg, dev, pred, gt, capacity, max_id, **kw):
    """one C call against the restatement, match tables included -> the device results"""
    ref, ram, rpm = inst_reference(pred, gt, max_id)
    out, am, pm = raw(pkg, dev, pred, gt, capacity, max_id, **kw)
    close(what, out, ref)
    assert np.array_equal(am.cpu().numpy(), ram), what
    assert np.array_equal(pm.cpu().numpy(), rpm), what
    return out, am, pm


def blocks(seed, shape, block, bg=0.25):
    """a seeded blocky label image: an id of its own per block, some blocks background"""
    rng = np.random.default_rng(seed)
    cy, cx = (shape[0] + block - 1) // block, (shape[1] + block - 1) // block
    coarse = rng.permutation(np.arange(1, cy * cx + 1)).reshape(cy, cx)
    coarse = np.where(rng.random(coarse.shape) < bg, 0, coarse)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, axis=0), block, axis=1)[:shape[0], :shape[1]].astype(np.int32))


@functools.lru_cache(maxsize=None)
def base():
    """-> (pred, gt) int32 [3, 672]: three 24 x 28 images, shared by the tests (never modified: copy first)"""
    pred = np.stack([blocks(910 + b, (24, 28), 5) for b in range(3)]).reshape(3, -1)
    gt = np.stack([blocks(920 + b, (24, 28), 4) for b in range(3)]).reshape(3, -1)
    return pred, gt


# ---- 1. the reference's numbers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_fixtures(pkg, dev, name):
    g = load_inst_golden(name)
    pred, gt = g["pred"].reshape(1, -1), g["gt"].reshape(1, -1)
    max_id = int(max(pred.max(), gt.max()))
    out, am, pm = check(name, pkg, dev, pred, gt, 256, max_id)
    row = out.cpu().numpy()[0]
    for col in ("aji", "dq", "pixel_f1"):
        assert np.float64(row[COL[col]]).tobytes() == np.float64(g[col]).tobytes(), col
    for col in ("sq", "pq"):
        print(name, col, row[COL[col]], float(g[col]))
        assert abs(row[COL[col]] - float(g[col])) <= ABS_FIXED, col
    lists = pq_lists(g["pred"], g["gt"], pm.cpu().numpy()[0])
    for got, key in zip(lists, ("paired_true", "paired_pred", "unpaired_true", "unpaired_pred")):
        assert np.array_equal(np.asarray(got, np.int64), g[key]), key
    assert same_bits(out, raw(pkg, dev, pred, gt, 256, max_id, tables=False)[0])  # NULL match tables: the same columns


# ---- 2. shapes at which the kernels can go wrong ---------------------------------------------------------------------------------------------
def test_ragged_single_row_image(pkg, dev):
    rng = np.random.default_rng(31)
    S = 1031  # no multiple of 4, 256 or 1024
    pred = np.repeat(rng.integers(0, 40, (2, 150)), 7, axis=1)[:, :S].astype(np.int32)
    gt = np.repeat(rng.integers(0, 30, (2, 210)), 5, axis=1)[:, :S].astype(np.int32)
    check("S = 1031", pkg, dev, np.ascontiguousarray(pred), np.ascontiguousarray(gt), 1024, 39)


def test_batch_of_three(pkg, dev):
    pred, gt = base()
    check("B = 3", pkg, dev, pred, gt, 256, int(max(pred.max(), gt.max())))


def test_130_by_97(pkg, dev):
    pred, gt = blocks(41, (130, 97), 9).reshape(1, -1), blocks(42, (130, 97), 7).reshape(1, -1)
    check("130 x 97", pkg, dev, pred, gt, 2048, int(max(pred.max(), gt.max())))


def test_pointers_offset_by_one_element_give_the_same_bits(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    aligned = raw(pkg, dev, pred, gt, 256, max_id)
    for skew in ((4, 4), (4, 0), (12, 8)):
        got = raw(pkg, dev, pred, gt, 256, max_id, skew=skew)
        assert all(torch.equal(a, b) if a.dtype == torch.int32 else same_bits(a, b) for a, b in zip(got, aligned)), skew


def test_row_longer_than_a_wave(pkg, dev):
    """gt id 1 over 130 two-pixel predictions (the last one half outside it) whose ids fall along the image: 129 equal IoUs, the lowest
    id wins; gt id 2 takes the prediction that gt id 1 left"""
    S = 320
    gt = np.zeros((1, S), np.int32)
    gt[0, :260], gt[0, 260:300] = 1, 2
    pred = np.zeros((1, S), np.int32)
    for k in range(130):
        pred[0, 1 + 2 * k:3 + 2 * k] = 130 - k
    out, am, _ = check("a row of 130", pkg, dev, pred, gt, 256, 130)
    assert am[0, 1] == 2 and am[0, 2] == 1  # (pred id 1 is the one that straddles the border: every other one ties, 2 is the lowest)


def test_long_walk(pkg, dev):
    """300 present gt ids of 2 x 2 pixels in 40 x 60, the predictions moved by one pixel and renumbered"""
    rng = np.random.default_rng(53)
    cells = np.zeros(600, np.int32)
    cells[rng.permutation(600)[:300]] = rng.permutation(np.arange(1, 301))
    gt = np.repeat(np.repeat(cells.reshape(20, 30), 2, axis=0), 2, axis=1)
    renumber = np.concatenate([[0], rng.permutation(np.arange(1, 301))]).astype(np.int32)
    pred = np.roll(renumber[gt], (1, 1), axis=(0, 1))
    ref = inst_reference(pred.reshape(1, -1), gt.reshape(1, -1), 300)[0]
    assert ref[0, COL["n_gt_ids"]] == 300 and ref[0, COL["n_pred_ids"]] == 300
    check("a walk of 300", pkg, dev, np.ascontiguousarray(pred.reshape(1, -1)), np.ascontiguousarray(gt.reshape(1, -1)), 4096, 300)


def test_ids_at_the_ceiling_and_at_the_floor(pkg, dev):
    pred, gt = (x[:1].copy() for x in base())
    top_p, top_g = pred.copy(), gt.copy()
    top_p[pred == pred.max()], top_g[gt == gt.max()] = 65535, 65535
    top_p[pred == 1], top_g[gt == 2] = 65534, 65533
    out, am, pm = check("ids 65535", pkg, dev, top_p, top_g, 256, 65535)
    assert am[0, 65535] > 0
    one_p, one_g = (pred > 0).astype(np.int32), (gt % 2 == 1).astype(np.int32)
    check("max_id = 1", pkg, dev, one_p, one_g, 64, 1)
    check("max_id = 1, no pred", pkg, dev, np.zeros_like(one_p), one_g, 64, 1)  # aji 0: the walk falls back to the absent pred id 1
    out, _, _ = check("max_id = 1, nothing", pkg, dev, np.zeros_like(one_p), np.zeros_like(one_g), 64, 1)
    assert bool(torch.isnan(out[0, COL["aji"]])) and bool(torch.isnan(out[0, COL["pq"]])) and float(out[0, COL["sq"]]) == 0


@pytest.mark.parametrize("max_id", (2047, 2048, 2049))
def test_ids_around_a_lane_and_a_step_of_the_scan(pkg, dev, max_id):
    """k_inst_scan gives a lane 8 ids and takes 2048 ids a step, with a carry from step to step.  Image 0: gt ids 63, 64, 65, 2047, 2048
    and 2049, each over two predictions; an id above max_id is a bad label (n_bad, NaN scores).  Image 1: the ids up to 2047 alone, so
    that it is scored at every max_id"""
    ids = (63, 64, 65, 2047, 2048, 2049)
    gt = np.zeros((2, 16, 16), np.int32)
    pred = np.zeros((2, 16, 16), np.int32)
    for k, j in enumerate(ids):
        gt[0, 2 * k + 1:2 * k + 3, 2:14] = j
        pred[0, 2 * k + 1:2 * k + 3, 1:9], pred[0, 2 * k + 1:2 * k + 3, 9:15] = ids[5 - k], 7 + k
    gt[1], pred[1] = np.where(gt[0] > 2047, 0, gt[0]), np.where(pred[0] > 2047, 3, pred[0])
    ref = inst_reference(pred.reshape(2, -1), gt.reshape(2, -1), max_id)[0]
    assert (ref[0, COL["n_bad"]] == 0) == (max_id == 2049) and ref[1, COL["n_bad"]] == 0 and ref[1, COL["n_gt_ids"]] == 4
    check("max_id %d" % max_id, pkg, dev, pred.reshape(2, -1), gt.reshape(2, -1), 256, max_id)


# ---- 3. bad labels and a full table ------------------------------------------------------------------------------------------------------------
def test_bad_labels_stay_in_their_image(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    clean = raw(pkg, dev, pred, gt, 256, max_id)
    bad_p, bad_g = pred.copy(), gt.copy()
    bad_p[1, 5] = -1
    bad_g[1, 600] = max_id + 1
    out, am, pm = check("bad labels", pkg, dev, bad_p, bad_g, 256, max_id)
    assert float(out[1, COL["n_bad"]]) == 2 and float(out[1, COL["n_overflow"]]) == 0 and bool(torch.isnan(out[1, 2:]).all())
    assert not bool(am[1].any()) and not bool(pm[1].any())
    for b in (0, 2):
        assert same_bits(out[b], clean[0][b]) and torch.equal(am[b], clean[1][b]) and torch.equal(pm[b], clean[2][b])


def test_full_table_ends_the_call_and_capacities_agree(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    pairs = [len(np.unique(pred[b].astype(np.int64) << 32 | gt[b])) for b in range(3)]
    assert min(pairs) > 64 and max(pairs) < 128, pairs
    out, am, pm = raw(pkg, dev, pred, gt, 64, max_id)  # 64 slots, 80 and more pairs per image: the call returns
    print("n_overflow", out[:, 0].tolist())
    assert bool((out[:, COL["n_overflow"]] > 0).all()) and bool((out[:, COL["n_bad"]] == 0).all()) and bool(torch.isnan(out[:, 2:]).all())
    assert not bool(am.any()) and not bool(pm.any())
    a = check("capacity 256", pkg, dev, pred, gt, 256, max_id)  # the same images at two capacities that hold them
    b = raw(pkg, dev, pred, gt, 4096, max_id)
    assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_several_hundred_pairs_at_two_capacities(pkg, dev):
    pred, gt = blocks(61, (40, 60), 3, bg=0.1).reshape(1, -1), blocks(62, (40, 60), 4, bg=0.1).reshape(1, -1)
    max_id = int(max(pred.max(), gt.max()))
    a = check("capacity 1024", pkg, dev, pred, gt, 1024, max_id)  # loaded to more than a half: collisions are certain
    b = raw(pkg, dev, pred, gt, 4096, max_id)
    assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_uninitialised_workspace_gives_nan_and_zero_tables(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    L = pkg._lib.lib()
    d = pkg._lib.PeaInstDesc()
    d.B, d.S, d.capacity, d.max_id, d.match_iou, d.flags = 3, pred.shape[1], 256, max_id, 0.5, 0
    nb = L.pea_inst_workspace_bytes(ctypes.byref(d))
    ws = torch.zeros(nb // 8, dtype=torch.float64, device=dev)  # no magic word
    out = torch.zeros((3, len(COLUMNS)), dtype=torch.float64, device=dev)
    match = torch.full((2, 3, max_id + 1), -9, dtype=torch.int32, device=dev)
    P, G = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    pkg._lib.check(L.pea_inst_scores(ctypes.byref(d), vp(P), vp(G), vp(out), vp(match[0]), vp(match[1]), vp(ws), nb, None), "pea_inst_scores")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and not bool(match.any())


# ---- 4. the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_instance_scores_inputs_and_properties(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    out, am, pm = raw(pkg, dev, pred, gt, 256, max_id)
    shaped = lambda x: x.reshape(3, 24, 28)
    for conv in (shaped, lambda x: shaped(x).astype(np.uint16), lambda x: torch.from_numpy(shaped(x)).long()):
        sc = pkg.instance_scores(conv(pred), conv(gt))  # host inputs: max_id is their maximum
        assert sc.max_id == max_id and sc.capacity == 256 and sc.table.is_cuda and same_bits(sc.table, out)
    on_dev = pkg.instance_scores(torch.from_numpy(shaped(pred)).to(dev), torch.from_numpy(shaped(gt)).to(dev))  # device inputs: 65535
    assert on_dev.max_id == 65535 and same_bits(on_dev.table, out)
    assert np.array_equal(on_dev.aji_match(1)[:max_id + 1], am[1].cpu().numpy()) and not on_dev.aji_match(1)[max_id + 1:].any()
    host = out.cpu().numpy()
    assert sc.aji == host[:, COL["aji"]].tolist() and sc.pq == host[:, COL["pq"]].tolist() and sc.n_bad == [0, 0, 0] and sc.n_overflow == [0, 0, 0]
    assert sc.tp == [int(v) for v in host[:, COL["tp"]]] and all(isinstance(v, int) for v in sc.fp + sc.fn)
    for b in range(3):
        assert np.array_equal(sc.aji_match(b), am[b].cpu().numpy())
        want = pq_lists(pred[b], gt[b], pm[b].cpu().numpy())
        for mine, ref in zip(sc.pq_pairs(b), want):
            assert np.array_equal(np.asarray(mine), np.asarray(ref))
    one = pkg.instance_scores(shaped(pred)[2], torch.from_numpy(shaped(gt)[2]).to(dev), max_id=max_id)  # [Y, X]: one image
    assert isinstance(one.aji, float) and one.aji == sc.aji[2] and one.dq == sc.dq[2] and one.sq == sc.sq[2] and one.pixel_f1 == sc.pixel_f1[2]
    assert isinstance(one.tp, int) and one.tp == sc.tp[2]
    with pytest.raises(ValueError, match="power of two"):
        pkg.instance_scores(shaped(pred), shaped(gt), capacity=100)
    with pytest.raises(IndexError):
        sc.aji_match(3)


def test_overflow_is_retried_once_at_four_times_the_capacity(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    ref = inst_reference(pred, gt, max_id)[0]
    pairs = [len(np.unique(pred[b].astype(np.int64) << 32 | gt[b])) for b in range(3)]
    assert min(pairs) > 64 and max(pairs) < 200, pairs  # more pairs than 64 slots, and 256 hold them
    sc = pkg.instance_scores(pred.reshape(3, 24, 28), gt.reshape(3, 24, 28), capacity=64)
    assert sc.capacity == 64  # nothing is read yet
    close("retried", sc._rows(), ref)
    assert sc.capacity == 256 and sc.n_overflow == [0, 0, 0]
    dense_p, dense_g = blocks(61, (40, 60), 2, bg=0.0), blocks(62, (40, 60), 3, bg=0.0)  # 600 pred ids: 256 slots overflow too
    sc = pkg.instance_scores(dense_p, dense_g, capacity=64)
    with pytest.raises(RuntimeError, match="overflowed at capacity 64 and at 256"):
        sc.aji


def test_mirrors_return_the_fixtures_numbers(pkg, dev):
    for name in GOLDENS:
        g = load_inst_golden(name)
        pred, gt = g["pred"].astype(np.uint16), g["gt"].astype(np.uint16)
        assert np.float64(pkg.agg_jc_index(gt, pred)).tobytes() == np.float64(g["aji"]).tobytes(), name
        assert np.float64(pkg.pixel_f1(gt, pred)).tobytes() == np.float64(g["pixel_f1"]).tobytes(), name
        (dq, sq, pq), lists = pkg.get_fast_pq(gt, pred, match_iou=0.5)
        assert np.float64(dq).tobytes() == np.float64(g["dq"]).tobytes(), name
        assert abs(sq - float(g["sq"])) <= ABS_FIXED and abs(pq - float(g["pq"])) <= ABS_FIXED, name
        assert len(lists) == 4
        for mine, key in zip(lists, ("paired_true", "paired_pred", "unpaired_true", "unpaired_pred")):
            assert np.array_equal(np.asarray(mine, np.int64), g[key]), (name, key)
    g = load_inst_golden("gis_blocky")
    strict = pkg.get_fast_pq(g["gt"], g["pred"], match_iou=0.9)[0]
    assert strict[0] <= float(g["dq"])
    assert pkg.agg_jc_index(torch.from_numpy(g["gt"]).to(dev), torch.from_numpy(g["pred"])) == float(g["aji"])


# ---- 5. a captured call -------------------------------------------------------------------------------------------------------------------------------
def test_graphed_call_replays_the_eager_bits(pkg, dev):
    pred, gt = base()
    max_id = int(max(pred.max(), gt.max()))
    P, G = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)

    def step(P, G):
        sc = pkg.instance_scores(P, G, max_id=max_id, capacity=256, batched=True)  # [3, S]: three flattened images
        return sc.table, sc.match

    eager = [t.clone() for t in step(P, G)]
    close("eager", eager[0], inst_reference(pred, gt, max_id)[0])
    g = pkg.graphed(step, P, G)
    first = [t.clone() for t in g.replay()]
    second = [t.clone() for t in g.replay()]
    for got in (first, second):
        assert same_bits(got[0], eager[0]) and torch.equal(got[1], eager[1])
