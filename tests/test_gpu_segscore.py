"""GPU: the segmentation scores (include/pea_segscore.h, csrc/pea_k_segscore.hip) through the C ABI, through segmentation_scores and
through the mirrors of utils/evaluate.py and utils/seg_scores.py, against the float64 restatement tests/segscore_reference.py (which
test_segscore_host.py holds to the reference's numbers and to sklearn) and the reference's own numbers (tests/golden/gss_*.npz).

Bars.  The integer columns (counts, squares, diff_fg, n_bad, n_overflow) are compared exactly.  are / are_precision / are_recall are
f64 quotients of exact integers: 1e-12 relative.  sbd, best_dice*, fgbg_dice and voi_* pass through fixed-point sums with 32
fractional bits, each term truncated once and the sum divided by at least the number of terms: 2^-24 absolute is the bar, with room
to spare.  Everything called bit-identical is compared on the bit patterns, NaNs included.  Every C call of this file starts from an
`out` filled with a pattern and checks afterwards that the workspace is all zero but for its magic word."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from arena import Arena
from segscore_reference import (ARE_COLUMNS, COL, COLUMNS, DICE_VOI_COLUMNS, GOLDENS, INTEGER_COLUMNS, contingency, load_seg_golden,
                                seg_reference)

pytestmark = pytest.mark.gpu
ABS_FIXED, REL_ARE = 2.0 ** -24, 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def raw_desc(pkg, B, S, capacity):
    d = pkg._lib.PeaSegDesc()
    d.B, d.S, d.capacity, d.flags = B, S, capacity, 0
    return d


def new_state(pkg, dev, d):
    L = pkg._lib.lib()
    nb = L.pea_seg_workspace_bytes(ctypes.byref(d))
    assert nb > 0
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    pkg._lib.check(L.pea_seg_workspace_init(vp(ws), nb, None), "pea_seg_workspace_init")
    return ws, nb


def is_clean(ws):
    words = ws.view(torch.int32)
    return int((words != 0).sum()) == 1 and int(words[0]) != 0


def raw_scores(pkg, dev, pred, gt, capacity, state=None, out=None, poison=-7.0):
    """pea_seg_scores on device tensors [B, S] -> out f64 [B, 19] (still on the device)"""
    L = pkg._lib.lib()
    B, S = int(pred.shape[0]), int(pred[0].numel())
    d = raw_desc(pkg, B, S, capacity)
    ws, nb = state if state is not None else new_state(pkg, dev, d)
    assert nb >= L.pea_seg_workspace_bytes(ctypes.byref(d))
    if out is None:
        out = torch.empty((B, len(COLUMNS)), dtype=torch.float64, device=dev)
    out.fill_(poison)
    pkg._lib.check(L.pea_seg_scores(ctypes.byref(d), vp(pred), vp(gt), vp(out), vp(ws), nb, None), "pea_seg_scores")
    torch.cuda.synchronize()
    assert is_clean(ws), "the workspace is not clean after the call"
    return out


def close(what, got, ref):
    """device columns [B, 19] against the restatement's: the bars of the module docstring"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for b in range(ref.shape[0]):
        for name in COLUMNS:
            g, r = got[b, COL[name]], ref[b, COL[name]]
            print("%s image %d %-14s %.17g ref %.17g" % (what, b, name, g, r))
            if np.isnan(r):
                assert np.isnan(g), (what, b, name, g)
            elif name in INTEGER_COLUMNS:
                assert g == r, (what, b, name, g, r)
            elif name in ARE_COLUMNS:
                assert g == r or abs(g - r) <= REL_ARE * abs(r), (what, b, name, g, r)
            else:
                assert name in DICE_VOI_COLUMNS and abs(g - r) <= ABS_FIXED, (what, b, name, g, r)


@functools.lru_cache(maxsize=None)
def base(dims):
    """-> (pred, gt) int32 [2, S]: seeded, shared by the tests (never modified: copy first)"""
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    pred = synth.synth_labels(2, dims, 901, cell=16, n=15).reshape(2, -1).astype(np.int32)
    gt = synth.synth_labels(2, dims, 902, cell=12, n=11).reshape(2, -1).astype(np.int32)
    return pred, gt


@functools.lru_cache(maxsize=None)
def base_ref(dims):
    return seg_reference(*base(dims))


FLAT, VOLUME = (1, 72, 88), (6, 48, 96)


# ---- 1. the base shapes at two capacities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,pairs", [(FLAT, (74, 76)), (VOLUME, (88, 94))], ids=["72x88", "6x48x96"])
def test_base_shapes_at_two_capacities(pkg, dev, dims, pairs):
    pred, gt = base(dims)
    ref = base_ref(dims)
    assert tuple(int(v) for v in ref[:, COL["n_pairs"]]) == pairs  # capacity 128 is loaded to 0.6 - 0.75: collisions are certain
    P, G = cu(pred, dev), cu(gt, dev)
    a = raw_scores(pkg, dev, P, G, 256)
    close("capacity 256", a, ref)
    state = new_state(pkg, dev, raw_desc(pkg, 2, P.shape[1], 128))
    b = raw_scores(pkg, dev, P, G, 128, state=state)
    close("capacity 128", b, ref)
    c = raw_scores(pkg, dev, P, G, 128, state=state, poison=3.0)  # the same workspace again, out from another pattern
    assert same_bits(a, b) and same_bits(b, c)


# ---- 2. a table with fewer slots than pairs ----------------------------------------------------------------------------------------------------
def test_full_table_ends_the_call_and_touches_nothing_else(pkg, dev):
    pred, gt = base(FLAT)
    L = pkg._lib.lib()
    ar = Arena(1 << 20, dev)
    nb = L.pea_seg_workspace_bytes(ctypes.byref(raw_desc(pkg, 2, pred.shape[1], 256)))
    P = ar.fill(ar.carve(pred.shape, torch.int32, name="pred"), pred)
    G = ar.fill(ar.carve(gt.shape, torch.int32, name="gt"), gt)
    out = ar.carve((2, len(COLUMNS)), torch.float64, name="out")
    ws = ar.carve((nb // 8,), torch.float64, name="workspace")
    pkg._lib.check(L.pea_seg_workspace_init(vp(ws), nb, None), "pea_seg_workspace_init")
    got = raw_scores(pkg, dev, P, G, 64, state=(ws, nb), out=out).cpu().numpy()  # 64 slots, 74 and 76 pairs
    ar.check(written=[out, ws], untouched=[P, G])
    print("n_overflow", got[:, 0])
    assert (got[:, COL["n_overflow"]] > 0).all() and (got[:, COL["n_bad"]] == 0).all() and np.isnan(got[:, 2:]).all()
    again = raw_scores(pkg, dev, P, G, 256, state=(ws, nb), out=out)  # the same workspace serves the next call
    ar.check(written=[out, ws], untouched=[P, G])
    close("after a full table", again, base_ref(FLAT))
    assert same_bits(again, raw_scores(pkg, dev, P, G, 256))


def test_uninitialised_workspace_gives_nan(pkg, dev):
    pred, gt = base(FLAT)
    d = raw_desc(pkg, 2, pred.shape[1], 256)
    nb = pkg._lib.lib().pea_seg_workspace_bytes(ctypes.byref(d))
    ws = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    out = torch.zeros((2, len(COLUMNS)), dtype=torch.float64, device=dev)
    pkg._lib.check(pkg._lib.lib().pea_seg_scores(ctypes.byref(d), vp(cu(pred, dev)), vp(cu(gt, dev)), vp(out), vp(ws), nb, None), "pea_seg_scores")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- 3. ragged tails and element-aligned pointers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [6336 - 3, 1])
def test_ragged_tail(pkg, dev, S):
    pred, gt = (np.ascontiguousarray(x[:, :S]) for x in base(FLAT))
    close("S = %d" % S, raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 256), seg_reference(pred, gt))


def test_pointers_offset_by_one_element_give_the_same_bits(pkg, dev):
    pred, gt = base(FLAT)
    aligned = raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 256)
    for skew_p, skew_g in ((4, 4), (4, 0), (12, 8)):
        ar = Arena(1 << 20, dev)
        P = ar.fill(ar.carve(pred.shape, torch.int32, skew_p, name="pred"), pred)
        G = ar.fill(ar.carve(gt.shape, torch.int32, skew_g, name="gt"), gt)
        out = ar.carve((2, len(COLUMNS)), torch.float64, 8, name="out")
        assert P.data_ptr() % 16 == skew_p and G.data_ptr() % 16 == skew_g
        got = raw_scores(pkg, dev, P, G, 256, out=out)
        ar.check(written=[out], untouched=[P, G])
        assert same_bits(got, aligned), (skew_p, skew_g)


# ---- 4. the edge cases of the scores -----------------------------------------------------------------------------------------------------------------
def test_edge_cases_of_the_scores(pkg, dev):
    pred, gt = base(FLAT)
    one = np.full_like(pred, 4)  # max == min
    got = raw_scores(pkg, dev, cu(one, dev), cu(gt, dev), 256)
    close("pred with one label", got, seg_reference(one, gt))
    assert (got[:, COL["sbd"]] == 0).all() and (got[:, COL["best_dice"]] == 0).all()
    zero = np.zeros_like(gt)  # N' = 0
    got = raw_scores(pkg, dev, cu(pred, dev), cu(zero, dev), 256)
    close("gt all zero", got, seg_reference(pred, zero))
    assert (got[:, COL["n_prime"]] == 0).all() and (got[:, COL["voi_split"]] == 0).all() and bool(torch.isnan(got[:, COL["are"]]).all())
    up_p, up_g = pred + 3, 2 * gt + 5  # the lowest label is not 0; every second integer of gt's range is absent
    got = raw_scores(pkg, dev, cu(up_p, dev), cu(up_g, dev), 256)
    ref = seg_reference(up_p, up_g)
    close("lowest label above 0", got, ref)
    assert np.array_equal(ref[:, COL["best_dice"]], base_ref(FLAT)[:, COL["best_dice"]]) and (ref[:, COL["n_prime"]] == pred.shape[1]).all()


def test_negative_labels_stay_in_their_image(pkg, dev):
    pred, gt = base(FLAT)
    clean = raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 256)
    bad_p, bad_g = pred.copy(), gt.copy()
    bad_p[1, [0, 100, 6335]] = (-1, -2 ** 31, -7)
    bad_g[1, [100, 4000]] = (-1, -3)  # pixel 100 holds two negative values: both are counted
    state = new_state(pkg, dev, raw_desc(pkg, 2, pred.shape[1], 256))
    got = raw_scores(pkg, dev, cu(bad_p, dev), cu(bad_g, dev), 256, state=state)
    close("negative labels", got, seg_reference(bad_p, bad_g))
    assert float(got[1, COL["n_bad"]]) == 5 and float(got[1, COL["n_overflow"]]) == 0 and bool(torch.isnan(got[1, 2:]).all())
    assert same_bits(got[0], clean[0])
    assert same_bits(raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 256, state=state), clean)


@functools.lru_cache(maxsize=None)
def many_ids():
    """1 x 64 x 64 with an id of its own in every 2 x 2 cell (1024 ids) against the blocky gt: some 1100 pairs, and a wave's 256 pixels
    (four image rows) meet more than 64 of them"""
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    pred = (1 + np.arange(1024, dtype=np.int32).reshape(32, 32)).repeat(2, axis=0).repeat(2, axis=1).reshape(1, -1)
    gt = synth.synth_labels(1, (1, 64, 64), 902, cell=11, n=11).reshape(1, -1).astype(np.int32)
    return np.ascontiguousarray(pred), gt


def test_many_ids(pkg, dev):
    pred, gt = many_ids()
    ref = seg_reference(pred, gt)
    assert ref[0, COL["n_pred_ids"]] == 1024 and 1024 < ref[0, COL["n_pairs"]] < 2048
    a = raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 4096)
    close("many ids", a, ref)
    assert same_bits(a, raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 8192))


# ---- 5. the table itself -------------------------------------------------------------------------------------------------------------------------------
def test_table_triples_equal_np_unique(pkg, dev):
    pred, gt = base(VOLUME)
    L = pkg._lib.lib()
    P, G = cu(pred, dev), cu(gt, dev)
    d = raw_desc(pkg, 2, pred.shape[1], 256)
    ws, nb = new_state(pkg, dev, d)
    for b in (1, 0):
        ids = torch.full((2, 256), -9, dtype=torch.int32, device=dev)
        counts = torch.full((256,), -9, dtype=torch.int64, device=dev)
        n_out = torch.full((3,), -9, dtype=torch.int64, device=dev)
        pkg._lib.check(L.pea_seg_table(ctypes.byref(d), vp(P), vp(G), b, vp(ids[0]), vp(ids[1]), vp(counts), vp(n_out), 256, vp(ws), nb, None),
                       "pea_seg_table")
        torch.cuda.synchronize()
        assert is_clean(ws)
        rp, rg, rn = contingency(pred[b], gt[b])
        assert n_out.tolist() == [len(rn), 0, 0]
        p, g, n = ids[0, :len(rn)].cpu().numpy(), ids[1, :len(rn)].cpu().numpy(), counts[:len(rn)].cpu().numpy()
        order = np.lexsort((g, p))
        assert np.array_equal(p[order], rp) and np.array_equal(g[order], rg) and np.array_equal(n[order], rn)
        assert bool((ids[:, len(rn):] == -9).all()) and bool((counts[len(rn):] == -9).all())
    close("after the tables", raw_scores(pkg, dev, P, G, 256, state=(ws, nb)), base_ref(VOLUME))  # the workspace serves either call
    sc = pkg.segmentation_scores(P.reshape(2, 6, 48, 96), G.reshape(2, 6, 48, 96), capacity=256)
    for b in (0, 1):
        for mine, want in zip(sc.contingency(b), contingency(pred[b], gt[b])):
            assert np.array_equal(mine, want)


# ---- 6. the Python layer ---------------------------------------------------------------------------------------------------------------------------------
def test_segmentation_scores_inputs_and_properties(pkg, dev):
    pred, gt = base(FLAT)
    ref = base_ref(FLAT)
    raw = raw_scores(pkg, dev, cu(pred, dev), cu(gt, dev), 256)
    shaped = lambda x: x.reshape(2, 72, 88)
    for conv in (lambda x: cu(shaped(x), dev), shaped, lambda x: torch.from_numpy(shaped(x)).long(), lambda x: shaped(x).astype(np.uint8),
                 lambda x: cu(shaped(x), dev).to(torch.int16), lambda x: shaped(x).astype(np.uint16), lambda x: cu(shaped(x), dev).long()):
        sc = pkg.segmentation_scores(conv(pred), conv(gt))
        assert sc.capacity == 256 and sc.table.is_cuda and same_bits(sc.table, raw)
    assert sc.sbd == [float(v) for v in raw[:, COL["sbd"]]] and sc.n_overflow == [0, 0] and sc.n_bad == [0, 0]
    assert sc.diff_fg == [int(v) for v in ref[:, COL["diff_fg"]]] and sc.abs_diff_fg == [abs(v) for v in sc.diff_fg]
    assert sc.voi == [a + b for a, b in zip(sc.voi_split, sc.voi_merge)]
    one = pkg.segmentation_scores(shaped(pred)[1], cu(shaped(gt)[1], dev))  # [Y, X]: one image; a host and a device operand
    assert isinstance(one.sbd, float) and one.sbd == sc.sbd[1] and one.are == sc.are[1] and one.voi == sc.voi[1]
    assert isinstance(one.diff_fg, int) and one.are_precision == sc.are_precision[1] and one.fgbg_dice == sc.fgbg_dice[1]
    with pytest.raises(ValueError, match="outside int32"):
        pkg.segmentation_scores(cu(shaped(pred), dev).long() + 2 ** 31, cu(shaped(gt), dev))
    with pytest.raises(ValueError, match="power of two"):
        pkg.segmentation_scores(shaped(pred), shaped(gt), capacity=100)


def test_overflow_is_retried_once_at_four_times_the_capacity(pkg, dev):
    pred, gt = base(FLAT)
    sc = pkg.segmentation_scores(pred.reshape(2, 72, 88), gt.reshape(2, 72, 88), capacity=64)
    assert sc.capacity == 64  # nothing is read yet
    close("retried", np.stack([np.asarray(sc._rows()[b]) for b in range(2)]), base_ref(FLAT))
    assert sc.capacity == 256 and sc.n_overflow == [0, 0]
    many_p, many_g = many_ids()
    sc = pkg.segmentation_scores(many_p.reshape(64, 64), many_g.reshape(64, 64), capacity=64)  # some 1100 pairs: 256 slots overflow too
    with pytest.raises(RuntimeError, match="overflowed at capacity 64 and at 256"):
        sc.sbd


def test_mirrors_return_the_goldens_values(pkg, dev):
    for name in GOLDENS:
        g = load_seg_golden(name)
        pred, gt = g["pred"], g["gt"]
        ref = seg_reference(pred[None], gt[None])[0]
        assert abs(pkg.BestDice(pred, gt) - float(g["best_dice"])) <= ABS_FIXED and abs(pkg.BestDice(gt, pred) - float(g["best_dice_rev"])) <= ABS_FIXED
        assert abs(pkg.SymmetricBestDice(cu(pred, dev), cu(gt, dev)) - float(g["sbd"])) <= ABS_FIXED
        assert abs(pkg.FGBGDice(pred, torch.from_numpy(gt)) - float(g["fgbg_dice"])) <= ABS_FIXED
        assert pkg.DiffFGLabels(pred, gt) == int(g["diff_fg"]) and pkg.AbsDiffFGLabels(pred, gt) == abs(int(g["diff_fg"]))
        for i, j, d in g["dice_ij"]:
            assert abs(pkg.Dice(pred, gt, int(i), int(j)) - d) <= 1e-12, (name, i, j)
        are, prec, rec = pkg.adapted_rand_error(gt, pred, ignore_labels=(0))
        for mine, col in ((are, "are"), (prec, "are_precision"), (rec, "are_recall")):
            assert abs(mine - ref[COL[col]]) <= REL_ARE * abs(ref[COL[col]]), (name, col)
        voi = pkg.variation_of_information(gt, pred)
        assert voi.shape == (2,) and abs(voi[0] - ref[COL["voi_split"]]) <= ABS_FIXED and abs(voi[1] - ref[COL["voi_merge"]]) <= ABS_FIXED
        all_ref = seg_reference(pred[None], gt[None] + 1)[0]  # nothing ignored: gt's ids moved off 0
        are0 = pkg.adapted_rand_error(gt, pred, ignore_labels=())[0]
        voi0 = pkg.variation_of_information(gt, pred, ignore_labels=())
        assert abs(are0 - all_ref[COL["are"]]) <= REL_ARE * abs(all_ref[COL["are"]]) and abs(voi0[0] - all_ref[COL["voi_split"]]) <= ABS_FIXED
        assert abs(voi0[1] - all_ref[COL["voi_merge"]]) <= ABS_FIXED


# ---- 7. a captured call -------------------------------------------------------------------------------------------------------------------------------------
def test_graphed_call_replays_the_eager_bits(pkg, dev):
    pred, gt = base(FLAT)
    P, G = cu(pred, dev), cu(gt, dev)

    def step(P, G):
        return (pkg.segmentation_scores(P, G, capacity=256, batched=True).table,)  # [2, S]: two flattened images

    eager = step(P, G)[0].clone()
    g = pkg.graphed(step, P, G)
    first = g.replay()[0].clone()
    assert same_bits(first, eager)
    close("graphed", first, base_ref(FLAT))
    # refill the static inputs: the replay follows, and equals the eager call on the new data
    with torch.no_grad():
        P.copy_(cu(np.roll(pred, 1, axis=0) + 2, dev))
    second = g.replay()[0].clone()
    assert same_bits(second, step(P, G)[0]) and not same_bits(second, first)
    close("graphed, refilled", second, seg_reference(np.roll(pred, 1, axis=0) + 2, gt))
