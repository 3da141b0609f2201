"""GPU: the validation pixel metrics (include/pea_metrics.h, csrc/pea_k_metrics.hip) through affinity_metrics, VolumeStitcher.finish
and cvppp_validation_section(metrics=True), against the numpy restatement tests/metrics_reference.py (which test_metrics_host.py
holds to the reference's own numbers).

Tolerance of mse / bce: relative 1e-5, the project's loss tolerance (tests/test_gpu_parity.py); every term is non-negative, so
nothing cancels.  Counts, stored values and everything called bit-identical are compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

from arena import Arena
from conftest import load_golden
from metrics_reference import f1, finished_pred, metrics_reference

pytestmark = pytest.mark.gpu
RTOL = 1e-5
NUMPY_CLIP = (np.float32(1e-6), np.float32(0.999999))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def close(table, ref, what=""):
    """table (device or numpy, [1 + C, 5]) against the restatement: mse / bce within RTOL (NaN where it is NaN), counts exact"""
    got = table.cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    assert got.shape == ref.shape and got.dtype == np.float64, what
    print(what, "mse/bce", got[0, :2], "ref", ref[0, :2], "counts", got[0, 2:])
    for col in (0, 1):
        for r in range(ref.shape[0]):
            a, b = got[r, col], ref[r, col]
            if np.isnan(b) or np.isinf(b):
                assert (np.isnan(a) and np.isnan(b)) or a == b, (what, r, col, a, b)
            else:
                assert abs(a - b) <= RTOL * abs(b), (what, r, col, a, b)
    assert np.array_equal(got[:, 2:], ref[:, 2:]), (what, got[:, 2:], ref[:, 2:])


def make(seed, B, CP, C, pred_dims, dims, mask_kind, divide):
    """seeded inputs (numpy): pred in (-0.3, 1.3) -- times the weight map with `divide` --, binary target, mask of the asked kind"""
    rng = np.random.default_rng(seed)
    wm = rng.uniform(0.5, 2.0, pred_dims).astype(np.float32) if divide else None
    pred = rng.uniform(-0.3, 1.3, (B, CP) + tuple(pred_dims)).astype(np.float32)
    pred.reshape(-1)[::7] = np.float32(0.0)   # the edges of relu, clip and the threshold, exactly
    pred.reshape(-1)[3::11] = np.float32(1.0)
    pred.reshape(-1)[5::13] = np.float32(0.5)
    if divide:
        pred = (pred * wm).astype(np.float32)
    target = (rng.random((B, C) + tuple(dims)) < 0.6).astype(np.float32)
    if mask_kind is None:
        mask = None
    elif mask_kind == "f32":
        mask = (rng.random(target.shape) < 0.8).astype(np.float32)
    else:
        mask = (rng.random(target.shape) < 0.8).astype(np.uint8 if mask_kind == "u8" else np.bool_)
    return pred, wm, target, mask


# ---- 1. the fixtures ---------------------------------------------------------------------------------------------------------------
def test_fixture_2d_through_affinity_metrics(pkg, dev):
    g = load_golden("gmetrics_2d")
    ref = metrics_reference(g["pred"], g["target"], g["mask"], relu=True)
    pred = cu(g["pred"], dev)
    met = pkg.affinity_metrics(pred, cu(g["target"], dev).float(), cu(g["mask"], dev), relu=True, store=True, clip=(0.0, 1.0))
    close(met.table, ref, "gmetrics_2d")
    assert abs(met.mse - float(g["mse"])) <= RTOL * float(g["mse"]) and abs(met.bce - float(g["bce"])) <= RTOL * float(g["bce"])
    assert same_bits(pred, cu(g["relu"], dev))  # F.relu(pred), stored
    assert met.f1 == f1(met.tp, met.fp, met.fn) and len(met.per_channel["mse"]) == 4


def test_fixture_3d_through_the_stitcher(pkg, dev):
    g = load_golden("gmetrics_3d")
    acc, pad = g["acc_f16"].astype(np.float32), tuple(int(v) for v in g["padding"])
    ref = metrics_reference(acc[None], g["gt"][None].astype(np.float32), None, weight_map=g["weight_map"], origin=pad, clip=NUMPY_CLIP)
    st, st2 = (pkg.VolumeStitcher(12, acc.shape[1:], (4, 8, 8), dev) for _ in range(2))
    for s in (st, st2):
        s.out_affs.copy_(cu(acc, dev))
        s.weight_map.copy_(cu(g["weight_map"], dev))
    out, met = st.finish(pad, cu(g["gt"], dev).float())
    want = st2.get_results(pad)
    assert out.shape == want.shape == (12, 4, 14, 16) and out.data_ptr() == st.out_affs[:, 1:, 3:, 4:].data_ptr()
    assert same_bits(st.out_affs, st2.out_affs) and same_bits(st.weight_map, st2.weight_map)  # the volume is where get_results leaves it
    assert same_bits(out[:3], cu(g["results"], dev))
    close(met.table, ref, "gmetrics_3d")
    assert abs(met.mse - float(g["mse"])) <= RTOL * float(g["mse"]) and abs(met.bce - float(g["bce"])) <= RTOL * float(g["bce"])
    assert [met.tp, met.fp, met.fn] == [int(v) for v in g["counts"]] and met.f1 == float(g["f1"])


# ---- 2. shapes where the walk can go wrong -----------------------------------------------------------------------------------------
# (name, B, CP, C, pred_dims, dims, origin, mask kind, divide)
SHAPES = [
    ("1x5x7_less_than_a_wave", 1, 2, 2, (1, 5, 7), (1, 5, 7), (0, 0, 0), "u8", False),
    ("1x9x33", 1, 3, 3, (1, 9, 33), (1, 9, 33), (0, 0, 0), "f32", False),
    ("3x17x64_ends_inside_a_workgroup_C1", 1, 1, 1, (3, 17, 64), (3, 17, 64), (0, 0, 0), "bool", False),
    ("3x40x70_spans_three_workgroups", 1, 2, 2, (3, 40, 70), (3, 40, 70), (0, 0, 0), None, True),
    ("one_run_and_one_element", 1, 1, 1, (1, 17, 241), (1, 17, 241), (0, 0, 0), "u8", False),     # 4097 elements
    ("C_CP_32", 2, 32, 32, (2, 5, 9), (2, 5, 9), (0, 0, 0), "u8", False),
    ("B3_CP12_C3", 3, 12, 3, (2, 9, 11), (2, 9, 11), (0, 0, 0), "f32", False),
    ("origin_0_3_5", 1, 12, 3, (6, 14, 21), (3, 8, 13), (0, 3, 5), None, True),
    ("origin_2_3_5", 1, 12, 3, (6, 14, 21), (3, 8, 13), (2, 3, 5), "u8", True),
    ("origin_2_3_5_B2_relu_only", 2, 4, 2, (6, 14, 21), (4, 11, 16), (2, 3, 5), "bool", False),
    ("crop_spans_workgroups", 1, 3, 2, (5, 40, 44), (3, 36, 40), (1, 2, 3), "f32", True),           # 8800 / 4320 elements per plane
]


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes_against_the_restatement(pkg, dev, case, store):
    name, B, CP, C, pdims, dims, origin, mk, divide = case
    pred, wm, target, mask = make(sum(map(ord, name)), B, CP, C, pdims, dims, mk, divide)
    clip = NUMPY_CLIP if divide else (0.0, 1.0)
    ref = metrics_reference(pred, target, mask, relu=True, weight_map=wm, origin=origin, clip=clip)
    P = cu(pred, dev)
    met = pkg.affinity_metrics(P, cu(target, dev), None if mask is None else cu(mask, dev), relu=True, store=store, clip=clip,
                               weight_map=None if wm is None else cu(wm, dev), origin=origin)
    close(met.table, ref, name)
    if store:  # every element of pred, all CP channels, the whole volume
        assert same_bits(P, cu(finished_pred(pred, relu=True, weight_map=wm), dev)), name
    else:
        assert same_bits(P, cu(pred, dev)), name


def test_channels_argument_and_2d_layout(pkg, dev):
    """[B, CP, H, W] is Z = 1; channels= must agree with the target"""
    pred, _, target, mask = make(3, 2, 5, 2, (1, 12, 18), (1, 12, 18), "u8", False)
    ref = metrics_reference(pred, target, mask)
    met = pkg.affinity_metrics(cu(pred[:, :, 0], dev), cu(target[:, :, 0], dev), cu(mask[:, :, 0], dev), channels=2)
    close(met.table, ref, "2d layout, no relu")
    with pytest.raises(ValueError):
        pkg.affinity_metrics(cu(pred[:, :, 0], dev), cu(target[:, :, 0], dev), channels=3)
    with pytest.raises(ValueError):  # STORE with neither relu nor a weight map
        pkg.affinity_metrics(cu(pred[:, :, 0], dev), cu(target[:, :, 0], dev), store=True)


# ---- 3. element-aligned pointers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [False, True])
def test_element_aligned_pointers_give_the_same_bits(pkg, dev, store):
    pdims, dims, origin, CP, C = (3, 10, 20), (2, 6, 12), (1, 2, 4), 4, 2
    pred, wm, target, mask = make(77, 1, CP, C, pdims, dims, "f32", True)
    ref = metrics_reference(pred, target, mask, relu=True, weight_map=wm, origin=origin, clip=NUMPY_CLIP)
    tables = []
    for skew in (0, 4, 12):
        ar = Arena(1 << 16, dev)
        P = ar.carve(pred.shape, torch.float32, skew, name="pred")
        Wm = ar.carve(wm.shape, torch.float32, skew, name="weight_map")
        T = ar.carve(target.shape, torch.float32, skew, name="target")
        M = ar.carve(mask.shape, torch.float32, skew, name="mask")
        for view, src in ((Wm, wm), (T, target), (M, mask)):
            ar.fill(view, src)
        if store:
            P.copy_(cu(pred, dev))  # (not remembered: a written view must leave the pattern in every element)
        else:
            ar.fill(P, pred)
        assert P.data_ptr() % 256 == skew and T.data_ptr() % 256 == skew
        met = pkg.affinity_metrics(P, T, M, relu=True, store=store, clip=NUMPY_CLIP, weight_map=Wm, origin=origin)
        tables.append(met.table.clone())
        ar.check(written=[P] if store else [], untouched=[Wm, T, M] + ([] if store else [P]))
        if store:
            assert same_bits(P, cu(finished_pred(pred, relu=True, weight_map=wm), dev))
    close(tables[0], ref, "skew 0")
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)) and torch.equal(tables[0].view(torch.int64), tables[2].view(torch.int64))


def test_dense_walk_at_every_skew(pkg, dev):
    """no crop (the 2D callers): pred, target and a u8 mask share the index; dwordx4 at skew 0, scalar at 4 and 12"""
    pred, _, target, mask = make(78, 2, 3, 3, (1, 21, 35), (1, 21, 35), "u8", False)
    tables = []
    for skew in (0, 4, 12):
        ar = Arena(1 << 16, dev)
        P = ar.carve(pred.shape, torch.float32, skew, name="pred")
        T = ar.fill(ar.carve(target.shape, torch.float32, skew, name="target"), target)
        M = ar.fill(ar.carve(mask.shape, torch.uint8, skew // 4, name="mask"), mask)
        P.copy_(cu(pred, dev))
        tables.append(pkg.affinity_metrics(P, T, M, relu=True, store=True).table.clone())
        ar.check(written=[P], untouched=[T, M])
        assert same_bits(P, torch.relu(cu(pred, dev)))
    close(tables[0], metrics_reference(pred, target, mask, relu=True), "dense")
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)) and torch.equal(tables[0].view(torch.int64), tables[2].view(torch.int64))


# ---- 4. STORE ------------------------------------------------------------------------------------------------------------------------
def test_store_bits_are_those_of_the_calls_it_replaces(pkg, dev):
    pred, wm, target, _ = make(41, 1, 12, 3, (6, 14, 22), (4, 8, 14), None, True)
    L, vp = pkg._lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    # DIVIDE: pea_stitch_finalize on a clone, all 12 channels, the whole volume
    P, Wm = cu(pred, dev), cu(wm, dev)
    want = P.clone()
    pkg._lib.check(L.pea_stitch_finalize(vp(want), vp(Wm), 12, 6 * 14 * 22, None), "pea_stitch_finalize")
    torch.cuda.synchronize()
    pkg.affinity_metrics(P, cu(target, dev), store=True, weight_map=Wm, origin=(1, 3, 4), clip=NUMPY_CLIP)
    assert same_bits(P, want)
    # RELU: relu_ on a clone (NaN, -0.0 and an infinity among the values)
    pred[0, 0, 0, 0, :4] = [np.nan, -0.0, -np.inf, np.inf]
    P = cu(pred, dev)
    want = pkg.relu_(P.clone())
    v0 = P._version
    pkg.affinity_metrics(P, cu(target, dev), relu=True, store=True, origin=(1, 3, 4))
    assert same_bits(P, want) and P._version > v0
    # without STORE pred is bit-unchanged
    P = cu(pred, dev)
    pkg.affinity_metrics(P, cu(target, dev), relu=True, weight_map=Wm, origin=(1, 3, 4))
    assert same_bits(P, cu(pred, dev))


# ---- 5. reproducibility and the state contract ---------------------------------------------------------------------------------------
def test_two_calls_agree_and_the_states_serve_a_later_call(pkg, dev):
    L, op = pkg._lib.lib(), pkg.affinity_op
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    pred, _, target, mask = make(5, 2, 4, 3, (2, 30, 50), (2, 30, 50), "u8", False)
    P, T, M = cu(pred, dev), cu(target, dev), cu(mask, dev)
    d = pkg._lib.PeaMetricsDesc()
    d.B, d.C, d.CP = 2, 3, 4
    d.dims[:], d.pred_dims[:], d.origin[:] = (2, 30, 50), (2, 30, 50), (0, 0, 0)
    d.flags, d.clip_lo, d.clip_hi = pkg._lib.MET_RELU, 0.0, 1.0
    nb = L.pea_metrics_workspace_bytes()

    def state():
        ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        pkg._lib.check(L.pea_workspace_init(vp(ws), nb, None), "pea_workspace_init")
        return ws

    ws = state()
    outs = [torch.empty((4, 5), dtype=torch.float64, device=dev) for _ in range(2)]
    for o in outs:
        pkg._lib.check(L.pea_affs_metrics(ctypes.byref(d), vp(P), None, vp(T), vp(M), vp(o), vp(ws), nb, None), "pea_affs_metrics")
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
    close(outs[0], metrics_reference(pred, target, mask, relu=True), "raw call")
    # the block is zero again (but for the magic words): an embedding_loss forward on it gives the bits of a fresh block
    words = ws.view(torch.int32).view(5, -1)
    assert int((words != 0).sum()) == 5 and bool((words[:, 0] != 0).all())
    spec = pkg.AffinitySpec(2, [(0, 1), (1, 0), (3, -2)], None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX, 1e-6)
    gen = torch.Generator(device=dev).manual_seed(9)
    e = torch.randn((2, 16, 40, 56), generator=gen, device=dev)
    t = (torch.rand((2, 3, 40, 56), generator=gen, device=dev) < 0.5).float()
    w = torch.rand((2, 3, 40, 56), generator=gen, device=dev) + 0.5
    pd = op.make_desc(spec, e)
    one = L.pea_workspace_bytes(ctypes.byref(pd))
    rows = []
    for block in (ws, state()):
        affs, loss = torch.empty_like(t), torch.empty(4, dtype=torch.float32, device=dev)
        pkg._lib.check(L.pea_affinity_fwd(ctypes.byref(pd), vp(e), None, vp(t), vp(w), None, vp(affs), None, vp(loss), vp(block), one, None),
                       "pea_affinity_fwd")
        torch.cuda.synchronize()
        rows.append((loss, affs))
    assert same_bits(rows[0][0], rows[1][0]) and same_bits(rows[0][1], rows[1][1]) and bool(torch.isfinite(rows[0][0]).all())
    # a block that was never initialised: NaN in every column
    raw = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    o = torch.zeros((4, 5), dtype=torch.float64, device=dev)
    pkg._lib.check(L.pea_affs_metrics(ctypes.byref(d), vp(P), None, vp(T), vp(M), vp(o), vp(raw), nb, None), "pea_affs_metrics")
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())


# ---- 6. the edges of the BCE -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [(0.0, 1.0), NUMPY_CLIP], ids=["torch_clamp", "numpy_clip"])
def test_bce_edges(pkg, dev, clip):
    """v exactly 0 against t = 1 and v exactly 1 against t = 0: 100 each with clip (0, 1) (nn.BCELoss's floor), -log(1e-6) / -log(1 - 0.999999)
    with the numpy clip"""
    rng = np.random.default_rng(6)
    pred = rng.uniform(0.05, 0.95, (1, 2, 1, 8, 16)).astype(np.float32)
    target = (rng.random(pred.shape) < 0.5).astype(np.float32)
    pred[0, 0, 0, 0, :4], target[0, 0, 0, 0, :4] = [0.0, 0.0, 1.0, 1.0], [1.0, 0.0, 0.0, 1.0]
    pred[0, 0, 0, 1, :2], target[0, 0, 0, 1, :2] = [-0.5, 1.5], [1.0, 0.0]    # relu / clip bring them to the same edges
    ref = metrics_reference(pred, target, None, relu=True, clip=clip)
    met = pkg.affinity_metrics(cu(pred, dev), cu(target, dev), relu=True, clip=clip)
    close(met.table, ref, "bce edges %s" % (clip,))
    if clip == (0.0, 1.0):  # four elements of channel 0 give exactly 100 each; the others at most -log(0.05)
        assert met.per_channel["bce"][0] * 128 > 400.0 and met.per_channel["bce"][0] * 128 < 400.0 + 124 * 3.0


# ---- 7. exact sums ---------------------------------------------------------------------------------------------------------------------
def test_counts_and_sums_are_exact_past_2_to_the_24(pkg, dev):
    n = (1 << 24) + 64
    H, W = 320, 52429
    assert H * W == n
    pred = torch.full((1, 1, H, W), 0.25, dtype=torch.float32, device=dev)
    target = torch.zeros((1, 1, H, W), dtype=torch.float32, device=dev)
    met = pkg.affinity_metrics(pred, target)
    print("2^24 + 64 elements:", met.table.cpu().numpy())
    assert (met.tp, met.fp, met.fn) == (n, 0, 0) and met.per_channel["tp"] == [n]
    assert met.mse == 0.0625 and met.per_channel["mse"] == [0.0625]
    assert abs(met.bce + np.log(0.75)) <= RTOL * -np.log(0.75)
    assert met.f1 == 1.0


# ---- 8. non-finite ---------------------------------------------------------------------------------------------------------------------
def test_one_nan_voxel_reaches_its_channel_and_the_total_only(pkg, dev):
    pred, _, target, mask = make(8, 1, 3, 3, (2, 20, 30), (2, 20, 30), "u8", False)
    mask[0, 1, 1, 7, 9], target[0, 1, 1, 7, 9] = 1, 0.0   # a boundary voxel that counts
    pred[0, 1, 1, 7, 9] = 0.25                             # .. predicted in the finite run
    T, M = cu(target, dev), cu(mask, dev)
    fin = pkg.affinity_metrics(cu(pred, dev), T, M, relu=True).table.cpu().numpy()
    bad = pred.copy()
    bad[0, 1, 1, 7, 9] = np.nan
    got = pkg.affinity_metrics(cu(bad, dev), T, M, relu=True).table.cpu().numpy()
    close(got, metrics_reference(bad, target, mask, relu=True), "one NaN voxel")
    assert np.isnan(got[2, :2]).all() and np.isnan(got[0, :2]).all()
    for r in (1, 3):
        assert np.array_equal(got[r].view(np.int64), fin[r].view(np.int64)), r
    # "not predicted": the voxel moves from tp to fn
    assert got[2, 2] == fin[2, 2] - 1 and got[2, 4] == fin[2, 4] + 1 and got[2, 3] == fin[2, 3]
    # the next call on the same states is finite again
    again = pkg.affinity_metrics(cu(pred, dev), T, M, relu=True).table.cpu().numpy()
    assert np.array_equal(again.view(np.int64), fin.view(np.int64))


def test_zero_over_zero_of_an_uncovered_voxel(pkg, dev):
    """a voxel no window covered: accumulators and weight map are 0 there, 0 / 0 = NaN in every channel"""
    pred, wm, target, _ = make(9, 1, 4, 3, (4, 12, 18), (2, 8, 12), None, True)
    z, y, x = 2, 5, 7  # inside the region (origin (1, 2, 3))
    pred[0, :, z, y, x], wm[z, y, x] = 0.0, 0.0
    target[0, :, z - 1, y - 2, x - 3] = [0.0, 1.0, 0.0]
    P = cu(pred, dev)
    met = pkg.affinity_metrics(P, cu(target, dev), store=True, weight_map=cu(wm, dev), origin=(1, 2, 3), clip=NUMPY_CLIP)
    got = met.table.cpu().numpy()
    ref = metrics_reference(pred, target, None, weight_map=wm, origin=(1, 2, 3), clip=NUMPY_CLIP)
    close(got, ref, "0 / 0")
    assert np.isnan(got[:, :2]).all() and bool(torch.isnan(P[0, :, z, y, x]).all())
    ok = pred.copy()
    ok[0, :, z, y, x], wm2 = 0.25, wm.copy()
    wm2[z, y, x] = 1.0
    fin = pkg.affinity_metrics(cu(ok, dev), cu(target, dev), weight_map=cu(wm2, dev), origin=(1, 2, 3), clip=NUMPY_CLIP).table.cpu().numpy()
    # "not predicted": boundary voxels (channels 0 and 2) move from tp to fn, the non-boundary one (channel 1) leaves fp
    assert np.array_equal(got[1:, 2:] - fin[1:, 2:], np.array([[-1, 0, 1], [0, -1, 0], [-1, 0, 1]], np.float64))


# ---- 9. graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_eager_table(pkg, dev):
    pred, _, target, mask = make(10, 1, 10, 10, (1, 40, 48), (1, 40, 48), "f32", False)
    P, T, M = cu(pred[:, :, 0], dev), cu(target[:, :, 0], dev), cu(mask[:, :, 0], dev)
    eager = pkg.affinity_metrics(P, T, M, relu=True).table.clone()
    g = pkg.graphed(lambda P, T, M: pkg.affinity_metrics(P, T, M, relu=True).table, P, T, M)
    first = g.replay().clone()
    assert torch.equal(first.view(torch.int64), eager.view(torch.int64))
    P.copy_(P * 0.5 + 0.1)  # new contents of the static input: the replay follows, and equals the eager call on them
    second = g.replay().clone()
    eager2 = pkg.affinity_metrics(P, T, M, relu=True).table
    assert torch.equal(second.view(torch.int64), eager2.view(torch.int64)) and not torch.equal(second, first)
    close(second, metrics_reference(P.cpu().numpy()[:, :, None], target, mask, relu=True), "graph replay")


# ---- 10. the validation section ------------------------------------------------------------------------------------------------------------
def test_validation_section_with_metrics(pkg, dev):
    g = load_golden("gsection_cvppp")
    offsets = g["offsets"].tolist()
    crit = pkg.WeightedMSE()
    embs = [cu(g["emb%d" % j], dev) for j in range(5)]
    downs = [torch.cat([cu(g["t%d" % j], dev), cu(g["w%d" % j], dev), cu(g["m%d" % j], dev).float()], dim=1) for j in range(1, 5)]
    T, M = cu(g["t0"], dev), cu(g["m0"], dev)
    args = (embs[0], embs[1:], T, cu(g["w0"], dev), M, downs, crit, offsets, 2)
    l0, p0 = pkg.cvppp_validation_section(*args)
    l1, p1, met = pkg.cvppp_validation_section(*args, metrics=True)
    assert same_bits(l1, l0) and same_bits(p1, p0) and isinstance(met, pkg.AffinityMetrics)
    # scripts_cvppp/main.py:396-397 on the same tensors
    am = M.float()
    mse = torch.nn.MSELoss()(p0 * am, T * am).item()
    bce = torch.nn.BCELoss()(torch.clamp(p0, 0.0, 1.0) * am, T * am).item()
    print("validation section: mse", met.mse, mse, "bce", met.bce, bce)
    assert abs(met.mse - mse) <= RTOL * abs(mse) and abs(met.bce - bce) <= RTOL * abs(bce)
    with pytest.raises(ValueError):
        pkg.cvppp_validation_section(*args, test_mode=True, metrics=True)
