"""GPU: target generation and class-balance weights on the device -- pea_gen_targets (k_gen_targets, k_gen_weights: csrc/pea_targets.h)
and pea_label_weights (k_label_counts, k_label_counts_lds, k_weight_table: csrc/pea_fused_labels.h) through the C ABI, and gen_targets,
gen_affs_ours, seg_to_aff and the tensor-path fallback of embedding_loss_from_labels in the Python layer, against the numpy restatement tests/targets_reference.py (which
test_targets_host.py holds to the oracle, to utils/synth.py, to the reference project's goldens and to hand-written class-balance values).

Every output is an integer, or an f32 rounded once from an f64 expression that the restatement evaluates identically: all comparisons are
torch.equal / np.array_equal, there is no tolerance anywhere.  Every C call of this file runs in a guard-banded arena (arena.py): the labels
come back untouched, every element of target, weight and wtab is written, nothing else changes; the workspace is lent as it is -- filled
with the arena's pattern, never prepared -- and each call runs twice on the same workspace with the same bits.  The mask holds bytes, which
the arena cannot tell from its pattern element by element, so it is lent as scratch and compared whole with the expected mask (the
pattern's bytes are 0xa5 and 0x7f, never 0 or 1: an unwritten element cannot pass).

Case sizing: targets_reference.py (GEOMETRIES, TABLES_2D, TABLES_3D) says which edge of which kernel each image and table reaches.
Which count kernel serves a call is not observable from outside; the cases are built from the launcher's conditions (X % 4, 16-byte
alignment of the label image, oz == 0, reach <= 28), a 4 / 8 / 12-byte skew of the labels or PEA_FORCE_DIRECT moves a call to the direct
route, and every route must give the restatement's bits."""
import ctypes

import numpy as np
import pytest
import torch

import targets_reference as tr
from arena import Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def tt(a):
    """a numpy array (the shared cases are read-only) as a CPU tensor of its own"""
    return torch.tensor(np.asarray(a))


def desc(pkg, shape, offsets):
    """the descriptor of the label -> target calls, built by hand: B, dims, K and the offsets are all they read"""
    B, Z, Y, X = shape
    offs = tr.offsets3(offsets)
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, (2 if Z == 1 else 3), B, 1, len(offs)
    d.dims[:] = [Z, Y, X]
    d.border, d.dtype, d.norm, d.flags, d.eps = pkg._lib.BORDER_CROP_ZERO, pkg._lib.F32, pkg._lib.NORM_FULL, 0, 1e-12
    for i, o in enumerate(offs):
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    return d


def raw_gen(pkg, dev, lab, offsets, flags, mask=True, weight=True, skew=(0, 0, 1, 0), stream=None):
    """pea_gen_targets on numpy labels [B, Z, Y, X] in an arena, twice on one unprepared workspace -> (target, mask or None, weight or
    None) as device clones.  skew: bytes (labels, target, mask, weight)."""
    L = pkg._lib.lib()
    lab = np.ascontiguousarray(lab)
    B, Z, Y, X = lab.shape
    d = desc(pkg, lab.shape, offsets)
    K, n = d.K, lab.size
    nb = L.pea_targets_workspace_bytes(ctypes.byref(d))
    assert nb >= B * K * 4 and nb % 4 == 0
    ar = Arena(n * 4 + n * K * 9 + nb + (1 << 15), dev)
    Lb = ar.fill(ar.carve(lab.shape, torch.int32, skew[0], name="labels"), tt(lab))
    T = ar.carve((B, K, Z, Y, X), torch.float32, skew[1], name="target")
    M = ar.carve((B, K, Z, Y, X), torch.uint8, skew[2], name="mask") if mask else None
    W = ar.carve((B, K, Z, Y, X), torch.float32, skew[3], name="weight") if weight else None
    ws = ar.carve((1, nb // 4), torch.int32, 4, name="workspace")  # (one batch item: the arena walks a view's batch in Python)
    assert Lb.data_ptr() % 16 == skew[0] % 16 and T.data_ptr() % 16 == skew[1] % 16
    first = None
    for _ in range(2):  # the second call runs on the workspace as the first one left it
        pkg._lib.check(L.pea_gen_targets(ctypes.byref(d), vp(Lb), flags, vp(T), vp(M), vp(W), vp(ws), nb, stream), "pea_gen_targets")
        torch.cuda.synchronize()
        got = tuple(None if t is None else t.clone() for t in (T, M, W))
        if first is not None:
            assert all(a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, got)), "the second call differs"
        first = got
    ar.check(written=[T] + ([W] if weight else []), untouched=[Lb], scratch=[ws] + ([M] if mask else []))
    return first


def raw_wtab(pkg, dev, lab, offsets, flags, skew=(0, 0), stream=None):
    """pea_label_weights in an arena, twice on one unprepared workspace -> wtab [B, K, 2] as a device clone.  skew: bytes (labels, wtab)."""
    L = pkg._lib.lib()
    lab = np.ascontiguousarray(lab)
    d = desc(pkg, lab.shape, offsets)
    nb = L.pea_targets_workspace_bytes(ctypes.byref(d))
    ar = Arena(lab.size * 4 + nb + (1 << 15), dev)
    Lb = ar.fill(ar.carve(lab.shape, torch.int32, skew[0], name="labels"), tt(lab))
    wtab = ar.carve((lab.shape[0], d.K, 2), torch.float32, skew[1], name="wtab")
    ws = ar.carve((1, nb // 4), torch.int32, 4, name="workspace")
    assert Lb.data_ptr() % 16 == skew[0] % 16
    first = None
    for _ in range(2):
        pkg._lib.check(L.pea_label_weights(ctypes.byref(d), vp(Lb), flags, vp(wtab), vp(ws), nb, stream), "pea_label_weights")
        torch.cuda.synchronize()
        got = wtab.clone()
        assert first is None or torch.equal(first.view(torch.int32), got.view(torch.int32)), "the second call differs"
        first = got
    ar.check(written=[wtab], untouched=[Lb], scratch=[ws])
    return first


def same(got, want):
    """bit for bit (f32 compared as int32: signed zeros and payloads count)"""
    want = tt(want)
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    return torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8))


def check(what, pkg, dev, lab, offsets, flags, ref=None, gen_skew=(0, 0, 1, 0), wtab_skew=(0, 0)):
    """both generators on one image against the restatement, and against each other -> (target, mask, weight, wtab) on the device"""
    rt, rm, rw, rtab, rcount = ref if ref is not None else tr.targets_reference(lab, offsets, flags)
    T, M, W = raw_gen(pkg, dev, lab, offsets, flags, skew=gen_skew)
    wtab = raw_wtab(pkg, dev, lab, offsets, flags, skew=wtab_skew)
    print(what, "flags", flags, "counts", rcount.tolist()[0][:6], "wtab", wtab[0, :3].tolist())
    assert same(T, rt), what + ": target"
    assert same(M, rm), what + ": mask"
    assert same(wtab, rtab), what + ": wtab"
    assert same(W, rw), what + ": weight"
    # the two generators agree: weight[b,i,p] = target[b,i,p] ? wtab[b,i,0] : wtab[b,i,1]
    sel = (slice(None), slice(None), None, None, None)
    both = torch.where(T != 0, wtab[..., 0][sel], wtab[..., 1][sel])
    assert torch.equal(W.view(torch.int32), both.view(torch.int32)), what + ": the weight tensor is not the table spread over the target"
    return T, M, W, wtab


# ---- 1. every named case under every flag combination ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", tr.FLAG_COMBOS)
@pytest.mark.parametrize("geometry,table", tr.CASES, ids=["%s-%s" % c for c in tr.CASES])
def test_named_cases(pkg, dev, geometry, table, flags):
    lab = tr.label_image(geometry)
    ref = tr.expected(geometry, table, flags)
    got = check("%s %s" % (geometry, table), pkg, dev, lab, tr.table(table), flags, ref=ref)
    if table.startswith("past_"):  # every neighbour of every channel is outside
        assert not bool(got[1].any()) and bool((got[0] == (1.0 if flags & tr.PADDING else 0.0)).all()) and bool((got[3] == 1).all())


@pytest.mark.parametrize("geometry,table", [("lds_37x100", "nb4_k10"), ("direct_33x67", "k6"), ("vol_5x19x23", "oz"), ("vol_3x8x12", "inplane"),
                                            ("tiny_3x5", "past_3x5")])
def test_mask_inside_changes_no_bit(pkg, dev, geometry, table):
    lab = tr.label_image(geometry)
    for flags in tr.FLAG_COMBOS:
        ref = tr.expected(geometry, table, flags)
        got = check("%s %s MASK_INSIDE" % (geometry, table), pkg, dev, lab, tr.table(table), flags | tr.MASK_INSIDE, ref=ref)
        plain = check("%s %s" % (geometry, table), pkg, dev, lab, tr.table(table), flags, ref=ref)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, plain))


def test_both_foreground_on_equal_negatives_and_zeros(pkg, dev):
    lab = tr.label_image("lds_37x100")
    for flags, neg in ((0, 1.0), (tr.BOTH_FOREGROUND, 0.0), (tr.PADDING | tr.BOTH_FOREGROUND, 0.0)):
        T = raw_gen(pkg, dev, lab, tr.table("k1"), flags, mask=False, weight=False)[0]
        assert bool((T[:, 0, 0, 2:4, 3:5] == neg).all()) and bool((T[:, 0, 0, 11:13, 1:3] == neg).all())  # ids -3 and 0
        assert bool((T[:, 0, 0, 13:15, 10:12] == 1).all())  # id 2^31 - 1 is foreground


# ---- 2. nullable outputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry,table", [("lds_37x100", "k6"), ("vol_5x19x23", "oz")])
def test_nullable_outputs(pkg, dev, geometry, table):
    lab = tr.label_image(geometry)
    for flags in (tr.PADDING, tr.PADDING | tr.BOTH_FOREGROUND):  # (the second: the flag pair no caller of the Python layer makes)
        rt, rm, rw, _, _ = tr.expected(geometry, table, flags)
        T, M, W = raw_gen(pkg, dev, lab, tr.table(table), flags, mask=False, weight=True)
        assert M is None and same(T, rt) and same(W, rw)
        T, M, W = raw_gen(pkg, dev, lab, tr.table(table), flags, mask=True, weight=False)
        assert W is None and same(T, rt) and same(M, rm)
        T, M, W = raw_gen(pkg, dev, lab, tr.table(table), flags, mask=False, weight=False)
        assert M is None and W is None and same(T, rt)


# ---- 3. class balance on its branches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,X,flags,want", tr.BALANCE, ids=["%s-%d-%d" % c[:3] for c in tr.BALANCE])
def test_class_balance_branches(pkg, dev, kind, X, flags, want):
    lab = tr.balance_labels(kind, X)
    table = [[0, -1]]
    ref = tr.targets_reference(lab, table, flags)
    assert ref[4].tolist() == [[tr.balance_count(kind, X, flags)]]
    hand = torch.tensor([[[want[0], want[1]]]], dtype=torch.float32)
    # X % 4 == 0 and aligned labels: the LDS route; labels skewed by 4 bytes: the direct route
    for lskew in ((0, 4) if X % 4 == 0 else (0,)):
        T, M, W, wtab = check("%s X=%d labels+%d" % (kind, X, lskew), pkg, dev, lab, table, flags, ref=ref, gen_skew=(lskew, 0, 1, 0),
                              wtab_skew=(lskew, 0))
        assert torch.equal(wtab.cpu().view(torch.int32), hand.view(torch.int32)), (wtab.tolist(), want)
        by_hand = torch.where(tt(ref[0]) != 0, hand[0, 0, 0], hand[0, 0, 1])
        assert torch.equal(W.cpu().view(torch.int32), by_hand.view(torch.int32))


# ---- 4. the routes of the count kernels -------------------------------------------------------------------------------------------------------
def test_route_boundary_reach_28_and_29(pkg, dev):
    """the same image under a table of reach 28 (the LDS route's last) and the same table with one offset a pixel longer: the channels
    they share must come out alike, and both equal the restatement"""
    for geometry in ("lds_37x100", "tiles_70x132"):
        lab = tr.label_image(geometry)
        for flags in tr.FLAG_COMBOS:
            a = check("reach 28", pkg, dev, lab, tr.table("reach28"), flags, ref=tr.expected(geometry, "reach28", flags))
            b = check("reach 29", pkg, dev, lab, tr.table("reach29"), flags, ref=tr.expected(geometry, "reach29", flags))
            assert torch.equal(a[3][:, 1:].view(torch.int32), b[3][:, 1:].view(torch.int32)) and torch.equal(a[0][:, 1:], b[0][:, 1:])


@pytest.mark.parametrize("geometry,table", [("lds_37x100", "k32"), ("lds_37x100", "nb4_k10"), ("tiles_70x132", "reach28"), ("vol_3x8x12", "inplane")])
def test_forced_direct_route_gives_the_same_bits(pkg, dev, geometry, table, monkeypatch):
    lab = tr.label_image(geometry)
    flags = tr.PADDING
    ref = tr.expected(geometry, table, flags)
    staged = raw_wtab(pkg, dev, lab, tr.table(table), flags)
    monkeypatch.setenv("PEA_FORCE_DIRECT", "1")  # (conftest's wrapper makes the library re-read its switches)
    direct = raw_wtab(pkg, dev, lab, tr.table(table), flags)
    monkeypatch.delenv("PEA_FORCE_DIRECT")
    assert same(staged, ref[3]) and same(direct, ref[3])


# ---- 5. pointers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry,table", [("lds_37x100", "nb4_k10"), ("vol_3x8x12", "inplane"), ("direct_33x67", "k5")])
def test_skewed_pointers(pkg, dev, geometry, table):
    lab = tr.label_image(geometry)
    flags = tr.PADDING
    ref = tr.expected(geometry, table, flags)
    aligned = check("aligned", pkg, dev, lab, tr.table(table), flags, ref=ref)
    for lskew in (4, 8, 12):  # the label image off its 16 bytes: pea_label_weights takes the direct route
        got = check("labels + %d" % lskew, pkg, dev, lab, tr.table(table), flags, ref=ref, gen_skew=(lskew, 0, 1, 0), wtab_skew=(lskew, 0))
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, aligned)), lskew
    for gen_skew, wtab_skew in (((0, 4, 2, 12), (0, 4)), ((0, 12, 3, 4), (0, 12)), ((8, 4, 1, 4), (4, 12))):
        got = check("skew %s %s" % (gen_skew, wtab_skew), pkg, dev, lab, tr.table(table), flags, ref=ref, gen_skew=gen_skew, wtab_skew=wtab_skew)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, aligned)), (gen_skew, wtab_skew)


# ---- 6. streams, graphs ---------------------------------------------------------------------------------------------------------------------------------
def test_two_streams_with_a_workspace_each(pkg, dev):
    L = pkg._lib.lib()
    geometry, table, flags = "lds_37x100", "nb4_k10", tr.PADDING
    lab = tr.label_image(geometry)
    rt, rm, rw, rtab, _ = tr.expected(geometry, table, flags)
    d = desc(pkg, lab.shape, tr.table(table))
    nb = L.pea_targets_workspace_bytes(ctypes.byref(d))
    Lb = tt(lab).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    new = lambda shape, dtype: [[torch.full(shape, 77, dtype=dtype, device=dev) for _ in range(5)] for _ in streams]
    T, M, W, tabs = new(rt.shape, torch.float32), new(rt.shape, torch.uint8), new(rt.shape, torch.float32), new(rtab.shape, torch.float32)
    work = [[torch.full((nb // 4,), 0x5a5a5a5a, dtype=torch.int32, device=dev) for _ in range(2)] for _ in streams]
    torch.cuda.synchronize()
    for k in range(5):  # five calls of each entry point on each of two streams that run side by side (a workspace per stream and entry point)
        for s, st in enumerate(streams):
            h = ctypes.c_void_p(st.cuda_stream)
            pkg._lib.check(L.pea_gen_targets(ctypes.byref(d), vp(Lb), flags, vp(T[s][k]), vp(M[s][k]), vp(W[s][k]), vp(work[s][0]), nb, h),
                           "pea_gen_targets")
            pkg._lib.check(L.pea_label_weights(ctypes.byref(d), vp(Lb), flags, vp(tabs[s][k]), vp(work[s][1]), nb, h), "pea_label_weights")
    torch.cuda.synchronize()
    for s in range(2):
        for k in range(5):
            assert same(T[s][k], rt) and same(M[s][k], rm) and same(W[s][k], rw) and same(tabs[s][k], rtab), (s, k)
    assert same(Lb, lab)


def test_graphed_step_replays_on_a_refilled_label_buffer(pkg, dev):
    geometry, flags = "direct_33x67", tr.PADDING
    table = tr.table("nb4_k10")
    first = tr.label_image(geometry)[:, 0]
    second = np.ascontiguousarray(first[::-1, ::-1, ::-1])
    Lb = tt(first).to(dev)

    def step(Lb):
        return pkg.gen_targets(Lb, table, padding=True)

    eager = [t.clone() for t in step(Lb)]
    ref = tr.expected(geometry, "nb4_k10", flags)
    assert all(same(a, b[:, :, 0]) for a, b in zip(eager, ref[:3]))
    g = pkg.graphed(step, Lb)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, eager))
    Lb.copy_(tt(second))  # the label buffer refilled: the replay answers for what it holds now
    got = [t.clone() for t in g.replay()]
    ref2 = tr.targets_reference(second[:, None], table, flags)
    assert not np.array_equal(ref2[0], ref[0])
    assert all(same(a, b[:, :, 0]) for a, b in zip(got, ref2[:3]))


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------------------------------
def test_gen_targets_and_gen_affs_ours(pkg, dev):
    geometry = "direct_33x67"
    lab = tr.label_image(geometry)
    Lb = tt(lab[:, 0]).to(dev)
    for padding, both in ((True, False), (False, False), (False, True), (True, True)):
        flags = (tr.PADDING if padding else 0) | (tr.BOTH_FOREGROUND if both else 0)
        rt, rm, rw, _, _ = tr.expected(geometry, "nb8_k12", flags)
        t, m, w = pkg.gen_targets(Lb, tr.table("nb8_k12"), padding=padding, both_foreground=both)
        assert same(t, rt[:, :, 0]) and same(m, rm[:, :, 0]) and same(w, rw[:, :, 0])
    t, m, w = pkg.gen_targets(Lb, tr.table("nb8_k12"), want_mask=False, want_weight=False)
    assert m is None and w is None and same(t, tr.expected(geometry, "nb8_k12", tr.PADDING)[0][:, :, 0])
    for padding in (True, False):
        rt, rm, _, _, _ = tr.expected(geometry, "nb8_k12", tr.PADDING if padding else 0)
        t, m = pkg.gen_affs_ours(Lb, tr.table("nb8_k12"), padding=padding)
        assert same(t, rt[:, :, 0]) and same(m, rm[:, :, 0])
    # int64 and uint8 label tensors are taken as their int32 values
    small = np.clip(lab[:, 0], 0, 200)
    rt, rm, rw, _, _ = tr.targets_reference(small[:, None].astype(np.int32), tr.table("k6"), tr.PADDING)
    for dtype in (torch.int64, torch.uint8):
        t, m, w = pkg.gen_targets(tt(small).to(dev).to(dtype), tr.table("k6"))
        assert same(t, rt[:, :, 0]) and same(m, rm[:, :, 0]) and same(w, rw[:, :, 0])


def test_gen_targets_with_a_table_that_reaches_past_the_image(pkg, dev):
    """what embedding_loss_from_labels falls back to on a scale smaller than the stencil's reach (gen_affs_ours shifts by the true offset)"""
    lab = tr.label_image("tiny_3x5")
    for flags in (tr.PADDING, 0):
        rt, rm, rw, _, _ = tr.expected("tiny_3x5", "past_3x5", flags)
        t, m, w = pkg.gen_targets(tt(lab[:, 0]).to(dev), tr.table("past_3x5"), padding=bool(flags))
        assert same(t, rt[:, :, 0]) and same(m, rm[:, :, 0]) and same(w, rw[:, :, 0])
    mixed = [[0, -1], [0, -5], [-1, 0], [-27, 0]]  # two channels inside, two past
    rt, rm, rw, _, _ = tr.targets_reference(lab, mixed, tr.PADDING)
    t, m, w = pkg.gen_targets(tt(lab[:, 0]).to(dev), mixed)
    assert same(t, rt[:, :, 0]) and same(m, rm[:, :, 0]) and same(w, rw[:, :, 0]) and bool(m[:, 0].any()) and not bool(m[:, 1].any())


def test_seg_to_aff(pkg, dev):
    geometry = "vol_5x19x23"
    seg = tr.label_image(geometry)
    S = tt(seg).to(dev)
    got = pkg.seg_to_aff(S)
    want = tr.seg_to_aff_reference(seg)
    assert same(got, want)
    plain = tr.expected(geometry, "norm5", tr.BOTH_FOREGROUND)[0][:, :3]
    assert not np.array_equal(want, plain)  # the 'replicate' rows differ from the plain targets
    assert same(pkg.seg_to_aff(S, pad=""), plain)
    nh = [[-2, 0, 0], [0, -3, 0], [0, 0, -3]]
    assert same(pkg.seg_to_aff(S, nh, pad=""), tr.seg_to_aff_reference(seg, nh, pad=""))
    assert same(pkg.seg_to_aff(S, tr.table("oz"), pad="replicate"), tr.expected(geometry, "oz", tr.BOTH_FOREGROUND)[0])  # not three edges: no rows


def test_embedding_loss_from_labels_on_a_scale_smaller_than_the_stencil(pkg, dev):
    """an offset as long as the image: no labels-in kernel applies, embedding_loss_from_labels generates the targets with the true offsets
    (every neighbour of those channels outside: mask 0, no loss) and takes the tensor path -- the same bits as that path on the restatement"""
    B, D, H, W = 2, 16, 20, 24
    offsets = tr.multi_offset([1, 3, 27], 4)
    lab = np.ascontiguousarray(tr.label_image("lds_37x100")[:, :, :H, :W])
    rt, rm, rw, _, _ = tr.targets_reference(lab, offsets, tr.PADDING)
    assert not rm[:, 4:].any() and rm[:, :4].any()
    e = torch.from_numpy(np.random.default_rng(9).standard_normal((B, D, H, W)).astype(np.float32)).to(dev)
    crit = pkg.WeightedMSE()
    e1 = e.clone().requires_grad_(True)
    loss1, affs1, parts1 = pkg.embedding_loss_from_labels(e1, tt(lab[:, 0]).to(dev), crit, offsets)
    loss1.backward()
    e2 = e.clone().requires_grad_(True)
    loss2, affs2, parts2 = pkg.embedding_loss(e2, tt(rt[:, :, 0]).to(dev), tt(rw[:, :, 0]).to(dev), tt(rm[:, :, 0]).to(dev), crit, offsets)
    loss2.backward()
    assert torch.equal(loss1, loss2) and torch.equal(affs1, affs2) and torch.equal(e1.grad, e2.grad)
    assert list(parts1) == list(parts2) and list(parts1)[4:] == [0.0, 0.0] and all(v > 0 for v in list(parts1)[:4])
