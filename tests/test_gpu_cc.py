"""GPU: connected components on the device (include/pea_cc.h, csrc/pea_k_cc.hip) through the C ABI, through connected_components,
remove_samll_object and foreground_mask(min_size=...), against the numpy restatement tests/cc_reference.py (which test_cc_host.py holds
to scipy.ndimage.label and to hand-written expectations).

Every output is an exact integer: all comparisons are torch.equal, there is no tolerance anywhere.  Every C call of this file runs in a
guard-banded arena (arena.py): the input comes back untouched, every element of labels_out and counts is written, nothing else changes;
the workspace is lent as it is -- filled with the arena's pattern, never prepared -- and each call runs twice on the same workspace.
mask_out holds bytes, which the arena cannot tell from its pattern element by element, so it is lent as scratch and compared whole with
the expected mask (the pattern's bytes are 0xa5 and 0x7f, never 0 or 1: an unwritten element cannot pass).

Case sizing: the kernel's tile is 32 x 32 pixels of one plane, so the cases of cc_reference.py are 70 x 150 and 5 x 37 x 70 -- at least
two whole tiles and a ragged one along every tiled axis, and ten flat runs of 1024 pixels and a ragged one."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

from arena import Arena
from cc_reference import H2, W2, cases_2d, cases_3d, cases_ids, cc_reference_batch, expected

pytestmark = pytest.mark.gpu
U8, I32 = 0, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def tt(a):
    """a numpy array (the shared cases are read-only) as a CPU tensor of its own"""
    return torch.tensor(np.asarray(a))


def raw(pkg, dev, x, connectivity, min_size=0, skew=(0, 0, 0), want="both", stream=None):
    """pea_cc_label on numpy x [B, Y, X] or [B, Z, Y, X] (uint8, bool or int32) in an arena, twice on one unprepared workspace
    -> (labels int32 or None, counts int32 [B, 2], mask uint8 or None) as device clones.  skew: bytes (in, labels_out, counts)."""
    L = pkg._lib.lib()
    x = np.ascontiguousarray(x)
    B, ndim = x.shape[0], x.ndim - 1
    d = pkg._lib.PeaCcDesc()
    d.ndim, d.B, d.in_type, d.connectivity, d.min_size, d.flags = ndim, B, (I32 if x.dtype == np.int32 else U8), connectivity, min_size, 0
    d.dims[:] = [1 if ndim == 2 else x.shape[1], x.shape[-2], x.shape[-1]]
    nb = L.pea_cc_workspace_bytes(ctypes.byref(d))
    n = x.size
    assert nb >= 8 * n and nb % 8 == 0
    ar = Arena(nb + 10 * n + (1 << 15), dev)
    tin = tt(x.view(np.uint8) if x.dtype == np.bool_ else x)
    X = ar.fill(ar.carve(x.shape, tin.dtype, skew[0], name="in"), tin)
    labels = ar.carve(x.shape, torch.int32, skew[1], name="labels_out") if want in ("both", "labels") else None
    mask = ar.carve(x.shape, torch.uint8, 3, name="mask_out") if want in ("both", "mask") else None
    counts = ar.carve((B, 2), torch.int32, skew[2], name="counts")
    ws = ar.carve((1, nb // 4), torch.int32, 4, name="workspace")  # (one batch item: the arena walks a view's batch in Python)
    assert X.data_ptr() % 16 == skew[0] % 16 and (labels is None or labels.data_ptr() % 16 == skew[1] % 16)
    first = None
    for _ in range(2):  # the second call runs on the workspace as the first one left it
        pkg._lib.check(L.pea_cc_label(ctypes.byref(d), vp(X), vp(labels), vp(mask), vp(counts), vp(ws), nb, stream), "pea_cc_label")
        torch.cuda.synchronize()
        got = tuple(None if t is None else t.clone() for t in (labels, counts, mask))
        if first is not None:
            assert all(a is None or torch.equal(a, b) for a, b in zip(first, got)), "the second call on the same workspace differs"
        first = got
    ar.check(written=[counts] + ([labels] if labels is not None else []), untouched=[X], scratch=[ws] + ([mask] if mask is not None else []))
    return first


def check(what, pkg, dev, x, connectivity, min_size=0, ref=None, **kw):
    """one arena call against the restatement -> the device results"""
    rl, rc = ref if ref is not None else cc_reference_batch(x, connectivity, min_size)
    labels, counts, mask = raw(pkg, dev, x, connectivity, min_size, **kw)
    print(what, "connectivity", connectivity, "min_size", min_size, "counts", counts.tolist(), "ref", rc.tolist())
    assert torch.equal(counts.cpu(), tt(rc)), what
    if labels is not None:
        assert torch.equal(labels.cpu(), tt(rl)), what
    if mask is not None:
        assert torch.equal(mask.cpu(), tt((rl != 0).astype(np.uint8))), what
    return labels, counts, mask


# ---- 1. the named cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("name", sorted(cases_2d()))
def test_2d(pkg, dev, name, connectivity):
    labels, counts, _ = check(name, pkg, dev, cases_2d()[name][None], connectivity, ref=expected("2d", name, connectivity))
    if name == "checkerboard":  # every foreground pixel its own component, or one
        assert counts.tolist() == ([[H2 * W2 // 2, H2 * W2 // 2]] if connectivity == 1 else [[1, 1]])
    if name in ("serpentine", "serpentine_t", "spiral", "comb", "u_shape", "all_foreground", "one_pixel"):
        assert counts.tolist() == [[1, 1]] and int(labels.max()) == 1
    if name == "all_background":
        assert counts.tolist() == [[0, 0]] and not bool(labels.any())


@pytest.mark.parametrize("connectivity", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(cases_3d()))
def test_3d(pkg, dev, name, connectivity):
    _, counts, _ = check(name, pkg, dev, cases_3d()[name][None], connectivity, ref=expected("3d", name, connectivity))
    if name == "helix":
        assert counts.tolist() == [[1, 1]]
    if name == "edge_touch":  # joined at 2 and 3, not at 1
        assert counts.tolist() == ([[2, 2]] if connectivity == 1 else [[1, 1]])
    if name == "corner_touch":  # joined at 3 only
        assert counts.tolist() == ([[1, 1]] if connectivity == 3 else [[2, 2]])


# ---- 2. label images ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases_ids()))
def test_label_image_is_split_into_its_pieces(pkg, dev, name):
    img = cases_ids()[name]
    assert (img < 0).any() and (img == 2 ** 30).any()
    for connectivity in range(1, img.ndim + 1):
        labels, counts, _ = check(name, pkg, dev, img[None], connectivity, ref=expected("ids", name, connectivity))
        assert int(counts[0, 0]) > len(np.unique(img)) - 1  # more pieces than ids: several ids occur in disconnected places
        # adjacent pixels of different ids never share a component
        lab = labels.cpu().numpy()[0]
        for axis in range(img.ndim):
            a, b = np.moveaxis(img, axis, 0), np.moveaxis(lab, axis, 0)
            differ = (a[1:] != a[:-1]) & (a[1:] != 0) & (a[:-1] != 0)
            assert (b[1:][differ] != b[:-1][differ]).all()


def test_one_mask_as_uint8_bool_and_int32(pkg, dev):
    m = cases_2d()["random_0.59"][None]
    for connectivity in (1, 2):
        ref = expected("2d", "random_0.59", connectivity)
        for x in (m, m.astype(np.bool_), m.astype(np.int32)):
            check(str(x.dtype), pkg, dev, x, connectivity, ref=ref)
        # any non-zero value of a mask is foreground of ITS value: one value, the same components
        check("uint8 255", pkg, dev, m * np.uint8(255), connectivity, ref=ref)
        check("int32 -7", pkg, dev, m.astype(np.int32) * -7, connectivity, ref=ref)


# ---- 3. min_size --------------------------------------------------------------------------------------------------------------------------------
def test_min_size_drops_below_and_keeps_at_and_above(pkg, dev):
    m = cases_2d()["sized"][None]
    for connectivity in (1, 2):
        labels, counts, mask = check("sized 25", pkg, dev, m, connectivity, 25, ref=expected("2d", "sized", connectivity, 25))
        assert counts.tolist() == [[4, 3]]
        lab = labels.cpu().numpy()[0]
        # 26 pixels, then 24 (dropped), then 25, then 40: the kept ones are numbered consecutively
        assert lab[1, 100] == 1 and lab[30, 30] == 0 and lab[50, 62] == 2 and lab[60, 120] == 3
        assert np.bincount(lab.ravel())[1:].tolist() == [26, 25, 40] and int(mask.sum()) == 91
        for ms, kept in ((0, 4), (1, 4), (24, 4), (26, 2), (27, 1), (40, 1), (41, 0)):
            _, counts, _ = check("sized", pkg, dev, m, connectivity, ms)
            assert counts.tolist() == [[4, kept]], ms
    for ms in (H2 * W2 + 1, 2 ** 31 - 1):  # larger than the image: nothing is kept
        labels, counts, mask = check("all foreground", pkg, dev, cases_2d()["all_foreground"][None], 2, ms)
        assert counts.tolist() == [[1, 0]] and not bool(labels.any()) and not bool(mask.any())
    labels, counts, _ = check("all foreground", pkg, dev, cases_2d()["all_foreground"][None], 1, H2 * W2)
    assert counts.tolist() == [[1, 1]] and bool((labels == 1).all())
    for connectivity in (1, 2):
        check("random 0.3 min_size 4", pkg, dev, cases_2d()["random_0.3"][None], connectivity, 4, ref=expected("2d", "random_0.3", connectivity, 4))


# ---- 4. batch, alignment, outputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch3():
    """three images, the middle one empty (never modified)"""
    c = cases_2d()
    return np.stack([c["random_0.59"], c["all_background"], c["serpentine"]])


@functools.lru_cache(maxsize=None)
def batch3_ref(connectivity, min_size=0):
    return cc_reference_batch(batch3(), connectivity, min_size)


def test_batch_of_three_restarts_the_ids(pkg, dev):
    for connectivity in (1, 2):
        labels, counts, _ = check("B = 3", pkg, dev, batch3(), connectivity, ref=batch3_ref(connectivity))
        assert counts[1].tolist() == [0, 0] and counts[2].tolist() == [1, 1] and int(labels[2].max()) == 1 and int(labels[0].max()) == int(counts[0, 1])
    check("B = 3, min_size 6", pkg, dev, batch3(), 1, 6, ref=batch3_ref(1, 6))
    vol = np.stack([cases_3d()["random3d_0.3"], cases_3d()["helix"]])
    check("B = 2, 3D", pkg, dev, vol, 2)


def test_skewed_pointers_and_single_outputs(pkg, dev):
    x, ref = batch3(), batch3_ref(2, 3)
    aligned = check("aligned", pkg, dev, x, 2, 3, ref=ref)
    for skew in ((1, 4, 4), (3, 12, 8), (2, 0, 12)):  # uint8 in by 1 .. 3 bytes, labels_out and counts by 4 / 12
        got = check("skew %s" % (skew,), pkg, dev, x, 2, 3, ref=ref, skew=skew)
        assert all(torch.equal(a, b) for a, b in zip(got, aligned)), skew
    xi = x.astype(np.int32) * 5
    for skew in ((4, 12, 0), (12, 4, 4)):  # int32 in by 4 / 12 bytes
        got = check("int32 skew %s" % (skew,), pkg, dev, xi, 2, 3, ref=ref, skew=skew)
        assert all(torch.equal(a, b) for a, b in zip(got, aligned)), skew
    only_l = check("labels only", pkg, dev, x, 2, 3, ref=ref, want="labels")
    only_m = check("mask only", pkg, dev, x, 2, 3, ref=ref, want="mask", skew=(1, 0, 4))
    assert only_l[2] is None and only_m[0] is None and torch.equal(only_l[0], aligned[0]) and torch.equal(only_m[2], aligned[2])


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------------------------------
def test_two_streams_and_ten_calls_give_the_same_labels(pkg, dev):
    L = pkg._lib.lib()
    x = np.stack([cases_2d()["serpentine"], cases_2d()["random_0.59"]])
    ref = cc_reference_batch(x, 1)
    d = pkg._lib.PeaCcDesc()
    d.ndim, d.B, d.in_type, d.connectivity, d.min_size, d.flags = 2, 2, U8, 1, 0, 0
    d.dims[:] = [1, H2, W2]
    nb = L.pea_cc_workspace_bytes(ctypes.byref(d))
    X = tt(x).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    work = [torch.empty(nb // 4, dtype=torch.int32, device=dev) for _ in streams]
    outs = [[torch.full(x.shape, -1, dtype=torch.int32, device=dev) for _ in range(5)] for _ in streams]
    counts = [[torch.full((2, 2), -1, dtype=torch.int32, device=dev) for _ in range(5)] for _ in streams]
    torch.cuda.synchronize()
    for k in range(5):  # ten calls, five on each of two streams that run side by side (a workspace per stream)
        for s, st in enumerate(streams):
            pkg._lib.check(L.pea_cc_label(ctypes.byref(d), vp(X), vp(outs[s][k]), None, vp(counts[s][k]), vp(work[s]), nb,
                                          ctypes.c_void_p(st.cuda_stream)), "pea_cc_label")
    torch.cuda.synchronize()
    for s in range(2):
        for k in range(5):
            assert torch.equal(outs[s][k].cpu(), tt(ref[0])) and torch.equal(counts[s][k].cpu(), tt(ref[1])), (s, k)


# ---- 6. the Python layer -------------------------------------------------------------------------------------------------------------------------------
def test_connected_components_on_dense_strided_and_expanded_inputs(pkg, dev):
    x = tt(batch3()).to(dev)
    for connectivity, c in ((None, 2), (1, 1), (2, 2)):
        rl, rc = batch3_ref(c)
        cc = pkg.connected_components(x, connectivity=connectivity, mask=True)
        assert cc.labels.dtype == torch.int32 and cc.labels.shape == x.shape and cc.mask.dtype == torch.uint8 and cc.counts.shape == (3, 2)
        assert torch.equal(cc.labels.cpu(), tt(rl)) and torch.equal(cc.counts.cpu(), tt(rc))
        assert torch.equal(cc.mask, (cc.labels != 0).to(torch.uint8))
    assert pkg.connected_components(x).mask is None
    wide = torch.zeros((3, H2, 2 * W2), dtype=torch.int32, device=dev)
    wide[:, :, ::2] = x.to(torch.int32) * 9
    for view in (wide[:, :, ::2], wide[::2, :, ::2], x.bool()[:, ::2], x[0].expand(2, H2, W2), x[:, None].expand(3, 2, H2, W2)):
        assert not view.is_contiguous()
        a, b = pkg.connected_components(view, min_size=2, mask=True), pkg.connected_components(view.clone().contiguous(), min_size=2, mask=True)
        assert torch.equal(a.labels, b.labels) and torch.equal(a.counts, b.counts) and torch.equal(a.mask, b.mask)
        ref = cc_reference_batch(view.cpu().numpy(), view.dim() - 1, 2)
        assert torch.equal(a.labels.cpu(), tt(ref[0])) and torch.equal(a.counts.cpu(), tt(ref[1]))
    vol = tt(cases_3d()["random3d_0.3"][None]).to(dev)
    for c in (1, 2, 3):
        got = pkg.connected_components(vol, connectivity=c)
        assert torch.equal(got.labels.cpu(), tt(expected("3d", "random3d_0.3", c)[0]))


def test_remove_samll_object_on_a_tensor_and_on_numpy(pkg, dev):
    m = cases_2d()["random_0.3"]
    want = (expected("2d", "random_0.3", 2, 25)[0][0] != 0).astype(np.uint8)
    assert 0 < want.sum() < m.sum()
    got = pkg.remove_samll_object(tt(m.copy()).to(dev))
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == m.shape and torch.equal(got.cpu(), tt(want))
    got = pkg.remove_samll_object(m.copy())
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(pkg.remove_samll_object(m.astype(np.int64)), want) and np.array_equal(pkg.remove_samll_object(m.astype(bool)), want)
    got = pkg.remove_samll_object(tt(batch3()).to(dev), min_size=6)  # a batch
    assert torch.equal(got.cpu(), tt((batch3_ref(2, 6)[0] != 0).astype(np.uint8)))


def test_foreground_mask_with_min_size(pkg, dev):
    rng = np.random.default_rng(5)
    logits = tt(rng.standard_normal((2, 2, 90, 120)).astype(np.float32) + np.array([0.0, -0.4], np.float32)[None, :, None, None]).to(dev)
    crop = ((9, 11), (4, 6))
    plain = pkg.foreground_mask(logits, crop=crop)
    assert plain.shape == (2, 70, 110) and torch.equal(plain, (logits[:, 1] > logits[:, 0])[:, 9:-11, 4:-6].to(torch.uint8))
    assert torch.equal(pkg.foreground_mask(logits, crop=crop, min_size=0), plain)  # today's output, bit for bit
    want = (cc_reference_batch(plain.cpu().numpy(), 2, 25)[0] != 0).astype(np.uint8)
    got = pkg.foreground_mask(logits, crop=crop, min_size=25)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), tt(want)) and 0 < int(got.sum()) < int(plain.sum())
    assert torch.equal(got, pkg.remove_samll_object(plain))


def test_graphed_step_replays_the_eager_result(pkg, dev):
    first, second = batch3(), np.ascontiguousarray(batch3()[::-1, :, ::-1])
    X = tt(first).to(dev)

    def step(X):
        cc = pkg.connected_components(X, connectivity=2, min_size=3, mask=True)
        return cc.labels, cc.counts, cc.mask

    eager = [t.clone() for t in step(X)]
    rl, rc = batch3_ref(2, 3)
    assert torch.equal(eager[0].cpu(), tt(rl)) and torch.equal(eager[1].cpu(), tt(rc))
    g = pkg.graphed(step, X)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
    X.copy_(tt(second))  # the input buffer refilled: the replay labels what it holds now
    got = [t.clone() for t in g.replay()]
    rl2, rc2 = cc_reference_batch(second, 2, 3)
    assert not np.array_equal(rl2, rl)
    assert torch.equal(got[0].cpu(), tt(rl2)) and torch.equal(got[1].cpu(), tt(rc2))
    assert torch.equal(got[2].cpu(), tt((rl2 != 0).astype(np.uint8)))
    assert all(torch.equal(a, b) for a, b in zip(step(X), got))


# ---- 7. the shape of the driver -----------------------------------------------------------------------------------------------------------------------
def test_more_chunk_totals_than_a_step_of_the_scan(pkg, dev):
    """k_cc_scan takes 256 chunk totals a step with a carry: 513 x 512 pixels are 257 chunks of 1024, an isolated pixel every third row
    and column is a component of its own, and min_size 0 keeps them all, so every id past the first step rests on the carry"""
    m = np.zeros((1, 513, 512), np.uint8)
    m[:, ::3, ::3] = 1
    labels, counts, _ = check("513 x 512 dots", pkg, dev, m, 2, 0)
    assert counts.tolist() == [[171 * 171, 171 * 171]] and int(labels[0, 510, 510]) == 171 * 171


def test_one_bbbc_image(pkg, dev):
    """1 x 520 x 696 with about 150 synthetic nuclei and 200 specks, once: connectivity 2, min_size 25 (remove_samll_object's call)"""
    import __graft_entry__ as ge
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    m = (synth.synth_nuclei(1, 520, 696, 150, 14, 39, specks=200) > 0).astype(np.uint8)
    labels, counts, mask = check("520 x 696", pkg, dev, m, 2, 25)
    assert int(counts[0, 0]) > int(counts[0, 1]) > 50
    assert torch.equal(pkg.remove_samll_object(tt(m[0]).to(dev)), mask[0])
