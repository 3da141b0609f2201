"""GPU: the region adjacency graph on the device (include/pea_rag.h, csrc/pea_k_rag.hip) through the C ABI, through region_adjacency,
project_node_labels and mc_baseline, against the numpy restatement tests/rag_reference.py (which test_rag_host.py holds to a brute-force
walk and to hand-written expectations).

uv, size, count, min, max, node_size and stats are compared for equality.  mean and the boundary mean must lie within
2^-32 + 2^-52 |value| of the reference's: every term is floored to 32 fractional bits (an error below 2^-32 per term, so below 2^-32
in a mean of them), the sum is rounded to f64 once and divided once (include/pea_rag.h).  The reference's own float64 sums of at most a
few hundred f32 terms below 2 are exact to 2^-44, far inside that.  (numpy's random f32 are multiples of 2^-24, which the fixed point
holds exactly; test_bad_ids_and_bad_samples scales two channels and a boundary plane down so that terms have digits below 2^-32.)

Every C call of this file runs in a guard-banded arena (arena.py) on element-offset views: the inputs come back untouched, every
element of every output is written (rows past the edge count are zero), nothing else changes; each call runs twice on one prepared
workspace and must give the same bits.

Case sizing: a wave owns 256 consecutive voxels and a workgroup 1024, so 37 x 53 (X % 4 = 1, 1961 voxels: one whole run of 1024 and a
ragged one) and 5 x 19 x 23 (2185 voxels) have rows that straddle wave runs, a ragged last quad and a ragged last wave."""
import ctypes

import numpy as np
import pytest
import torch

from arena import Arena
from rag_reference import (LOCAL3, SHAPE_3D, hub_image, mean_bound, offsets_for, project_reference, rag_reference, rag_reference_batch, stub_solver,
                           volume, volume_ref, voronoi)

pytestmark = pytest.mark.gpu
ONE_MINUS, IGNORE_ZERO = 1, 2
OUT = (("uv", torch.int32), ("size", torch.int64), ("count", torch.int64), ("mean", torch.float64), ("bmean", torch.float64),
       ("min", torch.float32), ("max", torch.float32), ("node_size", torch.int64), ("stats", torch.int64))
EXACT = ("uv", "size", "count", "min", "max")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def tt(a):
    return torch.tensor(np.asarray(a))


def raw(pkg, dev, frags, affs=None, offsets=(), boundary=None, max_id=None, capacity=1024, max_edges=512, flags=0, skew=(4, 12, 4, 8), calls=2, repeatable=True):
    """pea_rag_build on numpy frags [B, Z, Y, X] (affs [B, K, Z, Y, X], boundary [B, Z, Y, X]) in an arena, `calls` times on one
    prepared workspace -> dict of numpy arrays (of the last call; repeatable: every call gives the bits of the first).  skew: bytes of (fragments, affs / boundary, the 32-bit outputs, the 64-bit outputs)."""
    L = pkg._lib.lib()
    frags = np.ascontiguousarray(frags, np.int32)
    B, Z, Y, X = frags.shape
    ndim = 2 if Z == 1 else 3
    max_id = int(frags.max()) if max_id is None else max_id
    d = pkg._lib.PeaRagDesc()
    d.ndim, d.B, d.K, d.max_id, d.capacity, d.max_edges, d.flags = ndim, B, len(offsets), max_id, capacity, max_edges, flags
    d.dims[:] = [Z, Y, X]
    for k, o in enumerate(offsets):
        d.offsets[k][:] = list(o)
    assert L.pea_rag_validate(ctypes.byref(d)) == 0
    nb = L.pea_rag_workspace_bytes(ctypes.byref(d))
    shapes = {"uv": (B, max_edges, 2), "node_size": (B, max_id + 1), "stats": (B, 8)}
    out_bytes = sum(8 * int(np.prod(shapes.get(n, (B, max_edges)))) for n, _ in OUT)
    ar = Arena(nb + 4 * frags.size * (2 + len(offsets)) + out_bytes + (1 << 16), dev)
    F = ar.fill(ar.carve(frags.shape, torch.int32, skew[0], name="fragments"), tt(frags))
    A = ar.fill(ar.carve(affs.shape, torch.float32, skew[1], name="affs"), tt(affs)) if affs is not None else None
    Bd = ar.fill(ar.carve(boundary.shape, torch.float32, skew[1], name="boundary"), tt(boundary)) if boundary is not None else None
    outs = {n: ar.carve(shapes.get(n, (B, max_edges)), dt, skew[2] if dt in (torch.int32, torch.float32) else skew[3], name=n) for n, dt in OUT}
    ws = ar.carve((1, nb // 4), torch.int32, 8, name="workspace")
    io = pkg._lib.PeaRagBuffers()
    io.fragments, io.affs, io.boundary = F.data_ptr(), A.data_ptr() if A is not None else None, Bd.data_ptr() if Bd is not None else None
    for n, t in outs.items():
        setattr(io, n, t.data_ptr())
    assert F.data_ptr() % 16 == skew[0] % 16 and outs["uv"].data_ptr() % 16 == skew[2] % 16 and outs["mean"].data_ptr() % 16 == skew[3] % 16
    pkg._lib.check(L.pea_rag_workspace_init(ctypes.c_void_p(ws.data_ptr()), nb, None), "pea_rag_workspace_init")
    first = None
    for _ in range(calls):  # the second call runs on the workspace as the first one left it
        pkg._lib.check(L.pea_rag_build(ctypes.byref(d), ctypes.byref(io), ctypes.c_void_p(ws.data_ptr()), nb, None), "pea_rag_build")
        torch.cuda.synchronize()
        got = {n: t.clone() for n, t in outs.items()}
        if first is not None and repeatable:
            for n in got:
                assert torch.equal(first[n].view(torch.uint8), got[n].view(torch.uint8)), "the second call differs in " + n
        first = got
    ar.check(written=list(outs.values()), untouched=[t for t in (F, A, Bd) if t is not None], scratch=[ws])
    return {n: t.cpu().numpy() for n, t in first.items()}


def compare(what, got, refs, node_size=True):
    """the device tables of a batch against the reference's list of per-image results"""
    for b, r in enumerate(refs):
        n = len(r["uv"])
        print(what, "image", b, "stats", got["stats"][b].tolist(), "ref", r["stats"].tolist())
        assert got["stats"][b].tolist() == r["stats"].tolist(), (what, b)
        for k in EXACT:
            assert np.array_equal(got[k][b, :n], r[k]), (what, b, k)
            assert not got[k][b, n:].any(), (what, b, k, "rows past the edge count")
        if node_size:
            assert np.array_equal(got["node_size"][b], r["node_size"]), (what, b)
        for k in ("mean", "bmean"):
            err = np.abs(got[k][b, :n] - r[k])
            print("  ", k, "max error %.3e, bound %.3e" % (err.max() if n else 0.0, 2.0 ** -32))
            assert (err <= mean_bound(r[k])).all(), (what, b, k, float(err.max()))
            assert not got[k][b, n:].any(), (what, b, k)


# ---- 1. the shared volumes: norm5 offsets with long-range channels, B = 2 -------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, ONE_MINUS, ONE_MINUS | IGNORE_ZERO))
@pytest.mark.parametrize("kind", ("2d", "3d"))
def test_volumes(pkg, dev, kind, flags):
    f, a, b = volume(kind)
    refs = volume_ref(kind, bool(flags & ONE_MINUS), bool(flags & IGNORE_ZERO))
    got = raw(pkg, dev, f, a, offsets_for(kind), b, flags=flags)
    compare("%s flags %d" % (kind, flags), got, refs)
    assert all(r["stats"][4] > 0 for r in refs)  # the long-range channels met pairs that do not touch: skipped and counted
    # other pointer alignments, another capacity: the same bits
    again = raw(pkg, dev, f, a, offsets_for(kind), b, flags=flags, capacity=4096, skew=(0, 0, 0, 0), calls=1)
    for n in got:
        assert np.array_equal(got[n].view(np.uint8), again[n].view(np.uint8)), n


def test_without_affs_without_boundary_without_either(pkg, dev):
    f, a, b = volume("3d")
    refs = volume_ref("3d")
    got = raw(pkg, dev, f, None, (), b)
    for r_, g_ in zip(refs, range(2)):
        assert np.array_equal(got["uv"][g_, :len(r_["uv"])], r_["uv"]) and np.array_equal(got["size"][g_, :len(r_["uv"])], r_["size"])
        assert not got["count"][g_].any() and not got["mean"][g_].any() and not got["min"][g_].any()
        assert (np.abs(got["bmean"][g_, :len(r_["uv"])] - r_["bmean"]) <= mean_bound(r_["bmean"])).all()
    got = raw(pkg, dev, f, a, offsets_for("3d"), None)
    assert not got["bmean"].any()
    compare("no boundary", got, rag_reference_batch(f, a, offsets_for("3d"), None, max_id=int(f.max())))
    compare("graph only", raw(pkg, dev, f), rag_reference_batch(f, max_id=int(f.max())))


# ---- 2. the ends of a row, of a plane and of an image ------------------------------------------------------------------------------------------
def test_row_plane_and_image_ends_are_no_neighbours(pkg, dev):
    f = np.zeros((2, 3, 3, 5), np.int32)
    f[0, 0, 0, 4], f[0, 0, 1, 0] = 7, 8      # the last voxel of a row, the first of the next
    f[0, 0, 2, 4], f[0, 1, 0, 0] = 9, 10     # the last voxel of a plane, the first of the next
    f[0, 2, 2, 4], f[1, 0, 0, 0] = 11, 12    # the last voxel of image 0, the first of image 1
    a = np.random.default_rng(3).random((2, 3, 3, 3, 5), dtype=np.float32)
    refs = rag_reference_batch(f, a, LOCAL3, f.astype(np.float32), max_id=12)
    got = raw(pkg, dev, f, a, LOCAL3, f.astype(np.float32), max_id=12, capacity=64, max_edges=16)
    compare("ends", got, refs)
    assert got["uv"][0, :5].tolist() == [[0, 7], [0, 8], [0, 9], [0, 10], [0, 11]] and got["stats"][0, 0] == 5
    assert got["uv"][1, :1].tolist() == [[0, 12]] and got["stats"][1, 0] == 1
    # the same content as one image of 2D rows: X = 5, eighteen rows
    g = f.reshape(1, 1, 18, 5)
    compare("ends 2d", raw(pkg, dev, g, max_id=12, capacity=64, max_edges=16), rag_reference_batch(g, max_id=12))


# ---- 3. what is no id, what is no sample --------------------------------------------------------------------------------------------------------
def test_bad_ids_and_bad_samples_are_skipped_and_counted(pkg, dev):
    f, a, b = (x.copy() for x in volume("3d"))
    max_id = int(f.max()) - 2                     # the two highest ids are no ids
    f[0, 0, 0, :7], f[1, 2, 5, 5], f[1, 4, 18, 22] = -1, -2 ** 31, 2 ** 31 - 1
    a[0, 0, 1], a[0, 1, 2, 3], a[1, 2, :, :, 7], a[1, 5, 3] = np.nan, np.inf, 1e30, -np.inf
    a[0, 3] = -a[0, 3] * 5                        # negative samples
    a[1, 0] *= np.float32(1e-4)                   # samples with digits below 2^-32: the floor of a term is not the term
    a[1, 1] *= np.float32(-3e-5)
    b[0, 4] *= np.float32(1e-5)
    a[1, 4, 2, 2, 2] = 32768.0                    # the largest sample that counts
    a[1, 4, 2, 2, 3] = np.nextafter(np.float32(32768.0), np.float32(np.inf))
    b[0, 1, 3], b[1, 2, 2, 2] = np.nan, -1e30
    b[1, 3] = -b[1, 3]
    for flags in (0, ONE_MINUS | IGNORE_ZERO):
        refs = rag_reference_batch(f, a, offsets_for("3d"), b, max_id=max_id, one_minus=bool(flags & ONE_MINUS), ignore_zero=bool(flags & IGNORE_ZERO))
        assert all(r["stats"][3] > 0 and r["stats"][5] > 0 for r in refs) and (flags or (refs[0]["min"] < 0).any())
        compare("bad flags %d" % flags, raw(pkg, dev, f, a, offsets_for("3d"), b, max_id=max_id, flags=flags), refs)


# ---- 4. a hub, one id, every voxel its own id -----------------------------------------------------------------------------------------------------
def test_hub_single_id_and_singletons(pkg, dev):
    h = hub_image()[None]
    rng = np.random.default_rng(8)
    a = rng.random((1, 2, 1, 96, 96), dtype=np.float32)
    offs = [[0, -1, 0], [0, 0, -1]]
    refs = rag_reference_batch(h, a, offs, a[:, 0], max_id=1030)
    assert (refs[0]["uv"][:, 0] == 1).sum() == 1025
    compare("hub", raw(pkg, dev, h, a, offs, a[:, 0], max_id=1030, capacity=2048, max_edges=1100), refs)
    one = np.full((2, 1, 37, 53), 5, np.int32)
    got = raw(pkg, dev, one, a[:, :, :, :37, :53].repeat(2, 0), offs, None, max_id=5, capacity=64, max_edges=4)
    assert got["stats"].tolist() == [[0] * 8] * 2 and not got["uv"].any() and got["node_size"].tolist() == [[0, 0, 0, 0, 0, 1961]] * 2
    own = np.arange(2 * 24 * 31, dtype=np.int32).reshape(2, 1, 24, 31) % (24 * 31)
    refs = rag_reference_batch(own, a[:, :, :, :24, :31].repeat(2, 0), offs, None, max_id=24 * 31 - 1)
    assert refs[0]["stats"][0] == 23 * 31 + 24 * 30
    compare("singletons", raw(pkg, dev, own, a[:, :, :, :24, :31].repeat(2, 0), offs, None, max_id=24 * 31 - 1, capacity=4096, max_edges=1500), refs)


def test_ids_on_both_sides_of_a_step_of_the_row_start_scan(pkg, dev):
    """k_rag_scan takes 2048 ids a step and carries the row starts from one step to the next: ids 0 .. 2303 with edges on both sides of
    the step, then an image whose only ids lie around it"""
    own = np.arange(48 * 48, dtype=np.int32).reshape(1, 1, 48, 48)
    a = np.random.default_rng(48).random((1, 2, 1, 48, 48), dtype=np.float32)
    offs = [[0, -1, 0], [0, 0, -1]]
    refs = rag_reference_batch(own, a, offs, a[:, 0], max_id=2303)
    assert refs[0]["stats"][0] == 2 * 47 * 48 and (refs[0]["uv"][:, 0] < 2048).any() and (refs[0]["uv"][:, 0] >= 2048).any()
    compare("48 x 48 singletons", raw(pkg, dev, own, a, offs, a[:, 0], max_id=2303, capacity=8192, max_edges=4600), refs)
    few = np.array([[2047, 2048, 2049, 2049], [2049, 2047, 2048, 2048]], np.int32).reshape(1, 1, 2, 4)
    refs = rag_reference_batch(few, a[:, :, :, :2, :4], offs, None, max_id=2049)
    assert refs[0]["uv"].tolist() == [[2047, 2048], [2047, 2049], [2048, 2049]]
    compare("2047 2048 2049", raw(pkg, dev, few, a[:, :, :, :2, :4], offs, None, max_id=2049, capacity=64, max_edges=8), refs)


# ---- 5. a table and an edge list too small on purpose: the call returns and says so ---------------------------------------------------------------
def test_small_capacity_and_small_max_edges(pkg, dev):
    _, a, b = volume("3d")
    f = np.stack([voronoi(SHAPE_3D, 60, 21), voronoi(SHAPE_3D, 70, 22)])  # more edges than the smallest table holds
    refs = rag_reference_batch(f, a, offsets_for("3d"), b, max_id=int(f.max()))
    n = [len(r["uv"]) for r in refs]
    assert min(n) > 64 and max(n) < 500
    # which pairs find a slot in a full table depends on the order of arrival, so the two calls may differ; what is checked is the
    # second one, which finds the table as empty as the first one did
    got = raw(pkg, dev, f, a, offsets_for("3d"), b, capacity=64, max_edges=512, repeatable=False)
    for i in range(2):
        s = got["stats"][i]
        assert 0 < s[0] <= 64 and s[2] > 0 and s[1] == 0 and s[3] == 0
        assert int(got["size"][i].sum()) + int(s[2]) == int(refs[i]["size"].sum())  # every voxel pair is in the table or counted
    got = raw(pkg, dev, f, a, offsets_for("3d"), b, capacity=1024, max_edges=40)
    for i in range(2):
        assert got["stats"][i, :3].tolist() == [n[i], n[i] - 40, 0]
        for k in EXACT:  # the edges are sorted, so the first 40 are the reference's first 40
            assert np.array_equal(got[k][i], refs[i][k][:40]), k
    # the wrapper raises and names the parameter; with the defaults it retries once at four times the size
    F, A, Bd = tt(f[0]).to(dev), tt(a[0]).to(dev), tt(b[0]).to(dev)
    with pytest.raises(RuntimeError, match="pass a larger capacity"):
        pkg.region_adjacency(F, A, offsets_for("3d"), Bd, capacity=64).uv
    with pytest.raises(RuntimeError, match="pass a larger max_edges"):
        pkg.region_adjacency(F, A, offsets_for("3d"), Bd, capacity=1024, max_edges=40).uv  # (the default table of 256 is too small too)
    own = np.arange(256, dtype=np.int32).reshape(16, 16)
    rag = pkg.region_adjacency(tt(own).to(dev))      # 480 edges: the default table of 256 slots is retried at 1024
    assert rag.capacity == 256 and rag.n_edges == 480 and rag.capacity == 1024 and rag.max_edges == 512
    assert np.array_equal(rag.uv, rag_reference(own[None])["uv"])
    big = np.arange(1024, dtype=np.int32).reshape(32, 32)  # 1984 edges: the retry is too small as well
    with pytest.raises(RuntimeError, match="pass a larger"):
        pkg.region_adjacency(tt(big).to(dev)).uv


# ---- 6. the Python layer -------------------------------------------------------------------------------------------------------------------------------
def check_rag(rag, ref):
    assert rag.n_edges == len(ref["uv"]) and np.array_equal(rag.uv, ref["uv"]) and rag.uv.dtype == np.int32
    assert np.array_equal(rag.sizes, ref["size"]) and np.array_equal(rag.counts, ref["count"])
    assert np.array_equal(rag.min, ref["min"]) and np.array_equal(rag.max, ref["max"]) and np.array_equal(rag.node_sizes, ref["node_size"])
    assert (np.abs(rag.mean - ref["mean"]) <= mean_bound(ref["mean"])).all()
    assert (np.abs(rag.boundary_mean - ref["bmean"]) <= mean_bound(ref["bmean"])).all()
    assert [rag.stats[k] for k in ("edges", "edges_dropped", "pairs_dropped", "no_id", "not_touching", "skipped")] == ref["stats"][:6].tolist()


def test_region_adjacency(pkg, dev):
    for kind in ("2d", "3d"):
        f, a, b = volume(kind)
        offs = offsets_for(kind)
        offs_py = [o[1:] for o in offs] if kind == "2d" else offs
        sq = (lambda x: x[..., 0, :, :]) if kind == "2d" else (lambda x: x)
        refs, refs1 = volume_ref(kind), volume_ref(kind, True, True)
        F, A, Bd = tt(sq(f)).to(dev), tt(sq(a)).to(dev), tt(sq(b)).to(dev)
        rag = pkg.region_adjacency(F[1], A[1], offs_py, Bd[1])   # max_id from the data: one round trip
        assert rag.n_nodes == int(f[1].max()) + 1
        check_rag(rag, refs[1])
        check_rag(pkg.region_adjacency(sq(f)[1].copy(), sq(a)[1].copy(), offs_py, sq(b)[1].copy(), one_minus=True, ignore_zero=True), refs1[1])  # numpy in
        check_rag(pkg.region_adjacency(F[1].to(torch.int64), A[1].double(), offs_py, Bd[1].double()), refs[1])
        want = pkg.transform_probabilities_to_costs(rag.mean, 0.3, rag.sizes, 2.0)
        assert np.array_equal(rag.costs(0.3, 2.0), want) and rag.costs().dtype == np.float64
        # a batch, with everything named: no synchronisation
        M = int(f.max())
        ragb = pkg.region_adjacency(F, A, offs_py, Bd, max_id=M, capacity=1024, max_edges=512, batched=True)
        assert ragb.tensors["uv"].shape == (2, 512, 2) and ragb.tensors["uv"].is_cuda
        for i in range(2):
            assert np.array_equal(ragb.uv[i], refs[i]["uv"]) and np.array_equal(ragb.counts[i], refs[i]["count"])
            assert np.array_equal(ragb.node_sizes[i], refs[i]["node_size"]) and ragb.stats[i]["not_touching"] == refs[i]["stats"][4]
        # strided and permuted views against their dense clones
        wide = torch.zeros((2, len(offs)) + tuple(F.shape[1:-1]) + (2 * F.shape[-1],), device=dev)
        wide[..., ::2] = A
        perm = A.transpose(0, 1).contiguous().transpose(0, 1)
        for view in (wide[..., ::2], perm):
            assert not view.is_contiguous()
            r2 = pkg.region_adjacency(F, view, offs_py, Bd, max_id=M, capacity=1024, max_edges=512, batched=True)
            for n in ragb.tensors:
                assert torch.equal(r2.tensors[n].view(torch.uint8), ragb.tensors[n].view(torch.uint8)), n


def test_graphed_replay_gives_the_bits_of_the_eager_call(pkg, dev):
    f, a, b = volume("3d")
    F, A, Bd = tt(f).to(dev), tt(a).to(dev), tt(b).to(dev)
    M = int(f.max())
    names = [n for n, _ in OUT]

    def step(F, A, Bd):
        t = pkg.region_adjacency(F, A, offsets_for("3d"), Bd, one_minus=True, max_id=M, capacity=1024, max_edges=512, batched=True).tensors
        return tuple(t[n] for n in names)

    eager = [t.clone() for t in step(F, A, Bd)]
    again = [t.clone() for t in step(F, A, Bd)]
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(eager, again))
    compare("eager", {n: t.cpu().numpy() for n, t in zip(names, eager)}, volume_ref("3d", True))
    g = pkg.graphed(step, F, A, Bd)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got, eager))
    F.copy_(tt(f[::-1].copy()))  # the input buffers refilled: the replay sees what they hold now
    A.copy_(tt(a[::-1].copy()))
    Bd.copy_(tt(b[::-1].copy()))
    got = [t.clone() for t in g.replay()]
    compare("replay", {n: t.cpu().numpy() for n, t in zip(names, got)}, volume_ref("3d", True)[::-1])


def test_project_node_labels(pkg, dev):
    f = volume("3d")[0].copy()
    M = int(f.max())
    labels = np.random.default_rng(2).integers(-5, 1000, M + 1).astype(np.int32)
    F = tt(f).to(dev)
    seg = pkg.project_node_labels(F, tt(labels).to(dev))
    assert seg.dtype == torch.int32 and seg.shape == F.shape and seg.is_cuda and np.array_equal(seg.cpu().numpy(), labels[f])
    f[0, 0, 0, :9], f[1, 4, 18, 20:] = -3, M + 1  # no nodes: 0, counted
    want, n_bad = project_reference(f, labels)
    seg, bad = pkg.project_node_labels(tt(f).to(dev), labels.astype(np.int64), count_bad=True)
    assert np.array_equal(seg.cpu().numpy(), want) and int(bad) == n_bad == 12
    got = pkg.project_node_labels(f.astype(np.int64), labels)  # numpy in, numpy out
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
    # the C entry on element-offset views of every length around a quad and a run: every element written, nothing else
    L = pkg._lib.lib()
    flat = f.ravel()
    for n, skew in ((1, 4), (3, 8), (4, 0), (4099, 12), (4096, 4), (flat.size, 4)):
        ar = Arena(3 * 4 * n + 4 * (M + 1) + (1 << 14), dev)
        Fv = ar.fill(ar.carve((n,), torch.int32, skew, name="fragments"), tt(flat[:n]))
        Nv = ar.fill(ar.carve((M + 1,), torch.int32, 4, name="node_labels"), tt(labels))
        Sv = ar.carve((n,), torch.int32, (skew + 4) % 16, name="seg")
        Bv = ar.fill(ar.carve((1,), torch.int64, 8, name="n_bad"), tt(np.array([100], np.int64)))
        pkg._lib.check(L.pea_rag_project(n, Fv.data_ptr(), Nv.data_ptr(), M + 1, Sv.data_ptr(), Bv.data_ptr(), None), "pea_rag_project")
        torch.cuda.synchronize()
        w, nb = project_reference(flat[:n], labels)
        assert np.array_equal(Sv.cpu().numpy(), w) and int(Bv) == 100 + nb, n
        ar.check(written=[Sv], untouched=[Fv, Nv], scratch=[Bv])


def test_mc_baseline_with_a_stub_solver(pkg, dev):
    for kind, sq in (("3d", lambda x: x), ("2d", lambda x: x[..., 0, :, :])):
        f, a, _ = volume(kind)
        f, a = f[1], a[1, :3 if kind == "3d" else 2]
        inv = (np.float32(1) - a).astype(np.float32)
        boundary = np.maximum(inv[1], inv[2]) if kind == "3d" else np.maximum(inv[0], inv[1])
        offs3 = LOCAL3 if kind == "3d" else [[0, -1, 0], [0, 0, -1]]
        ref = rag_reference(f, a, offs3, boundary, one_minus=True)
        costs = pkg.transform_probabilities_to_costs(ref["mean"], edge_sizes=ref["size"])
        assert (costs < 0).any() and (costs > 0).any() and np.abs(costs).min() > 1e-6  # no cost so near 0 that 2^-32 in the mean turns its sign
        want = stub_solver(int(f.max()) + 1, ref["uv"], costs)[f].astype(np.int32)
        assert len(np.unique(want)) < len(np.unique(f))
        calls = []

        def solver(n_nodes, uvs, c):
            calls.append((n_nodes, np.array(uvs), np.array(c)))
            return stub_solver(n_nodes, uvs, c)

        A, F = tt(sq(a)).to(dev), tt(sq(f)).to(dev)
        seg = pkg.mc_baseline(A, F, solver=solver)
        assert seg.is_cuda and seg.dtype == torch.int32 and np.array_equal(seg.cpu().numpy(), sq(want))
        assert calls[0][0] == int(f.max()) + 1 and np.array_equal(calls[0][1], ref["uv"]) and np.allclose(calls[0][2], costs, rtol=0, atol=1e-6)
        got = pkg.mc_baseline(sq(a), sq(f).astype(np.uint64), solver=solver)  # numpy in (the reference's fragments are uint64), numpy out
        assert isinstance(got, np.ndarray) and np.array_equal(got, sq(want))
        got = pkg.multicut_multi(A, fragments=F, solver=solver)
        assert np.array_equal(got.cpu().numpy(), sq(want))
        # a strided and a permuted view of the affinities against the dense clone
        wide = torch.zeros(tuple(A.shape[:-1]) + (2 * A.shape[-1],), device=dev)
        wide[..., ::2] = A
        for view in (wide[..., ::2], A.transpose(0, 1).contiguous().transpose(0, 1)):
            assert not view.is_contiguous()
            assert torch.equal(pkg.mc_baseline(view, F, solver=solver), seg)
        # long-range channels through multicut_multi: pairs that do not touch are left out, the graph and the sizes stay
        if kind == "3d":
            a9 = volume(kind)[1][1]
            ref9 = rag_reference(f, a9, offsets_for(kind), boundary, one_minus=True)
            c9 = pkg.transform_probabilities_to_costs(ref9["mean"], edge_sizes=ref9["size"])
            want9 = stub_solver(int(f.max()) + 1, ref9["uv"], c9)[f].astype(np.int32)
            assert np.abs(c9).min() > 1e-6
            got9 = pkg.multicut_multi(tt(a9).to(dev), offsets_for(kind), F, stub_solver)
            assert np.array_equal(got9.cpu().numpy(), want9)
