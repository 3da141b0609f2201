"""CPU: the numpy restatement of target generation (tests/targets_reference.py) and the refusals of the label -> target entry points.

  * the restatement equals oracle.np_gen_targets and np_weight_binary_ratio (the pixel-by-pixel statement) on small cases, equals
    synth.affinity_targets and class_balance_weights (the slice statement, what bench.py feeds the loss with) on every shared case, and
    equals the reference project's own outputs in tests/golden/gtgt_2d_nb4.npz, gtgt_2d_nb8.npz and gseg2aff_3d.npz;
  * class balance on every branch of class_balance() against hand-written values;
  * pea_gen_targets, pea_label_weights and pea_targets_workspace_bytes: every refusal that launches nothing, with fake pointers, in the
    order csrc/pea_abi.hip and csrc/pea_k_labels.hip make the checks; and that an offset reaching past the image is NOT refused by
    these three (include/pea.h) while pea_desc_validate refuses it.

Everything is an integer or an f32 rounded once from one f64 expression: all comparisons are np.array_equal."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import targets_reference as tr
from conftest import load_golden

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


# ---- the restatement against the other statements ------------------------------------------------------------------------------------------
SMALL = [("lds_37x100", "nb4_k10"), ("direct_33x67", "far_halo"), ("tiny_3x5", "past_3x5"), ("tiny_3x5", "k1"), ("one_pixel", "past_1x1"),
         ("vol_5x19x23", "oz"), ("vol_3x8x12", "inplane"), ("vol_3x8x12", "oz")]


@pytest.mark.parametrize("geometry,table", SMALL, ids=["%s-%s" % c for c in SMALL])
def test_restatement_equals_the_oracle(orc, geometry, table):
    lab = tr.label_image(geometry)
    for flags in tr.FLAG_COMBOS:
        t, m, w, wtab, count = tr.expected(geometry, table, flags)
        o_t, o_m = orc.np_gen_targets(lab, tr.table(table), padding=bool(flags & tr.PADDING), both_foreground=bool(flags & tr.BOTH_FOREGROUND))
        assert np.array_equal(t, o_t) and np.array_equal(m, o_m), flags
        assert np.array_equal(w, orc.np_weight_binary_ratio(o_t)), flags
        assert w.dtype == np.float32 and t.dtype == np.float32 and m.dtype == np.uint8 and wtab.dtype == np.float32


@pytest.mark.parametrize("geometry,table", tr.CASES, ids=["%s-%s" % c for c in tr.CASES])
def test_restatement_equals_synth(synth, geometry, table):
    lab = tr.label_image(geometry)
    for flags in tr.FLAG_COMBOS:
        t, m, w, wtab, count = tr.expected(geometry, table, flags)
        s_t, s_m = synth.affinity_targets(lab, tr.offsets3(tr.table(table)), padding=bool(flags & tr.PADDING),
                                          both_foreground=bool(flags & tr.BOTH_FOREGROUND))
        assert np.array_equal(t, s_t) and np.array_equal(m, s_m), flags
        assert np.array_equal(w, synth.class_balance_weights(s_t)), flags
        # MASK_INSIDE speaks to the labels-in step only
        again = tr.targets_reference(lab, tr.table(table), flags | tr.MASK_INSIDE)
        assert all(np.array_equal(a, b) for a, b in zip(again, (t, m, w, wtab, count)))
        # the two forms of the weights are one statement
        sel = (slice(None), slice(None), None, None, None)
        assert np.array_equal(w, np.where(t != 0, wtab[..., 0][sel], wtab[..., 1][sel]))
        assert np.array_equal(count, (t != 0).reshape(t.shape[0], t.shape[1], -1).sum(axis=2))


@pytest.mark.parametrize("name", ["gtgt_2d_nb4", "gtgt_2d_nb8"])
def test_restatement_equals_the_reference_goldens(name):
    g = load_golden(name)
    lab = np.ascontiguousarray(g["labels"][:, None]).astype(np.int32)
    for flags, tag in ((tr.PADDING, "pad"), (0, "nopad")):
        t, m, w, _, _ = tr.targets_reference(lab, [list(o) for o in g["offsets"]], flags)
        assert np.array_equal(t[:, :, 0], g["target_" + tag]) and np.array_equal(m[:, :, 0], g["mask_" + tag])
        assert np.array_equal(w[:, :, 0], g["weight_" + tag])


def test_seg_to_aff_restatement_equals_the_reference_golden():
    g = load_golden("gseg2aff_3d")
    seg = np.ascontiguousarray(g["seg"][None]).astype(np.int32)
    assert np.array_equal(tr.seg_to_aff_reference(seg)[0], g["aff3_replicate"])
    nh = lambda a, b, c: [[-a, 0, 0], [0, -b, 0], [0, 0, -c]]
    a12 = np.concatenate([tr.seg_to_aff_reference(seg, n, pad="") for n in (nh(1, 1, 1), nh(2, 3, 3), nh(3, 9, 9), nh(4, 27, 27))], axis=1)
    assert np.array_equal(a12[0], g["aff12_nopad"])


def test_tables_and_label_images_are_what_the_cases_need(pkg):
    assert tr.multi_offset([1, 3, 5, 9, 27], 4) == pkg.multi_offset([1, 3, 5, 9, 27], 4) and len(tr.TABLES_2D["nb4_k10"]) == 10
    assert tr.multi_offset([1, 3, 9], 8) == pkg.multi_offset([1, 3, 9], 8) and len(tr.TABLES_2D["nb8_k12"]) == 12
    assert [len(tr.TABLES_2D[k]) for k in ("k1", "k5", "k6", "k32")] == [1, 5, 6, pkg._lib.PEA_MAX_K]
    reach = lambda t: max(max(abs(v) for v in o) for o in t)
    assert reach(tr.TABLES_2D["k32"]) == reach(tr.TABLES_2D["reach28"]) == reach(tr.TABLES_2D["far_halo"]) == tr.LDS_HALO
    assert reach(tr.TABLES_2D["reach29"]) == tr.LDS_HALO + 1
    assert any(o[0] > 0 for o in tr.TABLES_2D["far_halo"]) and any(o[1] > 0 for o in tr.TABLES_2D["far_halo"])
    # every channel of the past-the-image tables has no neighbour inside: the mask is zero everywhere
    for geometry, table in (("tiny_3x5", "past_3x5"), ("one_pixel", "past_1x1")):
        for flags in tr.FLAG_COMBOS:
            t, m, w, wtab, count = tr.expected(geometry, table, flags)
            assert not m.any() and (t == (1.0 if flags & tr.PADDING else 0.0)).all() and (w == 1).all() and (wtab == 1).all()
    Z = tr.GEOMETRIES["vol_5x19x23"][1]
    assert any(abs(o[0]) > Z for o in tr.TABLES_3D["oz"]) and all(o[0] == 0 for o in tr.TABLES_3D["inplane"])
    for g in tr.GEOMETRIES:
        lab = tr.label_image(g)
        assert lab.dtype == np.int32 and lab.min() > -2 ** 31  # never the outside marker of the LDS route
    lab = tr.label_image("lds_37x100")
    assert {-3, -7, 0, tr.INT_MAX, -tr.INT_MAX} <= set(np.unique(lab).tolist()) and (lab > 0).sum() > lab.size // 2


def test_both_foreground_gives_zero_on_equal_negatives_and_zeros():
    lab = tr.label_image("lds_37x100")
    assert (lab[:, 0, 2:4, 3:5] == -3).all() and (lab[:, 0, 11:13, 1:3] == 0).all() and (lab[:, 0, 13:15, 10:12] == tr.INT_MAX).all()
    plain = tr.expected("lds_37x100", "k1", 0)[0]
    fg = tr.expected("lds_37x100", "k1", tr.BOTH_FOREGROUND)[0]
    for rows, cols, want in ((slice(2, 4), slice(3, 5), 0.0), (slice(11, 13), slice(1, 3), 0.0), (slice(13, 15), slice(10, 12), 1.0)):
        assert (plain[:, 0, 0, rows, cols] == 1).all() and (fg[:, 0, 0, rows, cols] == want).all()


# ---- class balance on its branches ---------------------------------------------------------------------------------------------------------
def test_class_balance_by_hand():
    one = np.float32(1)
    assert tr.W19 == np.float32(19) and tr.W99 == np.float32(99)
    for count, S, want in ((0, 100, (1, 1)), (100, 100, (1, 1)), (50, 100, (1, 1)), (1, 2, (1, 1)),
                           (5, 100, (19, 1)), (1, 20, (19, 1)), (1, 21, (19, 1)), (4, 100, (19, 1)), (1, 10 ** 9, (19, 1)),
                           (99, 100, (1, 99)), (127, 128, (1, 99)), (10 ** 9 - 1, 10 ** 9, (1, 99)),
                           (1, 8, (7, 1)), (7, 8, (1, 7)), (1, 4, (3, 1)), (3, 4, (1, 3)),
                           (6, 100, (np.float32(0.94 / 0.06), 1)), (49, 100, (np.float32(0.51 / 0.49), 1)), (51, 100, (1, np.float32(0.51 / 0.49)))):
        got = tr.class_balance(count, S)
        assert got[0].dtype == np.float32 and got[1].dtype == np.float32
        assert got == (np.float32(want[0]), np.float32(want[1])), (count, S, got)
    assert tr.class_balance(1, 20)[0] != tr.class_balance(6, 100)[0]  # 0.05 and 0.06 are told apart
    assert one == tr.class_balance(1, 2)[0] == tr.class_balance(1, 2)[1]


@pytest.mark.parametrize("kind,X,flags,want", tr.BALANCE, ids=["%s-%d-%d" % c[:3] for c in tr.BALANCE])
def test_balance_images_have_the_counts_they_are_built_for(kind, X, flags, want):
    lab = tr.balance_labels(kind, X)
    t, m, w, wtab, count = tr.targets_reference(lab, [[0, -1]], flags)
    S = tr.BALANCE_Y * X
    assert count.tolist() == [[tr.balance_count(kind, X, flags)]]
    assert int(m.sum()) == S - tr.BALANCE_Y
    assert wtab[0, 0].tolist() == [float(np.float32(want[0])), float(np.float32(want[1]))]
    if kind == "distinct" and flags:
        assert (t[0, 0, 0, :, 0] == 1).all() and not t[0, 0, 0, :, 1:].any()
        assert (w[0, 0, 0, :, 0] == np.float32(want[0])).all() and (w[0, 0, 0, :, 1:] == 1).all()


# ---- the refusals, none of which launches anything -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def desc(pkg, B=2, dims=(1, 8, 12), offsets=((0, -1, 0), (0, 0, -1), (0, 3, 2))):
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, (2 if dims[0] == 1 else 3), B, 1, len(offsets)
    d.dims[:] = dims
    d.border, d.dtype, d.norm, d.flags, d.eps = pkg._lib.BORDER_CROP_ZERO, pkg._lib.F32, pkg._lib.NORM_FULL, 0, 1e-12
    for i, o in enumerate(offsets):
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    return d


P = ctypes.c_void_p
BIG = ctypes.c_size_t(1 << 40)


def gen(lib, d, labels=64, flags=0, target=128, mask=192, weight=256, ws=320, nbytes=BIG):
    return lib.pea_gen_targets(None if d is None else ctypes.byref(d), P(labels) if labels else None, flags, P(target) if target else None,
                               P(mask) if mask else None, P(weight) if weight else None, P(ws) if ws else None, nbytes, None)


def wts(lib, d, labels=64, flags=0, wtab=128, ws=320, nbytes=BIG):
    return lib.pea_label_weights(None if d is None else ctypes.byref(d), P(labels) if labels else None, flags, P(wtab) if wtab else None,
                                 P(ws) if ws else None, nbytes, None)


def test_workspace_bytes(pkg, lib):
    for B, dims, K in ((2, (1, 8, 12), 3), (2, (1, 37, 100), 10), (1, (1, 70, 132), 32), (2, (5, 19, 23), 11), (1, (1, 1, 1), 1), (3, (4, 33, 65), 2)):
        d = desc(pkg, B, dims, [(0, 0, 0)] * K)
        wgs = ((dims[2] + 63) // 64) * ((dims[1] + 31) // 32) * dims[0]  # one partial per 32 x 64 tile of a plane
        assert lib.pea_targets_workspace_bytes(ctypes.byref(d)) == B * K * 4 * wgs
    assert lib.pea_targets_workspace_bytes(None) == 0
    for field, value in (("abi", 1), ("K", 0), ("K", 33), ("B", 0), ("ndim", 4)):
        d = desc(pkg)
        setattr(d, field, value)
        assert lib.pea_targets_workspace_bytes(ctypes.byref(d)) == 0
    d = desc(pkg)
    d.dims[1] = 0
    assert lib.pea_targets_workspace_bytes(ctypes.byref(d)) == 0


def test_null_descriptor_and_bad_descriptor(pkg, lib):
    assert gen(lib, None) == E_NULL and wts(lib, None) == E_NULL
    for field, value in (("abi", 1), ("K", 0), ("K", 33), ("B", 0), ("ndim", 1)):
        d = desc(pkg)
        setattr(d, field, value)
        assert gen(lib, d) == E_DESC and wts(lib, d) == E_DESC
        assert gen(lib, d, labels=0) == E_DESC and wts(lib, d, wtab=0) == E_DESC  # the descriptor is judged before the pointers
    d = desc(pkg, dims=(2, 8, 12))
    d.ndim = 2  # two dimensions need Z == 1
    assert gen(lib, d) == E_DESC and wts(lib, d) == E_DESC


def test_an_offset_past_the_image_is_served_by_these_calls_only(pkg, lib):
    for off in ((0, -8, 0), (0, 8, 0), (0, 0, 12), (0, 0, -40), (-1, 0, 0), (5, 0, 0), (0, 2 ** 31 - 1, -2 ** 31)):
        d = desc(pkg, offsets=((0, -1, 0), off))
        assert lib.pea_desc_validate(ctypes.byref(d)) == E_DESC
        assert lib.pea_targets_workspace_bytes(ctypes.byref(d)) == 2 * 2 * 4
        # past the descriptor check: the next refusal in the order answers
        assert gen(lib, d, labels=0) == E_NULL and wts(lib, d, wtab=0) == E_NULL
        assert gen(lib, d, ws=0) == E_WORKSPACE and wts(lib, d, ws=0) == E_WORKSPACE


def test_null_pointers(pkg, lib):
    d = desc(pkg)
    assert gen(lib, d, labels=0) == E_NULL and gen(lib, d, target=0) == E_NULL
    assert wts(lib, d, labels=0) == E_NULL and wts(lib, d, wtab=0) == E_NULL
    # NULL comes before alignment, flags and workspace
    assert gen(lib, d, labels=0, target=129, flags=8, ws=0) == E_NULL and wts(lib, d, wtab=0, labels=65, flags=8, ws=0) == E_NULL


def test_alignment(pkg, lib):
    d = desc(pkg)
    for off in (1, 2, 3):
        for arg in ("labels", "target", "weight", "ws"):
            assert gen(lib, d, **{arg: 1024 + off}) == E_ALIGN, (arg, off)
        for arg in ("labels", "wtab", "ws"):
            assert wts(lib, d, **{arg: 1024 + off}) == E_ALIGN, (arg, off)
        # alignment comes before the flags and the workspace size; the mask is bytes
        assert gen(lib, d, target=1024 + off, flags=8, nbytes=0) == E_ALIGN and wts(lib, d, wtab=1024 + off, flags=8, nbytes=0) == E_ALIGN
        assert gen(lib, d, mask=1024 + off, ws=0) == E_WORKSPACE
    for off in (4, 8, 12):  # element alignment is enough
        assert gen(lib, d, labels=1024 + off, target=2048 + off, weight=4096 + off, ws=0) == E_WORKSPACE
        assert wts(lib, d, labels=1024 + off, wtab=2048 + off, ws=0) == E_WORKSPACE


def test_flags(pkg, lib):
    d = desc(pkg)
    for bad in (8, 16, 1 << 31, 8 | 1):  # 8 is PEA_TGT_ACCUMULATE: the labels-in step's, not theirs
        assert gen(lib, d, flags=bad) == E_DESC and wts(lib, d, flags=bad) == E_DESC
        assert gen(lib, d, flags=bad, ws=0) == E_DESC and wts(lib, d, flags=bad, ws=0) == E_DESC  # before the workspace
    for good in range(8):
        assert gen(lib, d, flags=good, ws=0) == E_WORKSPACE and wts(lib, d, flags=good, ws=0) == E_WORKSPACE


def test_workspace(pkg, lib):
    d = desc(pkg, B=2, dims=(1, 70, 132), offsets=[(0, 0, -1)] * 5)
    need_w = lib.pea_targets_workspace_bytes(ctypes.byref(d))
    need_g = 2 * 5 * 4  # pea_gen_targets keeps one count per (image, channel)
    assert need_w == need_g * 9
    assert gen(lib, d, ws=0) == E_WORKSPACE and wts(lib, d, ws=0) == E_WORKSPACE
    assert gen(lib, d, nbytes=ctypes.c_size_t(0)) == E_WORKSPACE and gen(lib, d, nbytes=ctypes.c_size_t(need_g - 1)) == E_WORKSPACE
    assert wts(lib, d, nbytes=ctypes.c_size_t(0)) == E_WORKSPACE and wts(lib, d, nbytes=ctypes.c_size_t(need_w - 1)) == E_WORKSPACE
    assert wts(lib, d, nbytes=ctypes.c_size_t(need_g)) == E_WORKSPACE


def test_grid_limits_are_refused_before_any_device_call(pkg, lib):
    # pea_gen_targets puts (image, channel) on a grid axis of 65535
    d = desc(pkg, B=2048, dims=(1, 1, 1), offsets=[(0, 0, 0)] * 32)
    assert d.B * d.K == 65536 and gen(lib, d) == E_UNSUPPORTED and gen(lib, d, mask=0, weight=0) == E_UNSUPPORTED
    d = desc(pkg, B=65536, dims=(1, 1, 1), offsets=[(0, 0, 0)])
    assert gen(lib, d) == E_UNSUPPORTED
    assert gen(lib, d, ws=0) == E_WORKSPACE and gen(lib, d, flags=8) == E_DESC and gen(lib, d, target=0) == E_NULL  # the last check of all
    # pea_label_weights puts (image, plane) on one
    for B, Z in ((1, 65536), (2, 32768), (65536, 1)):
        d = desc(pkg, B=B, dims=(Z, 1, 1), offsets=[(0, 0, 0)])
        assert wts(lib, d) == E_UNSUPPORTED
        assert wts(lib, d, ws=0) == E_WORKSPACE and wts(lib, d, flags=16) == E_DESC and wts(lib, d, labels=0) == E_NULL


def test_pixel_count_edge_of_the_descriptor(pkg, lib):
    """The label kernels index a plane with 32-bit integers (csrc/pea_targets.h: the pixel of a lane, the neighbour's flat index, the
    weight kernel's p = block * 256 + lane), which is safe only while S + 255 fits an int32: the descriptor check in front of them
    (csrc/pea_abi.hip validate: S <= 2^31 - 1 - 256) must sit exactly there.  S = 2^31 - 257 is the largest image served -- with a NULL
    label pointer the call gets as far as PEA_E_NULL, and the workspace query answers --; S = 2^31 - 256 .. 2^31 - 1 are refused with
    PEA_E_UNSUPPORTED whatever the pointers, and the query answers 0.  Nothing is launched."""
    top = 2 ** 31 - 257
    for S in (top - 1, top):
        for dims in ((1, 1, S), (1, S, 1)):
            d = desc(pkg, B=1, dims=dims, offsets=[(0, 0, 0)])
            wgs = ((dims[2] + 63) // 64) * ((dims[1] + 31) // 32)
            assert lib.pea_targets_workspace_bytes(ctypes.byref(d)) == 4 * wgs
            assert gen(lib, d, labels=0) == E_NULL and wts(lib, d, labels=0) == E_NULL
    d = desc(pkg, B=1, dims=(2, (top - 1) // 2, 1), offsets=[(0, 0, 0)])  # the same count as a volume
    assert gen(lib, d, labels=0) == E_NULL
    for S in (top + 1, top + 2, 2 ** 31 - 2, 2 ** 31 - 1):
        for dims in ((1, 1, S), (1, S, 1)):
            d = desc(pkg, B=1, dims=dims, offsets=[(0, 0, 0)])
            assert lib.pea_targets_workspace_bytes(ctypes.byref(d)) == 0
            assert gen(lib, d) == E_UNSUPPORTED and gen(lib, d, labels=0) == E_UNSUPPORTED
            assert wts(lib, d) == E_UNSUPPORTED and wts(lib, d, labels=0) == E_UNSUPPORTED
    d = desc(pkg, B=1, dims=(2, 2 ** 30 - 128, 1), offsets=[(0, 0, 0)])  # 2^31 - 256 voxels in two planes
    assert gen(lib, d, labels=0) == E_UNSUPPORTED and lib.pea_targets_workspace_bytes(ctypes.byref(d)) == 0
