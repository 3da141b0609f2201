"""GPU (-m gpu): up to four self losses per launch straight from label images (include/pea_multi_labels.h, op.MultiLabelsAffinityMSE,
embedding_loss_from_labels_multi, embedding_loss_norm1_from_labels_multi, the labels-in sections' label_downs=None / batched=True).

  1. the C ABI on a table of four ragged 2D entries (and its first one / two entries) against the C oracle fed by a NumPy chain:
     labels sampled with the step, np_gen_targets, np_weight_binary_ratio;
  2. the class-balance table computed by the call against a table from pea_label_weights: bit-equal results;
  3. four CROP_ZERO norm1 entries in 3D sampling one segmentation, the cropped border slices exactly 0;
  4. bit-reproducibility, the state blocks left ready for a following single call, a scratch full of 0xFF bytes;
  5. the sections with label_downs=None / batched=True against the reference's own run and against the unbatched path;
  6. the public functions against the single calls, and the fallbacks (a bf16 entry, a foreign criterion);
  7. pea.graphed over a batched labels-in section step.
Tolerances are those of tests/test_gpu_parity.py and tests/test_gpu_multi.py.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from conftest import load_golden

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-5, 1e-4
TGT_PADDING, TGT_BOTH_FOREGROUND, TGT_MASK_INSIDE = 1, 2, 4
FLAGS_2D, FLAGS_3D = TGT_PADDING | TGT_MASK_INSIDE, TGT_BOTH_FOREGROUND


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(ge.PKG_NAME + ".affinity_op")


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


FUSED = "pea_affinity_fwd_bwd_labels_multi"
SINGLE = ("pea_label_weights", "pea_affinity_fwd_bwd_labels", "pea_affinity_fwd_bwd_labels_ex", "pea_gen_targets")


class Spy(object):
    """return codes of the batched labels-in call, and the descriptors' image sizes of the single labels-in calls, made while it is installed"""

    def __init__(self, pkg, monkeypatch):
        L = pkg._lib.lib()
        self.fused, self.single = [], []
        real = getattr(L, FUSED)
        monkeypatch.setattr(L, FUSED, lambda *a, _real=real: (self.fused.append(_real(*a)), self.fused[-1])[1])
        for name in SINGLE:
            real = getattr(L, name)

            def wrapped(*a, _real=real, _name=name):
                d = a[0]._obj  # ctypes.byref(desc)
                self.single.append((_name, tuple(d.dims)))
                return _real(*a)
            monkeypatch.setattr(L, name, wrapped)


@pytest.fixture
def spy(pkg, monkeypatch):
    return Spy(pkg, monkeypatch)


def _degenerate_pixels(e):
    """zero-norm pixels and one pixel of norm 1e-14 (below eps = 1e-12: the clamp branch of F.normalize) in every batch item"""
    H, W = e.shape[-2:]
    for b in range(e.shape[0]):
        e[b, :, 0, 0] = 0.0
        e[b, :, H // 2, W // 2] = 0.0
        e[b, :, H - 1, W - 1] = 0.0
        e[b, :, H // 2, 0] = 0.0
        e[b, 0, H // 2, 0] = 1e-14
    return e


def _plant(lab):
    """[B,H,W] blocky labels with the planted features: a large background area, a region that differs from its neighbour across
    the WRAPPED border only (top rows 5, bottom rows 6, background in between on the left: compared modulo the image they would
    disagree, inside the image they never meet), and -- last batch item, where there is more than one -- a single label"""
    B, H, W = lab.shape
    lab = lab.copy()
    lab[:, H // 4:H // 2, : W // 2] = 0
    lab[:, : max(1, H // 8), :] = 5
    lab[:, H - max(1, H // 8):, :] = 6
    if B > 1:
        lab[B - 1] = 7
    return lab


def _sample(lab, dims, step):
    """labels[b][z * sz][y * sy][x * sx] for a [B, Z, Y, X] image"""
    return np.ascontiguousarray(lab[:, ::step[0], ::step[1], ::step[2]][:, :dims[0], :dims[1], :dims[2]])


# ----------------------------------------------------------------------------------------------------------------------------
# the table of (1): four ragged entries; inputs and oracle results are computed once and shared
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(pkg, orc, synth):
    mo = pkg.multi_offset
    shared = _plant(synth.synth_labels(3, (1, 74, 140), 901, cell=13)[:, 0])  # [3, 74, 140]: entries 0 and 1 sample it
    assert (shared[2] == 7).all() and (shared[0] == 0).mean() > 0.1
    own2 = _plant(synth.synth_labels(2, (1, 17, 40), 902, cell=6)[:, 0])
    own3 = _plant(synth.synth_labels(2, (1, 5, 6), 903, cell=2)[:, 0])
    cfg = [  # (B, D, H, W, offsets, label image, step, affs wanted, dloss, lambda)
        (3, 16, 37, 70, mo([1, 3, 5, 9], 4), shared, (1, 2, 2), True, 0.625, None),
        (1, 16, 19, 33, mo([1, 3, 5], 4), shared, (1, 4, 4), False, None, None),            # rows 73.., columns 129.. stay unread
        (2, 32, 17, 40, mo([1, 3], 8), own2, (1, 1, 1), True, 1.75, [2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0]),
        (2, 16, 5, 6, [[-4, 0], [0, -5]], own3, (1, 1, 1), True, None, None),               # smaller than a wavefront, offsets of size - 1
    ]
    out = []
    for j, (B, D, H, W, offsets, lab, step, want_affs, dloss, lam) in enumerate(cfg):
        e = _degenerate_pixels(synth.synth_embedding((B, D, H, W), 910 + j))
        K = len(offsets)
        assert K <= 12 and (j != 2 or any(o[0] < 0 < o[1] for o in offsets))  # entry 2: mixed-sign offsets
        mat = _sample(lab[:B, None], (1, H, W), step)  # [B, 1, H, W]: the label image this scale sees
        t, m = orc.np_gen_targets(mat, offsets, padding=True)
        t, m = t[:, :, 0], m[:, :, 0]
        w = orc.np_weight_binary_ratio(t)
        d = orc.desc_2d(e, offsets, lam)
        o_affs, o_loss = orc.c_fwd(d, e, None, t, w, m)
        o_grad, _ = orc.c_bwd(d, e, None, t, w, m, dloss=1.0 if dloss is None else dloss)
        out.append(dict(e=e, lab=lab, B=B, step=step, mat=mat[:, 0], offsets=offsets, lam=lam, want_affs=want_affs, dloss=dloss, K=K,
                        w=w, t=t, m=m, o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    # the planted features did what they are for
    assert (out[0]["w"][2] == 1.0).all() and (out[0]["t"][2] == 1.0).all()           # the single-label item: weights 1 / 1
    assert len(np.unique(out[0]["w"][0])) > 2                                        # other items: real ratios
    wrapped = np.roll(out[0]["mat"], 1, axis=1) == out[0]["mat"]                     # what a modular comparison would see for (-1, 0)
    assert not wrapped[0, 0].any() and (out[0]["t"][0, 0, 0] == 1.0).all()           # row 0: differs across the wrap, target = padding
    return out


def _spec2d(pkg, op, ent):
    L = pkg._lib
    return op.AffinitySpec(2, ent["offsets"], ent["lam"], L.BORDER_CIRCULAR, L.NORM_BX, 1e-12)


def _run_table(pkg, op, dev, ents, n, flags, fill=float("nan"), wtabs=None, scratch_byte=None, labels_cache=None):
    """pea_affinity_fwd_bwd_labels_multi through ctypes on the first n entries -> per entry (affs, loss_vec, de), the device-side
    entries and the workspace.  One device tensor per distinct label image: entries that share one pass the same pointer."""
    L = pkg._lib.lib()
    labels_cache = {} if labels_cache is None else labels_cache
    tab = (pkg._lib.PeaMultiLabels * n)()
    dv, outs = [], []
    for j, ent in enumerate(ents[:n]):
        E = cu(ent["e"], dev)
        lab = labels_cache.setdefault(id(ent["lab"]), cu(ent["lab"].astype(np.int32), dev))
        d = op.make_desc(ent["spec"] if "spec" in ent else _spec2d(pkg, op, ent), E)
        kshape = op._affs_shape(E, ent["K"])
        affs = torch.full(kshape, fill, dtype=torch.float32, device=dev) if ent["want_affs"] else None
        lv = torch.full((1 + ent["K"],), fill, dtype=torch.float32, device=dev)
        de = torch.full_like(E, fill)
        dl = None if ent["dloss"] is None else torch.tensor([ent["dloss"]], dtype=torch.float32, device=dev)
        a = tab[j]
        a.desc, a.e, a.labels = ctypes.pointer(d), E.data_ptr(), lab.data_ptr()
        a.label_dims[:] = [1] * (4 - lab.dim()) + list(lab.shape[1:])
        a.label_step[:] = ent["step"]
        a.wtab = None if wtabs is None else wtabs[j].data_ptr()
        a.affs = None if affs is None else affs.data_ptr()
        a.loss_out, a.de = lv.data_ptr(), de.data_ptr()
        a.dloss = None if dl is None else dl.data_ptr()
        dv.append(dict(E=E, lab=lab, d=d, kshape=kshape, dl=dl))
        outs.append((affs, lv, de))
    assert L.pea_multi_labels_supported(tab, n, flags) == 1
    sb = L.pea_multi_labels_scratch_bytes(tab, n)
    assert sb == 4 * sum(ent["B"] * ent["K"] for ent in ents[:n])
    scratch = torch.full((sb,), 0 if scratch_byte is None else scratch_byte, dtype=torch.uint8, device=dev)
    work, wsb = op.workspace(dev, dv[0]["d"], n)
    assert L.pea_affinity_fwd_bwd_labels_multi(tab, n, flags, op._ptr(work), wsb, op._ptr(scratch), sb, op._stream()) == 0
    torch.cuda.synchronize()
    return outs, dv, work


def _check_entry(j, ent, affs, lv, de):
    if affs is not None:
        assert np.abs(affs.cpu().numpy() - ent["o_affs"]).max() < AFFS_ATOL, j
    lv = lv.cpu().numpy().astype(np.float64)
    print("entry %d: loss %.9g oracle %.9g" % (j, lv[0], ent["o_loss"][0]))
    assert abs(lv[0] - ent["o_loss"][0]) <= LOSS_RTOL * abs(ent["o_loss"][0]), j
    assert np.all(np.abs(lv[1:] - ent["o_loss"][1:]) <= LOSS_RTOL * np.abs(ent["o_loss"][1:]) + 1e-30), j
    de = de.cpu().numpy()
    assert np.isfinite(de).all(), j
    print("entry %d: grad relmax %.3g" % (j, relmax(de, ent["o_grad"])))
    assert relmax(de, ent["o_grad"]) < GRAD_RTOL, j
    # the pixels on the clamp branch carry G / eps, 1e12 times a regular gradient: without them the same bound holds against the
    # largest REGULAR gradient
    reg = np.sqrt((ent["e"].astype(np.float64) ** 2).sum(axis=1, keepdims=True)) >= 1e-12
    reg = np.broadcast_to(reg, de.shape)
    assert relmax(np.where(reg, de, 0.0), np.where(reg, ent["o_grad"], 0.0)) < GRAD_RTOL, j


@pytest.mark.parametrize("n", [4, 2, 1])
def test_c_abi_table_matches_oracle(pkg, op, dev, table, n):
    outs, _, _ = _run_table(pkg, op, dev, table, n, FLAGS_2D)
    for j, (affs, lv, de) in enumerate(outs):
        _check_entry(j, table[j], affs, lv, de)


def _label_weight_tables(pkg, op, dev, ents, flags):
    """pea_label_weights on the MATERIALISED label image of every entry"""
    L = pkg._lib.lib()
    tabs = []
    for ent in ents:
        E = cu(ent["e"], dev)
        d = op.make_desc(ent["spec"] if "spec" in ent else _spec2d(pkg, op, ent), E)
        lab = cu(ent["mat"].astype(np.int32), dev)
        cb = L.pea_targets_workspace_bytes(ctypes.byref(d))
        counts = torch.empty(max(cb, 4) // 4, dtype=torch.int32, device=dev)
        wtab = torch.empty(ent["B"] * ent["K"] * 2, dtype=torch.float32, device=dev)
        assert L.pea_label_weights(ctypes.byref(d), op._ptr(lab), flags, op._ptr(wtab), op._ptr(counts), cb, op._stream()) == 0
        tabs.append(wtab)
    torch.cuda.synchronize()
    return tabs


def test_table_computed_by_the_call_equals_a_precomputed_one(pkg, op, dev, table):
    """(2) wtab = NULL against wtab from pea_label_weights on the materialised images: the same bits everywhere"""
    computed, _, _ = _run_table(pkg, op, dev, table, 4, FLAGS_2D)
    tabs = _label_weight_tables(pkg, op, dev, table, FLAGS_2D)
    for ent, wtab in zip(table, tabs):  # the tables themselves are the oracle's weights (weight_binary_ratio as two scalars)
        wt = wtab.cpu().numpy().reshape(ent["B"], ent["K"], 2)
        for pos, col in ((True, 0), (False, 1)):
            sel = (ent["t"] != 0) == pos
            for b in range(ent["B"]):
                for i in range(ent["K"]):
                    assert (ent["w"][b, i][sel[b, i]] == wt[b, i, col]).all(), (b, i)
    given, _, _ = _run_table(pkg, op, dev, table, 4, FLAGS_2D, wtabs=tabs)
    for a, b in zip(computed, given):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)


# ----------------------------------------------------------------------------------------------------------------------------
# (3) 3D
# ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_3d_norm1_table_matches_oracle(pkg, op, dev, orc, synth):
    Lm = pkg._lib
    seg = synth.synth_labels(2, (4, 32, 48), 931, cell=9)
    seg[:, :, 8:20, :20] = 0  # a background region
    assert (seg == 0).mean() > 0.1 and (seg > 0).mean() > 0.3
    ents = []
    for j, dloss in enumerate((0.5, None, 2.0, None)):
        dims, step = (4, 16 >> j, 24 >> j), (1, 2 << j, 2 << j)
        lam = [0.7, 1.0, 1.0]  # affs0_weight on loss0 (norm1)
        e = synth.synth_embedding((2, 16) + dims, 940 + j)
        e[:, :, 1, 1, 1] = 0.0
        e[:, :, 0, 0, 0] = 0.0
        e[:, 0, 0, 0, 0] = 1e-14
        mat = _sample(seg, dims, step)
        t, _ = orc.np_gen_targets(mat, orc.norm_offsets([1, 1, 1]), padding=False, both_foreground=True)
        w = orc.np_weight_binary_ratio(t)
        d = orc.desc_3d(e, [1, 1, 1], lam)
        o_affs, o_loss = orc.c_fwd(d, e, None, t, w, None)
        o_grad, _ = orc.c_bwd(d, e, None, t, w, None, dloss=1.0 if dloss is None else dloss)
        spec = op.AffinitySpec(3, orc.norm_offsets([1, 1, 1]), lam, Lm.BORDER_CROP_ZERO, Lm.NORM_CROPPED, 1e-12)
        ents.append(dict(e=e, lab=seg, B=2, step=step, K=3, want_affs=True, dloss=dloss, spec=spec, o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    outs, _, _ = _run_table(pkg, op, dev, ents, 4, FLAGS_3D, fill=7.0)
    for j, (affs, lv, de) in enumerate(outs):
        _check_entry(j, ents[j], affs, lv, de)
        affs = affs.cpu().numpy()
        # the cropped border slices: exactly 0 in the map (the buffer held 7.0)
        assert not affs[:, 0, :1].any() and not affs[:, 1, :, :1].any() and not affs[:, 2, :, :, :1].any(), j
        assert affs[:, 2, :, :, 1:].any(), j


# ----------------------------------------------------------------------------------------------------------------------------
# (4) bit-reproducibility and state hygiene
# ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_table_is_reproducible_and_leaves_the_states_ready(pkg, op, dev, table):
    first, dv, work = _run_table(pkg, op, dev, table, 4, FLAGS_2D)
    second, _, work2 = _run_table(pkg, op, dev, table, 4, FLAGS_2D, scratch_byte=0xFF)  # the call zeroes its scratch itself
    assert work.data_ptr() == work2.data_ptr()
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    # every state of the table's block serves a single pea_affinity_fwd as it is: the call left them zero
    L = pkg._lib.lib()
    ent, x = table[0], dv[0]
    state = L.pea_workspace_bytes(ctypes.byref(x["d"]))
    T, Wt, M = cu(ent["t"], dev), cu(ent["w"], dev), cu(ent["m"], dev)
    for i in range(4):
        lv = torch.empty(1 + ent["K"], dtype=torch.float32, device=dev)
        g = torch.empty(x["kshape"], dtype=torch.float32, device=dev)
        assert L.pea_affinity_fwd(ctypes.byref(x["d"]), op._ptr(x["E"]), None, op._ptr(T), op._ptr(Wt), op._ptr(M), None, op._ptr(g), op._ptr(lv),
                                  ctypes.c_void_p(work.data_ptr() + i * state), state, op._stream()) == 0
        torch.cuda.synchronize()
        assert abs(float(lv[0]) - ent["o_loss"][0]) <= LOSS_RTOL * abs(ent["o_loss"][0]), i


# ----------------------------------------------------------------------------------------------------------------------------
# (5) the sections
# ----------------------------------------------------------------------------------------------------------------------------
def _cvppp_golden_run(pkg, dev, g, label_downs, batched, **kw):
    offsets = g["offsets"].tolist()
    crit = pkg.WeightedMSE()
    embs = [cu(g["emb%d" % j], dev).requires_grad_(True) for j in range(5)]
    downs = None if not label_downs else [cu(g["lab%d" % j], dev) for j in range(1, 5)]
    loss, pred, _ = pkg.cvppp_loss_section_from_labels(embs[0], embs[1:], cu(g["ema"], dev), cu(g["lab0"], dev), downs, crit, offsets, 2,
                                                       relu_pred=True, batched=batched, **kw)
    loss.backward()
    return loss.item(), pred.cpu().numpy(), [x.grad.cpu().numpy() for x in embs]


def test_cvppp_section_from_one_label_image_matches_reference_golden(pkg, dev, spy):
    g = load_golden("gsection_cvppp")
    for j in range(1, 5):  # the fixture's small label images are the plain strides of the full one
        assert np.array_equal(g["lab%d" % j], g["lab0"][:, ::2 ** j, ::2 ** j])
    loss, pred, grads = _cvppp_golden_run(pkg, dev, g, False, True)
    assert spy.fused == [0]  # the four scales: one call, and no single labels-in call below full resolution
    assert all(dims == (1, 48, 64) for _, dims in spy.single), spy.single
    assert abs(loss - float(g["total"])) <= 1e-5 * abs(float(g["total"]))
    assert np.abs(pred - g["pred"]).max() < AFFS_ATOL
    for j in range(5):
        assert relmax(grads[j], g["grad%d" % j]) < GRAD_RTOL, j
    # explicit label_downs with batched=True, and label_downs=None without it: the same section
    spy.fused.clear()
    for downs, batched, ncalls in ((True, True, 1), (False, False, 0)):
        l2, p2, g2 = _cvppp_golden_run(pkg, dev, g, downs, batched)
        assert len(spy.fused) == ncalls and all(rc == 0 for rc in spy.fused)
        spy.fused.clear()
        assert abs(l2 - loss) <= LOSS_RTOL * abs(loss)
        assert np.abs(p2 - pred).max() < AFFS_ATOL
        for j in range(5):
            assert relmax(g2[j], grads[j]) < GRAD_RTOL, (downs, batched, j)


def test_cvppp_section_batched_takes_weight_tables(pkg, dev, spy):
    g = load_golden("gsection_cvppp")
    offsets = g["offsets"].tolist()
    tables = pkg.cvppp_label_weight_tables(cu(g["lab0"], dev), None, offsets, 2)
    explicit = pkg.cvppp_label_weight_tables(cu(g["lab0"], dev), [cu(g["lab%d" % j], dev) for j in range(1, 5)], offsets, 2)
    assert all(torch.equal(a, b) for a, b in zip(tables, explicit))
    spy.single.clear()
    base = _cvppp_golden_run(pkg, dev, g, False, True)
    with_tables = _cvppp_golden_run(pkg, dev, g, False, True, weight_tables=tables)
    assert spy.fused == [0, 0]
    assert with_tables[0] == base[0] and np.array_equal(with_tables[1], base[1])
    for a, b in zip(with_tables[2], base[2]):
        assert np.array_equal(a, b)


def test_ac3ac4_section_from_one_segmentation_equals_unbatched(pkg, dev, synth, spy):
    crit = pkg.WeightedMSE()
    B, D, Z, Y, X = 2, 16, 4, 64, 80
    seg = synth.synth_labels(B, (Z, Y, X), 951, cell=9)
    seg[:, :, 8:20, :20] = 0
    e0, ema = synth.synth_embedding((B, D, Z, Y, X), 952), cu(synth.synth_embedding((B, D, Z, Y, X), 953), dev)
    # emd1 .. emd4 pair with down4 .. down1 (scripts_ac3ac4/main.py:227-230): emd1 is the coarsest head
    emds = [synth.synth_embedding((B, D, Z, Y >> j, X >> j), 954 + j) for j in (4, 3, 2, 1)]
    seg_t = cu(seg, dev)
    downs = [cu(np.ascontiguousarray(seg[:, :, ::2 ** j, ::2 ** j]), dev) for j in (1, 2, 3, 4)]  # seg of down1 .. down4

    def run(label_downs, batched):
        xs = [cu(e0, dev).requires_grad_(True)] + [cu(x, dev).requires_grad_(True) for x in emds]
        loss, pred = pkg.ac3ac4_loss_section_from_labels(xs[0], xs[1:], ema, seg_t, label_downs, crit, embedding_mode=1, affs0_weight=0.7,
                                                         batched=batched)
        loss.backward()
        return loss.item(), pred.cpu().numpy(), [x.grad.cpu().numpy() for x in xs]

    ref = run(downs, False)
    assert spy.fused == []
    for label_downs, batched in ((None, True), (downs, True), (None, False)):
        spy.fused.clear()
        out = run(label_downs, batched)
        assert spy.fused == ([0] if batched else [])
        assert abs(out[0] - ref[0]) <= LOSS_RTOL * abs(ref[0])
        assert np.abs(out[1] - ref[1]).max() < AFFS_ATOL
        for j in range(5):
            assert relmax(out[2][j], ref[2][j]) < GRAD_RTOL, (batched, j)


# ----------------------------------------------------------------------------------------------------------------------------
# (6) the public functions against the single calls, and the fallbacks
# ----------------------------------------------------------------------------------------------------------------------------
def _leaves(dev, table, dtypes=(torch.float32,) * 4):
    return [cu(ent["e"], dev).to(dt).requires_grad_(True) for ent, dt in zip(table, dtypes)]


def _single_label_calls(pkg, crit, xs, table, dev, weights, need_affs=True):
    out = [pkg.embedding_loss_from_labels(x, cu(ent["mat"].astype(np.int32), dev), crit, ent["offsets"], need_affs=need_affs)
           for x, ent in zip(xs, table)]
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    return out


def _compare_public(out, ref, xs, ys):
    for j, ((l, a, parts), (rl, ra, rparts)) in enumerate(zip(out, ref)):
        assert abs(l.item() - rl.item()) <= LOSS_RTOL * abs(rl.item()), j
        assert np.allclose(list(parts), list(rparts), rtol=LOSS_RTOL, atol=0), j
        assert a.shape == ra.shape and (a.numel() == 0 or float((a - ra).abs().max()) < AFFS_ATOL), j
        gm, gr = xs[j].grad, ys[j].grad
        reg = (ys[j].detach().double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(gr)
        assert relmax(gm.cpu().numpy(), gr.cpu().numpy()) < GRAD_RTOL, j
        assert relmax(torch.where(reg, gm, 0 * gm).cpu().numpy(), torch.where(reg, gr, 0 * gr).cpu().numpy()) < GRAD_RTOL, j


def test_embedding_loss_from_labels_multi_equals_single_calls(pkg, op, dev, table, spy):
    crit = pkg.WeightedMSE()
    weights = [0.3, 1.0, 0.01, 2.0]
    offs = [ent["offsets"] for ent in table]
    ys = _leaves(dev, table)
    ref = _single_label_calls(pkg, crit, ys, table, dev, weights)
    # the list form: one label tensor per embedding, need_affs=True
    xs = _leaves(dev, table)
    out = pkg.embedding_loss_from_labels_multi(xs, [cu(ent["mat"].astype(np.int32), dev) for ent in table], crit, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.fused == [0]
    _compare_public(out, ref, xs, ys)
    # one tensor + steps (entries 0 and 1 sample the shared image; entry 1 has B = 1: its own slice of the batch), weight tables given
    tabs = _label_weight_tables(pkg, op, dev, table[:2], FLAGS_2D)
    for k, (ent, tab) in enumerate(zip(table[:2], tabs)):
        xs = _leaves(dev, [ent])
        shared = cu(ent["lab"][:ent["B"]].astype(np.int32), dev)
        out = pkg.embedding_loss_from_labels_multi(xs, shared, crit, [ent["offsets"]], label_steps=[ent["step"][1:]], weight_tables=[tab])
        (out[0][0] * weights[k]).backward()
        assert out[0][1].numel() == 0  # need_affs=False: no map
        _compare_public(out, [(ref[k][0], out[0][1], ref[k][2])], xs, [ys[k]])
    assert spy.fused == [0, 0, 0]
    # label_steps=None on a size that divides: entry 0's embedding against an image twice its size
    xs = _leaves(dev, table[:1])
    out = pkg.embedding_loss_from_labels_multi(xs, cu(table[0]["lab"].astype(np.int32), dev), crit, offs[:1], need_affs=True)
    (out[0][0] * weights[0]).backward()
    _compare_public(out, ref[:1], xs, ys[:1])


def test_embedding_loss_from_labels_multi_falls_back(pkg, dev, table, spy):
    """a bf16 entry: the table is outside the fused set, nothing batched is launched; a foreign criterion: the single calls"""
    crit = pkg.WeightedMSE()
    weights = [1.0, 0.5, 2.0, 1.0]
    offs = [ent["offsets"] for ent in table]
    labs = [cu(ent["mat"].astype(np.int32), dev) for ent in table]
    dts = (torch.float32, torch.bfloat16, torch.float32, torch.float32)
    xs = _leaves(dev, table, dts)
    out = pkg.embedding_loss_from_labels_multi(xs, labs, crit, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.fused == []
    ys = _leaves(dev, table, dts)
    ref = _single_label_calls(pkg, crit, ys, table, dev, weights)
    for j in range(4):
        assert torch.equal(out[j][0], ref[j][0]) and torch.equal(out[j][1], ref[j][1]) and torch.equal(xs[j].grad, ys[j].grad), j

    def foreign(pred, target, weight):  # a plain torch callable
        return (weight * (pred - target).abs()).mean()

    xs = _leaves(dev, table)
    out = pkg.embedding_loss_from_labels_multi(xs, labs, foreign, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.fused == []
    ys = _leaves(dev, table)
    ref = []
    for y, lab, o in zip(ys, labs, offs):
        t, m, w = pkg.gen_targets(lab, o, padding=True)
        ref.append(pkg.embedding_loss(y, t, w, m, foreign, o))
    sum(l * c for (l, _, _), c in zip(ref, weights)).backward()
    for j in range(4):
        assert torch.equal(out[j][0], ref[j][0]) and torch.equal(out[j][1], ref[j][1]) and torch.equal(xs[j].grad, ys[j].grad), j


def test_embedding_loss_norm1_from_labels_multi_equals_single_calls(pkg, dev, synth, spy):
    crit = pkg.WeightedMSE()
    seg = synth.synth_labels(2, (4, 32, 48), 961, cell=9)
    seg[:, :, 8:20, :20] = 0
    seg_t = cu(seg, dev)
    shapes = [(4, 16 >> j, 24 >> j) for j in range(4)]
    data = [synth.synth_embedding((2, 16) + s, 962 + j) for j, s in enumerate(shapes)]
    xs = [cu(e, dev).requires_grad_(True) for e in data]
    ys = [cu(e, dev).requires_grad_(True) for e in data]
    out = pkg.embedding_loss_norm1_from_labels_multi(xs, seg_t, crit, affs0_weight=0.7)
    sum(l for l, _ in out).backward()
    assert spy.fused == [0]
    ref = [pkg.embedding_loss_norm1_from_labels(y, cu(_sample(seg, s, (1, 2 << j, 2 << j)), dev), crit, affs0_weight=0.7)
           for j, (y, s) in enumerate(zip(ys, shapes))]
    sum(l for l, _ in ref).backward()
    for j in range(4):
        assert abs(out[j][0].item() - ref[j][0].item()) <= LOSS_RTOL * abs(ref[j][0].item()), j
        assert float((out[j][1] - ref[j][1]).abs().max()) < AFFS_ATOL, j
        assert relmax(xs[j].grad.cpu().numpy(), ys[j].grad.cpu().numpy()) < GRAD_RTOL, j


# ----------------------------------------------------------------------------------------------------------------------------
# (7) graph capture
# ----------------------------------------------------------------------------------------------------------------------------
def test_graphed_batched_labels_section_equals_eager(pkg, dev, synth, spy):
    """pea.graphed over a cvppp_loss_section_from_labels(label_downs=None, batched=True) step (forward + backward): the replay is
    bit-equal to the eager step, and after the static labels are refilled a second replay follows the new labels"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half, B, D, H, W = 2, 2, 16, 96, 96
    crit = pkg.WeightedMSE()

    def tensors(seed):
        embs = [synth.synth_embedding((B, D, H >> j, W >> j), seed + j) for j in range(5)]
        ema = synth.synth_embedding((B, D, H, W), seed + 5)
        lab = synth.synth_labels(B, (1, H, W), seed + 6, cell=12)[:, 0]
        return [cu(x, dev) for x in embs] + [cu(ema, dev), cu(lab, dev)]

    def step(*bufs):
        leaves = list(bufs[:5])
        for x in leaves:
            x.grad = None
        loss, pred, _ = pkg.cvppp_loss_section_from_labels(leaves[0], leaves[1:], bufs[5], bufs[6], None, crit, offsets, nb_half, batched=True)
        pkg.backward(loss)
        return loss, pred, [x.grad for x in leaves]

    static = tensors(971)
    for x in static[:5]:
        x.requires_grad_(True)
    g = pkg.graphed(step, *static)
    seen = []
    for seed in (971, 981):
        fresh = tensors(seed)
        if seed == 981:
            fresh[:6] = [x.detach().clone() for x in static[:6]]  # the same embeddings: only the labels are refilled
        with torch.no_grad():
            for dst, src in zip(static, fresh):
                dst.copy_(src)
        loss, pred, grads = g.replay()
        torch.cuda.synchronize()
        seen.append(float(loss.detach()))
        for x in fresh[:5]:
            x.requires_grad_(True)
        spy.fused.clear()
        e_loss, e_pred, e_grads = step(*fresh)
        assert spy.fused == [0]
        assert torch.equal(loss, e_loss) and torch.equal(pred, e_pred), seed
        for a, b in zip(grads, e_grads):
            assert torch.equal(a, b), seed
    assert seen[0] != seen[1]  # the second replay followed the new labels
