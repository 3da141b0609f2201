"""GPU (-m gpu): up to four self losses per launch (include/pea_multi.h, op.MultiAffinityMSE, embedding_loss_multi,
embedding_loss_norm1_multi, the sections' batched=True).

  1. the C ABI on a table of four ragged 2D entries (and its first one / two entries) against the C oracle, call by call;
  2. four CROP_ZERO norm1 entries in 3D against the oracle, the cropped border slices exactly 0;
  3. the sections with batched=True against the reference's own runs (tests/golden/gsection_*.npz);
  4. embedding_loss_multi against four embedding_loss calls;
  5. bit-reproducibility, and the state blocks left ready for a following single call;
  6. the fallbacks (a bf16 entry, a foreign criterion);
  7. pea.graphed over a batched section step.
Tolerances are those of tests/test_gpu_parity.py.
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


class Spy(object):
    """return codes of the two batched calls made while it is installed: shows that a test ran the fused launches (or did not)"""

    def __init__(self, pkg, monkeypatch):
        L = pkg._lib.lib()
        self.fwd, self.bwd = [], []
        for name, log in (("pea_affinity_fwd_multi", self.fwd), ("pea_affinity_bwd_multi", self.bwd)):
            real = getattr(L, name)
            monkeypatch.setattr(L, name, lambda *a, _real=real, _log=log: (_log.append(_real(*a)), _log[-1])[1])


@pytest.fixture
def spy(pkg, monkeypatch):
    return Spy(pkg, monkeypatch)


# ----------------------------------------------------------------------------------------------------------------------------
# the table of (1): four ragged entries; inputs and oracle results are computed once and shared
# ----------------------------------------------------------------------------------------------------------------------------
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


def _frac_mask(synth, shape, seed):
    """U(0, 1) with exact 0, 0.5, 1 and 1.5 sprinkled in (the reference multiplies by mask.float(): any value counts)"""
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.uint64)
    m = synth.hash_uniform(idx, seed)
    pick = (synth.hash_uniform(idx, seed + 1) * 8).astype(np.int64)
    for v, c in ((0.0, 0), (0.5, 1), (1.0, 2), (1.5, 3)):
        m = np.where(pick == c, v, m)
    return m.astype(np.float32).reshape(shape)


@pytest.fixture(scope="module")
def table(pkg, orc, synth):
    """per entry: numpy inputs, the oracle's affs / loss vector / gradient for its dloss"""
    mo = pkg.multi_offset
    cfg = [  # (B, D, H, W, offsets, mask kind, affs wanted, dloss, lambda)
        (3, 16, 37, 70, mo([1, 3, 5, 9], 4), "f32", True, 0.625, None),
        (1, 16, 19, 33, mo([1, 3, 5], 4), "u8", False, None, None),
        (2, 32, 17, 40, mo([1, 3], 8), None, True, 1.75, [2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0]),
        (2, 16, 5, 6, mo([1], 4), "u8", True, None, None),
    ]
    out = []
    for j, (B, D, H, W, offsets, mkind, want_affs, dloss, lam) in enumerate(cfg):
        e, t, w, m8 = synth.synth_inputs_2d(B, D, H, W, offsets, 410 + j)
        e = _degenerate_pixels(e)
        K = len(offsets)
        assert K <= 12 and (j != 2 or any(o[0] < 0 < o[1] for o in offsets))  # entry 2: mixed-sign offsets
        d = orc.desc_2d(e, offsets, lam)
        if mkind == "f32":
            # a fractional mask in the oracle (whose mask is u8): r = a m - t m = m (a - t), so w r^2 = (w m^2) (a - t)^2 and
            # g = 2 (w m^2) (a - t) / N -- the same loss and gradient with the weight w m^2 and no mask
            m = _frac_mask(synth, t.shape, 77)
            ow, om = (w.astype(np.float64) * m.astype(np.float64) ** 2).astype(np.float32), None
        else:
            m = m8 if mkind == "u8" else None
            ow, om = w, m
        o_affs, o_loss = orc.c_fwd(d, e, None, t, ow, om)
        o_grad, _ = orc.c_bwd(d, e, None, t, ow, om, dloss=1.0 if dloss is None else dloss)
        out.append(dict(e=e, t=t, w=w, m=m, offsets=offsets, lam=lam, want_affs=want_affs, dloss=dloss, K=K, packed=j == 0,
                        o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    return out


def _spec2d(pkg, op, ent):
    L = pkg._lib
    return op.AffinitySpec(2, ent["offsets"], ent["lam"], L.BORDER_CIRCULAR, L.NORM_BX, 1e-12)


def _device_entry(pkg, op, dev, ent, j):
    """the entry's tensors on the device; entry 0 passes target / weight (/ mask) as channel slices of ONE packed tensor"""
    E = cu(ent["e"], dev)
    K = ent["K"]
    if ent.get("packed"):
        packed = torch.cat([cu(ent["t"], dev), cu(ent["w"], dev), cu(ent["m"], dev)], dim=1)
        T, Wt, M = packed[:, 0:K], packed[:, K:2 * K], packed[:, 2 * K:3 * K]
        assert not T.is_contiguous()
    else:
        T, Wt, M = cu(ent["t"], dev), cu(ent["w"], dev), cu(ent["m"], dev)
    kshape = op._affs_shape(E, K)
    T, ts = op._batch_strided(T, "target", torch.float32, kshape)
    Wt, ws = op._batch_strided(Wt, "weightmap", torch.float32, kshape)
    M, ms, mflag = op.mask_arg(M, kshape)
    if ent.get("packed"):
        assert ts == 3 * K * E.shape[2] * E.shape[3] and mflag == pkg._lib.FLAG_MASK_F32  # a batch stride that is not dense
    d = op.make_desc(_spec2d(pkg, op, ent) if "spec" not in ent else ent["spec"], E, ts, ws, ms, mflag)
    return dict(E=E, T=T, W=Wt, M=M, d=d, kshape=kshape,
                dl=None if ent["dloss"] is None else torch.tensor([ent["dloss"]], dtype=torch.float32, device=dev))


def _run_table(pkg, op, dev, ents, n, fill=float("nan")):
    """pea_affinity_fwd_multi + pea_affinity_bwd_multi through ctypes on the first n entries -> per entry (affs, g, loss_vec, de),
    and the workspace"""
    L = pkg._lib.lib()
    dv = [_device_entry(pkg, op, dev, ent, j) for j, ent in enumerate(ents[:n])]
    arr = (ctypes.POINTER(pkg._lib.PeaDesc) * n)(*[ctypes.pointer(x["d"]) for x in dv])
    assert L.pea_multi_supported(arr, n) == 1
    work, wsb = op.workspace(dev, dv[0]["d"], n)
    ft, bt = (pkg._lib.PeaMultiFwd * n)(), (pkg._lib.PeaMultiBwd * n)()
    outs = []
    for j, x in enumerate(dv):
        affs = torch.full(x["kshape"], fill, dtype=torch.float32, device=dev) if ents[j]["want_affs"] else None
        g = torch.full(x["kshape"], fill, dtype=torch.float32, device=dev)
        lv = torch.full((1 + ents[j]["K"],), fill, dtype=torch.float32, device=dev)
        de = torch.full_like(x["E"], fill)
        a, b = ft[j], bt[j]
        a.desc, a.e, a.target, a.weight = ctypes.pointer(x["d"]), x["E"].data_ptr(), x["T"].data_ptr(), x["W"].data_ptr()
        a.mask = None if x["M"] is None else x["M"].data_ptr()
        a.affs = None if affs is None else affs.data_ptr()
        a.g_out, a.loss_out = g.data_ptr(), lv.data_ptr()
        b.desc, b.e, b.g, b.de = ctypes.pointer(x["d"]), x["E"].data_ptr(), g.data_ptr(), de.data_ptr()
        b.dloss = None if x["dl"] is None else x["dl"].data_ptr()
        outs.append((affs, g, lv, de))
    assert L.pea_affinity_fwd_multi(ft, n, op._ptr(work), wsb, op._stream()) == 0
    assert L.pea_affinity_bwd_multi(bt, n, op._stream()) == 0
    torch.cuda.synchronize()
    return outs, dv, work


@pytest.mark.parametrize("n", [4, 2, 1])
def test_c_abi_table_matches_oracle(pkg, op, dev, table, n):
    outs, _, _ = _run_table(pkg, op, dev, table, n)
    for j, (affs, g, lv, de) in enumerate(outs):
        ent = table[j]
        if affs is not None:
            assert np.abs(affs.cpu().numpy() - ent["o_affs"]).max() < AFFS_ATOL, j
        lv = lv.cpu().numpy().astype(np.float64)
        print("entry %d: loss %.9g oracle %.9g" % (j, lv[0], ent["o_loss"][0]))
        assert abs(lv[0] - ent["o_loss"][0]) <= LOSS_RTOL * abs(ent["o_loss"][0]), j
        assert np.all(np.abs(lv[1:] - ent["o_loss"][1:]) <= LOSS_RTOL * np.abs(ent["o_loss"][1:]) + 1e-30), j
        de = de.cpu().numpy()
        assert np.isfinite(de).all() and np.isfinite(g.cpu().numpy()).all(), j
        print("entry %d: grad relmax %.3g" % (j, relmax(de, ent["o_grad"])))
        assert relmax(de, ent["o_grad"]) < GRAD_RTOL, j
        # the pixels on the clamp branch carry G / eps, 1e12 times a regular gradient: without them the same bound holds against the
        # largest REGULAR gradient (both are f32 evaluations of a float64 reference, relative error ~1e-6)
        reg = np.sqrt((ent["e"].astype(np.float64) ** 2).sum(axis=1, keepdims=True)) >= 1e-12
        reg = np.broadcast_to(reg, de.shape)
        assert relmax(np.where(reg, de, 0.0), np.where(reg, ent["o_grad"], 0.0)) < GRAD_RTOL, j


def test_c_abi_table_is_reproducible_and_leaves_the_states_ready(pkg, op, dev, table):
    """(5) two runs agree bit for bit; then one of the table's state blocks serves a single pea_affinity_fwd as it is"""
    first, dv, work = _run_table(pkg, op, dev, table, 4)
    second, _, work2 = _run_table(pkg, op, dev, table, 4)
    assert work.data_ptr() == work2.data_ptr()
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)
    L = pkg._lib.lib()
    x = dv[0]
    state = L.pea_workspace_bytes(ctypes.byref(x["d"]))

    def single(ws_ptr):
        lv = torch.empty(1 + table[0]["K"], dtype=torch.float32, device=dev)
        g = torch.empty(x["kshape"], dtype=torch.float32, device=dev)
        assert L.pea_affinity_fwd(ctypes.byref(x["d"]), op._ptr(x["E"]), None, op._ptr(x["T"]), op._ptr(x["W"]), op._ptr(x["M"]), None,
                                  op._ptr(g), op._ptr(lv), ctypes.c_void_p(ws_ptr), state, op._stream()) == 0
        torch.cuda.synchronize()
        return lv

    own, _ = op.workspace(dev, x["d"])
    usual = single(own.data_ptr())
    for i in range(4):  # every state of the table's block, no re-initialisation
        assert torch.equal(single(work.data_ptr() + i * state), usual), i
    assert torch.isfinite(usual).all()
    assert abs(float(usual[0]) - table[0]["o_loss"][0]) <= LOSS_RTOL * abs(table[0]["o_loss"][0])


# ----------------------------------------------------------------------------------------------------------------------------
# (2) 3D
# ----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_3d_norm1_table_matches_oracle(pkg, op, dev, orc, synth):
    Lm = pkg._lib
    cfg = [((4, 16, 24), 1, 0.5), ((4, 8, 12), 2, None), ((4, 4, 6), 1, 2.0), ((3, 2, 3), 1, None)]  # dims, shift, dloss
    ents = []
    for j, (dims, shift, dloss) in enumerate(cfg):
        shifts = [shift] * 3
        lam = [0.7, 1.0, 1.0]  # affs0_weight on loss0 (norm1)
        e, t, w = synth.synth_inputs_3d(2, 16, dims[0], dims[1], dims[2], orc.norm_offsets(shifts), 520 + j)
        e[:, :, 1, 1, 1] = 0.0
        e[:, :, 0, 0, 0] = 0.0
        e[:, 0, 0, 0, 0] = 1e-14
        d = orc.desc_3d(e, shifts, lam)
        o_affs, o_loss = orc.c_fwd(d, e, None, t, w, None)
        o_grad, _ = orc.c_bwd(d, e, None, t, w, None, dloss=1.0 if dloss is None else dloss)
        spec = op.AffinitySpec(3, orc.norm_offsets(shifts), lam, Lm.BORDER_CROP_ZERO, Lm.NORM_CROPPED, 1e-12)
        ents.append(dict(e=e, t=t, w=w, m=None, K=3, want_affs=True, dloss=dloss, spec=spec, shift=shift,
                         o_affs=o_affs, o_loss=o_loss, o_grad=o_grad))
    outs, _, _ = _run_table(pkg, op, dev, ents, 4, fill=7.0)
    for j, (affs, g, lv, de) in enumerate(outs):
        ent, s = ents[j], ents[j]["shift"]
        affs, g = affs.cpu().numpy(), g.cpu().numpy()
        assert np.abs(affs - ent["o_affs"]).max() < AFFS_ATOL, j
        lv = lv.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(lv - ent["o_loss"]) <= LOSS_RTOL * np.abs(ent["o_loss"])), j
        assert relmax(de.cpu().numpy(), ent["o_grad"]) < GRAD_RTOL, j
        # the cropped border slices: exactly 0 in the map and in g (the buffers held 7.0)
        for x in (affs, g):
            assert not x[:, 0, :s].any() and not x[:, 1, :, :s].any() and not x[:, 2, :, :, :s].any(), j
        assert g[:, 0, s:].any() and affs[:, 2, :, :, s:].any(), j


# ----------------------------------------------------------------------------------------------------------------------------
# (3) the sections with batched=True against the reference's own runs
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["one_node", "composed"])
def test_cvppp_loss_section_batched_matches_reference_golden(pkg, dev, spy, path):
    g = load_golden("gsection_cvppp")
    offsets = g["offsets"].tolist()
    nb_half = 2
    crit = pkg.WeightedMSE()
    embs = [cu(g["emb%d" % j], dev).requires_grad_(True) for j in range(5)]
    ema = cu(g["ema"], dev)
    downs = [torch.cat([cu(g["t%d" % j], dev), cu(g["w%d" % j], dev), cu(g["m%d" % j], dev).float()], dim=1) for j in range(1, 5)]
    fn = pkg.cvppp_loss_section if path == "one_node" else pkg.cvppp_loss_section_composed
    kw = {"relu_pred": True} if path == "one_node" else {}
    loss, pred, parts = fn(embs[0], embs[1:], ema, cu(g["t0"], dev), cu(g["w0"], dev), cu(g["m0"], dev), downs, crit, offsets, nb_half,
                           batched=True, **kw)
    loss.backward()
    if path == "composed":
        pkg.finish_pred_2d_(pred)
    assert spy.fwd == [0] and spy.bwd == [0]  # the four scales ran as one launch each way
    assert abs(loss.item() - float(g["total"])) <= 1e-5 * abs(float(g["total"]))
    assert np.abs(pred.cpu().numpy() - g["pred"]).max() < AFFS_ATOL
    for j in range(5):
        assert relmax(embs[j].grad.cpu().numpy(), g["grad%d" % j]) < GRAD_RTOL, j


@pytest.mark.parametrize("name,path", [("gsection_ac3ac4_norm5", "one_node"), ("gsection_ac3ac4_norm5", "composed"),
                                       ("gsection_ac3ac4_norm1", "one_node"), ("gsection_ac3ac4_norm1", "composed")])
def test_ac3ac4_loss_section_batched_matches_reference_golden(pkg, dev, spy, name, path):
    g = load_golden(name)
    crit = pkg.WeightedMSE()
    emb = cu(g["emb"], dev).requires_grad_(True)
    emds = [cu(g["emd%d" % j], dev).requires_grad_(True) for j in range(1, 5)]
    downs = [cu(g["down%d" % j], dev) for j in range(1, 5)]
    fn = pkg.ac3ac4_loss_section if path == "one_node" else pkg.ac3ac4_loss_section_composed
    loss, pred = fn(emb, emds, cu(g["ema"], dev), cu(g["target"], dev), cu(g["weight"], dev), downs, crit,
                    embedding_mode=int(g["mode"]), affs0_weight=1, batched=True)
    loss.backward()
    pred = pkg.finish_pred_3d_(pred.clone())
    assert spy.fwd == [0] and spy.bwd == [0]
    assert abs(loss.item() - float(g["total"])) <= 1e-5 * abs(float(g["total"]))
    assert np.abs(pred.cpu().numpy() - g["pred"]).max() < AFFS_ATOL
    assert relmax(emb.grad.cpu().numpy(), g["grad_emb"]) < GRAD_RTOL
    for j in range(1, 5):
        assert relmax(emds[j - 1].grad.cpu().numpy(), g["grad_emd%d" % j]) < GRAD_RTOL, j


def test_validation_section_batched_equals_unbatched(pkg, dev, spy):
    g = load_golden("gsection_cvppp")
    offsets = g["offsets"].tolist()
    crit = pkg.WeightedMSE()
    embs = [cu(g["emb%d" % j], dev) for j in range(5)]
    downs = [torch.cat([cu(g["t%d" % j], dev), cu(g["w%d" % j], dev), cu(g["m%d" % j], dev).float()], dim=1) for j in range(1, 5)]
    args = (embs[0], embs[1:], cu(g["t0"], dev), cu(g["w0"], dev), cu(g["m0"], dev), downs, crit, offsets, 2)
    l0, p0 = pkg.cvppp_validation_section(*args)
    assert spy.fwd == []
    l1, p1 = pkg.cvppp_validation_section(*args, batched=True)
    assert spy.fwd == [0] and spy.bwd == []  # (under no_grad: no backward)
    assert abs(l1.item() - l0.item()) <= 1e-5 * abs(l0.item())
    assert torch.equal(p1, p0) and not l1.requires_grad


# ----------------------------------------------------------------------------------------------------------------------------
# (4), (6) the public functions against the single calls
# ----------------------------------------------------------------------------------------------------------------------------
def _public_inputs(dev, table, dtypes=(torch.float32,) * 4):
    xs = [cu(ent["e"], dev).to(dt).requires_grad_(True) for ent, dt in zip(table, dtypes)]
    # (the public functions take the self loss' lambda = 1: entry 2's lambda list belongs to the C-ABI test)
    return xs, [cu(ent["t"], dev) for ent in table], [cu(ent["w"], dev) for ent in table], [cu(ent["m"], dev) for ent in table]


def _single_calls(pkg, crit, xs, T, W, M, table, weights):
    out = [pkg.embedding_loss(x, t, w, m, crit, ent["offsets"]) for x, t, w, m, ent in zip(xs, T, W, M, table)]
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    return out


def test_embedding_loss_multi_equals_single_calls(pkg, dev, table, spy):
    crit = pkg.WeightedMSE()
    weights = [0.3, 1.0, 0.01, 2.0]
    xs, T, W, M = _public_inputs(dev, table)
    out = pkg.embedding_loss_multi(xs, T, W, M, crit, [ent["offsets"] for ent in table], need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.fwd == [0] and spy.bwd == [0]
    ys, _, _, _ = _public_inputs(dev, table)
    ref = _single_calls(pkg, crit, ys, T, W, M, table, weights)
    for j, ((l, a, parts), (rl, ra, rparts)) in enumerate(zip(out, ref)):
        assert abs(l.item() - rl.item()) <= 1e-6 * abs(rl.item()), j
        assert np.allclose(list(parts), list(rparts), rtol=1e-6, atol=0), j
        print("entry %d: affs max diff %.3g, grad relmax %.3g" % (j, float((a - ra).abs().max()),
                                                                   relmax(xs[j].grad.cpu().numpy(), ys[j].grad.cpu().numpy())))
        assert float((a - ra).abs().max()) <= 1e-6, j
        # 1e-5 of the largest regular gradient (the clamp-branch pixels carry G / eps; they are held to 1e-5 of their own max)
        gm, gr = xs[j].grad, ys[j].grad
        reg = (ys[j].detach().double().pow(2).sum(1, keepdim=True).sqrt() >= 1e-12).expand_as(gr)
        assert relmax(gm.cpu().numpy(), gr.cpu().numpy()) <= 1e-5, j
        assert relmax(torch.where(reg, gm, 0 * gm).cpu().numpy(), torch.where(reg, gr, 0 * gr).cpu().numpy()) <= 1e-5, j
    # need_affs=False: no map, the same losses
    out2 = pkg.embedding_loss_multi([x.detach() for x in xs], T, W, M, crit, [ent["offsets"] for ent in table])
    assert all(a is None for _, a, _ in out2) and all(torch.equal(l2, l.detach()) for (l2, _, _), (l, _, _) in zip(out2, out))


def test_embedding_loss_multi_falls_back(pkg, dev, table, spy):
    """(6) a bf16 entry: the table is outside the fused set, nothing batched is launched; a foreign criterion: the single calls"""
    crit = pkg.WeightedMSE()
    weights = [1.0, 0.5, 2.0, 1.0]
    offs = [ent["offsets"] for ent in table]
    dts = (torch.float32, torch.bfloat16, torch.float32, torch.float32)
    xs, T, W, M = _public_inputs(dev, table, dts)
    out = pkg.embedding_loss_multi(xs, T, W, M, crit, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.fwd == [] and spy.bwd == []
    ys, _, _, _ = _public_inputs(dev, table, dts)
    ref = _single_calls(pkg, crit, ys, T, W, M, table, weights)
    for j in range(4):
        assert torch.equal(out[j][0], ref[j][0]) and torch.equal(out[j][1], ref[j][1]) and torch.equal(xs[j].grad, ys[j].grad), j

    def foreign(pred, target, weight):  # a plain torch callable
        return (weight * (pred - target).abs()).mean()

    xs, T, W, M = _public_inputs(dev, table)
    M[2] = torch.ones_like(T[2], dtype=torch.uint8)  # (a foreign criterion multiplies by the mask: all ones where the table has none)
    out = pkg.embedding_loss_multi(xs, T, W, M, foreign, offs, need_affs=True)
    sum(l * c for (l, _, _), c in zip(out, weights)).backward()
    assert spy.fwd == []
    ys, _, _, _ = _public_inputs(dev, table)
    ref = [pkg.embedding_loss(y, t, w, m, foreign, o) for y, t, w, m, o in zip(ys, T, W, M, offs)]
    sum(l * c for (l, _, _), c in zip(ref, weights)).backward()
    for j in range(4):
        assert torch.equal(out[j][0], ref[j][0]) and torch.equal(out[j][1], ref[j][1]) and torch.equal(xs[j].grad, ys[j].grad), j


def test_embedding_loss_norm1_multi_equals_single_calls(pkg, dev, synth, orc, spy):
    crit = pkg.WeightedMSE()
    shapes = [(4, 16, 24), (4, 8, 12), (4, 4, 6), (3, 2, 3)]
    data = [synth.synth_inputs_3d(2, 16, z, y, x, orc.norm_offsets([1, 1, 1]), 620 + j) for j, (z, y, x) in enumerate(shapes)]
    xs = [cu(e, dev).requires_grad_(True) for e, _, _ in data]
    ys = [cu(e, dev).requires_grad_(True) for e, _, _ in data]
    T, W = [cu(t, dev) for _, t, _ in data], [cu(w, dev) for _, _, w in data]
    out = pkg.embedding_loss_norm1_multi(xs, T, W, crit, affs0_weight=0.7)
    sum(l for l, _ in out).backward()
    assert spy.fwd == [0] and spy.bwd == [0]
    ref = [pkg.embedding_loss_norm1(y, t, w, crit, affs0_weight=0.7) for y, t, w in zip(ys, T, W)]
    sum(l for l, _ in ref).backward()
    for j in range(4):
        assert abs(out[j][0].item() - ref[j][0].item()) <= 1e-6 * abs(ref[j][0].item()), j
        assert float((out[j][1] - ref[j][1]).abs().max()) <= 1e-6, j
        assert relmax(xs[j].grad.cpu().numpy(), ys[j].grad.cpu().numpy()) <= 1e-5, j


# ----------------------------------------------------------------------------------------------------------------------------
# (7) graph capture
# ----------------------------------------------------------------------------------------------------------------------------
def test_graphed_batched_section_equals_eager(pkg, dev, synth):
    """pea.graphed over a cvppp_loss_section(batched=True) step (forward + backward): the replay, also on refilled inputs, gives
    the eager step's total and gradients"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half, B, D, H, W = 2, 2, 16, 96, 96
    crit = pkg.WeightedMSE()

    def tensors(seed):
        e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, seed)
        ema = synth.synth_embedding((B, D, H, W), seed + 1)
        emds, downs = [], []
        for j in range(4):
            k = nb_half * (4 - j)
            ej, tj, wj, mj = synth.synth_inputs_2d(B, D, H >> (j + 1), W >> (j + 1), offsets[:k], seed + 2 + j)
            emds.append(ej)
            downs.append(np.concatenate([tj, wj, mj.astype(np.float32)], axis=1))
        return [cu(e, dev)] + [cu(x, dev) for x in emds] + [cu(ema, dev), cu(t, dev), cu(w, dev), cu(m, dev)] + [cu(x, dev) for x in downs]

    def step(*bufs):
        leaves = list(bufs[:5])
        for x in leaves:
            x.grad = None
        loss, pred, _ = pkg.cvppp_loss_section(leaves[0], leaves[1:], bufs[5], bufs[6], bufs[7], bufs[8], list(bufs[9:13]), crit, offsets,
                                               nb_half, batched=True)
        pkg.backward(loss)
        return loss, pred, [x.grad for x in leaves]

    static = tensors(171)
    for x in static[:5]:
        x.requires_grad_(True)
    g = pkg.graphed(step, *static)
    for seed in (171, 173):
        fresh = tensors(seed)
        with torch.no_grad():
            for dst, src in zip(static, fresh):
                dst.copy_(src)
        loss, pred, grads = g.replay()
        torch.cuda.synchronize()
        for x in fresh[:5]:
            x.requires_grad_(True)
        e_loss, e_pred, e_grads = step(*fresh)
        assert abs(loss.item() - e_loss.item()) <= 1e-6 * abs(e_loss.item()), seed
        assert torch.equal(pred, e_pred), seed
        for a, b in zip(grads, e_grads):
            assert torch.equal(a, b), seed
