"""GPU (-m gpu): the 3D losses on the ACTIVATED affinity map -- loss/embedding2affs_3d.py, loss/embedding2affs_3d_l2.py, the norm2 pair
of loss/loss_embedding_mse_3d.py, the PEA_FLAG_LOSS_ACT | PEA_FLAG_LOSS_BCE form of the tile-per-plane cross forward (k_fwd_xdma<.., ZF =
kXZ / 2, .., LACT, BCE>: the self loss; every other 3D call with the flag runs the tiled or direct kernels) and pea_affs_crop_zero
(include/pea_crop.h).

  (a) every tests/golden/ga3_*.npz fixture (the reference's own run, tests/golden/make_golden_act3d.py) through the public module:
      loss, stored map, gradient; four of them also through a foreign criterion;
  (b) the cross-kernel shape 2 x 16 x 6 x 48 x 96 (the `v3` family of tests/cross_stencils.py: whole 256-pixel blocks per plane, extents
      beyond the reach of 27 and the z shift of 4) against the float64 restatement of tests/act3d_reference.py: the norm5 and norm1
      tables, self and detached second operand, half + clamp and clamp, MSE and BCE -- each with default switches, under
      PEA_FWD_XDMA=0 and under PEA_FORCE_DIRECT=1;
  (c) pea_affs_crop_zero on a guard-banded buffer filled with a sentinel;
  (d) a second call is bit-identical;  (e) an embedding offset by one element;  (f) one NaN voxel;  (g) a captured step.

Tolerances are the existing suites' (test_gpu_act_loss.py): affs 1e-5 abs, loss 1e-5 rel, grad 1e-4 of its max; every term whose
float64 clamp input lies within 1e-4 of 0 or 1 has weight 0 on both sides, at most 0.2 % of the terms, asserted per case.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import act3d_reference as ref
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-5, 1e-4
HALF, CLAMP = ref.HALF, ref.CLAMP
GA3 = golden_names("ga3_")
LOSSES = [n for n in GA3 if not n.startswith("ga3_single")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def a3(pkg):
    return importlib.import_module(ge.PKG_NAME + ".loss._activated3d")


def cu(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _check(tag, loss, affs, grad, ref_loss, ref_affs, ref_grad):
    ea = float((affs.detach().double().cpu() - torch.as_tensor(ref_affs).double()).abs().max())
    eg = relmax(grad, torch.as_tensor(ref_grad))
    print("%s: loss %.9g (ref %.9g)  affs max err %.3g  grad rel err %.3g" % (tag, float(loss), float(ref_loss), ea, eg))
    assert abs(float(loss) - float(ref_loss)) <= LOSS_RTOL * abs(float(ref_loss)), tag
    assert ea < AFFS_ATOL, tag
    assert eg < GRAD_RTOL, tag


# ---- (a) the fixtures ----------------------------------------------------------------------------------------------------------------

def _call(pkg, g, dev, crit, e=None):
    fn = getattr(importlib.import_module(ge.PKG_NAME + ".loss." + str(g["module"])), str(g["fn"]))
    x = (cu(g["e"], dev) if e is None else e).requires_grad_(True)
    args = (x, cu(g["ema"], dev)) if "ema" in g else (x,)
    out = fn(*args, cu(g["target"], dev), cu(g["weight"], dev), crit, **ref.call_kwargs(g))
    assert isinstance(out, tuple) and len(out) == 2  # (loss, affs): the reference's return arity
    out[0].backward()
    torch.cuda.synchronize()
    assert not out[1].requires_grad
    return out[0].detach(), out[1].detach(), x.grad


@pytest.mark.parametrize("name", LOSSES)
def test_fixture_through_the_public_module(pkg, dev, name):
    """the reference's recorded loss, stored map (border rule and fill included) and gradient, with this package's criterion of the
    same name"""
    g = load_golden(name)
    assert int(g["edge_zeroed"]) <= ref.EDGE_MAX_FRACTION * int(g["terms"])
    loss, affs, grad = _call(pkg, g, dev, getattr(pkg, str(g["criterion"]))())
    _check(name, loss, affs, grad, g["loss"], g["affs"], g["grad"])


def _foreign_wmse(pred, target, weight):
    """a foreign criterion (no `pea_criterion` attribute) with WeightedMSE's arithmetic: sum(w (p - t)^2) / (B * prod(size[2:]))"""
    return torch.sum(weight * (pred - target) ** 2) / (pred.shape[0] * int(np.prod(pred.shape[2:])))


@pytest.mark.parametrize("name", ["ga3_norm1_fill", "ga3_norm2", "ga3_norm5_relu", "ga3_mse_ema_norm2"])
def test_fixture_through_a_foreign_criterion(pkg, dev, name):
    """any other criterion is called on the differentiable map (raw map's vjp, activation and border with torch ops): same numbers"""
    g = load_golden(name)
    assert str(g["criterion"]) == "WeightedMSE"
    loss, affs, grad = _call(pkg, g, dev, _foreign_wmse)
    _check(name, loss, affs, grad, g["loss"], g["affs"], g["grad"])


@pytest.mark.parametrize("name", ["ga3_single", "ga3_single_cos"])
def test_single_offset_fixture(pkg, dev, name):
    g = load_golden(name)
    fn = getattr(pkg.embedding2affs_3d, str(g["fn"]))
    for order in range(3):
        a = fn(cu(g["e"], dev), order, shift=int(g["shift"]))
        assert tuple(a.shape) == g["affs"][:, order].shape
        assert float((a.cpu() - torch.from_numpy(g["affs"][:, order])).abs().max()) < AFFS_ATOL
        assert not a.cpu().narrow(1 + order, 0, int(g["shift"])).view(torch.int32).any()  # an exact +0 on the border
    with pytest.raises(NotImplementedError):
        fn(cu(g["e"], dev), 3)


# ---- (b) the cross-kernel shape against float64 ----------------------------------------------------------------------------------------

V3 = (2, 16, 6, 48, 96)
TABLES = {"norm5": (list(ref.NORM5), 3), "norm1": ([1, 1, 1], 1)}
ACTS = {"half_clamp": HALF | CLAMP, "clamp": CLAMP}
CRITERIA = {"mse": "WeightedMSE", "bce": "WeightedBCE"}
_V3 = {}


def _two_instances(rng, n):
    """-> (e, ema or None): n noise draws around ONE instance-like embedding for the clamp(cos, 0, 1) + BCE cases: two labels in 8 x 8 cells, embedding +m or -m (|m| = 2) plus
    uniform noise of +-0.15 per channel (|noise| <= 0.6).  A pair across the labels has <e_p, e_q> <= -4 + 2 * 1.2 + 0.36 < 0 -- clamped
    to x = 0, slope 0 -- and a pair inside one has cos >= (4 - 2.4 - 0.36) / 2.6^2 = 0.18.

    Why these cases cannot use iid normal embeddings.  BCE's slope is w (x - y) / (x (1 - x)): a term at x carries the f32 rounding
    of the cosine, about 3e-8 absolute (sixteen products of O(1) values over norms of 4), amplified to 3e-8 / x RELATIVE -- 3e-4 of
    itself just outside the 1e-4 edge window, and that term is also the largest of the gradient.  No f32 kernel can then agree with
    float64 to 1e-4 of the gradient's maximum: with iid normal embeddings this case measured 8.3e-5 on the cross kernel and 1.6e-4 on
    the direct kernel that served it before (tests/test_gpu_bce.py leaves the end-to-end gradient of that module out for the same
    reason and holds g with x taken from the kernel).  Here no existing pair lies on the flank 0 < x < 0.02 or within 1e-3 below 1
    (asserted), so the bound means what it says; the x = 0 pairs against target 1 still cost 100 w each."""
    B, D, Z, Y, X = V3
    m = rng.standard_normal(D)
    m = (2.0 * m / np.linalg.norm(m)).astype(np.float32)
    lab = np.kron(rng.integers(0, 2, size=(B, Z, Y // 8, X // 8)), np.ones((8, 8), dtype=np.int64))
    sign = np.where(lab == 1, np.float32(1), np.float32(-1))[:, None]
    out = [(sign * m[None, :, None, None, None] + rng.uniform(-0.15, 0.15, size=V3)).astype(np.float32) for _ in range(n)]
    return out[0], (out[1] if n > 1 else None)


def _v3_case(table, other, act, crit):
    """inputs and the float64 reference of one case: computed once, shared by the three switch settings, never modified"""
    key = (table, other, act, crit)
    if key not in _V3:
        shifts, first = TABLES[table]
        rng = np.random.default_rng(7100 + 13 * sorted(TABLES).index(table) + 5 * int(other) + sorted(ACTS).index(act))
        if act == "clamp" and crit == "bce":
            e, ema = _two_instances(rng, 2 if other else 1)
        else:
            e = rng.standard_normal(V3).astype(np.float32)
            ema = (e + 0.5 * rng.standard_normal(V3)).astype(np.float32) if other else None
        kshape = (V3[0], len(shifts)) + V3[2:]
        t = (rng.random(kshape) < 0.6).astype(np.float32)
        w = (0.5 + 1.5 * rng.random(kshape)).astype(np.float32)
        v = ref.clamp_input64(e, ema, shifts, ACTS[act])
        if act == "clamp" and crit == "bce":  # well-conditioned by construction: no term on BCE's steep flanks
            vx = v[ref.exists(V3[2:], shifts)[None].expand(v.shape)]
            assert not (((vx > 0) & (vx < 0.02)) | ((vx > 1 - 1e-3) & (vx < 1))).any()
        near = ref.near_edge(v, ACTS[act]).numpy()
        assert near.mean() <= ref.EDGE_MAX_FRACTION, (key, near.mean())
        w = np.where(near, np.float32(0), w).astype(np.float32)
        loss, stored, grad, _ = ref.restate(e, ema, t, w, shifts, ACTS[act], "cropped", CRITERIA[crit], affs0_weight=0.75, first=first)
        _V3[key] = (e, ema, t, w, float(loss), stored.numpy(), grad.numpy(), float(near.mean()))
    return _V3[key]


@pytest.mark.parametrize("crit", sorted(CRITERIA))
@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("other", [False, True], ids=["self", "other"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_cross_kernel_shape_against_float64(pkg, a3, dev, monkeypatch, table, other, act, crit):
    shifts, first = TABLES[table]
    e, ema, t, w, ref_loss, ref_affs, ref_grad, dropped = _v3_case(table, other, act, crit)
    E, O, T, W = cu(e, dev), cu(ema, dev), cu(t, dev), cu(w, dev)
    criterion = getattr(pkg, CRITERIA[crit])()
    # the stencil and shape are ones the cross kernels take: with default switches the self loss' BCE forward is k_fwd_xdma<.., ZF, ..,
    # LACT, BCE>, the other cases decline to the tiled kernels (csrc/pea_k_xdma.hip says why); all must agree with float64
    flags = ACTS[act] | pkg._lib.FLAG_LOSS_ACT | (pkg._lib.FLAG_LOSS_BCE if crit == "bce" else 0)
    op = importlib.import_module(ge.PKG_NAME + ".affinity_op")
    d = op.make_desc(a3.spec3d(shifts, [1.0] * len(shifts), 1e-12, flags), E)
    assert op.cross_supported(d, 2 if other else 0)
    for name, value in ((None, None), ("PEA_FWD_XDMA", "0"), ("PEA_FORCE_DIRECT", "1")):
        if name:
            monkeypatch.setenv(name, value)
        x = E.clone().requires_grad_(True)
        loss, affs = a3.cropped_loss(x, O, T, W, criterion, shifts, 0.75, first, ACTS[act])
        loss.backward()
        torch.cuda.synchronize()
        tag = "%s %s %s %s [%s] (edge-zeroed %.4f %%)" % (table, "other" if other else "self", act, crit, name or "default", 100 * dropped)
        _check(tag, loss.detach(), affs, x.grad, ref_loss, ref_affs, ref_grad)
        if name:
            monkeypatch.delenv(name)


# ---- (c) pea_affs_crop_zero ------------------------------------------------------------------------------------------------------------

def test_crop_zero_touches_exactly_the_missing_pairs(pkg, dev):
    """a K = 12 norm5 table, then a diagonal 3D offset and a positive one; the map starts one element past a 16-byte boundary inside a
    guard-banded buffer of sentinels: exactly the non-existent pairs become +0.0, every other element and the guards keep their bits"""
    pp = importlib.import_module(ge.PKG_NAME + ".utils.postproc")
    B, Z, Y, X = 2, 6, 30, 29
    offsets = [tuple(-s if a == i % 3 else 0 for a in range(3)) for i, s in enumerate(ref.NORM5)] + [(1, -2, 3), (0, 4, 0)]
    K = len(offsets)
    N, G = B * K * Z * Y * X, 1024
    sentinel = np.int32(0x7fc12345)  # a NaN with a payload: no arithmetic produces it
    buf = torch.full((G + 1 + N + G,), int(sentinel), dtype=torch.int32, device=dev)
    affs = buf[G + 1:G + 1 + N].view(torch.float32).view(B, K, Z, Y, X)
    assert affs.data_ptr() % 16 == 4 and affs.is_contiguous()
    d = pp.crop_desc(affs.shape, offsets)
    rc = pkg._lib.lib().pea_affs_crop_zero(ctypes.byref(d), ctypes.c_void_p(affs.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    want = np.full((K, Z, Y, X), sentinel, np.int32)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    for k, (oz, oy, ox) in enumerate(offsets):
        inside = (zz + oz >= 0) & (zz + oz < Z) & (yy + oy >= 0) & (yy + oy < Y) & (xx + ox >= 0) & (xx + ox < X)
        want[k][~inside] = 0
    got = buf.cpu().numpy()
    assert (got[:G + 1] == sentinel).all() and (got[G + 1 + N:] == sentinel).all()
    assert np.array_equal(got[G + 1:G + 1 + N].reshape(B, K, Z, Y, X), np.broadcast_to(want, (B, K, Z, Y, X)))
    # the public wrapper: the same map again (idempotent), and the version counter moves
    ver = affs._version
    assert pkg.affs_crop_zero_(affs, offsets) is affs and affs._version > ver
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), got)


# ---- (d) .. (g) on the norm5 fixture ------------------------------------------------------------------------------------------------------

def test_second_call_is_bit_identical(pkg, dev):
    g = load_golden("ga3_norm5")
    a = _call(pkg, g, dev, pkg.WeightedMSE())
    b = _call(pkg, g, dev, pkg.WeightedMSE())
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("name", ["ga3_norm5", "ga3_norm5_wbce", "ga3_mse_ema_norm2"])
def test_embedding_offset_by_one_element(pkg, dev, name):
    """e starts 4 bytes past a 16-byte boundary: the cross kernels decline, the next family serves the call with the same results"""
    g = load_golden(name)
    flat = torch.zeros(g["e"].size + 1, dtype=torch.float32, device=dev)
    e = flat[1:].view(g["e"].shape)
    e.copy_(cu(g["e"], dev))
    assert e.data_ptr() % 16 == 4 and e.is_contiguous()
    loss, affs, grad = _call(pkg, g, dev, getattr(pkg, str(g["criterion"]))(), e=e.detach())
    _check(name + " (e + 1 element)", loss, affs, grad, g["loss"], g["affs"], g["grad"])


def test_one_nan_voxel(pkg, dev):
    """include/pea.h, non-finite embeddings: the loss is NaN and the stored map is NaN on the pairs that read the voxel -- and only
    there; the border stays 0"""
    g = load_golden("ga3_norm5")
    clean = _call(pkg, g, dev, pkg.WeightedMSE())[1].cpu()
    q = (3, 15, 20)
    e = g["e"].copy()
    e[0, 5, q[0], q[1], q[2]] = np.nan
    loss, affs, _ = _call(pkg, dict(g, e=e), dev, pkg.WeightedMSE())
    assert torch.isnan(loss)
    want = torch.zeros(clean.shape, dtype=torch.bool)
    dims = e.shape[2:]
    for i, s in enumerate(ref.NORM5):
        ax = i % 3
        if q[ax] >= s:  # the pair (q, q - s)
            want[(0, i) + q] = True
        if q[ax] + s < dims[ax]:  # the pair (q + s, q)
            p = list(q)
            p[ax] += s
            want[(0, i) + tuple(p)] = True
    affs = affs.cpu()
    assert torch.equal(torch.isnan(affs), want) and int(want.sum()) > 12
    assert float((affs[~want] - clean[~want]).abs().max()) < AFFS_ATOL


def test_graphed_step_replays_the_eager_values(pkg, dev):
    g = load_golden("ga3_norm5")
    crit = pkg.WeightedMSE()
    E, T, W = cu(g["e"], dev).requires_grad_(True), cu(g["target"], dev), cu(g["weight"], dev)

    def step(E, T, W):
        E.grad = None
        loss, affs = pkg.embedding2affs_3d.embedding_loss_norm5(E, T, W, crit, affs0_weight=2.0)
        pkg.backward(loss)
        return loss, affs, E.grad

    eager = [t.detach().clone() for t in step(E, T, W)]
    torch.cuda.synchronize()
    _check("eager", eager[0], eager[1], eager[2], g["loss"], g["affs"], g["grad"])
    graph = pkg.graphed(step, E, T, W)
    for _ in range(2):
        out = graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
