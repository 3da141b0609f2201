"""GPU (-m gpu): the binary cross-entropy criterion of the loss on the activated map (PEA_FLAG_LOSS_BCE), and the other criteria of
loss/loss.py (BCELoss, MSELoss) on the fused path.

  a. every tests/golden/gbce_*.npz fixture (the reference's loss modules run with its WeightedBCE / BCELoss / MSELoss by
     tests/golden/make_golden_bce.py) through the package's modules of the same names: loss and map always, the gradient for every
     module but loss_embedding_exp;
  b. the decomposed check: pea_affinity_fwd_ex's affs against the float64 restatement of test_gpu_act_loss.py, then loss_out and g_out
     against the closed form of include/pea.h evaluated in float64 from the kernel's OWN f32 u -- independent of BCE's conditioning;
  c. end to end against float64 autograd of F.binary_cross_entropy on the restated map (half shift + clamp);
  d. identities.

Tolerances are test_gpu_act_loss.py's: affs 1e-5 abs, loss 1e-5 rel, grad 1e-4 of its max (8e-3 for 16-bit storage).

Edges.  BCE's slope is 1 / x near x = 0 and 1 / (1 - x) near x = 1.  With clamp(cos, 0, 1) 6 - 12 % of random-embedding terms lie within
0.02 of an edge, where the f32 rounding of x is amplified past any fixed tolerance: that module's end-to-end gradient is not compared,
its g is held by (b), which takes x from the kernel.  In (b) the slope s = du / da comes from the float64 v, so terms whose float64
|v - edge| < 1e-4 are left out of the g comparison (the kernel may stand on the other side of the edge); in (c) terms whose float64 v
lies within 0.02 of 0 or 1 get weight 0 on both sides.  Both sets are asserted to be at most 0.2 % of the terms.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
import test_gpu_act_loss as al
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL, GRAD_RTOL_16 = al.AFFS_ATOL, al.LOSS_RTOL, al.GRAD_RTOL, al.GRAD_RTOL_16
EDGE, EDGE_MAX_FRACTION, NEAR = 1e-4, 0.002, 0.02
HALF, CLAMP, MASK_F32, LOSS_ACT, LOSS_BCE = 4, 8, 32, 64, 128
ACTS = {"half_clamp": HALF | CLAMP, "clamp": CLAMP}
GBCE = golden_names("gbce_")
cu, relmax = al.cu, al.relmax


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
    return importlib.import_module(pkg.__name__ + ".affinity_op")


@pytest.fixture
def switch(pkg):
    yield pkg._lib.set_switch
    pkg._lib.set_switch("PEA_FORCE_DIRECT", None)


# ---- a. the fixtures through the public modules -----------------------------------------------------------------------------------

def _call_module(pkg, g, dev):
    mod = getattr(pkg, str(g["module"])) if str(g["module"]) != "loss_embedding_mse" else importlib.import_module(
        pkg.__name__ + ".loss.loss_embedding_mse")
    crit = getattr(pkg, str(g["criterion"]))()
    x = cu(g["e"], dev).requires_grad_(True)
    offsets = [list(map(int, o)) for o in g["offsets"]]
    kw = {"affs0_weight": float(g["affs0_weight"])}
    if str(g["mode"]):
        kw["mode"] = str(g["mode"])
    args = (cu(g["target"], dev), cu(g["weight"], dev), cu(g["mask"], dev), crit, offsets)
    if "ema" in g:
        out = mod.ema_embedding_loss(x, cu(g["ema"], dev), *args, **kw)
    else:
        out = mod.embedding_loss(x, *args, **kw)
    out[0].backward()
    torch.cuda.synchronize()
    return out[0].detach(), out[1].detach(), x.grad


@pytest.mark.parametrize("name", GBCE)
def test_fixture_through_the_public_module(pkg, dev, name, monkeypatch):
    """the reference's recorded loss, map and gradient -- on the FUSED path: the composed one is made to raise"""
    def composed(*a, **k):
        raise AssertionError("the composed path ran: this criterion must take the fused forward")
    for m in ("_activated", "loss_embedding_mse"):
        monkeypatch.setattr(importlib.import_module(pkg.__name__ + ".loss." + m), "_foreign_criterion", composed)
    g = load_golden(name)
    loss, affs, grad = _call_module(pkg, g, dev)
    aerr = float((affs.cpu() - torch.from_numpy(g["affs"])).abs().max())
    gerr = relmax(grad, torch.from_numpy(g["grad"]))
    print("%s: loss %.9g (ref %.9g)  affs max err %.3g  grad rel err %.3g  within %.2f of an edge %d / %d" % (
        name, loss.item(), float(g["loss"]), aerr, gerr, NEAR, int(g["edge_near"]), int(g["terms"])))
    assert abs(loss.item() - float(g["loss"])) <= LOSS_RTOL * abs(float(g["loss"])), name
    assert aerr < AFFS_ATOL, name
    if str(g["module"]) != "loss_embedding_exp":  # (see "Edges" above)
        assert int(g["edge_near"]) <= EDGE_MAX_FRACTION * max(int(g["terms"]), 1), name
        assert gerr < GRAD_RTOL, name


# ---- the raw call and its float64 counterparts -------------------------------------------------------------------------------------

def _fwd_ex(pkg, op, E, other, T, W, M, offsets, lam, eps, flags, ndim=2, border=0, norm=2):
    """pea_affinity_fwd_ex through _lib -> affs, g_out, loss_out[1 + K] (the 1 / norm planes are handed over: the cross kernels of the
    loss with a second operand run only with them)"""
    L = pkg._lib
    spec = pkg.AffinitySpec(ndim, offsets, lam, border, norm, eps, False, flags)
    K = len(offsets)
    kshape = (E.shape[0], K) + tuple(E.shape[2:])
    Mc, ms, mflag = op.mask_arg(M, kshape)
    d = op.make_desc(spec, E, 0, 0, ms, mflag)
    affs = torch.empty(kshape, dtype=torch.float32, device=E.device)
    g = torch.full(kshape, float("nan"), dtype=torch.float32, device=E.device)
    loss = torch.empty(1 + K, dtype=torch.float32, device=E.device)
    inv = torch.empty(((2,) if other is not None else ()) + (E.shape[0],) + tuple(E.shape[2:]), dtype=torch.float32, device=E.device)
    work, wsb = op.workspace(E.device, d)
    p = op._ptr
    L.check(L.lib().pea_affinity_fwd_ex(ctypes.byref(d), p(E), p(other), p(T.contiguous()), p(W.contiguous()), p(Mc), p(affs), p(g),
                                        p(inv), p(loss), p(work), wsb, op._stream()), "pea_affinity_fwd_ex")
    torch.cuda.synchronize()
    return affs, g, loss


def _map64(E5, other5, offsets3, eps, act, border):
    """float64, 5D: v (what the clamp sees), u (what affs stores), ok (the pair exists) -- the arithmetic of al._restate"""
    x = E5.double()
    y = x if other5 is None else other5.double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
    vs, us, oks = [], [], []
    for o in offsets3:
        ys, ok = al._shifted(yn, o, border)
        a = (xn * ys).sum(1) * ok
        v, u = al._activate64(a, act)
        vs.append(v)
        us.append(u)
        oks.append(ok.expand(a.shape))
    return torch.stack(vs, 1), torch.stack(us, 1), torch.stack(oks, 1)


def _norms(pkg, B, dims, offsets3, norm):
    L = pkg._lib
    if norm == L.NORM_BX:
        return [B * dims[2]] * len(offsets3)
    if norm == L.NORM_FULL:
        return [B * dims[0] * dims[1] * dims[2]] * len(offsets3)
    return [B * int(np.prod([dims[a] - abs(int(o[a])) for a in range(3)])) for o in offsets3]


def _closed_form(u32, v64, ok, T, W, M, lam, ns, act):
    """include/pea.h, PEA_FLAG_LOSS_BCE, in float64 from the kernel's f32 u: -> loss_out[1 + K], g, the terms whose slope is safe"""
    x = u32.double() * M
    y = T.double() * M
    w = W.double()
    lx = torch.clamp(torch.log(x), min=-100.0)
    l1 = torch.clamp(torch.log1p(-x), min=-100.0)
    l = torch.where(ok, -w * (y * lx + (1 - y) * l1), torch.zeros_like(x))
    s = (0.5 if act & HALF else 1.0) * ((v64 >= 0) & (v64 <= 1)).double()
    gf = w * (x - y) / torch.clamp(x * (1 - x), min=1e-12) * M * s
    K = len(lam)
    view = [1, K] + [1] * (x.dim() - 2)
    lam_n = (torch.tensor(lam, dtype=torch.float64, device=x.device) / torch.tensor(ns, dtype=torch.float64, device=x.device)).view(view)
    g = torch.where(ok, gf * lam_n, torch.zeros_like(x))
    Li = l.sum(dim=[0] + list(range(2, x.dim()))) / torch.tensor(ns, dtype=torch.float64, device=x.device)
    total = (Li * torch.tensor(lam, dtype=torch.float64, device=x.device)).sum()
    safe = ~(ok & (((v64).abs() < EDGE) | ((v64 - 1).abs() < EDGE)))
    return torch.cat([total.view(1), Li]), g, safe


def _exact_mask(shape, dev, seed):
    """an f32 mask from {0, 0.25, 0.5, 1}: u * m is exact"""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, shape, generator=g)].to(dev)


def _decomposed(tag, pkg, op, E, other, T, W, M, offsets, lam, eps, act, ndim, border, norm):
    offsets3 = [[0] * (3 - len(o)) + [int(v) for v in o] for o in offsets]
    affs, g, loss = _fwd_ex(pkg, op, E, other, T, W, M, offsets, lam, eps, act | LOSS_ACT | LOSS_BCE, ndim, border, norm)
    five = (lambda t: t.unsqueeze(2)) if ndim == 2 else (lambda t: t)
    E5, other5 = five(E.float()), None if other is None else five(other.float())  # (v from the storage-rounded embedding)
    v64, u64, ok = _map64(E5, other5, offsets3, eps, act, border)
    M5 = torch.ones_like(u64) if M is None else five(M).double()
    ns = _norms(pkg, E.shape[0], E5.shape[2:], offsets3, norm)
    want_loss, want_g, safe = _closed_form(five(affs), v64, ok, five(T), five(W), M5, lam, ns, act)
    aerr = float((five(affs).double() - u64).abs().max())
    lerr = float(((loss.double() - want_loss).abs() / want_loss.abs().clamp_min(1e-300)).max())
    unsafe = float((~safe).double().mean())
    gd = (five(g).double() - want_g).abs()
    gmax = float((want_g.abs() * safe).max())
    gexcess = float(((gd - LOSS_RTOL * want_g.abs() - LOSS_RTOL * gmax) * safe).max())
    print("%s: loss %.9g (closed form %.9g)  worst loss_out rel err %.3g  affs max err %.3g  g: max |err| %.3g of max |g| %.3g  "
          "edge terms left out %.4f %%" % (tag, loss[0].item(), want_loss[0].item(), lerr, aerr, float((gd * safe).max()), gmax, 100 * unsafe))
    assert aerr < AFFS_ATOL, tag
    assert bool(torch.isfinite(loss).all()) and lerr <= LOSS_RTOL, tag
    assert unsafe <= EDGE_MAX_FRACTION, tag
    assert not bool(torch.isnan(g).any()), tag  # (every element of g_out was written)
    assert gexcess <= 0, tag
    assert bool((five(g)[~ok] == 0).all()), tag  # a cropped-away pair has g = 0


# (D, storage dtype, stencil, H, W, PEA_FORCE_DIRECT, 2D border): the f32 cross kernels at D = 16 / 32 / 64, the direct kernels, a diagonal
# stencil (the tiled kernels decline BCE: direct), 16-bit storage on the cross stencil (the 16-bit cross kernels decline: direct), and
# the cropped 2D border (cropped normaliser) on the cross and the direct kernel
B_CASES = {
    "xdma_d16": (16, torch.float32, "cross", 128, 128, False, 0),
    "xdma_d32": (32, torch.float32, "cross", 128, 128, False, 0),
    "xdma_d64": (64, torch.float32, "cross8", 128, 128, False, 0),
    "direct_d16": (16, torch.float32, "cross", 96, 128, True, 0),
    "diag_d16": (16, torch.float32, "diag", 96, 128, False, 0),
    "direct_d32_f16": (32, torch.float16, "cross", 128, 128, False, 0),
    "direct_d32_bf16": (32, torch.bfloat16, "cross", 128, 128, False, 0),
    "crop_xdma_d16": (16, torch.float32, "cross", 128, 128, False, 1),
    "crop_direct_d16": (16, torch.float32, "cross", 96, 128, True, 1),
}


@pytest.mark.parametrize("fmask", [False, True], ids=["u8", "f32mask"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("actname", sorted(ACTS))
@pytest.mark.parametrize("case", sorted(B_CASES))
def test_decomposed_closed_form(pkg, op, dev, synth, switch, case, actname, cross, fmask):
    D, dt, sname, H, W, direct, border = B_CASES[case]
    act = ACTS[actname]
    offsets = al._offs(pkg, sname)
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 900 + D + H + act)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt = cu(e, dev).to(dt), cu(t, dev), cu(w, dev)
    M = _exact_mask(T.shape, dev, 11 + D) if fmask else cu(m, dev)
    ema = cu(synth.synth_embedding((2, D, H, W), 901), dev).to(dt) if cross else None
    lam = [0.5 if i < 2 else 1.0 for i in range(len(offsets))]
    norm = pkg._lib.NORM_CROPPED if border else pkg._lib.NORM_FULL
    _decomposed("%s/%s/%s/%s" % (case, actname, "ema" if cross else "self", "f32mask" if fmask else "u8"), pkg, op, E, ema, T, Wt, M,
                offsets, lam, 1e-6, act, 2, border, norm)


@pytest.mark.parametrize("actname", sorted(ACTS))
@pytest.mark.parametrize("border", ["crop_zero_3d", "replicate_3d"])
def test_decomposed_closed_form_direct_only_descriptors(pkg, op, dev, synth, actname, border):
    """the two 3D descriptors of test_gpu_act_loss.py::test_direct_only_descriptors (no mask in 3D)"""
    L = pkg._lib
    act = ACTS[actname]
    if border == "crop_zero_3d":
        D, bcode, norm = 12, L.BORDER_CROP_ZERO, L.NORM_CROPPED
        offsets = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [0, 2, -2], [1, 1, 1]]
    else:
        D, bcode, norm = 8, L.BORDER_REPLICATE, L.NORM_FULL
        offsets = [[0, -1, -1], [0, 2, -2], [1, 1, 1], [-1, -3, 3], [0, -3, -1], [2, 1, -2], [-2, -1, -1], [0, 1, 3]]
    e, t, w = synth.synth_inputs_3d(2, D, 6, 40, 48, offsets, 40 + D)
    lam = [2.0 if i < 3 else 1.0 for i in range(len(offsets))]
    _decomposed("%s/%s" % (border, actname), pkg, op, cu(e, dev), None, cu(t, dev), cu(w, dev), None, offsets, lam, 1e-12, act, 3, bcode, norm)


# ---- c. end to end against float64 autograd ----------------------------------------------------------------------------------------

C_CASES = ["xdma_d16", "xdma_d32", "xdma_d64", "direct_d16", "direct_d32_bf16"]


@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("case", C_CASES)
def test_end_to_end_matches_float64_autograd(pkg, dev, synth, switch, case, cross):
    D, dt, sname, H, W, direct, _ = B_CASES[case]
    act = HALF | CLAMP
    offsets = al._offs(pkg, sname)
    offsets3 = [[0] + [int(v) for v in o] for o in offsets]
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 950 + D + H)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt, M = cu(e, dev).to(dt), cu(t, dev), cu(w, dev), cu(m, dev)
    ema = cu(synth.synth_embedding((2, D, H, W), 951), dev).to(dt) if cross else None
    lam = [0.5 if i < 2 else 1.0 for i in range(len(offsets))]
    eps = 1e-6
    E5, ema5 = E.float().unsqueeze(2), None if ema is None else ema.float().unsqueeze(2)
    v64, _, _ = _map64(E5, ema5, offsets3, eps, act, 0)
    near = ((v64 < NEAR) | (v64 > 1 - NEAR)).squeeze(2)
    frac = float(near.double().mean())
    Wt = torch.where(near, torch.zeros_like(Wt), Wt).contiguous()
    got = al._fused(pkg, E, ema, T, Wt, M, offsets, lam, eps, act | LOSS_ACT | LOSS_BCE, norm=pkg._lib.NORM_FULL)
    # float64: F.binary_cross_entropy (mean over [B,H,W]) on the restated map
    x = E5.double().requires_grad_(True)
    y = x if ema5 is None else ema5.double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
    o_loss, maps = 0.0, []
    for i, o in enumerate(offsets3):
        ys, _ = al._shifted(yn, o, 0)
        u = torch.clamp(((xn * ys).sum(1) + 1) / 2, 0.0, 1.0).squeeze(1)
        mi = M[:, i].double()
        o_loss = o_loss + lam[i] * F.binary_cross_entropy(u * mi, T[:, i].double() * mi, Wt[:, i].double())
        maps.append(u.detach())
    o_loss.backward()
    al._check("bce/%s/%s" % (case, "ema" if cross else "self"), got, (o_loss.detach(), torch.stack(maps, 1), x.grad.squeeze(2)), dt, frac)


# ---- d. identities -------------------------------------------------------------------------------------------------------------------

def _inputs(pkg, synth, dev, D, H, W, sname, seed, dt=torch.float32):
    offsets = al._offs(pkg, sname)
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, seed)
    return offsets, cu(e, dev).to(dt), cu(t, dev), cu(w, dev), cu(m, dev)


@pytest.mark.parametrize("case", ["xdma_d16", "xdma_d64", "direct_d16", "direct_d32_bf16", "crop_xdma_d16"])
def test_second_call_is_bit_identical(pkg, dev, synth, switch, case):
    D, dt, sname, H, W, direct, border = B_CASES[case]
    offsets, E, T, Wt, M = _inputs(pkg, synth, dev, D, H, W, sname, 600 + D, dt)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    lam = [1.0] * len(offsets)
    kw = dict(border=border, norm=pkg._lib.NORM_CROPPED if border else pkg._lib.NORM_FULL)
    a = al._fused(pkg, E, None, T, Wt, M, offsets, lam, 1e-6, HALF | CLAMP | LOSS_ACT | LOSS_BCE, **kw)
    b = al._fused(pkg, E, None, T, Wt, M, offsets, lam, 1e-6, HALF | CLAMP | LOSS_ACT | LOSS_BCE, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y), case


@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("actname", sorted(ACTS))
def test_direct_and_cross_kernel_agree(pkg, op, dev, synth, switch, actname, cross):
    offsets, E, T, Wt, M = _inputs(pkg, synth, dev, 16, 128, 128, "cross", 620)
    ema = cu(synth.synth_embedding((2, 16, 128, 128), 621), dev) if cross else None
    lam = [0.5 if i < 2 else 1.0 for i in range(len(offsets))]
    flags = ACTS[actname] | LOSS_ACT | LOSS_BCE
    a = _fwd_ex(pkg, op, E, ema, T, Wt, M, offsets, lam, 1e-6, flags)
    switch("PEA_FORCE_DIRECT", "1")
    b = _fwd_ex(pkg, op, E, ema, T, Wt, M, offsets, lam, 1e-6, flags)
    rel = ((a[2].double() - b[2].double()).abs() / b[2].double().abs()).max().item()
    print("cross vs direct (%s, %s): loss_out worst rel diff %.3g; affs bit-equal %.2f %%, g bit-equal %.2f %%" % (
        actname, "ema" if cross else "self", rel, 100 * (a[0] == b[0]).double().mean().item(), 100 * (a[1] == b[1]).double().mean().item()))
    assert rel <= LOSS_RTOL
    assert float((a[0] - b[0]).abs().max()) < AFFS_ATOL
    # the same a gives the same bits of g (bce_term is stated once): where the two kernels stored the same u, g agrees to the bit
    # wherever the clamp was not involved (u strictly inside (0, 1): v = u there)
    same = (a[0] == b[0]) & (a[0] > 0) & (a[0] < 1)
    assert bool(same.any()) and torch.equal(a[1][same], b[1][same])


@pytest.mark.parametrize("case", ["xdma_d16", "direct_d16"])
def test_without_the_bit_the_loss_is_the_squared_residual(pkg, op, dev, synth, switch, case):
    """the same descriptor without PEA_FLAG_LOSS_BCE: the LOSS_ACT loss of the public module with WeightedMSE, bit for bit -- another
    number than the BCE loss"""
    D, dt, sname, H, W, direct, _ = B_CASES[case]
    offsets, E, T, Wt, M = _inputs(pkg, synth, dev, D, H, W, sname, 640)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    lam = [0.5 if i < 2 else 1.0 for i in range(len(offsets))]
    bce = _fwd_ex(pkg, op, E, None, T, Wt, M, offsets, lam, 1e-6, HALF | CLAMP | LOSS_ACT | LOSS_BCE, norm=pkg._lib.NORM_BX)
    mse = _fwd_ex(pkg, op, E, None, T, Wt, M, offsets, lam, 1e-6, HALF | CLAMP | LOSS_ACT, norm=pkg._lib.NORM_BX)
    loss, affs = pkg.loss_embedding.embedding_loss(E.clone().requires_grad_(True), T, Wt, M, pkg.WeightedMSE(), offsets, affs0_weight=0.5)
    assert torch.equal(mse[2][0], loss.detach()) and torch.equal(mse[0], affs) and torch.equal(bce[0], affs)
    assert abs(bce[2][0].item() - mse[2][0].item()) > 1e-3 * abs(mse[2][0].item())
    assert not torch.equal(bce[1], mse[1])


@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("case", ["xdma_d16", "xdma_d32", "direct_d16", "direct_d32_bf16"])
def test_zero_mask_gives_zero_loss_and_zero_g(pkg, op, dev, synth, switch, case, cross):
    D, dt, sname, H, W, direct, _ = B_CASES[case]
    offsets, E, T, Wt, M = _inputs(pkg, synth, dev, D, H, W, sname, 660, dt)
    ema = cu(synth.synth_embedding((2, D, H, W), 661), dev).to(dt) if cross else None
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    for Z in (torch.zeros_like(M), torch.zeros_like(T)):  # u8 and f32
        affs, g, loss = _fwd_ex(pkg, op, E, ema, T, Wt, Z, offsets, [1.0] * len(offsets), 1e-6, HALF | CLAMP | LOSS_ACT | LOSS_BCE)
        assert bool((loss == 0).all()) and bool((g == 0).all()), case


@pytest.mark.parametrize("direct", [False, True], ids=["cross", "direct"])
def test_clamped_to_zero_against_target_one_costs_exactly_100_w(pkg, op, dev, switch, direct):
    """CLAMP01 alone with a < 0 everywhere (the second operand is the negated embedding of a constant direction): u = 0, and against
    t = 1 every term is -w max(log 0, -100) = 100 w; the slope is 0, so g = 0.  N = 2 * 128 * 128 is a power of two and the weights
    are small integers / 2: every sum is exact"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    K = len(offsets)
    gen = torch.Generator().manual_seed(77)
    c = torch.randn(1, 16, 1, 1, generator=gen)
    E = (c * (0.5 + torch.rand(2, 1, 128, 128, generator=gen))).to(dev).contiguous()
    ema = (-E).contiguous()
    T = torch.ones(2, K, 128, 128, device=dev)
    Wt = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (2, K, 128, 128), generator=gen)].to(dev)
    lam = [1.0] * K
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    affs, g, loss = _fwd_ex(pkg, op, E, ema, T, Wt, None, offsets, lam, 1e-6, CLAMP | LOSS_ACT | LOSS_BCE)
    assert bool((affs == 0).all()) and bool((g == 0).all())
    want = 100.0 * Wt.double().sum(dim=(0, 2, 3)) / (2 * 128 * 128)
    assert torch.equal(loss[1:], want.float())
    assert loss[0].item() == np.float32(want.sum().item())


@pytest.mark.parametrize("direct", [False, True], ids=["cross", "direct"])
def test_one_nan_pixel(pkg, op, dev, synth, switch, direct):
    """a NaN u gives a NaN loss and g = 0 on the pairs of that pixel (u == v is false there); every other g is the clean call's"""
    offsets, E, T, Wt, M = _inputs(pkg, synth, dev, 16, 128, 128, "cross", 680)
    M = torch.ones_like(M)
    lam = [1.0] * len(offsets)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    flags = HALF | CLAMP | LOSS_ACT | LOSS_BCE
    clean = _fwd_ex(pkg, op, E, None, T, Wt, M, offsets, lam, 1e-6, flags)
    qy, qx = 50, 70
    En = E.clone()
    En[1, 3, qy, qx] = float("nan")
    affs, g, loss = _fwd_ex(pkg, op, En, None, T, Wt, M, offsets, lam, 1e-6, flags)
    hit = torch.zeros_like(g, dtype=torch.bool)
    for i, (oy, ox) in enumerate(offsets):
        hit[1, i, qy, qx] = True                              # the pair (q, q + o_i)
        hit[1, i, (qy - oy) % 128, (qx - ox) % 128] = True    # the pair (q - o_i, q)
    assert bool(torch.isnan(loss).all())
    assert bool(torch.isnan(affs[hit]).all()) and not bool(torch.isnan(affs[~hit]).any())
    assert bool((g[hit] == 0).all())
    assert torch.equal(g[~hit], clean[1][~hit]) and torch.equal(affs[~hit], clean[0][~hit])
    # the state block is clean again: the next call's loss is the clean one
    again = _fwd_ex(pkg, op, E, None, T, Wt, M, offsets, lam, 1e-6, flags)
    assert torch.equal(again[2], clean[2])


def test_weightmap_none_and_unweighted_criteria_use_ones(pkg, dev, synth):
    offsets, E, T, Wt, M = _inputs(pkg, synth, dev, 16, 128, 128, "cross", 700)
    ones = torch.ones_like(T)
    a = pkg.loss_embedding.embedding_loss(E, T, None, M, pkg.WeightedBCE(), offsets)
    b = pkg.loss_embedding.embedding_loss(E, T, ones, M, pkg.WeightedBCE(), offsets)
    c = pkg.loss_embedding.embedding_loss(E, T, Wt, M, pkg.BCELoss(), offsets)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], b[1])
    d = pkg.loss_embedding.embedding_loss(E, T, Wt, M, pkg.WeightedBCE(), offsets)
    assert not torch.equal(d[0], a[0])


def test_graphed_step(pkg, dev, synth):
    """pea.graphed of a WeightedBCE training step replays to the eager step's values"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    e, t, w, m = synth.synth_inputs_2d(2, 16, 128, 128, offsets, 71)
    E, T, W, M = cu(e, dev).requires_grad_(True), cu(t, dev), cu(w, dev), cu(m, dev)
    crit = pkg.WeightedBCE()

    def step(E, T, W, M):
        E.grad = None
        loss, affs = pkg.loss_embedding.embedding_loss(E, T, W, M, crit, offsets, affs0_weight=0.5)
        pkg.backward(loss)
        return loss, affs, E.grad

    x = cu(e, dev).requires_grad_(True)
    l0, a0 = pkg.loss_embedding.embedding_loss(x, T, W, M, crit, offsets, affs0_weight=0.5)
    pkg.backward(l0)
    loss, affs, grad = pkg.graphed(step, E, T, W, M).replay()
    assert torch.equal(loss, l0.detach()) and torch.equal(affs, a0) and torch.equal(grad, x.grad)


@pytest.mark.parametrize("fn", ["embedding_loss_norm1", "embedding_loss_norm5", "ema_embedding_loss_norm1", "ema_embedding_loss_norm5"])
def test_mse_on_the_3d_losses_is_fused_and_equals_the_composed_path(pkg, dev, synth, fn, monkeypatch):
    """MSELoss on the raw-cosine 3D losses: nn.MSELoss's mean over each cropped slice is the fused loss' cropped normaliser with a ones
    weight; the composed path (criterion per cropped slice on the differentiable map) is the reference's statement of it"""
    m3 = importlib.import_module(pkg.__name__ + ".loss.loss_embedding_mse_3d")
    aff = importlib.import_module(pkg.__name__ + ".utils.affinity_ours")
    norm5 = "norm5" in fn
    shifts = list(aff.NORM5_SHIFTS) if norm5 else [2] * 3
    e, t, w = synth.synth_inputs_3d(1, 16, 6, 40, 48, aff.axis_offsets_3d(shifts), 73)
    T, Wt = cu(t, dev), cu(w, dev)
    ema = cu(synth.synth_embedding((1, 16, 6, 40, 48), 74), dev) if fn.startswith("ema") else None
    crit = pkg.MSELoss()
    x = cu(e, dev).requires_grad_(True)
    want_loss, want_affs = m3._foreign(x, ema, T, Wt, crit, shifts, m3._spec(shifts, 0.5, 3 if norm5 else 1))
    want_loss.backward()

    def composed(*a, **k):
        raise AssertionError("the composed path ran: MSELoss must take the fused forward")
    monkeypatch.setattr(m3, "_foreign", composed)
    y = cu(e, dev).requires_grad_(True)
    args = (y,) + ((ema,) if ema is not None else ()) + (T, Wt, crit)
    loss, affs = getattr(pkg, fn)(*args, affs0_weight=0.5, **({} if norm5 else {"shift": 2}))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - want_loss.item()) <= LOSS_RTOL * abs(want_loss.item())
    assert float((affs - want_affs).abs().max()) < AFFS_ATOL
    assert relmax(y.grad, x.grad) < GRAD_RTOL
