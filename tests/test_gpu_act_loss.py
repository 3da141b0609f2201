"""GPU (-m gpu): the loss on the ACTIVATED affinity map (PEA_FLAG_LOSS_ACT) through the public API.

  * every tests/golden/gal_*.npz fixture (the reference's loss_embedding / loss_embedding_exp / loss_embedding_norm modules, run by
    tests/golden/make_golden_actloss.py) through the package's modules of the same names: loss, map, gradient;
  * a float64 torch restatement of the closed form in include/pea.h (autograd for the gradient) against every kernel family;
  * half shift without clamp == 0.25 x the raw-cosine loss on target' = 2 t - 1 (needs no restatement);
  * a second call is bit-identical; the activation bits without the flag keep the raw-cosine loss.

Tolerances are the existing suites': test_gpu_parity.py (affs 1e-5 abs, loss 1e-5 rel, grad 1e-4 of its max) and, for 16-bit
storage, test_gpu_bf16.py / test_gpu_mask_f32.py (grad 8e-3: the stored gradient is rounded once).

The clamp edge.  Where v (what the clamp sees) lies within rounding of 0 or 1 the f32 kernel and the float64 reference may take
different branches of the clamp's slope, and one such term changes the gradient by its whole size.  No tolerance is loosened for
that: every term whose float64 |v - edge| < 1e-4 gets weight 0 on both sides (the fixtures come that way), and each case asserts
that at most 0.2 % of its terms were dropped.  16-bit cases compute v from the embedding already rounded to the storage type.
"""
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-5, 1e-4
GRAD_RTOL_16 = 8e-3
EDGE, EDGE_MAX_FRACTION = 1e-4, 0.002
HALF, CLAMP, LOSS_ACT = 4, 8, 64
ACTS = {"half_clamp": HALF | CLAMP, "clamp": CLAMP}
GAL = golden_names("gal_")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


@pytest.fixture
def switch(pkg):
    yield pkg._lib.set_switch
    pkg._lib.set_switch("PEA_FORCE_DIRECT", None)


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---- the fixtures -------------------------------------------------------------------------------------------------------------

def _call_module(pkg, g, dev, crit):
    mod = getattr(pkg, str(g["module"]))
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
    assert isinstance(out, tuple) and len(out) == 2  # (loss, affs): the reference's return arity
    out[0].backward()
    torch.cuda.synchronize()
    return out[0].detach(), out[1].detach(), x.grad


def _check_fixture(g, loss, affs, grad, name):
    assert int(g["edge_zeroed"]) <= EDGE_MAX_FRACTION * int(g["terms"]), name
    print("%s: loss %.9g (ref %.9g)  affs max err %.3g  grad rel err %.3g  edge-zeroed %d / %d" % (
        name, loss.item(), float(g["loss"]), float((affs.cpu() - torch.from_numpy(g["affs"])).abs().max()),
        relmax(grad, torch.from_numpy(g["grad"])), int(g["edge_zeroed"]), int(g["terms"])))
    assert abs(loss.item() - float(g["loss"])) <= LOSS_RTOL * abs(float(g["loss"])), name
    assert float((affs.cpu() - torch.from_numpy(g["affs"])).abs().max()) < AFFS_ATOL, name
    assert relmax(grad, torch.from_numpy(g["grad"])) < GRAD_RTOL, name


@pytest.mark.parametrize("name", GAL)
def test_fixture_through_the_public_module(pkg, dev, name):
    """the reference's recorded loss, map and gradient; one fused forward + one backward (WeightedMSE)"""
    g = load_golden(name)
    loss, affs, grad = _call_module(pkg, g, dev, pkg.WeightedMSE())
    _check_fixture(g, loss, affs, grad, name)


def _weighted_mse(pred, target, weight):
    """a foreign criterion (no `pea_fused` attribute) with WeightedMSE's arithmetic: sum(w (p - t)^2) / (B * W)"""
    return torch.sum(weight * (pred - target) ** 2) / (pred.shape[0] * pred.shape[-1])


@pytest.mark.parametrize("name", [n for n in GAL if n in ("gal_emb_ema_w", "gal_exp_self_w", "gal_norm_self_l2", "gal_emb_self_fmask")])
def test_fixture_through_a_foreign_criterion(pkg, dev, name):
    """any other criterion: the raw map's vjp + the activation with torch ops -- the same numbers"""
    g = load_golden(name)
    loss, affs, grad = _call_module(pkg, g, dev, _weighted_mse)
    _check_fixture(g, loss, affs, grad, name)


@pytest.mark.parametrize("name", [n for n in GAL if "ema" not in n])
def test_fixture_inference_half(pkg, dev, name):
    """embedding2affs of the same module gives the loss call's map"""
    g = load_golden(name)
    mod = getattr(pkg, str(g["module"]))
    kw = {"mode": str(g["mode"])} if str(g["mode"]) else {}
    affs = mod.embedding2affs(cu(g["e"], dev), [list(map(int, o)) for o in g["offsets"]], **kw)
    assert float((affs.cpu() - torch.from_numpy(g["affs"])).abs().max()) < AFFS_ATOL


# ---- float64 restatement of the closed form (include/pea.h, PEA_FLAG_LOSS_ACT) ----------------------------------------------------

def _shifted(y, o, border):
    """y [B,D,Z,Y,X] -> (y at p + o, [Z,Y,X] bool: the neighbour exists)"""
    dims = y.shape[2:]
    ok = torch.ones(dims, dtype=torch.bool, device=y.device)
    if border == 0:  # CIRCULAR
        return torch.roll(y, shifts=tuple(-int(v) for v in o), dims=(2, 3, 4)), ok
    out = y
    for ax, v in enumerate(o):
        idx = torch.arange(dims[ax], device=y.device) + int(v)
        inside = (idx >= 0) & (idx < dims[ax])
        out = out.index_select(2 + ax, idx.clamp(0, dims[ax] - 1))
        if border == 1:  # CROP_ZERO
            shape = [1, 1, 1]
            shape[ax] = dims[ax]
            ok = ok & inside.view(shape)
    return out, ok


def _activate64(a, act):
    v = (a + 1) / 2 if act & HALF else a
    return v, (torch.clamp(v, 0.0, 1.0) if act & CLAMP else v)


def _restate(pkg, E, other, T, W, M, offsets3, lam, eps, act, border, norm):
    """-> loss, affs (activated), d loss / d e, v (the clamp's input) in float64; 5D tensors"""
    L = pkg._lib
    x = E.double().requires_grad_(True)
    y = x if other is None else other.double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
    B, dims = x.shape[0], x.shape[2:]
    loss, maps, vs = 0.0, [], []
    for i, o in enumerate(offsets3):
        ys, ok = _shifted(yn, o, border)
        a = (xn * ys).sum(1) * ok
        v, u = _activate64(a, act)
        m = 1.0 if M is None else M[:, i].double()
        r = (u * m - T[:, i].double() * m) * ok
        if norm == L.NORM_BX:
            n = B * dims[2]
        elif norm == L.NORM_FULL:
            n = B * dims[0] * dims[1] * dims[2]
        else:
            n = B * int(np.prod([dims[a_] - abs(int(o[a_])) for a_ in range(3)]))
        loss = loss + lam[i] * (W[:, i].double() * r * r).sum() / n
        maps.append(u.detach())
        vs.append(torch.where(ok, v.detach(), torch.full_like(v.detach(), 0.5)))  # (a cropped pair has no term: never "near an edge")
    loss.backward()
    return loss.detach(), torch.stack(maps, 1), x.grad, torch.stack(vs, 1)


def _drop_edge_terms(pkg, E, other, W, offsets3, eps, act, border):
    """weight = 0 where the float64 |v - edge| < EDGE (clamp only); -> weight, fraction dropped"""
    if not act & CLAMP:
        return W, 0.0
    with torch.enable_grad():
        z = torch.zeros_like(W)
        _, _, _, v = _restate(pkg, E, other, z, z, None, offsets3, [1.0] * len(offsets3), eps, act, border, pkg._lib.NORM_FULL)
    near = ((v.abs() < EDGE) | ((v - 1).abs() < EDGE)).view(W.shape)
    return torch.where(near, torch.zeros_like(W), W), float(near.double().mean())


def _fused(pkg, E, other, T, W, M, offsets, lam, eps, act, ndim=2, border=0, norm=0):
    spec = pkg.AffinitySpec(ndim, offsets, lam, border, norm, eps, False, act)
    x = E.detach().clone().requires_grad_(True)
    loss, affs, parts = pkg.FusedAffinityMSE.apply(x, other, T, W, M, spec)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), affs.detach(), parts.detach(), x.grad


def _offs(pkg, name):
    return {"cross": pkg.multi_offset([1, 3, 5, 9, 27], 4), "cross8": pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8],
            "diag": pkg.multi_offset([1, 3, 9], 8)}[name]


def _frac_mask(shape, dev, seed):
    """U(0, 1), with exact 0, 0.25, 0.5, 1 and 1.5 values sprinkled in (test_gpu_mask_f32.py)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape, generator=g)
    pick = torch.randint(0, 8, shape, generator=g)
    for v, c in ((0.0, 0), (0.25, 1), (0.5, 2), (1.0, 3), (1.5, 4)):
        m = torch.where(pick == c, torch.full_like(m, v), m)
    return m.to(dev)


# the case table of test_gpu_mask_f32.py: (D, storage dtype, stencil, H, W, PEA_FORCE_DIRECT) -- the cross kernels at D = 16 / 32 / 64
# (f32 and 16-bit storage), the tiled kernels (a diagonal stencil), the chunked kernel's shape (D = 64, diagonal: no LOSS_ACT form
# there, the direct kernels take it), the direct kernels
CASES = {
    "xdma_d16": (16, torch.float32, "cross", 128, 128, False),
    "xdma_d32": (32, torch.float32, "cross", 128, 128, False),
    "xdma_h_d32_f16": (32, torch.float16, "cross", 128, 128, False),
    "xdma_h_d32_bf16": (32, torch.bfloat16, "cross", 128, 128, False),
    "xdma_h_d64_f16": (64, torch.float16, "cross8", 128, 128, False),
    "xdma_h_d64_bf16": (64, torch.bfloat16, "cross8", 128, 128, False),
    "tiled_d16": (16, torch.float32, "diag", 96, 128, False),
    "chunked_d64": (64, torch.float32, "diag", 96, 128, False),
    "direct_d16": (16, torch.float32, "cross", 96, 128, True),
    # beyond that table: the D = 64 f32 cross kernel, the tiled kernels at D = 32 and with 16-bit storage
    "xdma_d64": (64, torch.float32, "cross8", 128, 128, False),
    "tiled_d32": (32, torch.float32, "diag", 96, 128, False),
    "tiled_d16_bf16": (16, torch.bfloat16, "diag", 96, 128, False),
}


def _check(tag, got, want, dt, frac, cross=False):
    loss, affs, _, grad = got
    o_loss, o_affs, o_grad = want
    gerr, aerr = relmax(grad, o_grad), float((affs.double() - o_affs.reshape(affs.shape)).abs().max())
    print("%s: loss %.9g (f64 %.9g, rel %.3g)  affs max err %.3g  grad rel err %.3g  edge-dropped %.4f %%" % (
        tag, loss.item(), o_loss.item(), abs(loss.item() - o_loss.item()) / abs(o_loss.item()), aerr, gerr, 100 * frac))
    assert frac <= EDGE_MAX_FRACTION, tag
    assert abs(loss.item() - o_loss.item()) <= LOSS_RTOL * abs(o_loss.item()), tag
    assert aerr < AFFS_ATOL, tag
    assert gerr < (GRAD_RTOL if dt == torch.float32 else GRAD_RTOL_16), tag


@pytest.mark.parametrize("fmask", [False, True], ids=["u8", "f32mask"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("actname", sorted(ACTS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_family_matches_float64(pkg, dev, synth, switch, case, actname, cross, fmask):
    D, dt, sname, H, W, direct = CASES[case]
    act = ACTS[actname]
    offsets = _offs(pkg, sname)
    offsets3 = [[0] + [int(v) for v in o] for o in offsets]
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 300 + D + H + act)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt = cu(e, dev).to(dt), cu(t, dev), cu(w, dev)
    M = _frac_mask(T.shape, dev, 7 + D) if fmask else cu(m, dev)
    ema = cu(synth.synth_embedding((2, D, H, W), 301), dev).to(dt) if cross else None
    lam = [0.5 if i < 2 else 1.0 for i in range(len(offsets))]
    eps = 1e-6
    E5, ema5 = E.float().unsqueeze(2), None if ema is None else ema.float().unsqueeze(2)  # (v from the storage-rounded embedding)
    Wt, frac = _drop_edge_terms(pkg, E5, ema5, Wt.unsqueeze(2), offsets3, eps, act, 0)
    Wt = Wt.squeeze(2).contiguous()
    got = _fused(pkg, E, ema, T, Wt, M, offsets, lam, eps, act | LOSS_ACT)
    o_loss, o_affs, o_grad, _ = _restate(pkg, E5, ema5, T.unsqueeze(2), Wt.unsqueeze(2), M.unsqueeze(2).float(), offsets3, lam, eps, act, 0,
                                         pkg._lib.NORM_BX)
    _check("%s/%s/%s/%s" % (case, actname, "ema" if cross else "self", "f32mask" if fmask else "u8"), got,
           (o_loss, o_affs, o_grad.squeeze(2)), dt, frac)
    # the loss was really taken on the activated map: the raw-cosine loss of the same inputs is another number
    raw = _fused(pkg, E, ema, T, Wt, M, offsets, lam, eps, act)
    assert abs(raw[0].item() - o_loss.item()) > 1e-3 * abs(o_loss.item())
    assert float((raw[1] - got[1]).abs().max()) < AFFS_ATOL  # ... and the stored map is the same activated map either way


CROP_CASES = ["xdma_d16", "xdma_d32", "xdma_d64", "xdma_h_d32_f16", "xdma_h_d32_bf16", "xdma_h_d64_bf16", "tiled_d16", "tiled_d32",
              "tiled_d16_bf16", "direct_d16"]


@pytest.mark.parametrize("fmask", [False, True], ids=["u8", "f32mask"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("actname", sorted(ACTS))
@pytest.mark.parametrize("case", CROP_CASES)
def test_cropped_2d_border_matches_float64(pkg, dev, synth, switch, case, actname, cross, fmask):
    """2D images with PEA_BORDER_CROP_ZERO (the CROP = true forms of every family, the three-workgroup 16-bit form with an f32 mask
    among them): a pair whose neighbour leaves the image has no loss term and no gradient, and its stored value is act(0)"""
    L = pkg._lib
    D, dt, sname, H, W, direct = CASES[case]
    act = ACTS[actname]
    offsets = _offs(pkg, sname)
    offsets3 = [[0] + [int(v) for v in o] for o in offsets]
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 800 + D + H + act)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt = cu(e, dev).to(dt), cu(t, dev), cu(w, dev)
    M = _frac_mask(T.shape, dev, 9 + D) if fmask else cu(m, dev)
    ema = cu(synth.synth_embedding((2, D, H, W), 801), dev).to(dt) if cross else None
    lam = [0.5 if i < 2 else 1.0 for i in range(len(offsets))]
    eps = 1e-6
    E5, ema5 = E.float().unsqueeze(2), None if ema is None else ema.float().unsqueeze(2)
    Wt, frac = _drop_edge_terms(pkg, E5, ema5, Wt.unsqueeze(2), offsets3, eps, act, L.BORDER_CROP_ZERO)
    Wt = Wt.squeeze(2).contiguous()
    got = _fused(pkg, E, ema, T, Wt, M, offsets, lam, eps, act | LOSS_ACT, border=L.BORDER_CROP_ZERO, norm=L.NORM_CROPPED)
    o_loss, o_affs, o_grad, _ = _restate(pkg, E5, ema5, T.unsqueeze(2), Wt.unsqueeze(2), M.unsqueeze(2).float(), offsets3, lam, eps, act,
                                         L.BORDER_CROP_ZERO, L.NORM_CROPPED)
    _check("crop2d/%s/%s/%s/%s" % (case, actname, "ema" if cross else "self", "f32mask" if fmask else "u8"), got,
           (o_loss, o_affs, o_grad.squeeze(2)), dt, frac)


@pytest.mark.parametrize("actname", sorted(ACTS))
@pytest.mark.parametrize("border", ["crop_zero_3d", "replicate_3d"])
def test_direct_only_descriptors(pkg, dev, synth, actname, border):
    """3D volumes at a width no tiled kernel has: CROP_ZERO (D = 12, cropped normaliser) and REPLICATE (D = 8) reach the direct forward only"""
    L = pkg._lib
    act = ACTS[actname]
    if border == "crop_zero_3d":
        D, bcode, norm = 12, L.BORDER_CROP_ZERO, L.NORM_CROPPED
    else:
        D, bcode, norm = 8, L.BORDER_REPLICATE, L.NORM_FULL
    if border == "crop_zero_3d":
        offsets = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [0, 2, -2], [1, 1, 1]]
    else:
        # a clamped border pairs a pixel with ITSELF wherever every non-zero component of the offset is clamped away (a = 1: exactly on the
        # clamp's upper edge): 1 / n of the terms of an offset along one axis of extent n.  Offsets that step along y AND x keep such
        # pairs to the corners' rows (1 / (Y X)), inside the 0.2 % the edge rule allows
        offsets = [[0, -1, -1], [0, 2, -2], [1, 1, 1], [-1, -3, 3], [0, -3, -1], [2, 1, -2], [-2, -1, -1], [0, 1, 3]]
    e, t, w = synth.synth_inputs_3d(2, D, 6, 40, 48, offsets, 40 + D)
    E, T, Wt = cu(e, dev), cu(t, dev), cu(w, dev)
    lam = [2.0 if i < 3 else 1.0 for i in range(len(offsets))]
    eps = 1e-12
    Wt, frac = _drop_edge_terms(pkg, E, None, Wt, offsets, eps, act, bcode)
    got = _fused(pkg, E, None, T, Wt, None, offsets, lam, eps, act | LOSS_ACT, ndim=3, border=bcode, norm=norm)
    o_loss, o_affs, o_grad, _ = _restate(pkg, E, None, T, Wt, None, offsets, lam, eps, act, bcode, norm)
    _check("%s/%s" % (border, actname), got, (o_loss, o_affs, o_grad), torch.float32, frac)


# ---- identities -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["xdma_d16", "xdma_d32", "xdma_h_d32_bf16", "tiled_d16", "direct_d16"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "ema"])
def test_half_shift_is_a_quarter_of_the_raw_loss(pkg, dev, synth, switch, case, cross):
    """no clamp: r = ((a + 1) / 2 - t) m = (a - (2 t - 1)) m / 2, so loss = L_raw(target' = 2 t - 1) / 4 and so is its gradient"""
    D, dt, sname, H, W, direct = CASES[case]
    offsets = _offs(pkg, sname)
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 500 + D + H)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt, M = cu(e, dev).to(dt), cu(t, dev), cu(w, dev), cu(m, dev)
    ema = cu(synth.synth_embedding((2, D, H, W), 501), dev).to(dt) if cross else None
    lam = [1.0] * len(offsets)
    a = _fused(pkg, E, ema, T, Wt, M, offsets, lam, 1e-6, HALF | LOSS_ACT)
    b = _fused(pkg, E, ema, 2 * T - 1, Wt, M, offsets, lam, 1e-6, 0)
    assert abs(a[0].item() - 0.25 * b[0].item()) <= LOSS_RTOL * abs(0.25 * b[0].item())
    assert relmax(a[2], 0.25 * b[2]) < LOSS_RTOL
    assert relmax(a[3].float(), 0.25 * b[3].float()) < (GRAD_RTOL if dt == torch.float32 else GRAD_RTOL_16)
    assert float((a[1] - (b[1] + 1) / 2).abs().max()) < AFFS_ATOL


@pytest.mark.parametrize("case", sorted(CASES))
def test_second_call_is_bit_identical(pkg, dev, synth, switch, case):
    D, dt, sname, H, W, direct = CASES[case]
    offsets = _offs(pkg, sname)
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 600 + D)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt, M = cu(e, dev).to(dt), cu(t, dev), cu(w, dev), cu(m, dev)
    lam = [1.0] * len(offsets)
    a = _fused(pkg, E, None, T, Wt, M, offsets, lam, 1e-6, CLAMP | LOSS_ACT)
    b = _fused(pkg, E, None, T, Wt, M, offsets, lam, 1e-6, CLAMP | LOSS_ACT)
    for x, y in zip(a, b):
        assert torch.equal(x, y), case


@pytest.mark.parametrize("case", ["xdma_d16", "xdma_h_d32_f16", "tiled_d16", "direct_d16"])
def test_activation_bits_without_the_flag_keep_the_raw_loss(pkg, dev, synth, switch, case):
    """HALF_SHIFT | CLAMP01 alone still only changes the stored map: loss and per-offset losses equal the plain call's bit for bit, the
    gradient to rounding (with an activation the backward does not take the kernels that read the raw map)"""
    D, dt, sname, H, W, direct = CASES[case]
    offsets = _offs(pkg, sname)
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 650 + D)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt, M = cu(e, dev).to(dt), cu(t, dev), cu(w, dev), cu(m, dev)
    lam = [1.0] * len(offsets)
    a = _fused(pkg, E, None, T, Wt, M, offsets, lam, 1e-12, HALF | CLAMP)
    b = _fused(pkg, E, None, T, Wt, M, offsets, lam, 1e-12, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert relmax(a[3].float(), b[3].float()) < (GRAD_RTOL if dt == torch.float32 else GRAD_RTOL_16)
    assert torch.equal(a[1], torch.clamp((b[1] + 1.0) * 0.5, 0.0, 1.0))


def test_graphed_step(pkg, dev, synth):
    """pea.graphed of a training step on the activated-map loss replays to the eager step's values"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    e, t, w, m = synth.synth_inputs_2d(2, 16, 128, 128, offsets, 71)
    E, T, W, M = cu(e, dev).requires_grad_(True), cu(t, dev), cu(w, dev), cu(m, dev)
    crit = pkg.WeightedMSE()

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
