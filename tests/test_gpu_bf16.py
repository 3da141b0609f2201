"""GPU (-m gpu): bfloat16 embedding storage (PEA_BF16) through the public API.

The contract is the f16 one: the embedding is stored in bf16, every load widens to f32, all arithmetic is f32, affs / target / weight /
1/norm stay f32 and the gradient comes back in bf16, rounded once (to nearest even) from the f32 value.  The reference for every check
is the f32 path -- itself held to the reference's golden vectors and the CPU oracle by test_gpu_parity.py -- run on exactly the rounded
inputs (`x.to(torch.bfloat16).float()`).

Tolerances: affs abs 1e-5, loss rel 1e-5, gradient rel-to-max 8e-3 (bf16 rounding of the stored gradient), and per element within one
bf16 ulp of the f32 gradient rounded to bf16 (test_rounding_contract_*).
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-5, 8e-3
G2D = [n for n in golden_names("g2d_") if "summary" not in n]
G3D = [n for n in golden_names("g3d_") if "march" not in n]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bf(a, dev):
    """numpy f32 -> (bf16 tensor, the f32 tensor of the same rounded values) on dev"""
    x = cu(a, dev).to(torch.bfloat16)
    return x, x.float()


def relmax(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _mono(x):
    """bf16 bit patterns -> integers ordered like the values (+0 and -0 both 0): adjacent bf16 numbers differ by 1"""
    u = x.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(u >= 0x8000, -(u & 0x7FFF), u)


def assert_within_one_ulp(g16, g32):
    """g16 (bf16) within one bf16 ulp of g32.to(bf16) at every element.  Where |g32| is below 2^-16 of the largest element, two f32
    computations of it in different orders may already differ by more than a bf16 ulp of so small a value: there the f32 reordering
    bound 2^-20 * max|g32| is accepted instead."""
    assert g16.dtype == torch.bfloat16 and g32.dtype == torch.float32
    d = (_mono(g16) - _mono(g32.to(torch.bfloat16))).abs()
    gmax = float(g32.abs().max())
    small = g32.abs() < gmax * 2.0 ** -16
    assert int(d[~small].max()) <= 1 if (~small).any() else True
    far = (d > 1) & ((g16.float() - g32).abs() > gmax * 2.0 ** -20)
    assert int(far.sum()) == 0, "%d elements beyond one bf16 ulp" % int(far.sum())


def cross(pkg, spec, e, mode):
    op = pkg.affinity_op
    return op.cross_supported(op.make_desc(spec, e), mode)


def check_pair(r16, r32, grad_ulp=True):
    """r = (loss, affs, [grads]) from the bf16 and the f32 run on the same rounded values"""
    l16, a16, g16 = r16
    l32, a32, g32 = r32
    assert a16.dtype == torch.float32
    assert float((a16 - a32).abs().max()) < AFFS_ATOL
    assert abs(float(l16) - float(l32)) <= LOSS_RTOL * max(abs(float(l32)), 1e-30)
    for x, y in zip(g16, g32):
        assert x.dtype == torch.bfloat16
        assert relmax(x, y) < GRAD_RTOL
        if grad_ulp:
            assert_within_one_ulp(x, y)


# ---- the reference's golden cases, stored in bf16 -------------------------------------------------------------------------

def _run_golden(pkg, g, dev, x, ema):
    e = x.clone().requires_grad_(True)
    crit = pkg.WeightedMSE()
    kind = str(g["kind"])
    ema_t = None
    if ema is not None:
        ema_t = ema.clone().requires_grad_("detach" in g and not bool(g["detach"]))
    t, w = cu(g["target"], dev), cu(g["weight"], dev)
    if kind.startswith("2d"):
        offsets, m = g["offsets"].tolist(), cu(g["mask"], dev)
        mode = str(g["mode"]) if "mode" in g else "ours"
        if kind == "2d_ema":
            loss, affs = pkg.ema_embedding_loss(e, ema_t, t, w, m, crit, offsets, affs0_weight=float(g["affs0_weight"]))
        else:
            loss, affs, _ = pkg.embedding_loss(e, t, w, m, crit, offsets, mode=mode)
    else:
        a0, sh = float(g["affs0_weight"]), int(g["shift"])
        if kind == "3d_norm1":
            loss, affs = pkg.embedding_loss_norm1(e, t, w, crit, affs0_weight=a0, shift=sh)
        elif kind == "3d_norm5":
            loss, affs = pkg.embedding_loss_norm5(e, t, w, crit, affs0_weight=a0)
        elif kind == "3d_norm1_ema":
            loss, affs = pkg.ema_embedding_loss_norm1(e, ema_t, t, w, crit, affs0_weight=a0, shift=sh)
        else:
            loss, affs = pkg.ema_embedding_loss_norm5(e, ema_t, t, w, crit, affs0_weight=a0)
    loss.backward()
    grads = [e.grad] + ([ema_t.grad] if ema_t is not None and ema_t.requires_grad else [])
    return loss.detach(), affs.detach(), grads


@pytest.mark.parametrize("name", G2D + G3D)
def test_golden_cases_in_bf16(pkg, dev, name):
    g = load_golden(name)
    x16, x32 = bf(g["e"], dev)
    m16, m32 = bf(g["ema"], dev) if "ema" in g else (None, None)
    r16 = _run_golden(pkg, g, dev, x16, m16)
    r32 = _run_golden(pkg, g, dev, x32, m32)
    check_pair(r16, r32)
    if "affs_infer" in g and str(g["kind"]).startswith("2d"):
        mode = str(g["mode"]) if "mode" in g else "ours"
        offsets = g["offsets"].tolist()
        i16 = pkg.embedding2affs(x16, offsets, mode=mode)
        assert i16.dtype == torch.float32
        assert float((i16 - pkg.embedding2affs(x32, offsets, mode=mode)).abs().max()) < AFFS_ATOL


# ---- the rounding contract on the cross kernels and on the fallbacks ------------------------------------------------------

def _self_loss(pkg, x, t, w, m, spec):
    e = x.clone().requires_grad_(True)
    loss, affs = pkg.affinity_op.FusedAffinityMSE.apply(e, None, t, w, m, spec)[:2]
    (loss * 0.5).backward()
    return loss.detach(), affs.detach(), [e.grad]


@pytest.mark.parametrize("path", ["cross", "tiled", "direct"])
@pytest.mark.parametrize("D,H,W,border", [(16, 544, 544, 0), (16, 544, 544, 1), (64, 136, 200, 0)])
def test_rounding_contract(pkg, dev, synth, monkeypatch, path, D, H, W, border):
    """544^2 K = 10 (circular and CROP_ZERO) and D = 64 with offsets[:8]: on the LDS-DMA cross kernels (pea_xdma_h16.h), on the
    tiled kernels (PEA_FWD_XDMA=0 PEA_BWD_XDMA=0) and on the direct kernels (PEA_FORCE_DIRECT=1)"""
    if path == "tiled":
        monkeypatch.setenv("PEA_FWD_XDMA", "0")
        monkeypatch.setenv("PEA_BWD_XDMA", "0")
    elif path == "direct":
        monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
    op = pkg.affinity_op
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    if D == 64:
        offsets = offsets[:8]
    B = 2
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, 301 + D + border)
    x16, x32 = bf(e, dev)
    spec = op.AffinitySpec(2, offsets, None, border, pkg._lib.NORM_BX)
    on_cross = cross(pkg, spec, x16, 0) and cross(pkg, spec, x16, 1)
    assert on_cross == (path == "cross")
    T, Wt, M = cu(t, dev), cu(w, dev), cu(m, dev)
    check_pair(_self_loss(pkg, x16, T, Wt, M, spec), _self_loss(pkg, x32, T, Wt, M, spec))


def test_configs4_full_size(pkg, dev, synth):
    """BASELINE configs[4] in bf16: B=8 x 64 x 544^2, offsets[:8], on the cross kernels"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8]
    e, t, w, m = synth.synth_inputs_2d(8, 64, 544, 544, offsets, 311)
    x16, x32 = bf(e, dev)
    del e
    T, Wt, M = cu(t, dev), cu(w, dev), cu(m, dev)
    spec = pkg.affinity_op.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    assert cross(pkg, spec, x16, 0) and cross(pkg, spec, x16, 1)
    r16 = _self_loss(pkg, x16, T, Wt, M, spec)
    r32 = _self_loss(pkg, x32, T, Wt, M, spec)
    check_pair(r16, r32)
    # two runs are bit-identical
    r16b = _self_loss(pkg, x16, T, Wt, M, spec)
    assert torch.equal(r16[0], r16b[0]) and torch.equal(r16[1], r16b[1]) and torch.equal(r16[2][0], r16b[2][0])


def test_d32_704_and_inference_relu(pkg, dev, synth):
    """BASELINE configs[2] shape in bf16 (D = 32, 704^2) on the cross kernels; inference with the relu epilogue"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 11], 4)
    e, t, w, m = synth.synth_inputs_2d(1, 32, 704, 704, offsets, 321)
    x16, x32 = bf(e, dev)
    spec = pkg.affinity_op.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    assert cross(pkg, spec, x16, 0) and cross(pkg, spec, x16, 1)
    T, Wt, M = cu(t, dev), cu(w, dev), cu(m, dev)
    check_pair(_self_loss(pkg, x16, T, Wt, M, spec), _self_loss(pkg, x32, T, Wt, M, spec))
    a16 = pkg.embedding2affs(x16, offsets, activation="relu")
    a32 = pkg.embedding2affs(x32, offsets, activation="relu")
    assert a16.dtype == torch.float32 and float(a16.min()) >= 0.0
    assert float((a16 - a32).abs().max()) < AFFS_ATOL


@pytest.mark.parametrize("D,H,W", [(16, 256, 320), (32, 200, 256), (64, 136, 200)])
def test_ema_cross_loss_detached_bf16(pkg, dev, synth, D, H, W):
    """ema_embedding_loss with a detached bf16 second operand: the role-A cross kernels (k_fwd_xdma_h / k_bwd_xdma_h <.., OTHER>)"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    if D == 64:
        offsets = offsets[:8]
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 331 + D)
    x16, x32 = bf(e, dev)
    m16, m32 = bf(synth.synth_embedding((2, D, H, W), 332 + D), dev)
    spec = pkg.affinity_op.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    assert cross(pkg, spec, x16, 2)
    T, Wt, M = cu(t, dev), cu(w, dev), cu(m, dev)

    def run(x, ema):
        xe = x.clone().requires_grad_(True)
        loss, affs = pkg.ema_embedding_loss(xe, ema.detach(), T, Wt, M, pkg.WeightedMSE(), offsets, affs0_weight=2)
        loss.backward()
        return loss.detach(), affs.detach(), [xe.grad]
    check_pair(run(x16, m16), run(x32, m32))
    # a mixed pair keeps the .to(e.dtype) rule: an f32 second operand is rounded to bf16 first
    check_pair(run(x16, m32), run(x32, m16.float()))


# ---- shapes that fall back to the generic kernels ------------------------------------------------------------------------

def test_fallback_odd_width(pkg, dev, synth):
    """X % 8 != 0: the tiled kernels"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    e, t, w, m = synth.synth_inputs_2d(2, 16, 96, 132, offsets, 341)
    x16, x32 = bf(e, dev)
    spec = pkg.affinity_op.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    assert not cross(pkg, spec, x16, 0)
    T, Wt, M = cu(t, dev), cu(w, dev), cu(m, dev)
    check_pair(_self_loss(pkg, x16, T, Wt, M, spec), _self_loss(pkg, x32, T, Wt, M, spec))


def test_fallback_generic_d5(pkg, dev):
    """D = 5: the direct forward and the runtime-D backward"""
    g = load_golden("g2d_d5_generic")
    offsets = g["offsets"].tolist()
    x16, x32 = bf(g["e"], dev)
    T, Wt, M = cu(g["target"], dev), cu(g["weight"], dev), cu(g["mask"], dev)

    def run(x):
        xe = x.clone().requires_grad_(True)
        loss, affs, _ = pkg.embedding_loss(xe, T, Wt, M, pkg.WeightedMSE(), offsets)
        loss.backward()
        return loss.detach(), affs.detach(), [xe.grad]
    check_pair(run(x16), run(x32))


@pytest.mark.parametrize("ema", [False, True])
def test_fallback_ac3ac4_norm5(pkg, dev, synth, ema):
    """AC3/AC4 crops, 18 x 160 x 160, norm5 (and the EMA form), inference included"""
    B, D, Z, Y, X = 1, 16, 18, 160, 160
    x16, x32 = bf(synth.synth_embedding((B, D, Z, Y, X), 351), dev)
    m16, m32 = bf(synth.synth_embedding((B, D, Z, Y, X), 352), dev)
    t = cu((np.random.RandomState(353).rand(B, 12, Z, Y, X) > 0.5).astype(np.float32), dev)
    w = cu(np.random.RandomState(354).rand(B, 12, Z, Y, X).astype(np.float32) + 0.5, dev)

    def run(x, m):
        xe = x.clone().requires_grad_(True)
        if ema:
            loss, affs = pkg.ema_embedding_loss_norm5(xe, m.detach(), t, w, pkg.WeightedMSE(), affs0_weight=2)
        else:
            loss, affs = pkg.embedding_loss_norm5(xe, t, w, pkg.WeightedMSE(), affs0_weight=2)
        loss.backward()
        return loss.detach(), affs.detach(), [xe.grad]
    check_pair(run(x16, m16), run(x32, m32))
    if not ema:
        i16 = pkg.inf_embedding_loss_norm5(x16)
        assert float((i16 - pkg.inf_embedding_loss_norm5(x32)).abs().max()) < AFFS_ATOL


@pytest.mark.parametrize("name", golden_names("g3r_norm6"))
def test_fallback_norm6(pkg, dev, name):
    """PEA_BORDER_REPLICATE (embedding_loss_norm6 / ema_embedding_loss_norm6), a non-detached EMA operand included"""
    g = load_golden(name)
    offs = [list(map(int, o)) for o in g["offsets"]]
    x16, x32 = bf(g["e"], dev)
    m16, m32 = bf(g["ema"], dev) if "ema" in g else (None, None)
    T, Wt = cu(g["target"], dev), cu(g["weight"], dev)

    def run(x, m):
        xe = x.clone().requires_grad_(True)
        if m is not None:
            mt = m.clone().requires_grad_("grad_ema" in g)
            loss, affs = pkg.ema_embedding_loss_norm6(xe, mt, T, Wt, pkg.WeightedMSE(), shift=offs)
        else:
            mt = None
            loss, affs = pkg.embedding_loss_norm6(xe, T, Wt, pkg.WeightedMSE(), shift=offs)
        loss.backward()
        return loss.detach(), affs.detach(), [xe.grad] + ([mt.grad] if mt is not None and mt.requires_grad else [])
    check_pair(run(x16, m16), run(x32, m32))


@pytest.mark.parametrize("ema", [False, True])
def test_fallback_labels_in(pkg, dev, synth, ema):
    """the labels-in step (pea_affinity_fwd_bwd_labels) in bf16 against the same step on the rounded values in f32"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    B, D, H, W = 3, 16, 80, 136
    lab_t = torch.from_numpy(synth.synth_labels(B, (1, H, W), 361, cell=11)[:, 0]).to(dev)
    x16, x32 = bf(synth.synth_embedding((B, D, H, W), 362), dev)
    m16, m32 = bf(synth.synth_embedding((B, D, H, W), 363), dev)
    crit = pkg.WeightedMSE()

    def run(x, m):
        xe = x.clone().requires_grad_(True)
        if ema:
            loss, affs = pkg.ema_embedding_loss_from_labels(xe, m, lab_t, crit, offsets, affs0_weight=2)
        else:
            loss, affs, _ = pkg.embedding_loss_from_labels(xe, lab_t, crit, offsets)
        (loss * 0.5).backward()
        return loss.detach(), affs.detach(), [xe.grad]
    check_pair(run(x16, m16), run(x32, m32))


# ---- loss sections, graphs, tiny magnitudes ------------------------------------------------------------------------------

def _section_inputs(synth, offsets, nb_half, B, D, H, W, seed):
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, seed)
    ema = synth.synth_embedding((B, D, H, W), seed + 1)
    emds, downs = [], []
    for j in range(4):
        k = nb_half * (4 - j)
        ej, tj, wj, mj = synth.synth_inputs_2d(B, D, H >> (j + 1), W >> (j + 1), offsets[:k], seed + 2 + j)
        emds.append(ej)
        downs.append(np.concatenate([tj, wj, mj.astype(np.float32)], axis=1))
    return e, ema, t, w, m, emds, downs


@pytest.mark.parametrize("which", ["node", "composed", "from_labels"])
def test_cvppp_loss_section_bf16(pkg, dev, synth, which):
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half, B, D, H, W = 2, 2, 16, 96, 96
    e, ema, t, w, m, emds, downs = _section_inputs(synth, offsets, nb_half, B, D, H, W, 371)
    crit = pkg.WeightedMSE()
    labs = [torch.from_numpy(synth.synth_labels(B, (1, H >> j, W >> j), 372 + j, cell=11)[:, 0]).to(dev) for j in range(5)]

    def run(dtype):
        et = cu(e, dev).to(dtype).requires_grad_(True)
        emd_t = [cu(x, dev).to(dtype).requires_grad_(True) for x in emds]
        ema_t = cu(ema, dev).to(dtype)
        if which == "from_labels":
            loss, pred, _ = pkg.cvppp_loss_section_from_labels(et, emd_t, ema_t, labs[0], labs[1:], crit, offsets, nb_half,
                                                               deep_weight=2, self_emb=0.7, cross_emb=1.3)
        else:
            fn = pkg.cvppp_loss_section if which == "node" else pkg.cvppp_loss_section_composed
            loss, pred, _ = fn(et, emd_t, ema_t, cu(t, dev), cu(w, dev), cu(m, dev), [cu(x, dev) for x in downs], crit, offsets, nb_half,
                               deep_weight=2, self_emb=0.7, cross_emb=1.3)
        (loss * 0.5).backward()
        return loss.detach(), pred.detach(), [et.grad] + [x.grad for x in emd_t]
    r16 = run(torch.bfloat16)

    # the f32 run on the rounded values
    def rnd(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()
    e, ema, emds = rnd(e), rnd(ema), [rnd(x) for x in emds]
    r32 = run(torch.float32)
    check_pair(r16, r32, grad_ulp=False)


def test_graphed_bf16_equals_eager(pkg, dev, synth):
    """pea.graphed over a bf16 embedding_loss + backward: replay equals eager bit for bit"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    crit = pkg.WeightedMSE()
    e, t, w, m = synth.synth_inputs_2d(1, 16, 544, 544, offsets, seed=381)
    e2 = synth.synth_embedding((1, 16, 544, 544), 382)
    E = cu(e, dev).to(torch.bfloat16).requires_grad_(True)
    T, W, M = cu(t, dev), cu(w, dev), cu(m, dev)

    def step(E, T, W, M):
        E.grad = None
        loss, affs, parts = pkg.embedding_loss(E, T, W, M, crit, offsets)
        pkg.backward(loss)
        return loss, affs, E.grad

    def eager(ev):
        x = cu(ev, dev).to(torch.bfloat16).requires_grad_(True)
        loss, affs, _ = pkg.embedding_loss(x, T, W, M, crit, offsets)
        pkg.backward(loss)
        return loss.detach().clone(), affs.clone(), x.grad.clone()

    g = pkg.graphed(step, E, T, W, M)
    for ev in (e, e2, e):
        with torch.no_grad():
            E.copy_(cu(ev, dev).to(torch.bfloat16))
        loss, affs, grad = g.replay()
        l0, a0, g0 = eager(ev)
        assert grad.dtype == torch.bfloat16
        assert torch.equal(loss, l0) and torch.equal(affs, a0) and torch.equal(grad, g0)


@pytest.mark.parametrize("scale", [1e-20, 1e-30])
def test_tiny_magnitude_embeddings(pkg, dev, orc, synth, scale):
    """bf16 has the f32 exponent range, so these values are normal bf16 numbers (unlike f16, test_f16_denormal_embeddings), but every
    product of two of them is an f32 denormal (1e-20) or below the f32 range (1e-30), and the norms are under eps (the clamp branch of
    F.normalize).  The forward on the cross kernels (v_dot2c_f32_bf16) against the oracle on the same rounded values"""
    op = pkg.affinity_op
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8]
    B, D, H, W = 1, 64, 48, 72
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, 5)
    x16 = cu(e * scale, dev).to(torch.bfloat16)
    ef = x16.float().cpu().numpy()
    spec = op.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    assert cross(pkg, spec, x16, 0)
    d = orc.make_desc(B, D, [1, H, W], offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX, ndim=2)
    o_affs, o_loss = orc.c_fwd(d, ef, None, t, w, m)
    loss, affs, _ = op.FusedAffinityMSE.apply(x16, None, cu(t, dev), cu(w, dev), cu(m, dev), spec)
    assert np.abs(affs.cpu().numpy().reshape(o_affs.shape) - o_affs).max() < AFFS_ATOL
    assert abs(loss.item() - o_loss[0]) <= LOSS_RTOL * o_loss[0]
    inf = op.affinity_infer(x16, None, spec)
    assert np.abs(inf.cpu().numpy().reshape(o_affs.shape) - o_affs).max() < AFFS_ATOL


def test_c_abi_scale_inplace_bf16(pkg, dev):
    """pea_scale_inplace on a bf16 buffer: each element times the scale, rounded once to bf16"""
    x = (torch.randn(1001, device=dev) * 3).to(torch.bfloat16)
    want = (x.float() * 0.37).to(torch.bfloat16)
    sc = torch.tensor([0.37], device=dev)
    L = pkg._lib.lib()
    rc = L.pea_scale_inplace(ctypes.c_void_p(x.data_ptr()), pkg._lib.BF16, ctypes.c_size_t(x.numel()), ctypes.c_void_p(sc.data_ptr()),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(x, want)
