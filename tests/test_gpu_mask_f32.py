"""GPU (-m gpu): float32 loss masks (PEA_FLAG_MASK_F32) through the public API.

A float32 mask goes to the fused forward kernels as it is.  Two contracts:
  * a float mask of 0.0 / 1.0 computes exactly what the u8 mask of the same values computes, on every kernel family (torch.equal);
  * a fractional mask gives the reference's loss and gradient (`affs * mask`, `target * mask` after `mask.float()`), held to the
    float64 torch restatement of the oracle at the parity tests' tolerances.
"""
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-5, 1e-4
GRAD_RTOL_16 = 8e-3  # (16-bit storage: the stored gradient is rounded once, test_gpu_bf16.py)


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


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _offs(pkg, name):
    return {"cross": pkg.multi_offset([1, 3, 5, 9, 27], 4), "cross8": pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8],
            "diag": pkg.multi_offset([1, 3, 9], 8)}[name]


def _frac_mask(shape, dev, seed):
    """U(0, 1), with exact 0, 0.25, 0.5, 1 and 1.5 values sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape, generator=g)
    pick = torch.randint(0, 8, shape, generator=g)
    for v, c in ((0.0, 0), (0.25, 1), (0.5, 2), (1.0, 3), (1.5, 4)):
        m = torch.where(pick == c, torch.full_like(m, v), m)
    return m.to(dev)


# (D, storage dtype, stencil, H, W, PEA_FORCE_DIRECT): the cross kernels at D = 16 / 32 / 64 (f32 and 16-bit storage), the tiled
# kernels (a diagonal stencil), the chunked kernel (D = 64, diagonal), the direct kernels
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
}


def _run(pkg, E, T, W, M, offsets, ema=None):
    x = E.detach().clone().requires_grad_(True)
    crit = pkg.WeightedMSE()
    if ema is None:
        loss, affs, parts = pkg.embedding_loss(x, T, W, M, crit, offsets)
        parts = parts.tensor  # (the LossList's device tensor: K un-weighted per-offset losses)
    else:
        loss, affs = pkg.ema_embedding_loss(x, ema, T, W, M, crit, offsets)
        parts = None
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), affs.detach(), parts, x.grad


@pytest.fixture
def switch(pkg):
    yield pkg._lib.set_switch
    pkg._lib.set_switch("PEA_FORCE_DIRECT", None)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("cross", [False, True])
def test_binary_float_mask_equals_u8(pkg, dev, synth, switch, case, cross):
    D, dt, sname, H, W, direct = CASES[case]
    offsets = _offs(pkg, sname)
    e, t, w, m = synth.synth_inputs_2d(2, D, H, W, offsets, 900 + D + H)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt = cu(e, dev).to(dt), cu(t, dev), cu(w, dev)
    ema = cu(synth.synth_embedding((2, D, H, W), 901), dev).to(dt) if cross else None
    M8 = cu(m, dev)
    Mf = M8.float()
    a = _run(pkg, E, T, Wt, M8, offsets, ema)
    b = _run(pkg, E, T, Wt, Mf, offsets, ema)
    for x, y in zip(a, b):
        if x is not None:
            assert torch.equal(x, y), case


def _oracle(orc, E, T, W, M, offsets, ema=None):
    x = E.detach().double().requires_grad_(True)
    loss, affs, parts = orc.torch_embedding_loss(x, T.double(), W.double(), M.double(), offsets,
                                                 ema=None if ema is None else ema.double())
    loss.backward()
    return loss.detach(), affs, torch.stack([p.detach() for p in parts]), x.grad


@pytest.mark.parametrize("case", ["xdma_d16", "xdma_d32", "xdma_h_d32_bf16", "tiled_d16", "chunked_d64", "direct_d16"])
@pytest.mark.parametrize("cross", [False, True])
def test_fractional_mask_matches_reference(pkg, dev, orc, synth, switch, case, cross):
    """fractional values are honoured (today's u8 conversion truncated them to 0 / 1)"""
    D, dt, sname, H, W, direct = CASES[case]
    offsets = _offs(pkg, sname)
    e, t, w, _ = synth.synth_inputs_2d(2, D, H, W, offsets, 700 + D + H)
    if direct:
        switch("PEA_FORCE_DIRECT", "1")
    E, T, Wt = cu(e, dev).to(dt), cu(t, dev), cu(w, dev)
    M = _frac_mask(T.shape, dev, 5 + D)
    ema = cu(synth.synth_embedding((2, D, H, W), 702), dev).to(dt) if cross else None
    loss, affs, parts, grad = _run(pkg, E, T, Wt, M, offsets, ema)
    o_loss, o_affs, o_parts, o_grad = _oracle(orc, E.float(), T, Wt, M, offsets, None if ema is None else ema.float())
    assert abs(loss.item() - o_loss.item()) <= LOSS_RTOL * abs(o_loss.item()), case
    if parts is not None:
        assert relmax(parts, o_parts) < LOSS_RTOL, case
    if not cross:
        assert float((affs.double().cpu() - o_affs.double().cpu()).abs().max()) < AFFS_ATOL
    assert relmax(grad, o_grad) < (GRAD_RTOL if dt == torch.float32 else GRAD_RTOL_16), case
    # and the u8 truncation would have been visibly wrong here
    t_loss = _run(pkg, E, T, Wt, M.to(torch.uint8), offsets, ema)[0]
    assert abs(t_loss.item() - o_loss.item()) > 1e-3 * abs(o_loss.item())


def _section_inputs(synth, offsets, nb_half, B, D, H, W, seed, frac):
    e, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, seed)
    ema = synth.synth_embedding((B, D, H, W), seed + 1)
    rng = np.random.default_rng(seed)
    if frac:
        m = rng.random(m.shape).astype(np.float32)
    emds, downs = [], []
    for j in range(4):
        k = nb_half * (4 - j)
        h, ww = H >> (j + 1), W >> (j + 1)
        ej, tj, wj, mj = synth.synth_inputs_2d(B, D, h, ww, offsets[:k], seed + 2 + j)
        mj = rng.random(mj.shape).astype(np.float32) if frac else mj.astype(np.float32)
        emds.append(ej)
        downs.append(np.concatenate([tj, wj, mj], axis=1))  # packed thirds, the mask as float (scripts_cvppp/main.py:284-287)
    return e, ema, t, w, m, emds, downs


def _section(pkg, dev, inputs, nb_half, offsets, composed=False, u8=False):
    e, ema, t, w, m, emds, downs = inputs
    et = cu(e, dev).requires_grad_(True)
    emd_t = [cu(x, dev).requires_grad_(True) for x in emds]
    down_t = [cu(x, dev) for x in downs]
    mt = cu(m, dev)
    if u8:
        mt = mt.to(torch.uint8)
        down_t = [(d, d[:, 2 * nb_half * (4 - j):].to(torch.uint8)) for j, d in enumerate(down_t)]
    kw = dict(deep_weight=2, self_emb=0.7, cross_emb=1.3)
    if composed:
        # (cvppp_loss_section_composed takes the masks from the packed tensors: its statements with u8 thirds instead)
        loss, pred, _ = _composed_u8(pkg, et, emd_t, cu(ema, dev), cu(t, dev), cu(w, dev), mt, down_t, offsets, nb_half, **kw)
    else:
        loss, pred, _ = pkg.cvppp_loss_section(et, emd_t, cu(ema, dev), cu(t, dev), cu(w, dev), mt, down_t, pkg.WeightedMSE(), offsets,
                                               nb_half, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), pred.detach(), et.grad, [x.grad for x in emd_t]


def _composed_u8(pkg, et, emd_t, ema, t, w, m, down_t, offsets, nb_half, deep_weight, self_emb, cross_emb):
    """cvppp_loss_section_composed's statements (scripts_cvppp/main.py:284-310) with the deep-supervision masks as u8 tensors"""
    crit = pkg.WeightedMSE()
    dwf = pkg.deep_weight_factor(deep_weight)
    losses = []
    for j, (emd, (down, m8)) in enumerate(zip(emd_t, down_t)):
        k = nb_half * (4 - j)
        losses.append(pkg.embedding_loss(emd, down[:, 0:k], down[:, k:2 * k], m8, crit, offsets[:k])[0])
    le, pred, _ = pkg.embedding_loss(et, t, w, m, crit, offsets)
    lx, _ = pkg.ema_embedding_loss(et, ema, t, w, m, crit, offsets)
    loss = (sum(losses[j] * dwf[j + 1] for j in range(4)) + le * dwf[0]) * self_emb + lx * dwf[0] * cross_emb
    return loss, pred, None


def test_section_packed_binary_float_masks(pkg, dev, synth):
    """cvppp_loss_section on packed float downN tensors (mask thirds are channel slices, taken without a copy) agrees with the
    call-by-call composition given the same values as u8 masks"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half = 2
    inputs = _section_inputs(synth, offsets, nb_half, 2, 16, 96, 96, 61, frac=False)
    inputs = inputs[:4] + (inputs[4].astype(np.float32),) + inputs[5:]
    a = _section(pkg, dev, inputs, nb_half, offsets)
    b = _section(pkg, dev, inputs, nb_half, offsets, composed=True, u8=True)
    assert abs(a[0].item() - b[0].item()) <= LOSS_RTOL * abs(b[0].item())
    assert float((a[1] - b[1]).abs().max()) < AFFS_ATOL
    assert relmax(a[2], b[2]) < GRAD_RTOL
    for x, y in zip(a[3], b[3]):
        assert relmax(x, y) < GRAD_RTOL


def test_section_packed_fractional_masks(pkg, dev, orc, synth):
    """fractional mask thirds: the section against a float64 restatement of scripts_cvppp/main.py:284-310, call by call"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    nb_half = 2
    inputs = _section_inputs(synth, offsets, nb_half, 2, 16, 96, 96, 63, frac=True)
    loss, pred, g_e, g_emd = _section(pkg, dev, inputs, nb_half, offsets)
    e, ema, t, w, m, emds, downs = inputs
    d64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    dwf = pkg.deep_weight_factor(2)
    x = d64(e).requires_grad_(True)
    xs = [d64(a).requires_grad_(True) for a in emds]
    ls = []
    for j in range(4):
        k = nb_half * (4 - j)
        dj = d64(downs[j])
        ls.append(orc.torch_embedding_loss(xs[j], dj[:, :k], dj[:, k:2 * k], dj[:, 2 * k:], offsets[:k])[0])
    le = orc.torch_embedding_loss(x, d64(t), d64(w), d64(m), offsets)[0]
    lx = orc.torch_embedding_loss(x, d64(t), d64(w), d64(m), offsets, ema=d64(ema))[0]
    want = (sum(ls[j] * dwf[j + 1] for j in range(4)) + le * dwf[0]) * 0.7 + lx * dwf[0] * 1.3
    want.backward()
    assert abs(loss.item() - want.item()) <= LOSS_RTOL * abs(want.item())
    assert relmax(g_e, x.grad) < GRAD_RTOL
    for a, b in zip(g_emd, xs):
        assert relmax(a, b.grad) < GRAD_RTOL


def test_graphed_step_with_float_mask(pkg, dev, synth):
    """pea.graphed of a training step with a float mask replays to the eager step's values"""
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    e, t, w, _ = synth.synth_inputs_2d(2, 16, 128, 128, offsets, 31)
    e2 = synth.synth_embedding((2, 16, 128, 128), 32)
    E, T, W = cu(e, dev).requires_grad_(True), cu(t, dev), cu(w, dev)
    M = _frac_mask(T.shape, dev, 33)
    crit = pkg.WeightedMSE()

    def step(E, T, W, M):
        E.grad = None
        loss, affs, _ = pkg.embedding_loss(E, T, W, M, crit, offsets)
        pkg.backward(loss)
        return loss, affs, E.grad

    def eager(ev):
        x = cu(ev, dev).requires_grad_(True)
        loss, affs, _ = pkg.embedding_loss(x, T, W, M, crit, offsets)
        pkg.backward(loss)
        return loss.detach().clone(), affs.clone(), x.grad.clone()

    g = pkg.graphed(step, E, T, W, M)
    for ev in (e, e2):
        with torch.no_grad():
            E.copy_(cu(ev, dev))
        loss, affs, grad = g.replay()
        l0, a0, g0 = eager(ev)
        assert torch.equal(loss, l0) and torch.equal(affs, a0) and torch.equal(grad, g0)
