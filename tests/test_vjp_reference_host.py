"""CPU: the float64 vjp of tests/vjp_reference.py and the upstream gradient of make_g, which tests/test_gpu_vjp.py holds every backward
family to.  This file validates the REFERENCE, not the kernels.

At 2 x 16 x 3 x 20 x 40 with three unit steps, three longer negative ones and +9 along y and x (every offset crops at least one pair),
CIRCULAR and CROP_ZERO, one zero-norm pixel:

    (a) own-g identity   with g_i = lambda_i 2 w m (a m - t m) / N_i built from cosine_loss's own map, vjp(...) is cosine_loss(...)["de"]:
                         <= 1e-12 of max (3e-16 measured).  Under CROP_ZERO that g is NOT zero on the cropped pairs (a = 0, t != 0): the
                         selects of the vjp drop them as the loss does
    (b) poison invariance  vjp(G) and vjp(G_alt) are torch.equal under CROP_ZERO
    (c) noise floor      the same vjp evaluated in float32 torch differs from float64 by 2e-7 of max at K = 8 (measured): < 1e-5, so the
                         standing 1e-4 GPU tolerance sits far above the f32 noise floor for this G distribution
    (d) make_g           no zero, no non-finite value, the poison exactly on the ~ok set of shifted
"""
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from cross_stencils import lambdas, relmax
from f64_reference import BORDER_CIRCULAR, BORDER_CROP_ZERO, cosine_loss, normaliser, shifted
from vjp_reference import POISON, POISON_ALT, gone_mask, make_g, vjp

B, D, DIMS, EPS, DLOSS = 2, 16, (3, 20, 40), 1e-12, 0.625
O3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [0, 9, 0], [0, 0, 9]]
K = len(O3)
BORDERS = [pytest.param(BORDER_CIRCULAR, id="circ"), pytest.param(BORDER_CROP_ZERO, id="crop")]


@pytest.fixture(scope="module")
def I():
    ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    Z, Y, X = DIMS
    S = Z * Y * X
    e = synth.synth_embedding((B, D, S), 41).reshape(B, D, Z, Y, X)
    e[0, :, 1, 7, 11] = 0.0   # the eps branch
    idx = np.arange(B * K * S, dtype=np.uint64)
    t = (synth.hash_uniform(idx, 42) < 0.6).astype(np.float32).reshape(B, K, Z, Y, X)
    w = (0.5 + synth.hash_uniform(idx, 43)).astype(np.float32).reshape(B, K, Z, Y, X)
    m = (synth.hash_uniform(idx, 44) < 0.9).astype(np.uint8).reshape(B, K, Z, Y, X)
    return dict(E=torch.from_numpy(e), T=torch.from_numpy(t), W=torch.from_numpy(w), M=torch.from_numpy(m), o3=O3, lam=lambdas(K), B=B, K=K,
                dims=DIMS)


def _regular(I, a):
    reg = (I["E"].double().pow(2).sum(1, keepdim=True).sqrt() >= EPS).expand_as(a)
    return torch.where(reg, a, torch.zeros_like(a))


@pytest.mark.parametrize("border", BORDERS)
def test_own_g_identity(I, border):
    norm = 1 if border else 0
    ref = cosine_loss(I["E"], None, I["T"], I["W"], I["M"], O3, I["lam"], EPS, border, norm, dloss=DLOSS)
    m, a = I["M"].double(), ref["affs"]
    g = torch.stack([I["lam"][i] * 2.0 * I["W"][:, i].double() * m[:, i] * (a[:, i] * m[:, i] - I["T"][:, i].double() * m[:, i])
                     / normaliser(norm, B, DIMS, O3[i]) for i in range(K)], 1)
    if border:
        gone = gone_mask(I, border).unsqueeze(0).expand_as(g)
        assert bool(g[gone].any()), "this g is not zero on the cropped pairs: the vjp's selects are exercised"
    got = vjp(I["E"], None, g, O3, EPS, border, DLOSS)
    assert torch.equal(got["affs"], ref["affs"])
    r, rr = relmax(got["de"], ref["de"]), relmax(_regular(I, got["de"]), _regular(I, ref["de"]))
    print("own-g identity, border %d: %.3g of max, %.3g over the regular pixels" % (border, r, rr))
    assert r <= 1e-12 and rr <= 1e-12


def test_poison_invariance(I):
    G, G_alt = make_g(I, BORDER_CROP_ZERO, 5)
    for i, o in enumerate(O3):
        _, ok = shifted(I["E"][:, :1], o, BORDER_CROP_ZERO)
        assert bool((~ok).any()), "offset %d crops nothing" % i
    other = torch.roll(I["E"], 1, 0)
    for o, og in ((None, False), (other, True)):
        a, b = vjp(I["E"], o, G, O3, EPS, BORDER_CROP_ZERO, DLOSS, other_grad=og), vjp(I["E"], o, G_alt, O3, EPS, BORDER_CROP_ZERO, DLOSS,
                                                                                    other_grad=og)
        assert torch.equal(a["de"], b["de"])
        assert (a["de_other"] is None and not og) or torch.equal(a["de_other"], b["de_other"])
    # ... and the poison is not inert by accident: with the pairs kept (CIRCULAR) the two gradients differ
    assert not torch.equal(vjp(I["E"], None, G, O3, EPS, BORDER_CIRCULAR, DLOSS)["de"], vjp(I["E"], None, G_alt, O3, EPS, BORDER_CIRCULAR, DLOSS)["de"])


@pytest.mark.parametrize("border", BORDERS)
def test_f32_noise_floor(I, border):
    G, _ = make_g(I, border, 6)
    hi = vjp(I["E"], None, G, O3, EPS, border, DLOSS)["de"]
    lo = vjp(I["E"], None, G, O3, EPS, border, DLOSS, dtype=torch.float32)["de"]
    r, rr = relmax(lo, hi), relmax(_regular(I, lo.double()), _regular(I, hi))
    print("f32 evaluation of the vjp, border %d: %.3g of max, %.3g over the regular pixels" % (border, r, rr))
    assert r < 1e-5 and rr < 1e-5


@pytest.mark.parametrize("border", BORDERS)
def test_make_g(I, border):
    G, G_alt = make_g(I, border, 7)
    assert G.shape == (B, K) + DIMS and G.dtype == torch.float32
    assert bool(torch.isfinite(G).all()) and not bool((G == 0).any())
    assert bool((G < 0).any()) and bool((G > 0).any())
    G2, _ = make_g(I, border, 7)
    assert torch.equal(G, G2) and not torch.equal(G, make_g(I, border, 8)[0])   # hash-seeded, no global state
    assert not torch.equal(G[:, 0], G[:, 1])                                    # a stream per channel
    if not border:
        assert G_alt is None and float(G.abs().max()) <= 1.5 and float(G.abs().min()) >= 2.0 ** -9
        return
    gone = gone_mask(I, border).unsqueeze(0).expand_as(G)
    assert torch.equal(G == POISON, gone) and torch.equal(G_alt == POISON_ALT, gone)
    assert torch.equal(G[~gone], G_alt[~gone]) and float(G[~gone].abs().max()) <= 1.5
    assert bool(torch.isfinite(G_alt).all()) and not bool((G_alt == 0).any())
    for t in (torch.float16, torch.bfloat16):   # exact in every storage type
        assert float(torch.tensor(POISON).to(t)) == POISON and float(torch.tensor(POISON_ALT).to(t)) == POISON_ALT
