"""float64 vector-Jacobian product of the raw-cosine affinity map for an ARBITRARY upstream gradient G, and the G the vjp tests feed; a
helper module (no tests here), CPU or GPU tensors.

include/pea.h: the g of pea_affinity_bwd / _bwd_ex / _bwd_ex2 / _bwd_dual_ex / _bwd_multi is "either what pea_affinity_fwd wrote or any
upstream gradient d(criterion) / d(affs)".  The g the forward writes is exactly 0 on every pair CROP_ZERO removes, smooth and ~1e-6; the G
of make_g is none of that:

    de = dloss * d/dE sum_i sum_p G_i(p) a_i(p),     a_i(p) = < ehat(p), ehat_other(p + o_i) >  (0, and no term, where the pair does not exist)

with the selects of tests/f64_reference.py::cosine_loss (torch.where(ok, ...), never "* ok"), so that a pair that does not exist
contributes nothing WHATEVER G holds there.  16-bit storage is evaluated on the embedding as rounded (E is upcast as it is).
"""
import importlib

import numpy as np
import torch

import __graft_entry__ as ge
from f64_reference import BORDER_CROP_ZERO, shifted

POISON, POISON_ALT = 64.0, -3.0   # on the pairs that do not exist; both exact in f32, f16 and bf16


def vjp(E, other, G, offsets3, eps, border, dloss, other_grad=False, dtype=torch.float64):
    """E, other [B,D,Z,Y,X]; G [B,K,Z,Y,X]; dloss a float or None (= 1) -> dict(de, de_other (None unless other_grad), affs [B,K,Z,Y,X]),
    evaluated in `dtype` (float64; float32 measures the noise floor of an f32 evaluation)"""
    with torch.enable_grad():
        x = E.detach().to(dtype).requires_grad_(True)
        y = x if other is None else other.detach().to(dtype).requires_grad_(bool(other_grad))
        xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
        yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
        total, maps = 0.0, []
        for i, o in enumerate(offsets3):
            ys, ok = shifted(yn, o, border)
            ys = torch.where(ok, ys, torch.zeros_like(ys))
            a = (xn * ys).sum(1)
            a = torch.where(ok, a, torch.zeros_like(a))
            term = torch.where(ok, G[:, i].to(dtype) * a, torch.zeros_like(a))
            total = total + term.sum()
            maps.append(a.detach())
        (total * (1.0 if dloss is None else float(dloss))).backward()
    return dict(de=x.grad, de_other=y.grad if (other is not None and other_grad) else None, affs=torch.stack(maps, 1))


def gone_mask(I, border):
    """[K,Z,Y,X] bool: the pairs (p, p + o_i) that do not exist (~ok of shifted); all False unless CROP_ZERO"""
    probe = I["E"][:1, :1]
    return torch.stack([~shifted(probe, o, border)[1] for o in I["o3"]])


def make_g(I, border, seed):
    """-> (G, G_alt), [B,K,Z,Y,X] f32 on the device of I["E"].  Dense (no zero anywhere), random sign per element, magnitude
    2^-j (0.5 + u) with j uniform in 0 .. 8 and NO 1 / N scale: a dropped or doubled term is O(1) of the result.  Every channel has
    its own hash streams (no global RNG state).  CROP_ZERO: G = 64.0 and G_alt = -3.0 on every pair that does not exist, equal
    elsewhere; any other border: every pair exists and G_alt is None."""
    ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    B, K, dims = I["B"], I["K"], tuple(I["dims"])
    n = B * int(np.prod(dims))
    idx = np.arange(n, dtype=np.uint64)
    g = np.empty((B, K) + dims, np.float32)
    for k in range(K):
        s = 7000 + 1009 * int(seed) + 3 * k
        sign = np.where(synth.hash_uniform(idx, s) < 0.5, -1.0, 1.0)
        j = np.floor(synth.hash_uniform(idx, s + 1) * 9.0)
        mag = np.exp2(-j) * (0.5 + synth.hash_uniform(idx, s + 2))
        g[:, k] = (sign * mag).astype(np.float32).reshape((B,) + dims)
    G = torch.from_numpy(g).to(I["E"].device)
    if border != BORDER_CROP_ZERO:
        return G, None
    gone = gone_mask(I, border).unsqueeze(0).expand_as(G)
    return torch.where(gone, torch.full_like(G, POISON), G), torch.where(gone, torch.full_like(G, POISON_ALT), G)
