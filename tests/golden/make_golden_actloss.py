#!/usr/bin/env python3
"""Generate tests/golden/gal_*.npz: the reference's three loss modules that take the loss on the ACTIVATED affinity map, run as
they are; and tests/golden/gnf_2d.npz: the same modules and the raw-cosine one on an embedding with a NaN / an inf in it
(`python tests/golden/make_golden_actloss.py nonfinite` writes that file alone).

Run in the build container only (needs /root/reference; the GPU box has neither):
    python tests/golden/make_golden_actloss.py

What is imported from the reference (nothing is copied; the files are loaded where they lie):
    scripts_cvppp/loss/loss_embedding.py        embedding_loss, ema_embedding_loss       clamp((cos + 1) / 2, 0, 1)
    scripts_cvppp/loss/loss_embedding_exp.py    embedding_loss                           clamp(cos, 0, 1)
    scripts_cvppp/loss/loss_embedding_norm.py   embedding_loss, ema_embedding_loss       F.normalize, mode 'cos' and the L2 mode
    scripts_cvppp/loss/loss.py                  WeightedMSE (its `.cuda()` call made a no-op on this GPU-less host, as make_golden.py does)
    scripts_cvppp/utils/affinity_ours.py        multi_offset, gen_affs_ours

Every fixture is data only: the inputs (e, optional ema, target, weight, mask, offsets, affs0_weight), the reference's outputs
(loss, affs, grad = d loss / d e) and the parameter names of the reference functions (for a signature test).

The clamp edge.  Where v (the value the clamp sees) lies within rounding of 0 or 1, an f32 kernel and the reference may take
different branches of the clamp's slope, and one such term changes the gradient by its whole size.  So every term whose float64
|v - edge| < 1e-4 gets weight 0 here -- both sides drop it -- and the count is stored (`edge_zeroed`, of `terms`); the test
asserts that it stays below 0.2 % of the terms.
"""
import importlib.util
import inspect
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
EDGE = 1e-4


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MODULES = {"loss_embedding": load("ref_le", "scripts_cvppp/loss/loss_embedding.py"),
           "loss_embedding_exp": load("ref_le_exp", "scripts_cvppp/loss/loss_embedding_exp.py"),
           "loss_embedding_norm": load("ref_le_norm", "scripts_cvppp/loss/loss_embedding_norm.py")}
refloss = load("ref_loss", "scripts_cvppp/loss/loss.py")
refaff = load("ref_aff", "scripts_cvppp/utils/affinity_ours.py")
torch.Tensor.cuda = lambda self, *a, **k: self  # loss.py:116 norm_term.cuda(): the identity on a CPU-only host
criterion = refloss.WeightedMSE()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def weight_binary_ratio(label, alpha=1.0):
    """data_segmentation.py:205-228 (mask=None branch; its module needs skimage), as in make_golden.py"""
    if label.max() == label.min():
        return np.ones_like(label, np.float32)
    label = (label != 0).astype(int)
    f = float(np.clip(float(label.sum()) / np.prod(label.shape), 5e-2, 0.99))
    w = label + alpha * f / (1 - f) * (1 - label) if f > 0.5 else alpha * (1 - f) / f * label + (1 - label)
    return w.astype(np.float32)


def targets_2d(rng, B, H, W, offsets, cell=8, n=12):
    K = len(offsets)
    t, m, w = np.zeros((B, K, H, W), np.float32), np.zeros((B, K, H, W), np.uint8), np.zeros((B, K, H, W), np.float32)
    for b in range(B):
        coarse = rng.integers(0, n + 1, size=(-(-H // cell), -(-W // cell)))
        lab = np.kron(coarse, np.ones((cell, cell), dtype=coarse.dtype))[:H, :W].astype(np.float32)
        t[b], m[b] = refaff.gen_affs_ours(lab, offsets, ignore=False, padding=True)
        for i in range(K):
            w[b, i] = weight_binary_ratio(t[b, i])
    return t, w, m


def clamp_input(e, other, offsets, eps, half):
    """float64: the value v that torch.clamp sees, [B,K,H,W] (cosine with each norm clamped at eps; (a + 1) / 2 when half)"""
    x = T(e).double()
    y = x if other is None else T(other).double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
    v = torch.stack([(xn * torch.roll(yn, shifts=(-o[0], -o[1]), dims=(2, 3))).sum(1) for o in offsets], 1)
    return ((v + 1) / 2 if half else v).numpy()


def case(name, module, seed, B, D, H, W, ema=False, affs0_weight=1, mode=None, float_mask=False, K=None):
    rng = np.random.default_rng(seed)
    mod = MODULES[module]
    offsets = refaff.multi_offset([1, 3, 5, 9, 27], neighbor=4)[:K]
    e = rng.standard_normal((B, D, H, W)).astype(np.float32)
    other = (e + 0.5 * rng.standard_normal((B, D, H, W))).astype(np.float32) if ema else None
    t, w, m = targets_2d(rng, B, H, W, offsets)
    if float_mask:  # fractional values, exact 0 and 1 among them
        m = np.where(m != 0, rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 1.5], np.float32), size=m.shape), 0).astype(np.float32)
        m = np.where(rng.random(m.shape) < 0.5, rng.random(m.shape).astype(np.float32), m).astype(np.float32)
    v = clamp_input(e, other, offsets, 1e-12 if module == "loss_embedding_norm" else 1e-6, module != "loss_embedding_exp")
    near = (np.abs(v) < EDGE) | (np.abs(v - 1) < EDGE)
    w = np.where(near, np.float32(0), w).astype(np.float32)
    et = T(e).requires_grad_(True)
    kw = {} if mode is None else {"mode": mode}
    if ema:
        fn = mod.ema_embedding_loss
        loss, affs = fn(et, T(other), T(t), T(w), T(m), criterion, offsets, affs0_weight=affs0_weight, **kw)
    else:
        fn = mod.embedding_loss
        loss, affs = fn(et, T(t), T(w), T(m), criterion, offsets, affs0_weight=affs0_weight, **kw)
    loss.backward()
    out = dict(module=module, fn=fn.__name__, offsets=np.array(offsets, np.int32), e=e, target=t, weight=w, mask=m,
               affs0_weight=np.float32(affs0_weight), mode="" if mode is None else mode, loss=np.float32(loss.item()),
               affs=affs.detach().numpy(), grad=et.grad.numpy(), edge_zeroed=np.int64(near.sum()), terms=np.int64(near.size))
    if ema:
        out["ema"] = other
    for f in ("embedding_loss", "embedding2affs", "ema_embedding_loss"):
        if hasattr(mod, f):
            out["params_" + f] = np.array(list(inspect.signature(getattr(mod, f)).parameters))
            out["defaults_" + f] = np.array([repr(p.default) for p in inspect.signature(getattr(mod, f)).parameters.values()
                                             if p.default is not inspect.Parameter.empty])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(x) for k, x in out.items()})
    print("%-24s %7.1f KB   edge-zeroed %d of %d (%.4f %%)" % (name, os.path.getsize(path) / 1024, near.sum(), near.size,
                                                           100.0 * near.sum() / near.size))


def nonfinite_case(name="gnf_2d"):
    """One NaN / one +inf channel value in a small embedding through embedding_loss of the raw-cosine module (loss_embedding_mse.py) and
    of the two clamp modules: where the reference's map, loss and gradient are NaN (tests/test_nonfinite_host.py).  No edge rule is
    needed: only NaN positions and the values away from them are compared, with the same module's clean run."""
    rng = np.random.default_rng(31)
    mods = dict(MODULES, loss_embedding_mse=load("ref_le_mse", "scripts_cvppp/loss/loss_embedding_mse.py"))
    B, D, H, W = 2, 4, 6, 10
    offsets = refaff.multi_offset([1, 3], neighbor=8)
    e = rng.standard_normal((B, D, H, W)).astype(np.float32)
    t, w, m = targets_2d(rng, B, H, W, offsets, cell=3, n=3)
    out = dict(offsets=np.array(offsets, np.int32), e=e, target=t, weight=w, mask=m, q_nan=np.array([0, 2, 7], np.int32),
               q_inf=np.array([0, 0, 0], np.int32), channel=np.int32(1))
    for module in ("loss_embedding_mse", "loss_embedding", "loss_embedding_exp"):
        for tag, val in (("clean", None), ("nan", np.nan), ("inf", np.inf)):
            x = e.copy()
            if val is not None:
                q = out["q_" + tag]
                x[0, 1, q[1], q[2]] = val
            et = T(x).requires_grad_(True)
            res = mods[module].embedding_loss(et, T(t), T(w), T(m), criterion, offsets)
            res[0].backward()
            out["loss_%s_%s" % (module, tag)] = np.float32(res[0].item())
            out["affs_%s_%s" % (module, tag)] = res[1].detach().numpy()
            out["grad_%s_%s" % (module, tag)] = et.grad.numpy()
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(x) for k, x in out.items()})
    print("%-24s %7.1f KB" % (name, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if sys.argv[1:] == ["nonfinite"]:  # the one fixture alone (the gal_* files are not rewritten)
        nonfinite_case()
        sys.exit(0)
    case("gal_emb_self", "loss_embedding", 11, 2, 16, 40, 72)
    case("gal_emb_ema_w", "loss_embedding", 12, 2, 16, 32, 48, ema=True, affs0_weight=0.5)
    case("gal_exp_self_w", "loss_embedding_exp", 13, 2, 16, 40, 72, affs0_weight=2.0)
    case("gal_exp_self_d32", "loss_embedding_exp", 14, 2, 32, 32, 32, K=8)
    case("gal_norm_self_cos", "loss_embedding_norm", 15, 2, 16, 40, 72, mode="cos")
    case("gal_norm_self_l2", "loss_embedding_norm", 16, 2, 16, 40, 72, mode="l2", affs0_weight=3.0)
    case("gal_norm_ema_cos", "loss_embedding_norm", 17, 2, 16, 32, 48, ema=True, mode="cos")
    case("gal_norm_ema_l2_w", "loss_embedding_norm", 18, 2, 16, 32, 48, ema=True, mode="l2", affs0_weight=0.25)
    case("gal_emb_self_fmask", "loss_embedding", 19, 2, 16, 40, 72, float_mask=True, affs0_weight=1.5)
    nonfinite_case()
