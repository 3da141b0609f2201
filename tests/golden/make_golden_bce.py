#!/usr/bin/env python3
"""Generate tests/golden/gbce_*.npz: the reference's loss modules run with its OTHER criteria -- WeightedBCE, BCELoss, MSELoss
(loss/loss.py:126-152; the `loss_func` choices of scripts_cvppp/main.py:182-189 beside WeightedMSE).

Needs a checkout of the reference (weih527/Pixel-Embedded-Affinity) and no GPU:
    PEA_REFERENCE_DIR=/path/to/Pixel-Embedded-Affinity python tests/golden/make_golden_bce.py

What is imported from the reference (nothing is copied; the files are loaded where they lie):
    scripts_cvppp/loss/loss_embedding.py        embedding_loss, ema_embedding_loss       clamp((cos + 1) / 2, 0, 1)
    scripts_cvppp/loss/loss_embedding_exp.py    embedding_loss                           clamp(cos, 0, 1)
    scripts_cvppp/loss/loss_embedding_norm.py   embedding_loss, ema_embedding_loss       F.normalize, mode 'cos' and the L2 mode
    scripts_cvppp/loss/loss_embedding_mse.py    embedding_loss, ema_embedding_loss       the raw cosine (MSELoss only)
    scripts_cvppp/loss/loss.py                  WeightedBCE, BCELoss, MSELoss
    scripts_cvppp/utils/affinity_ours.py        multi_offset, gen_affs_ours

Field names and shapes follow make_golden_actloss.py (gal_*.npz), plus `criterion` (the class name).  Every fixture is data only:
the inputs, the reference's loss, map and gradient.

The clamp edge and BCE's conditioning.  BCE's slope is 1 / x near x = 0 and 1 / (1 - x) near x = 1, so a term within 0.02 of an
edge amplifies the f32 rounding of x past any fixed gradient tolerance.  With (cos + 1) / 2 no term of these inputs lies there
(`edge_near` records the count: 0 in every half-shift fixture, asserted below), so those fixtures' gradients are comparable as they
are; with clamp(cos, 0, 1) 6 % of the terms do, and the test compares loss and map only (tests/test_gpu_bce.py holds that module's g
through its decomposed check).  `edge_near` / `terms` are stored for the test's cap.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("PEA_REFERENCE_DIR") or sys.exit("set PEA_REFERENCE_DIR to a checkout of the reference")
OUT = os.path.dirname(os.path.abspath(__file__))
NEAR = 0.02


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MODULES = {"loss_embedding": load("ref_le", "scripts_cvppp/loss/loss_embedding.py"),
           "loss_embedding_exp": load("ref_le_exp", "scripts_cvppp/loss/loss_embedding_exp.py"),
           "loss_embedding_norm": load("ref_le_norm", "scripts_cvppp/loss/loss_embedding_norm.py"),
           "loss_embedding_mse": load("ref_le_mse", "scripts_cvppp/loss/loss_embedding_mse.py")}
refloss = load("ref_loss", "scripts_cvppp/loss/loss.py")
refaff = load("ref_aff", "scripts_cvppp/utils/affinity_ours.py")
CRITERIA = {"WeightedBCE": refloss.WeightedBCE, "BCELoss": refloss.BCELoss, "MSELoss": refloss.MSELoss}


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


def case(name, module, crit, seed, B, D, H, W, ema=False, affs0_weight=1, mode=None, float_mask=False):
    rng = np.random.default_rng(seed)
    mod = MODULES[module]
    offsets = refaff.multi_offset([1, 3, 5, 9, 27], neighbor=4)
    e = rng.standard_normal((B, D, H, W)).astype(np.float32)
    other = (e + 0.5 * rng.standard_normal((B, D, H, W))).astype(np.float32) if ema else None
    t, w, m = targets_2d(rng, B, H, W, offsets)
    if float_mask:  # an f32 mask of exact 0 / 1 values (BCE needs m in [0, 1]): some inside pixels switched off
        m = np.where(rng.random(m.shape) < 0.2, 0, m).astype(np.float32)
    near, terms = 0, 0
    if module != "loss_embedding_mse":
        half = module != "loss_embedding_exp"
        v = clamp_input(e, other, offsets, 1e-12 if module == "loss_embedding_norm" else 1e-6, half)
        near, terms = int(((v < NEAR) | (v > 1 - NEAR)).sum()), v.size
        assert not half or near == 0, (name, near)
    et = T(e).requires_grad_(True)
    kw = {} if mode is None else {"mode": mode}
    criterion = CRITERIA[crit]()
    if ema:
        fn = mod.ema_embedding_loss
        res = fn(et, T(other), T(t), T(w), T(m), criterion, offsets, affs0_weight=affs0_weight, **kw)
    else:
        fn = mod.embedding_loss
        res = fn(et, T(t), T(w), T(m), criterion, offsets, affs0_weight=affs0_weight, **kw)
    loss, affs = res[0], res[1]
    loss.backward()
    out = dict(module=module, fn=fn.__name__, criterion=crit, offsets=np.array(offsets, np.int32), e=e, target=t, weight=w, mask=m,
               affs0_weight=np.float32(affs0_weight), mode="" if mode is None else mode, loss=np.float32(loss.item()),
               affs=affs.detach().numpy(), grad=et.grad.numpy(), edge_near=np.int64(near), terms=np.int64(terms))
    if ema:
        out["ema"] = other
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(x) for k, x in out.items()})
    print("%-28s %7.1f KB   loss %.6f   within %.2f of an edge: %d of %d" % (name, os.path.getsize(path) / 1024, loss.item(), NEAR,
                                                                         near, terms))


if __name__ == "__main__":
    case("gbce_emb_self_wbce", "loss_embedding", "WeightedBCE", 21, 2, 16, 40, 72)
    case("gbce_emb_ema_wbce_w", "loss_embedding", "WeightedBCE", 22, 2, 16, 32, 48, ema=True, affs0_weight=0.5)
    case("gbce_emb_self_bce", "loss_embedding", "BCELoss", 23, 2, 16, 40, 72, affs0_weight=2.0)
    case("gbce_emb_ema_bce", "loss_embedding", "BCELoss", 24, 2, 16, 32, 48, ema=True)
    case("gbce_exp_self_wbce_w", "loss_embedding_exp", "WeightedBCE", 25, 2, 16, 40, 72, affs0_weight=2.0)
    case("gbce_exp_self_bce", "loss_embedding_exp", "BCELoss", 26, 2, 16, 32, 48)
    case("gbce_norm_self_cos_wbce", "loss_embedding_norm", "WeightedBCE", 27, 2, 16, 40, 72, mode="cos")
    case("gbce_norm_self_l2_wbce_w", "loss_embedding_norm", "WeightedBCE", 28, 2, 16, 32, 48, mode="l2", affs0_weight=3.0)
    case("gbce_norm_ema_l2_bce_w", "loss_embedding_norm", "BCELoss", 29, 2, 16, 32, 48, ema=True, mode="l2", affs0_weight=0.25)
    case("gbce_emb_self_fmask_wbce_w", "loss_embedding", "WeightedBCE", 30, 2, 16, 40, 72, float_mask=True, affs0_weight=1.5)
    case("gbce_emb_self_mse", "loss_embedding", "MSELoss", 31, 2, 16, 32, 48, affs0_weight=0.5)
    case("gbce_mse_self_mse", "loss_embedding_mse", "MSELoss", 32, 2, 16, 40, 72)
    case("gbce_mse_ema_mse_w", "loss_embedding_mse", "MSELoss", 33, 2, 16, 32, 48, ema=True, affs0_weight=0.5)
