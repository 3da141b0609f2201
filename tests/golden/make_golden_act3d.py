#!/usr/bin/env python3
"""Generate tests/golden/ga3_*.npz: the reference's 3D losses on the ACTIVATED affinity map, run as they are.

Run in the build container only (needs /root/reference; the GPU box has neither):
    python tests/golden/make_golden_act3d.py

What is imported from the reference (nothing is copied; the files are loaded where they lie):
    scripts_ac3ac4/loss/embedding2affs_3d.py     embedding_loss_norm1, _norm1_relu, _norm2, _norm3, _norm4, _norm5, _norm5_relu,
                                                 embedding_single_offset, embedding_single_offset_cos
    scripts_ac3ac4/loss/embedding2affs_3d_l2.py  embedding_loss_l21, _l22, _l25
    scripts_ac3ac4/loss/loss_embedding_mse.py    embedding_loss_norm2, ema_embedding_loss_norm2  (:70-140)
    scripts_ac3ac4/loss/loss.py                  WeightedMSE, BCELoss, WeightedBCE (WeightedMSE's `.cuda()` call made a no-op on this
                                                 GPU-less host, as make_golden.py does)

Every fixture is data only: the inputs (e, optional ema, target, weight), the call's keyword arguments (affs0_weight, shift, fill), the
criterion's name, the reference's outputs (loss, affs, grad = d loss / d e) and the parameter names of the reference function (for a
signature test).  The two single-offset fixtures hold one map per axis and no loss; embedding_single_offset gets a NORMALISED
embedding, as its callers in the reference give it.

The clamp edge: the rule of make_golden_actloss.py.  Where v (the value the clamp sees) lies within rounding of 0 or 1 an f32 kernel
and the reference may take different branches of the clamp's slope, so every term whose float64 |v - edge| < 1e-4 gets weight 0 --
both sides drop it -- and the count is stored (`edge_zeroed`, of `terms`); it stays below 0.2 % of the terms, asserted here and in
the tests.  An unweighted criterion cannot drop a term: its fixtures use the half shift, where no term lies at an edge (asserted).
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
NORM5 = [1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27]
MAX_BYTES = 1 << 20


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MODULES = {"embedding2affs_3d": load("ref_e2a3d", "scripts_ac3ac4/loss/embedding2affs_3d.py"),
           "embedding2affs_3d_l2": load("ref_e2a3d_l2", "scripts_ac3ac4/loss/embedding2affs_3d_l2.py"),
           "loss_embedding_mse_3d": load("ref_lem3d", "scripts_ac3ac4/loss/loss_embedding_mse.py")}
refloss = load("ref_loss3d", "scripts_ac3ac4/loss/loss.py")
torch.Tensor.cuda = lambda self, *a, **k: self  # loss.py:116 norm_term.cuda(): the identity on a CPU-only host
CRITERIA = {"WeightedMSE": refloss.WeightedMSE, "BCELoss": refloss.BCELoss, "WeightedBCE": refloss.WeightedBCE}

# fn -> (shift table or None = [shift] * 3, half shift, clamp)
FORMS = {"embedding_loss_norm1": (None, True, True), "embedding_loss_norm1_relu": (None, False, True),
         "embedding_loss_norm2": (None, True, True), "ema_embedding_loss_norm2": (None, True, True),
         "embedding_loss_norm3": (None, True, True), "embedding_loss_norm4": (NORM5, True, True),
         "embedding_loss_norm5": (NORM5, True, True), "embedding_loss_norm5_relu": (NORM5, False, True),
         "embedding_loss_l21": (None, True, False), "embedding_loss_l22": (None, True, False), "embedding_loss_l25": (NORM5, True, False)}


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


def targets_3d(rng, B, K, Z, Y, X):
    t = (rng.random((B, K, Z, Y, X)) < 0.7).astype(np.float32)
    w = np.stack([np.stack([weight_binary_ratio(t[b, i]) for i in range(K)]) for b in range(B)])
    return t, w.astype(np.float32)


def clamp_input(e, other, shifts, eps, half):
    """float64: the value v the clamp sees on every EXISTING pair, NaN elsewhere, [B,K,Z,Y,X]"""
    x = T(e).double()
    y = x if other is None else T(other).double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
    v = torch.full((x.shape[0], len(shifts)) + tuple(x.shape[2:]), float("nan"), dtype=torch.float64)
    for i, s in enumerate(shifts):
        ax = 2 + i % 3
        n = x.shape[ax] - s
        v[:, i].narrow(ax - 1, s, n).copy_((xn.narrow(ax, s, n) * yn.narrow(ax, 0, n)).sum(1))
    return ((v + 1) / 2 if half else v).numpy()


def save(name, **out):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(x) for k, x in out.items()})
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    return size


def case(name, module, fn_name, seed, B, Z, Y, X, crit="WeightedMSE", ema=False, D=16, **kw):
    rng = np.random.default_rng(seed)
    fn = getattr(MODULES[module], fn_name)
    table, half, clamp = FORMS[fn_name]
    shifts = table if table is not None else [kw.get("shift", 1)] * 3
    e = rng.standard_normal((B, D, Z, Y, X)).astype(np.float32)
    other = (e + 0.5 * rng.standard_normal(e.shape)).astype(np.float32) if ema else None
    t, w = targets_3d(rng, B, len(shifts), Z, Y, X)
    near = np.zeros(t.shape, bool)
    if clamp:
        v = clamp_input(e, other, shifts, 1e-6 if fn_name == "embedding_loss_norm3" else 1e-12, half)
        near = (np.abs(v) < EDGE) | (np.abs(v - 1) < EDGE)  # (NaN, the pairs that do not exist, compares False)
        w = np.where(near, np.float32(0), w).astype(np.float32)
    if crit == "BCELoss":
        assert not near.any(), "an unweighted criterion cannot drop an edge term"
    assert near.sum() <= 0.002 * near.size, (name, near.sum(), near.size)
    et = T(e).requires_grad_(True)
    args = (et, T(other)) if ema else (et,)
    loss, affs = fn(*args, T(t), T(w), CRITERIA[crit](), **kw)
    loss.backward()
    sig = inspect.signature(fn).parameters
    out = dict(module=module, fn=fn_name, criterion=crit, e=e, target=t, weight=w, loss=np.float32(loss.item()),
               affs=affs.detach().numpy(), grad=et.grad.numpy(), edge_zeroed=np.int64(near.sum()), terms=np.int64(near.size),
               params=np.array(list(sig)),
               defaults=np.array([repr(p.default) for p in sig.values() if p.default is not inspect.Parameter.empty]),
               kw_names=np.array(sorted(kw)), kw_values=np.array([float(kw[k]) for k in sorted(kw)], np.float64))
    if ema:
        out["ema"] = other
    size = save(name, **out)
    print("%-22s %7.1f KB   loss %.6f   edge-zeroed %d of %d (%.4f %%)" % (name, size / 1024, loss.item(), near.sum(), near.size,
                                                                          100.0 * near.sum() / near.size))


def single_case(name, fn_name, seed, B, Z, Y, X, shift, D=16):
    rng = np.random.default_rng(seed)
    fn = getattr(MODULES["embedding2affs_3d"], fn_name)
    e = rng.standard_normal((B, D, Z, Y, X)).astype(np.float32)
    if fn_name == "embedding_single_offset":  # its callers normalise first (embedding2affs_3d.py:127, :175)
        e = F.normalize(T(e), p=2, dim=1).numpy()
    affs = np.stack([fn(T(e), order, shift=shift).numpy() for order in range(3)], 1)
    sig = inspect.signature(fn).parameters
    size = save(name, module="embedding2affs_3d", fn=fn_name, e=e, shift=np.int32(shift), affs=affs, params=np.array(list(sig)))
    print("%-22s %7.1f KB" % (name, size / 1024))


if __name__ == "__main__":
    S3, S3B, S12 = (1, 6, 20, 24), (2, 6, 20, 24), (1, 6, 28, 32)
    E, L2, M3 = "embedding2affs_3d", "embedding2affs_3d_l2", "loss_embedding_mse_3d"
    case("ga3_norm1_fill", E, "embedding_loss_norm1", 41, *S3B, affs0_weight=0.5, shift=1, fill=True)
    case("ga3_norm1_nofill", E, "embedding_loss_norm1", 42, *S3, affs0_weight=2.0, shift=1, fill=False)
    case("ga3_norm1_s2", E, "embedding_loss_norm1", 43, *S3, affs0_weight=1.5, shift=2, fill=True)
    case("ga3_norm1_relu", E, "embedding_loss_norm1_relu", 44, *S3, affs0_weight=0.5, shift=1)
    case("ga3_norm2", E, "embedding_loss_norm2", 45, *S3, shift=1)
    case("ga3_norm2_bce", E, "embedding_loss_norm2", 46, *S3B, crit="BCELoss", shift=1)
    case("ga3_norm3", E, "embedding_loss_norm3", 47, *S3, shift=2)
    case("ga3_norm4", E, "embedding_loss_norm4", 48, *S12)
    case("ga3_norm5", E, "embedding_loss_norm5", 49, *S12, affs0_weight=2.0)
    case("ga3_norm5_wbce", E, "embedding_loss_norm5", 50, *S12, crit="WeightedBCE", affs0_weight=0.5)
    case("ga3_norm5_relu", E, "embedding_loss_norm5_relu", 51, *S12, affs0_weight=1.5)
    case("ga3_l21", L2, "embedding_loss_l21", 52, *S3, affs0_weight=0.5, shift=1)
    case("ga3_l22", L2, "embedding_loss_l22", 53, *S3, shift=2)
    case("ga3_l25", L2, "embedding_loss_l25", 54, *S12, affs0_weight=2.0)
    case("ga3_mse_norm2", M3, "embedding_loss_norm2", 55, *S3, affs0_weight=0.5, shift=1, fill=True)
    case("ga3_mse_ema_norm2", M3, "ema_embedding_loss_norm2", 56, 2, 5, 16, 24, ema=True, affs0_weight=2.0, shift=1, fill=False)
    single_case("ga3_single", "embedding_single_offset", 57, *S3, shift=2)
    single_case("ga3_single_cos", "embedding_single_offset_cos", 58, *S3, shift=1)
