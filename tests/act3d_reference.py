"""A float64 restatement of the reference's 3D losses on the ACTIVATED affinity map (scripts_ac3ac4/loss/embedding2affs_3d.py,
embedding2affs_3d_l2.py, loss_embedding_mse.py:70-140): the loss, the stored map with its border rule and fill, and the gradient by
autograd.  A helper module (no tests here): tests/test_act3d_host.py holds it to every tests/golden/ga3_*.npz fixture on the CPU,
tests/test_gpu_act3d.py holds the kernels to it.

Channel i compares voxel p with p - shifts[i] along axis i % 3 of (z, y, x); the pair exists where p[axis] >= shifts[i].
    a = <ehat(p), ehat_other(p - s)>,  ehat = e / max(|e|, eps)
    v = (a + 1) / 2 under the half shift, else a;   u = clamp(v, 0, 1) under the clamp, else v
mode 'cropped': sum_i lambda_i criterion(u_i, t_i, w_i) on the existing pairs of channel i (lambda = affs0_weight on channels < first)
mode 'whole':   ONE criterion call over [B,K,Z,Y,X] with u = 0, t = 0, w = 0 on the `masked` border
mode 'norm4':   as 'whole', but only a one-slice border of channels 0..2 is masked; on the other non-existent pairs u = 0 meets the
                given t and w
The stored map holds u on the existing pairs and 0 elsewhere; with fill_shift = s the first s slices of channel c along axis c hold
the next s.
"""
import numpy as np
import torch
import torch.nn.functional as F

NORM5 = (1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27)
HALF, CLAMP = 4, 8
EDGE, EDGE_MAX_FRACTION = 1e-4, 0.002

# (module, fn) -> shift table (None: [shift] * 3), activation, mode, channels that carry affs0_weight, honours `fill`, eps
FORMS = {
    ("embedding2affs_3d", "embedding_loss_norm1"): (None, HALF | CLAMP, "cropped", 1, True, 1e-12),
    ("embedding2affs_3d", "embedding_loss_norm1_relu"): (None, CLAMP, "cropped", 1, False, 1e-12),
    ("embedding2affs_3d", "embedding_loss_norm2"): (None, HALF | CLAMP, "whole", 0, False, 1e-12),
    ("embedding2affs_3d", "embedding_loss_norm3"): (None, HALF | CLAMP, "whole", 0, False, 1e-6),
    ("embedding2affs_3d", "embedding_loss_norm4"): (NORM5, HALF | CLAMP, "norm4", 0, False, 1e-12),
    ("embedding2affs_3d", "embedding_loss_norm5"): (NORM5, HALF | CLAMP, "cropped", 3, False, 1e-12),
    ("embedding2affs_3d", "embedding_loss_norm5_relu"): (NORM5, CLAMP, "cropped", 3, False, 1e-12),
    ("embedding2affs_3d_l2", "embedding_loss_l21"): (None, HALF, "cropped", 1, False, 1e-12),
    ("embedding2affs_3d_l2", "embedding_loss_l22"): (None, HALF, "whole", 0, False, 1e-12),
    ("embedding2affs_3d_l2", "embedding_loss_l25"): (NORM5, HALF, "cropped", 3, False, 1e-12),
    ("loss_embedding_mse_3d", "embedding_loss_norm2"): (None, HALF | CLAMP, "cropped", 1, True, 1e-12),
    ("loss_embedding_mse_3d", "ema_embedding_loss_norm2"): (None, HALF | CLAMP, "cropped", 1, True, 1e-12),
}


def criterion64(name):
    """the reference's criteria (loss/loss.py:106-152) on float64 tensors"""
    if name == "WeightedMSE":
        return lambda p, t, w: (w * (p - t) ** 2).sum() / (p.shape[0] * int(np.prod(p.shape[2:])))
    if name == "MSELoss":
        return lambda p, t, w: ((p - t) ** 2).mean()
    if name == "BCELoss":
        return lambda p, t, w: F.binary_cross_entropy(p, t)
    if name == "WeightedBCE":
        return lambda p, t, w: F.binary_cross_entropy(p, t, w)
    raise KeyError(name)


def activate64(a, act):
    v = (a + 1) / 2 if act & HALF else a
    return v, (torch.clamp(v, 0.0, 1.0) if act & CLAMP else v)


def _pad_front(u, ax, s):
    """u on the cropped extent -> the full extent, zeros on the first s slices of axis ax"""
    shape = list(u.shape)
    shape[ax] = s
    return torch.cat([torch.zeros(shape, dtype=u.dtype), u], ax)


def exists(shape, shifts):
    """[K,Z,Y,X] bool: the pair of channel i at p exists"""
    ok = torch.ones((len(shifts),) + tuple(shape), dtype=torch.bool)
    for i, s in enumerate(shifts):
        ok[i].narrow(i % 3, 0, s).zero_()
    return ok


def restate(e, ema, target, weight, shifts, act, mode, criterion, affs0_weight=1.0, first=0, eps=1e-12, fill_shift=0):
    """-> loss (0-dim), stored map [B,K,Z,Y,X], d loss / d e, v [B,K,Z,Y,X] (the clamp's input; 0.5 where the pair does not exist): float64"""
    crit = criterion64(criterion)
    x = torch.as_tensor(e).double().clone().requires_grad_(True)
    y = x if ema is None else torch.as_tensor(ema).double()
    t, w = torch.as_tensor(target).double(), torch.as_tensor(weight).double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
    loss, us, vs = 0.0, [], []
    for i, s in enumerate(shifts):
        ax = 2 + i % 3
        n = x.shape[ax] - s
        a = torch.einsum("bdzyx,bdzyx->bzyx", xn.narrow(ax, s, n), yn.narrow(ax, 0, n)).unsqueeze(1)  # (no [B,D,..] product is kept)
        v, u = activate64(a, act)
        if mode == "cropped":
            lam = float(affs0_weight) if i < first else 1.0
            loss = loss + lam * crit(u, t[:, i:i + 1].narrow(ax, s, n), w[:, i:i + 1].narrow(ax, s, n))
        us.append(_pad_front(u, ax, s))
        vs.append(_pad_front(v.detach() - 0.5, ax, s) + 0.5)
    full = torch.cat(us, 1)
    if mode != "cropped":
        masked = exists(x.shape[2:], shifts if mode == "whole" else [1] * 3 + [0] * (len(shifts) - 3)).to(torch.float64)[None]
        loss = crit(full, t * masked, w * masked)
    loss.backward()
    stored = full.detach().clone()
    if fill_shift:
        for c in range(3):
            stored[:, c].narrow(1 + c, 0, fill_shift).copy_(stored[:, c].narrow(1 + c, fill_shift, fill_shift).clone())
    return loss.detach(), stored, x.grad, torch.cat(vs, 1)


def clamp_input64(e, ema, shifts, act, eps=1e-12):
    """v of restate() alone (no criterion, no gradient): what the edge rule needs before the weights exist"""
    with torch.no_grad():
        x = torch.as_tensor(e).double()
        y = x if ema is None else torch.as_tensor(ema).double()
        xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
        yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
        vs = []
        for i, s in enumerate(shifts):
            ax = 2 + i % 3
            n = x.shape[ax] - s
            a = torch.einsum("bdzyx,bdzyx->bzyx", xn.narrow(ax, s, n), yn.narrow(ax, 0, n)).unsqueeze(1)
            vs.append(_pad_front(activate64(a, act)[0] - 0.5, ax, s) + 0.5)
        return torch.cat(vs, 1)


def form_of(g):
    """a ga3_* fixture -> the keyword arguments of restate() for its recorded call"""
    table, act, mode, first, fills, eps = FORMS[(str(g["module"]), str(g["fn"]))]
    kw = call_kwargs(g)
    shift = int(kw.get("shift", 1))
    return dict(shifts=list(table) if table is not None else [shift] * 3, act=act, mode=mode, criterion=str(g["criterion"]),
                affs0_weight=float(kw.get("affs0_weight", 1.0)), first=first, eps=eps,
                fill_shift=shift if (fills and kw.get("fill", True)) else 0)


def call_kwargs(g):
    """the keyword arguments the fixture's reference call was made with (affs0_weight: float, shift: int, fill: bool)"""
    cast = {"affs0_weight": float, "shift": int, "fill": bool}
    return {str(k): cast[str(k)](v) for k, v in zip(g["kw_names"], g["kw_values"])}


def near_edge(v, act):
    """bool like v: a term whose clamp input lies within EDGE of 0 or 1 (no clamp: none)"""
    if not act & CLAMP:
        return torch.zeros_like(v, dtype=torch.bool)
    return (v.abs() < EDGE) | ((v - 1).abs() < EDGE)


def single_offset64(e, order, shift, eps):
    """embedding_single_offset(_cos): [B,Z,Y,X] float64 -- clamp((cos + 1) / 2, 0, 1), 0 on the first `shift` slices of axis `order`"""
    x = torch.as_tensor(e).double()
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
    ax = 2 + order
    n = x.shape[ax] - shift
    a = (xn.narrow(ax, shift, n) * xn.narrow(ax, 0, n)).sum(1, keepdim=True)
    return _pad_front(activate64(a, HALF | CLAMP)[1], ax, shift)[:, 0]
