"""float64 torch restatement of the raw-cosine loss of include/pea.h (autograd for the gradient); a helper module, CPU or GPU tensors.

    a_i(p) = < ehat(p), ehat_other(p + o_i) >,  ehat = e / max(|e|, eps)
    r_i(p) = a_i(p) m_i(p) - t_i(p) m_i(p),     L_i = sum w r^2 / N_i,    loss = sum_i lambda_i L_i

with the three borders (CIRCULAR: modular, CROP_ZERO: no pair and a = 0 where the neighbour leaves the volume, REPLICATE: clamped), the
three normalisers (BX, CROPPED, FULL), an optional second operand (detached or not), a u8 or float mask of any value and dloss.  The
pattern is that of _restate / _shifted in tests/test_gpu_act_loss.py without the activation.
"""
import numpy as np
import torch

BORDER_CIRCULAR, BORDER_CROP_ZERO, BORDER_REPLICATE = 0, 1, 2
NORM_BX, NORM_CROPPED, NORM_FULL = 0, 1, 2


def shifted(y, o, border):
    """y [B,D,Z,Y,X] -> (y at p + o, [Z,Y,X] bool: the pair exists)"""
    dims = y.shape[2:]
    ok = torch.ones(tuple(dims), dtype=torch.bool, device=y.device)
    if border == BORDER_CIRCULAR:
        return torch.roll(y, shifts=tuple(-int(v) for v in o), dims=(2, 3, 4)), ok
    out = y
    for ax, v in enumerate(o):
        idx = torch.arange(dims[ax], device=y.device) + int(v)
        inside = (idx >= 0) & (idx < dims[ax])
        out = out.index_select(2 + ax, idx.clamp(0, dims[ax] - 1))
        if border == BORDER_CROP_ZERO:
            shape = [1, 1, 1]
            shape[ax] = dims[ax]
            ok = ok & inside.view(shape)
    return out, ok


def normaliser(norm, B, dims, o):
    if norm == NORM_BX:
        return B * dims[2]
    if norm == NORM_FULL:
        return B * dims[0] * dims[1] * dims[2]
    return B * int(np.prod([dims[a] - abs(int(o[a])) for a in range(3)]))


def inv_norm_plane(E, eps):
    """[B,Z,Y,X] float64: 1 / max(|e|, eps), negated where |e| < eps (include/pea.h, pea_affinity_fwd_ex)"""
    n = E.double().norm(dim=1)
    inv = 1.0 / n.clamp_min(eps)
    return torch.where(n < eps, -inv, inv)


def cosine_loss(E, other, T, W, M, offsets3, lam, eps, border, norm, dloss=None, other_grad=False):
    """E, other [B,D,Z,Y,X]; T, W, M [B,K,Z,Y,X] (M None = ones) -> dict of float64 tensors:
    loss, parts [K] (the un-weighted L_i), affs [B,K,Z,Y,X], de = dloss * d loss / d E, de_other (None unless other_grad)"""
    with torch.enable_grad():
        x = E.detach().double().requires_grad_(True)
        if other is None:
            y = x
        else:
            y = other.detach().double().requires_grad_(bool(other_grad))
        xn = x / x.norm(dim=1, keepdim=True).clamp_min(eps)
        yn = y / y.norm(dim=1, keepdim=True).clamp_min(eps)
        B, dims = x.shape[0], tuple(x.shape[2:])
        loss, parts, maps = 0.0, [], []
        for i, o in enumerate(offsets3):
            ys, ok = shifted(yn, o, border)
            # selects, not "* ok": a pair that does not exist is 0 and has no gradient whatever the clamped index read (NaN * 0 is NaN)
            ys = torch.where(ok, ys, torch.zeros_like(ys))
            a = (xn * ys).sum(1)
            a = torch.where(ok, a, torch.zeros_like(a))
            m = 1.0 if M is None else M[:, i].double()
            r = a * m - T[:, i].double() * m
            r = torch.where(ok, r, torch.zeros_like(r))
            Li = (W[:, i].double() * r * r).sum() / normaliser(norm, B, dims, o)
            loss = loss + float(lam[i]) * Li
            parts.append(Li.detach())
            maps.append(a.detach())
        (loss * (1.0 if dloss is None else float(dloss))).backward()
    return dict(loss=loss.detach(), parts=torch.stack(parts), affs=torch.stack(maps, 1), de=x.grad,
                de_other=y.grad if (other is not None and other_grad) else None)
