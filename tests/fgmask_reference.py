"""A float64 numpy restatement of the closed form of include/pea_fgmask.h (a plain helper, no GPU):

    y = [label > 0],  d = l1 - l0,  nll = softplus(d) for y = 0, softplus(-d) for y = 1   (max(z, 0) + log1p(exp(-|z|)))
    loss = S0 / (2 n0) + S1 / (2 n1);  dl1 = (p1 - y) c_y,  dl0 = -dl1,  p1 = 1 / (1 + exp(-d)),  c_y = dloss / (2 n_y)

with both rules for an absent class: the reference's (0 / 0: NaN loss, every gradient element NaN) and skip_empty (the absent class
counts 0, the class that is present keeps its c_y).

    loss, stats, dlogits = fgmask_reference(logits, labels, dloss=1.0, skip_empty=False)     # float64; stats = (loss, S0/n0, S1/n1, n0, n1)
    mask = mask_reference(logits, crop=((top, bottom), (left, right)))                      # uint8 [B, H', W']
"""
import numpy as np


def fgmask_reference(logits, labels, dloss=1.0, skip_empty=False):
    l = np.asarray(logits).astype(np.float64)
    y = np.asarray(labels) > 0
    assert l.ndim == 4 and l.shape[1] == 2 and y.shape == (l.shape[0],) + l.shape[2:]
    with np.errstate(all="ignore"):
        d = l[:, 1] - l[:, 0]
        z = np.where(y, -d, d)
        nll = np.where(z > 0, z, 0.0) + np.log1p(np.exp(-np.abs(z)))
        n1, n0 = float(y.sum()), float((~y).sum())
        S0, S1 = float(nll[~y].sum()), float(nll[y].sum())
        t0 = 0.0 if (skip_empty and n0 == 0) else np.float64(S0) / np.float64(n0)
        t1 = 0.0 if (skip_empty and n1 == 0) else np.float64(S1) / np.float64(n1)
        loss = 0.5 * (t0 + t1)
        if not skip_empty and (n0 == 0 or n1 == 0):
            c0 = c1 = np.nan
        else:
            c0, c1 = np.float64(dloss) / np.float64(2.0 * n0), np.float64(dloss) / np.float64(2.0 * n1)
        s = 1.0 / (1.0 + np.exp(-z))                 # the softmax of the wrong class: p1 for y = 0, 1 - p1 for y = 1
        q = np.where(y, -s * c1, s * c0)             # (p1 - y) c_y
    dlogits = np.stack([-q, q], axis=1)
    return float(loss), np.array([loss, t0, t1, n0, n1], dtype=np.float64), dlogits


def mask_reference(logits, crop=((0, 0), (0, 0))):
    l = np.asarray(logits).astype(np.float64)
    (top, bottom), (left, right) = crop
    with np.errstate(invalid="ignore"):
        m = (l[:, 1] > l[:, 0]).astype(np.uint8)     # a tie or a NaN: 0
    return np.ascontiguousarray(m[:, top:m.shape[1] - bottom, left:m.shape[2] - right])
