"""The discriminative (pull / push) instance loss in float64 numpy, written from the formulas of include/pea_disc.h -- what the GPU
tests compare the kernels with.  tests/test_disc_host.py holds it to the reference's own float64 numbers (tests/golden/gdisc_*.npz)."""
import numpy as np

from conftest import load_golden


def load_disc_golden(name):
    """a gdisc_* fixture with e (float32, from the float16 array that holds it exactly) and de (the reference's float32 gradient, from
    its bit distance to float32(de64)) put back together (tests/golden/make_golden_disc.py)"""
    g = load_golden(name)
    g["e"] = g["e16"].astype(np.float32)
    near = np.ascontiguousarray(g["de64"].astype(np.float32))
    g["de"] = (near.view(np.int32).astype(np.int64) + g["de_ulp"]).astype(np.int32).view(np.float32)
    g["background"] = bool(g["background"])
    return g


def disc_reference(e, labels, background=False, delta_v=0.5, delta_d=1.5, alpha=1.0, beta=1.0, gama=0.001, dloss=1.0, num_ids=None):
    """-> (loss, stats [5 + 4 B], de [B, D, *spatial]) in float64.  stats = (loss, var, dist, reg, n_bad, then var_b, dist_b, reg_b,
    C_b per image).  num_ids: labels outside [0, num_ids) are counted in n_bad and skipped; loss and stats[0..3] are then NaN."""
    e = np.asarray(e, dtype=np.float64)
    B, D = e.shape[:2]
    x = e.reshape(B, D, -1)
    lab = np.asarray(labels).reshape(B, -1).astype(np.int64)
    de = np.zeros_like(x)
    stats = np.zeros(5 + 4 * B)
    n_bad = 0
    for b in range(B):
        ok = np.ones(lab.shape[1], bool) if num_ids is None else (lab[b] >= 0) & (lab[b] < num_ids)
        n_bad += int((~ok).sum())
        ids = [int(c) for c in np.unique(lab[b][ok]) if background or c != 0]
        C = len(ids)
        stats[5 + 4 * b + 3] = C
        if C == 0:
            continue
        mu = np.stack([x[b][:, ok & (lab[b] == c)].mean(axis=1) for c in ids])          # [C, D]
        G = np.zeros_like(mu)                                                           # d loss / d mu_c
        var_b = 0.0
        for i, c in enumerate(ids):
            sel = ok & (lab[b] == c)
            n = int(sel.sum())
            diff = x[b][:, sel] - mu[i][:, None]
            nr = np.sqrt((diff * diff).sum(axis=0))
            h = np.maximum(nr - delta_v, 0.0)
            u = np.divide(diff, nr, out=np.zeros_like(diff), where=nr > 0)
            var_b += (h * h).sum() / n / C
            k = 2.0 * alpha / (B * C * n)
            de[b][:, sel] += k * h * u
            G[i] -= k * (h * u).sum(axis=1)
        dist_b = 0.0
        if C > 1:
            dm = mu[:, None, :] - mu[None, :, :]
            dist = np.sqrt((dm * dm).sum(axis=2))
            hinge = np.maximum(2.0 * delta_d - dist, 0.0)
            np.fill_diagonal(hinge, 0.0)
            dist_b = (hinge * hinge).sum() / (C * (C - 1)) / 2.0
            unit = np.divide(dm, dist[:, :, None], out=np.zeros_like(dm), where=dist[:, :, None] > 0)
            G += -2.0 * beta / (B * C * (C - 1)) * (hinge[:, :, None] * unit).sum(axis=1)
        mn = np.sqrt((mu * mu).sum(axis=1))
        reg_b = mn.sum() / C
        G += gama / (B * C) * np.divide(mu, mn[:, None], out=np.zeros_like(mu), where=mn[:, None] > 0)
        for i, c in enumerate(ids):
            sel = ok & (lab[b] == c)
            de[b][:, sel] += (G[i] / int(sel.sum()))[:, None]
        stats[5 + 4 * b:5 + 4 * b + 3] = var_b, dist_b, reg_b
    per = stats[5:].reshape(B, 4)
    stats[1], stats[2], stats[3] = per[:, 0].sum() / B, per[:, 1].sum() / B, per[:, 2].sum() / B
    stats[0] = alpha * stats[1] + beta * stats[2] + gama * stats[3]
    stats[4] = n_bad
    if n_bad:
        stats[:4] = np.nan
    return float(stats[0]), stats, (dloss * de).reshape(e.shape)
