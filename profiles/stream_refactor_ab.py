#!/usr/bin/env python3
"""The stream refactor (csrc/pea_stream.h: the walks, the tail quad, the wave reductions, the peel, the cropped cursor and the table
workspace of pea_k_metrics.hip, pea_k_fgmask.hip, pea_k_disc.hip and pea_k_segscore.hip stated once): the parent's library against
this tree's, loaded as two ctypes.CDLLs in ONE process, this tree launched twice.

bits    One SHA-256 per output tensor (bytes, so NaN payloads count): workspace tables, loss, stats, dlogits, ctx, de, the stored
        pred, the argmax mask, the rows of pea_seg_scores, the triples of pea_seg_table sorted by key.  The shapes are the smallest at
        which each shared piece can go wrong (the docstrings of lane_run_cases and wave_run_cases); every input pointer 0, 1 and 3
        elements off alignment; a never-initialised workspace for each family.  The contract is 0 digests differ, from the parent
        and between the two launches of this tree.  -> profiles/stream_refactor_bits.json
timing  HIP events around batches of 100 calls, parent and change alternating batch by batch, 7 batches each, at the shapes of the
        families' own A/B records.  Per leg: the change's median lies inside the parent's [min, max] over its batches, or below it.
        -> profiles/stream_refactor_ab.json, every batch in it

  python profiles/stream_refactor_ab.py --parent PATH/libpea_hip.so [--skip-timing]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

RELU, DIVIDE, STORE, MASK_F32 = 1, 2, 4, 8
BACKGROUND, NEED_GRAD = 1, 2
DT = {"f32": (torch.float32, 0), "f16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}
SKEWS = (0, 1, 3)
dev = torch.device("cuda:0")


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def off(t, skew):
    """a copy of t whose first element lies `skew` elements past a 16-byte boundary"""
    if t is None:
        return None
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[skew:skew + t.numel()].view(t.shape)
    v.copy_(t)
    return v


class Book(object):
    """digests of the parent, the change and the change again, case by case"""

    def __init__(self, libs):
        self.libs, self.rows = libs, {k: {} for k in libs}

    def run(self, case, fn):
        for k, L in self.libs.items():
            out = fn(L)
            torch.cuda.synchronize()
            self.rows[k][case] = {o: sha(t) for o, t in out.items()}


def ok(rc, what):
    assert rc == 0, "%s: rc %d" % (what, rc)


def loss_state(L, nb, prepared=True):
    work = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    if prepared:
        ok(L.pea_workspace_init(P(work), nb, None), "pea_workspace_init")
    return work


# ---- the lane-run families -------------------------------------------------------------------------------------------------------------------
def metrics_call(lib, L, B, C, CP, dims, pdims, origin, flags, pred, wmap, tgt, mask, prepared=True):
    d = lib.PeaMetricsDesc()
    d.B, d.C, d.CP, d.flags, d.clip_lo, d.clip_hi = B, C, CP, flags, 0.0, 1.0
    d.dims[:], d.pred_dims[:], d.origin[:] = dims, pdims, origin
    nb = int(L.pea_metrics_workspace_bytes())
    work = loss_state(L, nb, prepared)
    out = torch.full((1 + C, 5), -7.0, dtype=torch.float64, device=dev)
    pv = off(pred, (pred.data_ptr() % 16) // 4) if flags & STORE else pred  # (a copy at the same skew: the input survives the store)
    ok(L.pea_affs_metrics(ctypes.byref(d), P(pv), P(wmap), P(tgt), P(mask), P(out), P(work), nb, None), "pea_affs_metrics")
    res = {"out": out, "state": work}
    if flags & STORE:
        res["pred"] = pv
    return res


def fg_call(lib, L, B, Y, X, code, lcode, lg, lab, origin=(0, 0), out_dims=None, prepared=True):
    d = lib.PeaFgDesc()
    d.B, d.Y, d.X, d.logits_dtype, d.labels_type, d.flags = B, Y, X, code, lcode, 0
    d.origin[:], d.out_dims[:] = list(origin), list(out_dims or (Y, X))
    nb = int(L.pea_fgmask_workspace_bytes())
    work = loss_state(L, nb, prepared)
    loss = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    stats = torch.full((5,), -7.0, dtype=torch.float64, device=dev)
    ok(L.pea_fgmask_loss_fwd(ctypes.byref(d), P(lg), P(lab), P(loss), P(stats), P(work), nb, None), "pea_fgmask_loss_fwd")
    dlg = off(torch.zeros_like(lg), (lg.data_ptr() % 16) // lg.element_size())
    ok(L.pea_fgmask_loss_bwd(ctypes.byref(d), P(lg), P(lab), P(stats), None, P(dlg), None), "pea_fgmask_loss_bwd")
    m = torch.full((B, d.out_dims[0], d.out_dims[1]), 9, dtype=torch.uint8, device=dev)
    m = off(m, (lg.data_ptr() % 16) // lg.element_size())
    ok(L.pea_fgmask_argmax(ctypes.byref(d), P(lg), P(m), None), "pea_fgmask_argmax")
    return {"loss": loss, "stats": stats, "state": work, "dlogits": dlg, "mask": m}


def lane_run_cases(book, lib):
    """metrics and fgmask.  n = 1; n = 4096 exactly (one full run); n = 67 x 71 = 4757 (two workgroups, a last quad of one element); each
    with the base pointers 0, 1 and 3 elements off alignment.  fgmask: f32 / f16 / bf16 logits x i32 / u8 labels, forward, backward and
    argmax, and the three with a crop of origin (1, 2) inside 37 x 53.  metrics: dense with a u8 mask, an f32 mask and no mask; cropped
    without STORE; cropped divide-and-store with C < CP; the two crops with origin (1, 2, 3) in a 5 x 20 x 24 volume.  A NaN and an inf
    sit in every float input."""
    g = torch.Generator().manual_seed(2026)
    for Y, X in ((1, 1), (64, 64), (67, 71)):
        B, C = 2, 3
        pred = (torch.rand((B, C, 1, Y, X), generator=g) * 1.4 - 0.2).to(dev)
        tgt = (torch.rand((B, C, 1, Y, X), generator=g) < 0.5).float().to(dev)
        if Y > 1:
            pred[0, 1, 0, 5, 7], pred[1, 2, 0, 9, 3] = float("nan"), float("inf")
        masks = {"u8": ((torch.rand(pred.shape, generator=g) < 0.8).to(torch.uint8).to(dev), 0),
                 "f32": (torch.rand(pred.shape, generator=g).to(dev), MASK_F32), "none": (None, 0)}
        logits = torch.randn((2, 2, Y, X), generator=g) * 3
        if Y > 1:
            logits[0, 0, 3, 3], logits[1, 1, 6, 2] = float("nan"), float("inf")
        labels = (torch.rand((2, Y, X), generator=g) < 0.3).int() * 5 - (torch.rand((2, Y, X), generator=g) < 0.1).int()
        for skew in SKEWS:
            for mname, (M, mflag) in masks.items():
                a = [off(pred, skew), off(tgt, skew), off(M, skew)]
                book.run("metrics/dense/%dx%d/skew%d/mask_%s" % (Y, X, skew, mname),
                         lambda L, a=a, mflag=mflag: metrics_call(lib, L, B, C, C, [1, Y, X], [1, Y, X], [0, 0, 0], RELU | mflag, a[0], None, a[1], a[2]))
            for dname, (dt, code) in DT.items():
                for lname, lt, lcode in (("i32", torch.int32, 0), ("u8", torch.uint8, 1)):
                    lg = off(logits.to(dt).to(dev), skew)
                    lab = off((labels if lcode == 0 else (labels > 0)).to(lt).to(dev), skew)
                    book.run("fgmask/%dx%d/skew%d/%s_%s" % (Y, X, skew, dname, lname),
                             lambda L, lg=lg, lab=lab, code=code, lcode=lcode: fg_call(lib, L, 2, Y, X, code, lcode, lg, lab))
    # the crops
    Y, X = 37, 53
    logits = torch.randn((2, 2, Y, X), generator=g) * 3
    labels = (torch.rand((2, Y, X), generator=g) < 0.3).int() * 5
    for skew in SKEWS:
        for dname, (dt, code) in DT.items():
            lg, lab = off(logits.to(dt).to(dev), skew), off(labels.to(dev), skew)
            book.run("fgmask/crop/skew%d/%s" % (skew, dname),
                     lambda L, lg=lg, lab=lab, code=code: fg_call(lib, L, 2, Y, X, code, 0, lg, lab, origin=(1, 2), out_dims=(33, 47)))
    PZ, PY, PX, C, CP = 5, 20, 24, 3, 4
    Z, RY, RX = 3, 15, 19
    vol = (torch.rand((1, CP, PZ, PY, PX), generator=g) * 1.4 - 0.2).to(dev)
    vol[0, 1, 2, 4, 5] = float("nan")
    wmap = (torch.rand((PZ, PY, PX), generator=g) + 0.5).to(dev)
    tg3 = (torch.rand((1, C, Z, RY, RX), generator=g) < 0.5).float().to(dev)
    m3 = (torch.rand(tg3.shape, generator=g) < 0.8).to(torch.uint8).to(dev)
    for skew in SKEWS:
        a = [off(vol, skew), off(wmap, skew), off(tg3, skew), off(m3, skew)]
        for name, flags, cp, w in (("crop_relu", RELU, C, None), ("crop_divide", DIVIDE, C, a[1]), ("crop_divide_store", DIVIDE | STORE, CP, a[1]),
                                   ("crop_relu_store", RELU | STORE, CP, None)):
            pv = a[0] if cp == CP else off(vol[:, :C].contiguous(), skew)
            for mname, M in (("u8", a[3]), ("none", None)):
                book.run("metrics/%s/skew%d/mask_%s" % (name, skew, mname),
                         lambda L, flags=flags, cp=cp, w=w, pv=pv, M=M: metrics_call(lib, L, 1, C, cp, [Z, RY, RX], [PZ, PY, PX], [1, 2, 3], flags,
                                                                                    pv, w, a[2], M))
    # a workspace that was never prepared: NaN everywhere
    book.run("metrics/uninitialised", lambda L: metrics_call(lib, L, 1, C, CP, [Z, RY, RX], [PZ, PY, PX], [1, 2, 3], RELU | STORE, vol, None, tg3,
                                                            None, prepared=False))
    lg, lab = logits.to(dev), labels.to(dev)
    book.run("fgmask/uninitialised", lambda L: fg_call(lib, L, 2, Y, X, 0, 0, lg, lab, prepared=False))


# ---- the wave-run families -------------------------------------------------------------------------------------------------------------------
def disc_call(lib, L, e, labels, num_ids, flags, code, prepared=True):
    d = lib.PeaDiscDesc()
    d.B, d.D, d.S, d.num_ids, d.dtype, d.flags = e.shape[0], e.shape[1], e.shape[2], num_ids, code, flags
    d.delta_v, d.delta_d, d.alpha, d.beta, d.gamma = 0.5, 1.5, 1.0, 1.0, 0.001
    nb = int(L.pea_disc_workspace_bytes(ctypes.byref(d)))
    work = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    if prepared:
        ok(L.pea_disc_workspace_init(P(work), nb, None), "pea_disc_workspace_init")
    loss = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    stats = torch.full((5 + 4 * d.B,), -7.0, dtype=torch.float64, device=dev)
    ctx = torch.full((int(L.pea_disc_context_bytes(ctypes.byref(d))) // 8,), -7.0, dtype=torch.float64, device=dev)
    ok(L.pea_disc_loss_fwd(ctypes.byref(d), P(e), P(labels), P(loss), P(stats), P(ctx), P(work), nb, None), "pea_disc_loss_fwd")
    res = {"loss": loss, "stats": stats, "ctx": ctx, "tables": work}
    if flags & NEED_GRAD:
        de = off(torch.zeros_like(e), (e.data_ptr() % 16) // e.element_size())
        ok(L.pea_disc_loss_bwd(ctypes.byref(d), P(e), P(labels), P(ctx), None, P(de), None), "pea_disc_loss_bwd")
        res["de"] = de
    return res


def seg_call(lib, L, pred, gt, capacity, prepared=True):
    d = lib.PeaSegDesc()
    d.B, d.S, d.capacity, d.flags = pred.shape[0], pred.shape[1], capacity, 0
    nb = int(L.pea_seg_workspace_bytes(ctypes.byref(d)))
    work = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    if prepared:
        ok(L.pea_seg_workspace_init(P(work), nb, None), "pea_seg_workspace_init")
    out = torch.full((d.B, lib.SEG_COLS), -7.0, dtype=torch.float64, device=dev)
    ok(L.pea_seg_scores(ctypes.byref(d), P(pred), P(gt), P(out), P(work), nb, None), "pea_seg_scores")
    # Where an image's table overflows, WHICH pairs were dropped depends on the order in which the waves arrive (pea_segscore.h), so
    # n_overflow and the triples are not reproducible from run to run of ONE library; of such an image the record keeps that it
    # overflowed, n_bad and the NaN columns.
    over = out[:, 0] > 0
    res = {"out": torch.where(over[:, None] & (torch.arange(lib.SEG_COLS, device=dev) == 0)[None, :], torch.ones_like(out), out)}
    n_max = int(min(capacity, d.S))
    for b in range(d.B):
        ids = torch.zeros((2, n_max), dtype=torch.int32, device=dev)
        counts = torch.zeros(n_max, dtype=torch.int64, device=dev)
        n_out = torch.full((3,), -7, dtype=torch.int64, device=dev)
        ok(L.pea_seg_table(ctypes.byref(d), P(pred), P(gt), b, P(ids[0]), P(ids[1]), P(counts), P(n_out), n_max, P(work), nb, None), "pea_seg_table")
        if int(n_out[1]) > 0:  # (overflowed: see above)
            res["triples%d" % b] = torch.stack([n_out[1] > 0, n_out[2]]).to(torch.int64)
            continue
        n = max(0, min(n_max, int(n_out[0])))
        key = (ids[0, :n].long() << 32) | ids[1, :n].long()
        order = torch.argsort(key)
        res["triples%d" % b] = torch.cat([key[order], counts[:n][order], n_out])  # (slot placement depends on arrival order: sorted by key)
    res["tables"] = work
    return res


def blocky(g, B, S, n_ids, run):
    """labels that change every `run` pixels or so, ids in [0, n_ids)"""
    ids = torch.randint(0, n_ids, (B, (S + run - 1) // run), generator=g)
    return ids.repeat_interleave(run, dim=1)[:, :S].to(torch.int32).contiguous()


def wave_run_cases(book, lib):
    """disc and segscore.  S = 1; S = 256 (one full wave); S = 1024 (one full workgroup); S = 70 x 61 = 4270 (a fifth workgroup whose
    first wave ends in a quad of two); the pointers 0, 1 and 3 elements off alignment.  disc: D = 1, 5 (a partial last channel group),
    16, 64, with and without PEA_DISC_BACKGROUND and PEA_DISC_NEED_GRAD, f32 and bf16, B = 2; 400 ids in 40 x 40 (every pixel of a wave
    has another id: 256 rounds of the peel).  segscore: a wave with more than 64 distinct (pred, gt) keys (checked here on the CPU), negative ids in
    one image of two, a capacity of 64 that overflows."""
    g = torch.Generator().manual_seed(2027)
    for S in (1, 256, 1024, 4270):
        labels = blocky(g, 2, S, 48, 7)
        for D in (1, 5, 16, 64):
            e32 = torch.randn((2, D, S), generator=g)
            for dname in ("f32", "bf16"):
                dt, code = DT[dname]
                for skew in SKEWS:
                    e, lab = off(e32.to(dt).to(dev), skew), off(labels.to(dev), skew)
                    for flags in (0, BACKGROUND, NEED_GRAD, BACKGROUND | NEED_GRAD):
                        book.run("disc/S%d/D%d/%s/skew%d/flags%d" % (S, D, dname, skew, flags),
                                 lambda L, e=e, lab=lab, flags=flags, code=code: disc_call(lib, L, e, lab, 48, flags, code))
        pred, gt = blocky(g, 2, S, 30, 5), blocky(g, 2, S, 30, 9)
        for skew in SKEWS:
            p, q = off(pred.to(dev), skew), off(gt.to(dev), skew)
            book.run("seg/S%d/skew%d" % (S, skew), lambda L, p=p, q=q: seg_call(lib, L, p, q, 1024))  # (at most 900 pairs)
    # 400 ids in 40 x 40: every pixel of a wave's 256 has another id
    labels = (torch.arange(1600) % 400).to(torch.int32).reshape(1, 1600).repeat(2, 1).contiguous().to(dev)
    e = torch.randn((2, 16, 1600), generator=g).to(dev)
    for flags in (NEED_GRAD, BACKGROUND | NEED_GRAD):
        book.run("disc/cache_overflow/flags%d" % flags, lambda L, flags=flags: disc_call(lib, L, e, labels, 512, flags, 0))
    # segscore: more than 64 keys in one wave, so that the flush at lane 64 runs
    S = 4270
    pred = (torch.arange(S) // 2).to(torch.int32).reshape(1, S).repeat(2, 1).contiguous()
    gt = (torch.arange(S) // 3).to(torch.int32).reshape(1, S).repeat(2, 1).contiguous()
    keys = {(int(a), int(b)) for a, b in zip(pred[0, :256], gt[0, :256])}
    assert len(keys) > 64, len(keys)
    book.run("seg/flush", lambda L: seg_call(lib, L, pred.to(dev), gt.to(dev), 4096))
    book.run("seg/overflow_capacity64", lambda L: seg_call(lib, L, pred.to(dev), gt.to(dev), 64))
    neg = blocky(g, 2, S, 30, 5)
    neg[1, 100:140] = -3
    pos = blocky(g, 2, S, 30, 9)
    book.run("seg/negative_ids", lambda L: seg_call(lib, L, neg.to(dev), pos.to(dev), 1024))
    book.run("seg/uninitialised", lambda L: seg_call(lib, L, pos.to(dev), pos.to(dev), 256, prepared=False))
    lab = blocky(g, 2, 1024, 48, 7).to(dev)
    e = torch.randn((2, 5, 1024), generator=g).to(dev)
    book.run("disc/uninitialised", lambda L: disc_call(lib, L, e, lab, 48, NEED_GRAD, 0, prepared=False))


# ---- timing ----------------------------------------------------------------------------------------------------------------------------------
def legs(lib):
    """name -> f(L): one call of the leg on library L, at the shapes of the families' own A/B records"""
    g = torch.Generator().manual_seed(7)
    out = {}
    # metrics at 1 x 10 x 544 x 544, relu + store
    pred = (torch.rand((1, 10, 1, 544, 544), generator=g) * 1.4 - 0.2).to(dev)
    tgt = (torch.rand(pred.shape, generator=g) < 0.5).float().to(dev)
    msk = (torch.rand(pred.shape, generator=g) < 0.8).to(torch.uint8).to(dev)
    md = lib.PeaMetricsDesc()
    md.B, md.C, md.CP, md.flags, md.clip_lo, md.clip_hi = 1, 10, 10, RELU | STORE, 0.0, 1.0
    md.dims[:], md.pred_dims[:], md.origin[:] = [1, 544, 544], [1, 544, 544], [0, 0, 0]
    mout = torch.zeros((11, 5), dtype=torch.float64, device=dev)
    # fgmask forward + backward at 8 x 2 x 256 x 256
    lg = (torch.randn((8, 2, 256, 256), generator=g) * 3).to(dev)
    fl = ((torch.rand((8, 256, 256), generator=g) < 0.3).int() * 5).to(dev)
    fd = lib.PeaFgDesc()
    fd.B, fd.Y, fd.X, fd.logits_dtype, fd.labels_type, fd.flags = 8, 256, 256, 0, 0, 0
    fd.origin[:], fd.out_dims[:] = [0, 0], [256, 256]
    floss, fstats, dlg = torch.zeros(1, device=dev), torch.zeros(5, dtype=torch.float64, device=dev), torch.zeros_like(lg)
    # disc forward + backward at 8 x 16 x 256 x 256, about 40 ids per image (blocks of 41 x 41 pixels)
    yy, xx = torch.meshgrid(torch.arange(256) // 41, torch.arange(256) // 41, indexing="ij")
    dl = ((yy * 7 + xx) + 1).to(torch.int32).reshape(1, -1).repeat(8, 1).contiguous().to(dev)
    de_in = torch.randn((8, 16, 256 * 256), generator=g).to(dev)
    dd = lib.PeaDiscDesc()
    dd.B, dd.D, dd.S, dd.num_ids, dd.dtype, dd.flags = 8, 16, 256 * 256, 64, 0, NEED_GRAD
    dd.delta_v, dd.delta_d, dd.alpha, dd.beta, dd.gamma = 0.5, 1.5, 1.0, 1.0, 0.001
    dloss, dstats, dde = torch.zeros(1, device=dev), torch.zeros(5 + 32, dtype=torch.float64, device=dev), torch.zeros_like(de_in)
    # pea_seg_scores at 1 x 544 x 544, capacity 16384 (profiles/segscore_ab.json: cvppp_1x544x544)
    sy, sx = torch.meshgrid(torch.arange(544) // 130, torch.arange(544) // 130, indexing="ij")
    sp = (sy * 5 + sx).to(torch.int32).reshape(1, -1).contiguous().to(dev)
    sg_ = ((sy * 5 + sx + (torch.arange(544)[None, :] // 61) % 3)).to(torch.int32).reshape(1, -1).contiguous().to(dev)
    sd = lib.PeaSegDesc()
    sd.B, sd.S, sd.capacity, sd.flags = 1, 544 * 544, 16384, 0
    sout = torch.zeros((1, lib.SEG_COLS), dtype=torch.float64, device=dev)
    state = {}

    def ws(L, key, nb, init):  # ONE block per leg for both libraries (a call leaves it prepared; the layouts and magic words are equal):
        w = state.get(key)     # with a block each, the disc leg read 0.6 % apart on byte-identical kernels
        if w is None:
            w = state[key] = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
            ok(init(P(w), nb, None), key)
        return w

    def metrics(L):
        nb = int(L.pea_metrics_workspace_bytes())
        ok(L.pea_affs_metrics(ctypes.byref(md), P(pred), None, P(tgt), P(msk), P(mout), P(ws(L, "metrics", nb, L.pea_workspace_init)), nb, None), "metrics")

    def fgmask(L):
        nb = int(L.pea_fgmask_workspace_bytes())
        ok(L.pea_fgmask_loss_fwd(ctypes.byref(fd), P(lg), P(fl), P(floss), P(fstats), P(ws(L, "fg", nb, L.pea_workspace_init)), nb, None), "fg fwd")
        ok(L.pea_fgmask_loss_bwd(ctypes.byref(fd), P(lg), P(fl), P(fstats), None, P(dlg), None), "fg bwd")

    def disc(L):
        nb = int(L.pea_disc_workspace_bytes(ctypes.byref(dd)))
        ctx = ws(L, "disc_ctx", int(L.pea_disc_context_bytes(ctypes.byref(dd))), lambda *a: 0)
        ok(L.pea_disc_loss_fwd(ctypes.byref(dd), P(de_in), P(dl), P(dloss), P(dstats), P(ctx), P(ws(L, "disc", nb, L.pea_disc_workspace_init)), nb, None),
           "disc fwd")
        ok(L.pea_disc_loss_bwd(ctypes.byref(dd), P(de_in), P(dl), P(ctx), None, P(dde), None), "disc bwd")

    def seg(L):
        nb = int(L.pea_seg_workspace_bytes(ctypes.byref(sd)))
        ok(L.pea_seg_scores(ctypes.byref(sd), P(sp), P(sg_), P(sout), P(ws(L, "seg", nb, L.pea_seg_workspace_init)), nb, None), "seg")

    out["metrics_1x10x544x544_relu_store"] = metrics
    out["fgmask_fwd_bwd_8x2x256x256"] = fgmask
    out["disc_fwd_bwd_8x16x256x256_40ids"] = disc
    out["seg_scores_1x544x544_cap16384"] = seg
    return out


def timing(libs, lib, batches=7, reps=100):
    rec = {}
    for name, f in legs(lib).items():
        per = {k: [] for k in libs}
        for L in libs.values():  # warm-up: the workspaces, the code objects
            for _ in range(5):
                f(L)
        torch.cuda.synchronize()
        for i in range(batches):
            for k, L in (list(libs.items())[::-1] if i % 2 else libs.items()):  # the order flips every round
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(reps):
                    f(L)
                t1.record()
                t1.synchronize()
                per[k].append(t0.elapsed_time(t1) * 1000.0 / reps)
        med = {k: statistics.median(v) for k, v in per.items()}
        lo, hi = min(per["parent"]), max(per["parent"])
        rec[name] = {"us_per_call_batches": {k: [round(x, 3) for x in v] for k, v in per.items()},
                     "median_us": {k: round(v, 3) for k, v in med.items()}, "parent_min_max_us": [round(lo, 3), round(hi, 3)],
                     "change_median_inside_or_below": bool(med["change"] <= hi)}
        print("%-40s parent %.2f [%.2f, %.2f]  change %.2f  %s" % (name, med["parent"], lo, hi, med["change"],
                                                                   "ok" if med["change"] <= hi else "ABOVE"))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libpea_hip.so built from the parent commit")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--skip-timing", action="store_true")
    a = ap.parse_args()
    t0 = time.time()
    pkg = ge.load_package()
    lib = pkg._lib
    change = lib.lib()
    parent = ctypes.CDLL(os.path.abspath(a.parent))
    assert os.path.realpath(a.parent) != os.path.realpath(lib.SO_PATH)
    for f in dir(change):  # the same prototypes on both handles
        if f.startswith("pea_"):
            getattr(parent, f).restype, getattr(parent, f).argtypes = getattr(change, f).restype, getattr(change, f).argtypes
    os.makedirs(a.out_dir, exist_ok=True)
    book = Book({"parent": parent, "change": change, "change_again": change})
    lane_run_cases(book, lib)
    wave_run_cases(book, lib)
    par = book.rows["parent"]
    differ = sorted("%s:%s:%s" % (k, c, o) for k in ("change", "change_again") for c in par for o in set(par[c]) | set(book.rows[k][c])
                    if par[c].get(o) != book.rows[k][c].get(o))
    assert book.rows["change"].keys() == book.rows["change_again"].keys() == par.keys()
    differ += sorted("again:%s:%s" % (c, o) for c in par for o in book.rows["change"][c] if book.rows["change"][c][o] != book.rows["change_again"][c].get(o))
    n = sum(len(v) for v in par.values())
    groups = {}  # the record keeps one digest per family and kind of case: SHA-256 over its cases' output digests in sorted order
    for c in sorted(par):
        key = "/".join(c.split("/")[:2]) if c.split("/")[1] in ("crop", "dense", "uninitialised", "cache_overflow", "flush") else c.split("/")[0]
        h = groups.setdefault(key, [hashlib.sha256(), 0])
        for o in sorted(par[c]):
            h[0].update(("%s:%s=%s\n" % (c, o, book.rows["change"][c][o])).encode())
            h[1] += 1
    rec = {"what": "SHA-256 of every output tensor: parent library, this tree, this tree again, one process; every digest is compared, kept is one "
                   "per group of cases", "device": torch.cuda.get_device_name(0), "cases": len(par), "digests": n, "differ": differ,
           "seconds": round(time.time() - t0, 1), "groups": {k: "%d %s" % (v[1], v[0].hexdigest()) for k, v in groups.items()}}
    json.dump(rec, open(os.path.join(a.out_dir, "stream_refactor_bits.json"), "w"), indent=1)
    print("bits: %d cases, %d digests, %d differ, %.1f s" % (len(par), n, len(differ), time.time() - t0))
    for c in differ[:40]:
        print("  differs:", c)
    if not a.skip_timing:
        trec = {"what": "HIP events around batches of 100 calls; parent library and this tree alternate batch by batch in one process; 7 batches each",
                "device": torch.cuda.get_device_name(0), "legs": timing({"parent": parent, "change": change}, lib)}
        json.dump(trec, open(os.path.join(a.out_dir, "stream_refactor_ab.json"), "w"), indent=1)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
