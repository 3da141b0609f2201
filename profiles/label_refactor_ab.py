#!/usr/bin/env python3
"""The label refactor (csrc/pea_carve.h: one carver for the workspace blocks; csrc/pea_stream.h: one workgroup scan, one set of relaxed
accesses, one launch chain, for pea_k_disc.hip, pea_k_segscore.hip, pea_k_instscore.hip, pea_k_cc.hip, pea_k_rag.hip and pea_k_ws.hip):
the parent's library against this tree's, loaded as two ctypes.CDLLs in ONE process, this tree launched twice.  Written after
profiles/stream_refactor_ab.py, whose helpers and disc / segscore calls it reuses.

bits    One SHA-256 per output tensor of every entry point of the six families, at the smallest shapes of their own A/B scripts and
        at the scan-boundary cases of the tests (ids on both sides of a 2048-id step of k_rag_scan and k_inst_scan, more than 256 chunk
        totals in k_cc_scan, 257 planes in k_ws_offsets); every input pointer 0, 1 and 3 elements off alignment.  Hash tables are
        digested as the families' A/B scripts digest them: rows sorted by key, not slots.  The contract is 0 digests differ, from the
        parent and between the two launches of this tree.  -> profiles/label_refactor_bits.json
timing  HIP events around batches of calls, parent and change alternating batch by batch, 7 batches each, at the shapes of
        profiles/cc_ab.py, ws_ab.py, rag_ab.py, instscore_ab.py, segscore_ab.py and disc_ab.py (--large adds their largest legs).  Per
        leg: the change's median lies inside the parent's [min, max] over its batches, or below it.  A leg that fails is reported, not
        retried.  -> profiles/label_refactor_ab.json, every batch in it

The script sets no time limits of its own and stops at the first call that fails.  Run its two steps as two processes, each under a
limit, the second only after the first has ended well:

  timeout -k 10 420 python profiles/label_refactor_ab.py --parent PATH/libpea_hip.so --skip-timing &&
  timeout -k 10 420 python profiles/label_refactor_ab.py --parent PATH/libpea_hip.so --skip-bits [--large]"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as ge  # noqa: E402
import cc_ab  # noqa: E402
import instscore_ab  # noqa: E402
import rag_ab  # noqa: E402
import ws_ab  # noqa: E402
from stream_refactor_ab import NEED_GRAD, SKEWS, Book, P, blocky, dev, disc_call, off, ok, seg_call  # noqa: E402

STACK_IDS, FIELD = 1, 2
RAG_OUT = (("uv", torch.int32, 2), ("size", torch.int64, 1), ("count", torch.int64, 1), ("mean", torch.float64, 1), ("bmean", torch.float64, 1),
           ("min", torch.float32, 1), ("max", torch.float32, 1))


def like(t, skew, fill=0):
    """an output tensor of t's shape and dtype, `skew` elements past a 16-byte boundary, filled"""
    return off(torch.full(t.shape, fill, dtype=t.dtype, device=dev), skew)


def scratch(nb):
    """an unprepared workspace: every byte 0x5a"""
    return torch.full((nb // 4 + 2,), 0x5a5a5a5a, dtype=torch.int32, device=dev)


# ---- the calls, on one library handle ---------------------------------------------------------------------------------------------------------
def cc_desc(lib, x, conn, min_size):
    d = lib.PeaCcDesc()
    d.ndim, d.B, d.in_type, d.connectivity, d.min_size, d.flags = x.dim() - 1, x.shape[0], (1 if x.dtype == torch.int32 else 0), conn, min_size, 0
    d.dims[:] = [1 if x.dim() == 3 else x.shape[1], x.shape[-2], x.shape[-1]]
    return d


def cc_call(lib, L, x, conn, min_size, skew=0):
    d = cc_desc(lib, x, conn, min_size)
    nb = int(L.pea_cc_workspace_bytes(ctypes.byref(d)))
    labels, mask = like(x.to(torch.int32), skew, -7), like(x.to(torch.uint8), skew, 9)
    counts = torch.full((d.B, 2), -7, dtype=torch.int32, device=dev)
    ok(L.pea_cc_label(ctypes.byref(d), P(x), P(labels), P(mask), P(counts), P(scratch(nb)), nb, None), "pea_cc_label")
    return {"labels": labels, "mask": mask, "counts": counts}


def ws_desc(lib, shape, threshold=.25, ss=2., sw=2., alpha=.9, mc=2, sc=1, min_size=0, flags=0):
    d = lib.PeaWsDesc()
    d.N, d.Y, d.X = shape
    d.threshold, d.sigma_seeds, d.sigma_weights, d.alpha = threshold, ss, sw, alpha
    d.maxima_connectivity, d.seed_connectivity, d.min_size, d.flags = mc, sc, min_size, flags
    return d


def ws_seeds_call(lib, L, b, skew=0, **kw):
    d = ws_desc(lib, b.shape, **kw)
    field = bool(d.flags & FIELD)
    nb = int(L.pea_ws_seeds_workspace_bytes(ctypes.byref(d)))
    dt2 = None if field else like(b.to(torch.int32), skew, -7)
    dts, seeds = like(b, skew, -7.0), like(b.to(torch.int32), skew, -7)
    hmap = None if field else like(b, skew, -7.0)
    counts = torch.full((d.N,), -7, dtype=torch.int32, device=dev)
    ok(L.pea_ws_seeds(ctypes.byref(d), P(b), P(dt2), P(dts), P(hmap), P(seeds), P(counts), P(scratch(nb)), nb, None), "pea_ws_seeds")
    res = {"dts": dts, "seeds": seeds, "counts": counts}
    if not field:
        res.update(dt2=dt2, hmap=hmap)
    return res


def ws_flood_call(lib, L, hmap, seeds, min_size, flags, skew=0):
    d = ws_desc(lib, hmap.shape, min_size=min_size, flags=flags)
    nb = int(L.pea_ws_flood_workspace_bytes(ctypes.byref(d)))
    labels = like(seeds, skew, -7)
    counts, stats = (torch.full((d.N, 2), -7, dtype=torch.int32, device=dev) for _ in range(2))
    ok(L.pea_ws_flood(ctypes.byref(d), P(hmap), P(seeds), P(labels), P(counts), P(stats), P(scratch(nb)), nb, None), "pea_ws_flood")
    return {"labels": labels, "counts": counts, "stats": stats}


def rag_desc(lib, F, offsets, max_id, capacity, max_edges, flags):
    B, Z, Y, X = F.shape
    d = lib.PeaRagDesc()
    d.ndim, d.B, d.K, d.max_id, d.capacity, d.max_edges, d.flags = (2 if Z == 1 else 3), B, len(offsets), max_id, capacity, max_edges, flags
    d.dims[:] = [Z, Y, X]
    for k, o in enumerate(offsets):
        d.offsets[k][:] = list(o)
    return d


def rag_call(lib, L, F, A, offsets, Bd, max_id, capacity, max_edges, flags=0, skew=0, prepared=True):
    """pea_rag_build (the outputs are rows sorted by (u, v): no slot order in them) and pea_rag_project"""
    d = rag_desc(lib, F, offsets, max_id, capacity, max_edges, flags)
    nb = int(L.pea_rag_workspace_bytes(ctypes.byref(d)))
    work = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    if prepared:
        ok(L.pea_rag_workspace_init(P(work), nb, None), "pea_rag_workspace_init")
    out = {n: off(torch.full((d.B, max_edges, w), -7, dtype=dt, device=dev), skew if dt in (torch.int32, torch.float32) else 2 * (skew % 2))
           for n, dt, w in RAG_OUT}
    out["node_size"] = torch.full((d.B, max_id + 1), -7, dtype=torch.int64, device=dev)
    out["stats"] = torch.full((d.B, 8), -7, dtype=torch.int64, device=dev)
    io = lib.PeaRagBuffers()
    io.fragments, io.affs, io.boundary = F.data_ptr(), (A.data_ptr() if A is not None else None), (Bd.data_ptr() if Bd is not None else None)
    for n, t in out.items():
        setattr(io, n, t.data_ptr())
    ok(L.pea_rag_build(ctypes.byref(d), ctypes.byref(io), P(work), nb, None), "pea_rag_build")
    out["tables"] = work
    node_labels = ((torch.arange(max_id + 1, device=dev) * 7 + 3) % 11).to(torch.int32)
    seg, n_bad = like(F, skew, -7), torch.full((1,), -7, dtype=torch.int64, device=dev)
    ok(L.pea_rag_project(F.numel(), P(F), P(node_labels), max_id + 1, P(seg), P(n_bad), None), "pea_rag_project")
    out.update(seg=seg, n_bad=n_bad)
    return out


def inst_call(lib, L, pred, gt, capacity, max_id, prepared=True):
    d = lib.PeaInstDesc()
    d.B, d.S, d.capacity, d.max_id, d.match_iou, d.flags = pred.shape[0], pred.shape[1], capacity, max_id, 0.5, 0
    nb = int(L.pea_inst_workspace_bytes(ctypes.byref(d)))
    work = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    if prepared:
        ok(L.pea_inst_workspace_init(P(work), nb, None), "pea_inst_workspace_init")
    out = torch.full((d.B, lib.INST_COLS), -7.0, dtype=torch.float64, device=dev)
    am, pm = (torch.full((d.B, max_id + 1), -7, dtype=torch.int32, device=dev) for _ in range(2))
    ok(L.pea_inst_scores(ctypes.byref(d), P(pred), P(gt), P(out), P(am), P(pm), P(work), nb, None), "pea_inst_scores")
    return {"out": out, "aji_match": am, "pq_match": pm, "tables": work}


# ---- bits -----------------------------------------------------------------------------------------------------------------------------------------
def bits_cases(book, lib, synth):
    g = torch.Generator().manual_seed(2028)
    # cc: the smallest legs of profiles/cc_ab.py; 513 x 512 with an isolated pixel every third row and column (more than 256 chunk totals)
    masks = {"bbbc_8x256x256": (torch.from_numpy(cc_ab.make_mask(synth, "bbbc_8x256x256")), 2, 25),
             "vol_1x18x160x160": (torch.from_numpy(cc_ab.make_mask(synth, "vol_1x18x160x160")), 1, 25)}
    dots = torch.zeros((1, 513, 512), dtype=torch.uint8)
    dots[:, ::3, ::3] = 1
    masks["dots_1x513x512"] = (dots, 2, 0)
    for name, (m, conn, ms) in masks.items():
        for skew in SKEWS:
            for tname, x in (("u8", m), ("i32", m.to(torch.int32) * 5)):
                xs = off(x.to(dev), skew)
                book.run("cc/%s/%s/skew%d" % (name, tname, skew), lambda L, xs=xs, conn=conn, ms=ms, skew=skew: cc_call(lib, L, xs, conn, ms, skew))
    # ws: the smallest leg of profiles/ws_ab.py, seeds then the flood on what the parent's seeds call gave; a field; 257 planes of 2 x 2
    b = torch.from_numpy(ws_ab.make_boundary(synth, "ac3_18x160x160"))
    for skew in SKEWS:
        bs = off(b.to(dev), skew)
        book.run("ws/seeds/ac3_18x160x160/skew%d" % skew, lambda L, bs=bs, skew=skew: ws_seeds_call(lib, L, bs, skew))
        book.run("ws/seeds/field/skew%d" % skew, lambda L, bs=bs, skew=skew: ws_seeds_call(lib, L, bs, skew, ss=1., sw=0., alpha=0., flags=FIELD))
        s = ws_seeds_call(lib, book.libs["parent"], bs, skew)
        for ms, flags in ((0, 0), (100, STACK_IDS)):
            book.run("ws/flood/ac3_18x160x160/min%d/skew%d" % (ms, skew),
                     lambda L, s=s, ms=ms, flags=flags, skew=skew: ws_flood_call(lib, L, s["hmap"], s["seeds"], ms, flags, skew))
    h = torch.zeros((257, 2, 2), dtype=torch.float32, device=dev)
    sd = torch.zeros((257, 2, 2), dtype=torch.int32, device=dev)
    sd[:, 1, 0] = 3
    book.run("ws/flood/257_planes_stacked", lambda L: ws_flood_call(lib, L, h, sd, 0, STACK_IDS))
    # rag: the smallest legs of profiles/rag_ab.py; 48 x 48 singletons (ids 0 .. 2303); ids 2047, 2048, 2049 alone
    for name in ("cells_1x520x696", "vol_2x18x160x160"):
        F, A, Bd = rag_ab.make_inputs(synth, name, dev)
        kw = rag_ab.LEGS[name]
        for skew in SKEWS:
            a = [off(F, skew), off(A, skew), off(Bd, skew)]
            book.run("rag/%s/skew%d" % (name, skew), lambda L, a=a, kw=kw, skew=skew, mid=int(F.max()): rag_call(
                lib, L, a[0], a[1], kw["offsets"], a[2], mid, kw["capacity"], kw["capacity"] // 2, 1, skew))
    own = torch.arange(48 * 48, dtype=torch.int32).reshape(1, 1, 48, 48).to(dev)
    A = torch.rand((1, 2, 1, 48, 48), generator=g).to(dev)
    offs = [[0, -1, 0], [0, 0, -1]]
    few = torch.tensor([[2047, 2048, 2049, 2049], [2049, 2047, 2048, 2048]], dtype=torch.int32).reshape(1, 1, 2, 4).to(dev)
    for skew in SKEWS:
        a = [off(own, skew), off(A, skew), off(few, skew), off(A[..., :2, :4].contiguous(), skew)]
        book.run("rag/singletons_48x48/skew%d" % skew, lambda L, a=a, skew=skew: rag_call(lib, L, a[0], a[1], offs, a[1][:, 0], 2303, 8192, 4600, 0, skew))
        book.run("rag/ids_2047_2048_2049/skew%d" % skew, lambda L, a=a, skew=skew: rag_call(lib, L, a[2], a[3], offs, None, 2049, 64, 8, 0, skew))
    book.run("rag/uninitialised", lambda L: rag_call(lib, L, few, None, [], None, 2049, 64, 8, prepared=False))
    # inst: the smallest leg of profiles/instscore_ab.py; gt ids 63, 64, 65, 2047, 2048, 2049 at max_id 2047, 2048, 2049
    kw = instscore_ab.LEGS["bbbc_8x256x256"]
    gt = torch.from_numpy(instscore_ab.nuclei(700, kw["B"], kw["Y"], kw["X"], kw["n"], kw["radius"])).reshape(kw["B"], -1).to(torch.int32)
    pred = torch.from_numpy(instscore_ab.nuclei(700, kw["B"], kw["Y"], kw["X"], kw["n"], kw["radius"], jitter=3, drop=2)).reshape(kw["B"], -1).to(torch.int32)
    ids = (63, 64, 65, 2047, 2048, 2049)
    g2, p2 = torch.zeros((2, 16, 16), dtype=torch.int32), torch.zeros((2, 16, 16), dtype=torch.int32)
    for k, j in enumerate(ids):
        g2[0, 2 * k + 1:2 * k + 3, 2:14] = j
        p2[0, 2 * k + 1:2 * k + 3, 1:9], p2[0, 2 * k + 1:2 * k + 3, 9:15] = ids[5 - k], 7 + k
    g2[1], p2[1] = torch.where(g2[0] > 2047, 0, g2[0]), torch.where(p2[0] > 2047, 3, p2[0])
    for skew in SKEWS:
        a = [off(pred.to(dev), skew), off(gt.to(dev), skew), off(p2.reshape(2, -1).to(dev), skew), off(g2.reshape(2, -1).to(dev), skew)]
        book.run("inst/bbbc_8x256x256/skew%d" % skew, lambda L, a=a, mid=int(max(pred.max(), gt.max())): inst_call(lib, L, a[0], a[1], 2048, mid))
        for mid in (2047, 2048, 2049):
            book.run("inst/scan_step/max_id%d/skew%d" % (mid, skew), lambda L, a=a, mid=mid: inst_call(lib, L, a[2], a[3], 256, mid))
    book.run("inst/uninitialised", lambda L: inst_call(lib, L, p2.reshape(2, -1).to(dev), g2.reshape(2, -1).to(dev), 256, 2049, prepared=False))
    # seg and disc: the calls of profiles/stream_refactor_ab.py (scores, sorted triples, tables; loss, stats, ctx, de, tables)
    for S in (1024, 4270):
        p, q = blocky(g, 2, S, 30, 5), blocky(g, 2, S, 30, 9)
        labels = blocky(g, 2, S, 48, 7)
        e = torch.randn((2, 16, S), generator=g)
        for skew in SKEWS:
            a = [off(p.to(dev), skew), off(q.to(dev), skew), off(e.to(dev), skew), off(labels.to(dev), skew)]
            book.run("seg/S%d/skew%d" % (S, skew), lambda L, a=a: seg_call(lib, L, a[0], a[1], 1024))
            for flags in (0, NEED_GRAD):
                book.run("disc/S%d/skew%d/flags%d" % (S, skew, flags), lambda L, a=a, flags=flags: disc_call(lib, L, a[2], a[3], 48, flags, 0))


# ---- timing ---------------------------------------------------------------------------------------------------------------------------------------
def legs(lib, synth, large):
    """name -> (f(L): one call of the leg on library L, calls per batch), at the shapes of the families' own A/B records"""
    out = {}
    g = torch.Generator().manual_seed(7)

    def keep(nb):  # one block per leg for both libraries: the layouts are equal
        return torch.zeros(nb // 8 + 1, dtype=torch.float64, device=dev)

    for name, kw in cc_ab.LEGS.items():
        x = torch.from_numpy(cc_ab.make_mask(synth, name)).to(dev)
        d = cc_desc(lib, x, kw["connectivity"], kw["min_size"])
        st = dict(labels=torch.zeros(x.shape, dtype=torch.int32, device=dev), mask=torch.zeros_like(x), counts=torch.zeros((d.B, 2), dtype=torch.int32, device=dev))

        def cc(L, x=x, d=d, st=st):
            nb = int(L.pea_cc_workspace_bytes(ctypes.byref(d)))
            w = st.setdefault("w", keep(nb))
            ok(L.pea_cc_label(ctypes.byref(d), P(x), P(st["labels"]), P(st["mask"]), P(st["counts"]), P(w), nb, None), "cc")
        out["cc_" + name] = (cc, 50)
    for name in ws_ab.LEGS:
        if name == "ac3_100x1024x1024" and not large:
            continue
        b = torch.from_numpy(ws_ab.make_boundary(synth, name)).to(dev)
        d = ws_desc(lib, b.shape, ws_ab.THRESHOLD, ws_ab.SIGMA_SEEDS, ws_ab.SIGMA_WEIGHTS, ws_ab.ALPHA, min_size=ws_ab.MIN_SIZE, flags=STACK_IDS)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        st = dict(dt2=i32(*b.shape), dts=torch.zeros_like(b), hmap=torch.zeros_like(b), seeds=i32(*b.shape), labels=i32(*b.shape), n=i32(d.N),
                  counts=i32(d.N, 2), stats=i32(d.N, 2))

        def ws(L, b=b, d=d, st=st):
            ns, nf = int(L.pea_ws_seeds_workspace_bytes(ctypes.byref(d))), int(L.pea_ws_flood_workspace_bytes(ctypes.byref(d)))
            w = st.setdefault("w", keep(max(ns, nf)))
            ok(L.pea_ws_seeds(ctypes.byref(d), P(b), P(st["dt2"]), P(st["dts"]), P(st["hmap"]), P(st["seeds"]), P(st["n"]), P(w), ns, None), "ws seeds")
            ok(L.pea_ws_flood(ctypes.byref(d), P(st["hmap"]), P(st["seeds"]), P(st["labels"]), P(st["counts"]), P(st["stats"]), P(w), nf, None), "ws flood")
        out["ws_" + name] = (ws, 2 if name == "ac3_100x1024x1024" else 10)
    for name, kw in rag_ab.LEGS.items():
        if name == "vol_1x100x1024x1024" and not large:
            continue
        F, A, Bd = rag_ab.make_inputs(synth, name, dev)
        mid, cap = int(F.max()), kw["capacity"]
        d = rag_desc(lib, F, kw["offsets"], mid, cap, cap // 2, 1)
        outs = {n: torch.zeros((d.B, cap // 2, w), dtype=dt, device=dev) for n, dt, w in RAG_OUT}
        outs["node_size"], outs["stats"] = torch.zeros((d.B, mid + 1), dtype=torch.int64, device=dev), torch.zeros((d.B, 8), dtype=torch.int64, device=dev)
        io = lib.PeaRagBuffers()
        io.fragments, io.affs, io.boundary = F.data_ptr(), A.data_ptr(), Bd.data_ptr()
        for n, t in outs.items():
            setattr(io, n, t.data_ptr())
        st = {"keep": (F, A, Bd, outs)}

        def rag(L, d=d, io=io, st=st):
            nb = int(L.pea_rag_workspace_bytes(ctypes.byref(d)))
            if "w" not in st:
                st["w"] = keep(nb)
                ok(L.pea_rag_workspace_init(P(st["w"]), nb, None), "rag init")
            ok(L.pea_rag_build(ctypes.byref(d), ctypes.byref(io), P(st["w"]), nb, None), "rag")
        out["rag_" + name] = (rag, 3 if name == "vol_1x100x1024x1024" else 30)
    for name, kw in instscore_ab.LEGS.items():
        gt = torch.from_numpy(instscore_ab.nuclei(700, kw["B"], kw["Y"], kw["X"], kw["n"], kw["radius"])).reshape(kw["B"], -1).to(torch.int32).to(dev)
        pred = torch.from_numpy(instscore_ab.nuclei(700, kw["B"], kw["Y"], kw["X"], kw["n"], kw["radius"], jitter=3, drop=max(1, kw["n"] // 20)))
        pred = pred.reshape(kw["B"], -1).to(torch.int32).to(dev)
        d = lib.PeaInstDesc()
        d.B, d.S, d.max_id, d.match_iou, d.flags = kw["B"], kw["Y"] * kw["X"], int(max(pred.max(), gt.max())), 0.5, 0
        d.capacity = min(32768, max(256, 1 << ((d.S + 31) // 32 - 1).bit_length()))  # (harness/segscore.py: default_capacity)
        st = dict(out=torch.zeros((d.B, lib.INST_COLS), dtype=torch.float64, device=dev), m=torch.zeros((2, d.B, d.max_id + 1), dtype=torch.int32, device=dev))

        def inst(L, d=d, pred=pred, gt=gt, st=st):
            nb = int(L.pea_inst_workspace_bytes(ctypes.byref(d)))
            if "w" not in st:
                st["w"] = keep(nb)
                ok(L.pea_inst_workspace_init(P(st["w"]), nb, None), "inst init")
            ok(L.pea_inst_scores(ctypes.byref(d), P(pred), P(gt), P(st["out"]), P(st["m"][0]), P(st["m"][1]), P(st["w"]), nb, None), "inst")
        out["inst_" + name] = (inst, 50)
    seg_legs = {"cvppp_1x544x544": (1, 544, 544, (96, 80), (20, 18)), "bbbc_8x256x256": (8, 256, 256, (24, 20), (60, 50))}
    if large:
        seg_legs["large_24x1024x1024"] = (24, 1024, 1024, (16, 12), (4000, 3000))
    for name, (B, Y, X, cells, n_ids) in seg_legs.items():
        pred = torch.from_numpy(synth.synth_labels(B, (1, Y, X), 901, cell=cells[0], n=n_ids[0])[:, 0].astype(np.int32)).reshape(B, -1).to(dev)
        gt = torch.from_numpy(synth.synth_labels(B, (1, Y, X), 902, cell=cells[1], n=n_ids[1])[:, 0].astype(np.int32)).reshape(B, -1).to(dev)
        d = lib.PeaSegDesc()
        d.B, d.S, d.flags = B, Y * X, 0
        d.capacity = min(32768, max(256, 1 << ((d.S + 31) // 32 - 1).bit_length()))
        st = dict(out=torch.zeros((B, lib.SEG_COLS), dtype=torch.float64, device=dev))

        def seg(L, d=d, pred=pred, gt=gt, st=st):
            nb = int(L.pea_seg_workspace_bytes(ctypes.byref(d)))
            if "w" not in st:
                st["w"] = keep(nb)
                ok(L.pea_seg_workspace_init(P(st["w"]), nb, None), "seg init")
            ok(L.pea_seg_scores(ctypes.byref(d), P(pred), P(gt), P(st["out"]), P(st["w"]), nb, None), "seg")
        out["seg_" + name] = (seg, 10 if name.startswith("large") else 50)
    # disc forward + backward: blocks of about 40 ids per image (profiles/disc_ab.json's shapes)
    for name, (B, S, side) in {"bbbc_8x16x256x256": (8, 256 * 256, 256), "cvppp_1x16x544x544": (1, 544 * 544, 544),
                               "ac3ac4_2x16x18x160x160": (2, 18 * 160 * 160, 160)}.items():
        i = torch.arange(S)
        lab = ((((i // side) % side) // (side // 6 + 1)) * 7 + (i % side) // (side // 6 + 1) + 1).to(torch.int32).reshape(1, S).repeat(B, 1).contiguous().to(dev)
        e = torch.randn((B, 16, S), generator=g).to(dev)
        d = lib.PeaDiscDesc()
        d.B, d.D, d.S, d.num_ids, d.dtype, d.flags = B, 16, S, 64, 0, NEED_GRAD
        d.delta_v, d.delta_d, d.alpha, d.beta, d.gamma = 0.5, 1.5, 1.0, 1.0, 0.001
        st = dict(loss=torch.zeros(1, device=dev), stats=torch.zeros(5 + 4 * B, dtype=torch.float64, device=dev), de=torch.zeros_like(e))

        def disc(L, d=d, e=e, lab=lab, st=st):
            nb = int(L.pea_disc_workspace_bytes(ctypes.byref(d)))
            if "w" not in st:
                st["w"], st["ctx"] = keep(nb), keep(int(L.pea_disc_context_bytes(ctypes.byref(d))))
                ok(L.pea_disc_workspace_init(P(st["w"]), nb, None), "disc init")
            ok(L.pea_disc_loss_fwd(ctypes.byref(d), P(e), P(lab), P(st["loss"]), P(st["stats"]), P(st["ctx"]), P(st["w"]), nb, None), "disc fwd")
            ok(L.pea_disc_loss_bwd(ctypes.byref(d), P(e), P(lab), P(st["ctx"]), None, P(st["de"]), None), "disc bwd")
        out["disc_fwd_bwd_" + name] = (disc, 50)
    return out


def timing(libs, all_legs, batches=7):
    rec = {}
    for name, (f, reps) in all_legs.items():
        per = {k: [] for k in libs}
        for L in libs.values():  # warm-up: the workspaces, the code objects
            for _ in range(3):
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
        rec[name] = {"calls_per_batch": reps, "us_per_call_batches": {k: [round(x, 3) for x in v] for k, v in per.items()},
                     "median_us": {k: round(v, 3) for k, v in med.items()}, "parent_min_max_us": [round(lo, 3), round(hi, 3)],
                     "change_median_inside_or_below": bool(med["change"] <= hi)}
        print("%-40s parent %.2f [%.2f, %.2f]  change %.2f  %s" % (name, med["parent"], lo, hi, med["change"], "ok" if med["change"] <= hi else "ABOVE"),
              flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libpea_hip.so built from the parent commit")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-bits", action="store_true")
    ap.add_argument("--large", action="store_true", help="also the largest legs of ws_ab.py, rag_ab.py and segscore_ab.py")
    a = ap.parse_args()
    t0 = time.time()
    pkg = ge.load_package()
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    lib = pkg._lib
    change = lib.lib()
    parent = ctypes.CDLL(os.path.abspath(a.parent))
    assert os.path.realpath(a.parent) != os.path.realpath(lib.SO_PATH)
    for f in dir(change):  # the same prototypes on both handles
        if f.startswith("pea_"):
            getattr(parent, f).restype, getattr(parent, f).argtypes = getattr(change, f).restype, getattr(change, f).argtypes
    os.makedirs(a.out_dir, exist_ok=True)
    differ = []
    if not a.skip_bits:
        book = Book({"parent": parent, "change": change, "change_again": change})
        bits_cases(book, lib, synth)
        par = book.rows["parent"]
        assert book.rows["change"].keys() == book.rows["change_again"].keys() == par.keys()
        differ = sorted("%s:%s:%s" % (k, c, o) for k in ("change", "change_again") for c in par for o in set(par[c]) | set(book.rows[k][c])
                        if par[c].get(o) != book.rows[k][c].get(o))
        n = sum(len(v) for v in par.values())
        rec = {"what": "SHA-256 of every output tensor, case by case: the parent library's digest; `differ` names every tensor of which this "
                       "tree's first or second launch gave another one (one process, three runs of every case)",
               "device": torch.cuda.get_device_name(0), "cases": len(par), "digests": n, "differ": differ, "seconds": round(time.time() - t0, 1),
               "sha256": {c: {o: par[c][o] for o in sorted(par[c])} for c in sorted(par)}}
        json.dump(rec, open(os.path.join(a.out_dir, "label_refactor_bits.json"), "w"), indent=1)
        print("bits: %d cases, %d digests, %d differ, %.1f s" % (len(par), n, len(differ), time.time() - t0), flush=True)
        for c in differ[:40]:
            print("  differs:", c)
    if not a.skip_timing:
        trec = {"what": "HIP events around batches of calls (calls_per_batch); parent library and this tree alternate batch by batch in one process; 7 "
                        "batches each", "device": torch.cuda.get_device_name(0),
                "legs": timing({"parent": parent, "change": change}, legs(lib, synth, a.large))}
        json.dump(trec, open(os.path.join(a.out_dir, "label_refactor_ab.json"), "w"), indent=1)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
