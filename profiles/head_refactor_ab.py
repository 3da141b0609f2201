#!/usr/bin/env python3
"""The head refactor (one k_head_dx / k_head_dw template for f32, f16 and bf16 features, csrc/pea_head.h): the parent's library against
this tree's, loaded as two ctypes.CDLLs in ONE process.

  bits     SHA-256 of e, dx, dW, db from pea_head_fwd / pea_head_bwd (f32) and pea_head_fwd_t / pea_head_bwd_t (f16 / bf16 features, the
           embedding in the same type and in f32) at the shapes of tests/test_gpu_head16.py::SHAPES and its three sets of pointer
           residues (the f32 calls: the residues rounded down to a multiple of 4 bytes).  Equality is the contract: the sums go through
           the same instruction sequence in both builds.  -> profiles/head_refactor_bits.json
  timing   pea_head_bwd on f32 features, with dx and with dx = NULL -- the one call whose device code changed --, parent and change
           alternating batch by batch after warm-up; a batch times `--reps` calls between two HIP events; min / median / max of the
           batches in microseconds per call.  The bar is the parent's own batch-to-batch interval of the same run: `inside` = the change's
           median lies in the parent's [min, max]; otherwise `excess_us` (median - parent max) against `parent_spread_us` (max - min),
           `regression` = excess beyond the spread.  Shapes: the three LEGS of head16_ab.py, and 8 x 64 -> 16 x 272^2 and
           8 x 64 -> 32 x 352^2 for the two dW instantiations whose registers moved.  -> profiles/head_refactor_ab.json

  python profiles/head_refactor_ab.py --parent PATH/libpea_hip.so [--batches 7] [--reps 20] [--warmup 3] [--skip-timing] [--skip-bits]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

LEGS = {"cvppp_B8": (8, 32, 16, (544, 544)), "bbbc_B8": (8, 32, 32, (704, 704)), "ac3ac4_B2": (2, 28, 16, (18, 160, 160)),
        "dw_64to16_B8": (8, 64, 16, (272, 272)), "dw_64to32_B8": (8, 64, 32, (352, 352))}
HEAD_FNS = ("pea_head_workspace_bytes", "pea_head_fwd", "pea_head_bwd", "pea_head_supported_t", "pea_head_fwd_t", "pea_head_bwd_t")


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def carve(buf, cursor, shape, dtype, residue):
    """a tensor of `shape` inside the byte buffer at the next 256-byte boundary + residue -> (view, new cursor)"""
    n = 1
    for v in shape:
        n *= v
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    start = (cursor + 255) // 256 * 256 + residue
    view = buf[start:start + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % 256 == residue
    return view, start + nbytes


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def bits(libs, h16, dev):
    """{case: {output: digest}} per library; a case = (C, D, shape, types, residue set)"""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    out = {k: {} for k in libs}
    for (C, D), sp in h16.SHAPES:
        for xdt, edt in ((torch.float32, torch.float32), (torch.float16, torch.float16), (torch.float16, torch.float32),
                         (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)):
            x, W, bias, de = h16.make_inputs(C, D, sp, xdt, edt, 3000 * C + D + len(sp))
            B, S = x.shape[0], x[0, 0].numel()
            for rname, res in h16.RESIDUES.items():
                f32 = xdt == torch.float32
                rx, rdx = (res["x"] // 4 * 4, res["dx"] // 4 * 4) if f32 else (res["x"], res["dx"])
                re = res["e32"] if edt == torch.float32 else res["e16"]
                for k, L in libs.items():
                    wsb = L.pea_head_workspace_bytes(C, D)
                    buf = torch.zeros(wsb + 2 * x.numel() * x.element_size() + 2 * de.numel() * de.element_size() + 3 * W.numel() * 4 + 16384,
                                      dtype=torch.uint8, device=dev)
                    cur = 0
                    xv, cur = carve(buf, cur, x.shape, xdt, rx)
                    Wv, cur = carve(buf, cur, W.shape, torch.float32, res["W"])
                    bv, cur = carve(buf, cur, bias.shape, torch.float32, res["bias"])
                    dv, cur = carve(buf, cur, de.shape, edt, re)
                    e, cur = carve(buf, cur, de.shape, edt, re)
                    dx, cur = carve(buf, cur, x.shape, xdt, rdx)
                    dW, cur = carve(buf, cur, W.shape, torch.float32, res["dW"])
                    db, cur = carve(buf, cur, bias.shape, torch.float32, res["db"])
                    ws, cur = carve(buf, cur, (wsb // 4,), torch.float32, res["ws"])
                    assert cur <= buf.numel()
                    for v, src in ((xv, x), (Wv, W), (bv, bias), (dv, de)):
                        v.copy_(src)
                    if f32:
                        rc = (L.pea_head_fwd(B, C, D, S, p(xv), p(Wv), p(bv), p(e), st),
                              L.pea_head_bwd(B, C, D, S, p(xv), p(Wv), p(dv), p(dx), p(dW), p(db), p(ws), wsb, st))
                    else:
                        rc = (L.pea_head_fwd_t(B, C, D, S, p(xv), code[xdt], p(Wv), p(bv), p(e), code[edt], st),
                              L.pea_head_bwd_t(B, C, D, S, p(xv), code[xdt], p(Wv), p(dv), code[edt], p(dx), p(dW), p(db), p(ws), wsb, st))
                    torch.cuda.synchronize()
                    assert rc == (0, 0), (k, C, D, sp, xdt, edt, rname, rc)
                    case = "%dto%d_%s_x%s_e%s_%s" % (C, D, "x".join(map(str, sp)), str(xdt)[6:], str(edt)[6:], rname)
                    out[k][case] = {"e": sha(e), "dx": sha(dx), "dW": sha(dW), "db": sha(db)}
    return out


def timing(libs, dev, a):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(31)
    rows = {}
    for name, (B, C, D, sp) in LEGS.items():
        S = 1
        for v in sp:
            S *= v
        x = torch.randn((B, C) + sp, generator=gen, device=dev)
        de = torch.randn((B, D) + sp, generator=gen, device=dev)
        W = torch.randn((D, C), generator=gen, device=dev) * 0.2
        dx, dW, db = torch.empty_like(x), torch.empty_like(W), torch.empty(D, device=dev)
        wsb = libs["parent"].pea_head_workspace_bytes(C, D)
        work = torch.empty(wsb // 4, device=dev)
        row = {"shape": [B, C, D] + list(sp)}
        for form, dxa in (("with_dx", dx), ("dx_null", None)):
            def call(L):
                rc = L.pea_head_bwd(B, C, D, S, p(x), p(W), p(de), p(dxa), p(dW), p(db), p(work), wsb, st)
                assert rc == 0, rc
            for L in libs.values():
                for _ in range(a.warmup):
                    call(L)
            torch.cuda.synchronize()
            times = {k: [] for k in libs}
            for _ in range(a.batches):
                for k, L in libs.items():
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s0.record()
                    for _ in range(a.reps):
                        call(L)
                    s1.record()
                    torch.cuda.synchronize()
                    times[k].append(s0.elapsed_time(s1) * 1e3 / a.reps)
            res = {k: {"min_us": min(t), "median_us": statistics.median(t), "max_us": max(t), "batches_us": t} for k, t in times.items()}
            par, chg = res["parent"], res["change"]
            spread = par["max_us"] - par["min_us"]
            excess = chg["median_us"] - par["max_us"]
            res["verdict"] = {"inside": bool(par["min_us"] <= chg["median_us"] <= par["max_us"]), "parent_spread_us": spread,
                              "excess_us": max(excess, 0.0), "regression": bool(excess > spread),
                              "change_over_parent_median": chg["median_us"] / par["median_us"]}
            row[form] = res
        rows[name] = row
        print(name, json.dumps(row), flush=True)
        del x, de, dx, work
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libpea_hip.so built from the parent commit")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-bits", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    pkg = ge.load_package()
    change = pkg._lib.lib()
    parent = ctypes.CDLL(os.path.abspath(a.parent))
    assert os.path.realpath(a.parent) != os.path.realpath(pkg._lib.SO_PATH)
    for f in HEAD_FNS:  # the same prototypes on both handles
        getattr(parent, f).restype, getattr(parent, f).argtypes = getattr(change, f).restype, getattr(change, f).argtypes
    libs = {"parent": parent, "change": change}
    dev = torch.device("cuda:0")
    os.makedirs(a.out_dir, exist_ok=True)
    if not a.skip_bits:
        import test_gpu_head16 as h16
        d = bits(libs, h16, dev)
        assert d["parent"].keys() == d["change"].keys()
        differ = sorted("%s/%s" % (c, o) for c in d["parent"] for o in d["parent"][c] if d["parent"][c][o] != d["change"][c][o])
        n = sum(len(v) for v in d["parent"].values())
        rec = {"what": "SHA-256 of e, dx, dW, db: pea_head_fwd / pea_head_bwd and pea_head_fwd_t / pea_head_bwd_t, parent library against this tree",
               "device": torch.cuda.get_device_name(0), "cases": len(d["parent"]), "digests": n, "differ": differ, "sha256": d["change"]}
        json.dump(rec, open(os.path.join(a.out_dir, "head_refactor_bits.json"), "w"), indent=1)
        print("bits: %d cases, %d digests, %d differ" % (len(d["parent"]), n, len(differ)), flush=True)
        for c in differ:
            print("  differs:", c)
    if not a.skip_timing:
        rows = timing(libs, dev, a)
        rec = {"what": "pea_head_bwd on f32 features, parent library against this tree, alternating batches in one process",
               "device": torch.cuda.get_device_name(0), "batches": a.batches, "reps_per_batch": a.reps, "warmup": a.warmup, "us_per_call": rows}
        json.dump(rec, open(os.path.join(a.out_dir, "head_refactor_ab.json"), "w"), indent=1)
        for name, row in rows.items():
            for form in ("with_dx", "dx_null"):
                print("timing %-14s %-8s parent %.1f [%.1f, %.1f]  change %.1f  %s" % (
                    name, form, row[form]["parent"]["median_us"], row[form]["parent"]["min_us"], row[form]["parent"]["max_us"],
                    row[form]["change"]["median_us"], json.dumps(row[form]["verdict"])))


if __name__ == "__main__":
    main()
