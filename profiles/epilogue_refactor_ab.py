#!/usr/bin/env python3
"""The epilogue refactor (csrc/pea_epilogue.h: the loss term, its quad form and the partial tail stated once; loss_row_collect in
csrc/pea_loss.h; block_sums in csrc/pea_quad.h): the parent's library against this tree's, loaded as two ctypes.CDLLs in ONE process.

One SHA-256 per output tensor (bytes, so NaN payloads count) of
  * every subject of tests/test_gpu_loss_reduction.py::SUBJECTS -- the alignment suite's CASES with their switches, the direct kernel,
    the pair, both labels-in steps, the batched tables -- through the rigs of tests/test_gpu_nonfinite.py (forward AND backward: affs,
    g, the 1 / norm planes, the loss row, de),
  * the activated-map families of tests/test_gpu_nonfinite.py::LACT_CASES, self and ema, under each activation of LACTS, with and
    without PEA_FLAG_LOSS_BCE (a family that declines a form declines it in both libraries: recorded as the return code),
each with a u8 mask, an f32 mask and no mask, and with NaN (interior) / +inf (corner) in the embedding as that suite poisons it;
  * pea_affs_metrics and pea_fgmask_loss_fwd at 67 x 71 (4757 elements: two workgroups per plane, a last quad of one element).
The contract is 0 digests differ.  -> profiles/epilogue_refactor_bits.json

  python profiles/epilogue_refactor_ab.py --parent PATH/libpea_hip.so"""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

MASK_F32, LOSS_ACT, LOSS_BCE = 32, 64, 128


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Book(object):
    """digests of both libraries, case by case"""

    def __init__(self, libs):
        self.libs, self.rows = libs, {k: {} for k in libs}

    def run(self, case, fn):
        """fn(L) -> {output: tensor}; an AssertionError (a declined form: `rc -3`) is recorded as its text"""
        for k, L in self.libs.items():
            try:
                out = {o: sha(t) for o, t in fn(L).items()}
            except AssertionError as ex:
                out = {"declined": str(ex).split(": ")[-1][:60]}
            torch.cuda.synchronize()
            self.rows[k][case] = out


def reload_both(libs, env):
    for name in ("PEA_FORCE_DIRECT", "PEA_ZMARCH"):
        os.environ.pop(name, None)
    if env:
        os.environ[env[0]] = env[1]
    for L in libs.values():
        L.pea_reload_env()


def mask_variants(N, I, dev):
    """(name, mask tensor, extra descriptor flags): u8, f32, none"""
    shape = tuple(I["T"].shape)
    g = torch.Generator().manual_seed(77)
    if I["M"] is not None and I["M"].dtype == torch.uint8:
        u8 = I["M"]
    else:
        u8 = (torch.rand(shape, generator=g) < 0.8).to(torch.uint8).to(dev)
    f32 = I["M"] if (I["M"] is not None and I["M"].dtype == torch.float32) else N.A.frac_mask(shape, 78).to(dev)
    return (("u8", u8, 0), ("f32", f32, MASK_F32), ("none", None, 0))


def loss_cases(book, N, name, rig, dev):
    """the rig's run() under the three masks and with a poisoned embedding; rig.L is swapped per library"""
    j = getattr(rig, "j", None)
    descs = [rig.descs[j]] if j is not None else [rig.d] + ([rig.dc] if hasattr(rig, "dc") else [])
    I0 = rig.I
    flags0 = [d.flags for d in descs]
    has_mask = rig.tensors()["W"] is not None  # (the labels-in steps take no weight / mask tensors)

    def with_mask(M, extra):
        I = dict(I0, M=M)
        rig.I = I
        if j is not None:
            rig.ents = list(rig.ents)
            rig.ents[j] = I
        for d, f in zip(descs, flags0):
            d.flags = (f & ~MASK_F32) | extra

    def call(L, **kw):
        rig.L = L
        return rig.run(**kw)

    variants = mask_variants(N, I0, dev) if has_mask else (("own", I0.get("M"), 0),)
    for mname, M, extra in variants:
        with_mask(M, extra)
        book.run("%s/mask_%s" % (name, mname), call)
    with_mask(I0.get("M"), flags0[0] & MASK_F32)
    dims = rig.c["dims"]
    for vname, value, q in (("nan", float("nan"), N.interior(dims)), ("inf", float("inf"), (0, 0, 0))):
        for operand in rig.operands:
            key = "E" if operand == "e" else "O"
            bad = N.poisoned(rig.tensors()[key], q, value)
            book.run("%s/%s_in_%s" % (name, vname, operand), lambda L: call(L, **{key: bad}))
    rig.I = I0


def subjects(book, pkg, op, synth, dev):
    import test_gpu_nonfinite as N  # (N.A: tests/test_gpu_alignment.py, N.R: tests/test_gpu_loss_reduction.py)
    for name in N.R.SUBJECTS:
        reload_both(book.libs, N.ENV.get(name))
        rig = N.make_rig(pkg, op, dev, synth, name)
        loss_cases(book, N, name, rig, dev)
    for case in sorted(N.LACT_CASES):
        D, dtype, offs, env = N.LACT_CASES[case]
        reload_both(book.libs, env)
        for other in (None, "detached"):
            c = N.A.case(D=D, dtype=dtype, offs=offs, other=other, seed=60 + sorted(N.LACT_CASES).index(case))
            I = N.A.make_inputs(synth, dev, c)
            for aname, act in N.LACTS.items():
                for bname, bce in (("mse", 0), ("bce", LOSS_BCE)):
                    if bce and not act & N.CLAMP:
                        continue  # (pea_desc_validate: the cross-entropy's argument must lie in [0, 1])
                    name = "lact/%s_%s_%s_%s" % (case, "ema" if other else "self", aname, bname)
                    rig = N.LossRig(pkg, op, dev, c, I, name, flags=act | LOSS_ACT | bce)
                    loss_cases(book, N, name, rig, dev)
    reload_both(book.libs, None)


def streaming(book, pkg, dev):
    lib = pkg._lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(91)
    Y, X = 67, 71  # 4757 elements: two workgroups per plane, the last quad holds one element
    # pea_affs_metrics: dense 2D (relu), and a cropped 3D divide-and-store walk
    B, C = 2, 3
    pred = (torch.rand((B, C, 1, Y, X), generator=g) * 1.4 - 0.2).to(dev)
    tgt = (torch.rand((B, C, 1, Y, X), generator=g) < 0.5).float().to(dev)
    pred[0, 1, 0, 5, 7] = float("nan")
    masks = {"u8": ((torch.rand(pred.shape, generator=g) < 0.8).to(torch.uint8).to(dev), 0),
             "f32": (torch.rand(pred.shape, generator=g).to(dev), 8), "none": (None, 0)}
    for mname, (M, mflag) in masks.items():
        def fn(L, M=M, mflag=mflag):
            d = lib.PeaMetricsDesc()
            d.B, d.C, d.CP, d.flags, d.clip_lo, d.clip_hi = B, C, C, 1 | mflag, 0.0, 1.0
            d.dims[:], d.pred_dims[:], d.origin[:] = [1, Y, X], [1, Y, X], [0, 0, 0]
            nb = int(L.pea_metrics_workspace_bytes())
            work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
            assert L.pea_workspace_init(P(work), nb, st) == 0
            out = torch.zeros((1 + C, 5), dtype=torch.float64, device=dev)
            rc = L.pea_affs_metrics(ctypes.byref(d), P(pred), None, P(tgt), P(M), P(out), P(work), nb, st)
            assert rc == 0, "rc %d" % rc
            torch.cuda.synchronize()
            return {"out": out, "state": work}
        book.run("metrics/dense_relu_mask_%s" % mname, fn)
    PZ, PY, PX, CP = 3, Y + 2, X + 3, 4
    vol = (torch.rand((1, CP, PZ, PY, PX), generator=g) + 0.1).to(dev)
    wmap = (torch.rand((PZ, PY, PX), generator=g) + 0.5).to(dev)
    tg3 = (torch.rand((1, C, 2, Y, X), generator=g) < 0.5).float().to(dev)

    def fn3(L):
        d = lib.PeaMetricsDesc()
        d.B, d.C, d.CP, d.flags, d.clip_lo, d.clip_hi = 1, C, CP, 2 | 4, 0.0, 1.0
        d.dims[:], d.pred_dims[:], d.origin[:] = [2, Y, X], [PZ, PY, PX], [1, 1, 2]
        nb = int(L.pea_metrics_workspace_bytes())
        work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        assert L.pea_workspace_init(P(work), nb, st) == 0
        out = torch.zeros((1 + C, 5), dtype=torch.float64, device=dev)
        pv = vol.clone()
        rc = L.pea_affs_metrics(ctypes.byref(d), P(pv), P(wmap), P(tg3), None, P(out), P(work), nb, st)
        assert rc == 0, "rc %d" % rc
        torch.cuda.synchronize()
        return {"out": out, "pred": pv, "state": work}
    book.run("metrics/crop_divide_store", fn3)
    # pea_fgmask_loss_fwd
    logits = torch.randn((2, 2, Y, X), generator=g) * 3
    labels = (torch.rand((2, Y, X), generator=g) < 0.3).int() * 5 - (torch.rand((2, Y, X), generator=g) < 0.1).int()
    for dname, dt, code in (("f32", torch.float32, 0), ("f16", torch.float16, 1), ("bf16", torch.bfloat16, 2)):
        for lname, lt, lcode in (("i32", torch.int32, 0), ("u8", torch.uint8, 1)):
            lg, lab = logits.to(dt).to(dev), (labels if lcode == 0 else (labels > 0)).to(lt).to(dev)

            def fn(L, lg=lg, lab=lab, code=code, lcode=lcode):
                d = lib.PeaFgDesc()
                d.B, d.Y, d.X, d.logits_dtype, d.labels_type, d.flags = 2, Y, X, code, lcode, 0
                d.origin[:], d.out_dims[:] = [0, 0], [Y, X]
                nb = int(L.pea_fgmask_workspace_bytes())
                work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
                assert L.pea_workspace_init(P(work), nb, st) == 0
                loss = torch.zeros(1, dtype=torch.float32, device=dev)
                stats = torch.zeros(5, dtype=torch.float64, device=dev)
                rc = L.pea_fgmask_loss_fwd(ctypes.byref(d), P(lg), P(lab), P(loss), P(stats), P(work), nb, st)
                assert rc == 0, "rc %d" % rc
                torch.cuda.synchronize()
                return {"loss": loss, "stats": stats, "state": work}
            book.run("fgmask/%s_%s" % (dname, lname), fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libpea_hip.so built from the parent commit")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    t0 = time.time()
    pkg = ge.load_package()
    change = pkg._lib.lib()
    parent = ctypes.CDLL(os.path.abspath(a.parent))
    assert os.path.realpath(a.parent) != os.path.realpath(pkg._lib.SO_PATH)
    for f in dir(change):  # the same prototypes on both handles
        if f.startswith("pea_"):
            getattr(parent, f).restype, getattr(parent, f).argtypes = getattr(change, f).restype, getattr(change, f).argtypes
    book = Book({"parent": parent, "change": change})
    dev = torch.device("cuda:0")
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    op = importlib.import_module(ge.PKG_NAME + ".affinity_op")
    subjects(book, pkg, op, synth, dev)
    streaming(book, pkg, dev)
    par, chg = book.rows["parent"], book.rows["change"]
    assert par.keys() == chg.keys()
    differ = sorted("%s:%s" % (c, o) for c in par for o in set(par[c]) | set(chg[c]) if par[c].get(o) != chg[c].get(o))
    n = sum(len(v) for v in par.values())
    declined = sorted(c for c in chg if "declined" in chg[c])
    groups = {}  # the record keeps one digest per subject: SHA-256 over its cases' output digests in sorted order, and their number
    for c in sorted(chg):
        key = c.split("/")[0] if not c.startswith("lact/") else "lact/" + c.split("/")[1].split("_self_")[0].split("_ema_")[0]
        g = groups.setdefault(key, [hashlib.sha256(), 0])
        for o in sorted(chg[c]):
            g[0].update(("%s:%s=%s\n" % (c, o, chg[c][o])).encode())
            g[1] += 1
    rec = {"what": "SHA-256 of every output tensor, parent library against this tree, one process; every digest is compared, kept is one per subject",
           "device": torch.cuda.get_device_name(0), "cases": len(par), "digests": n, "declined_in_both": len(declined), "differ": differ,
           "seconds": round(time.time() - t0, 1), "subjects": {k: "%d %s" % (v[1], v[0].hexdigest()) for k, v in groups.items()}}
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(rec, open(os.path.join(a.out_dir, "epilogue_refactor_bits.json"), "w"), indent=1)
    print("bits: %d cases (%d declined by both), %d digests, %d differ, %.1f s" % (len(par), len(declined), n, len(differ), time.time() - t0))
    for c in differ:
        print("  differs:", c)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
