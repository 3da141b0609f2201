#!/usr/bin/env python3
"""The stage refactor (csrc/pea_stage.h: the staging geometry, the neighbour slots, the LDS-DMA issue and the load-counted hand-off of
the cross / march / box kernels stated once): the parent's library against this tree's, loaded as two ctypes.CDLLs in ONE process.

One SHA-256 per output tensor (bytes, so NaN payloads count) of
  * forward (and the backward behind it), through the rigs of tests/test_gpu_nonfinite.py: every subject of
    tests/test_gpu_loss_reduction.py::SUBJECTS, and every (family, stencil) of tests/cross_stencils.py whose forward the cross kernels
    accept, under both borders (3D: CROP_ZERO), plus a stencil of reach 1 (most waves issue no DMA at all);
  * backward, through family_inputs / shape_inputs / protocol / launch of tests/test_gpu_vjp.py with its arbitrary upstream g:
    k_bwd_xdma at D = 16, _pf (with the map and with affs = NULL) and _pfo, role A with and without PEA_FLAG_ACCUMULATE_DE, the 16-bit
    kernels (_h, _hqs; f16 and bf16; self and detached), the pair, ZP, the march in one, two and three segments, k_bwd_box / k_bwd_boxm
    (and the box forward as pea_affinity_infer).
Every case runs on the parent's library once and on this tree's TWICE: a hand-off that lets a load slip shows as identical launches
disagreeing.  The contract is 0 digests differ, both ways.  -> profiles/stage_refactor_bits.json

  python profiles/stage_refactor_ab.py --parent PATH/libpea_hip.so"""
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

FLAG_ACCUMULATE = 16


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


class Book(object):
    """digests case by case: the parent's library, this tree's, and this tree's again"""

    def __init__(self, pkg, parent, change):
        self.pkg, self.libs = pkg, (("parent", parent), ("change", change), ("again", change))
        self.rows = {k: {} for k, _ in self.libs}
        self.tags = {}

    def run(self, case, fn, **tags):
        """fn(L) -> {output: tensor or None}; a declined form (AssertionError) is recorded as its text"""
        self.tags[case] = tags
        for k, L in self.libs:
            self.pkg._lib._lib = L  # what pkg._lib.lib() hands to the tests' helpers
            L.pea_reload_env()
            try:
                out = {o: sha(t) for o, t in fn(L).items() if t is not None}
            except AssertionError as ex:
                out = {"declined": str(ex).split(": ")[-1][:60]}
            torch.cuda.synchronize()
            self.rows[k][case] = out


def set_env(env):
    for name in ("PEA_FORCE_DIRECT", "PEA_ZMARCH", "PEA_ZSEG", "PEA_BOXM", "PEA_H16_HW"):
        os.environ.pop(name, None)
    for k, v in env:
        os.environ[k] = v


def reach(o3):
    return max(abs(v) for o in o3 for v in o[1:])


def forwards(book, pkg, op, synth, dev):
    import cross_stencils as X
    import test_gpu_nonfinite as N
    for name in N.R.SUBJECTS:
        set_env([N.ENV[name]] if name in N.ENV else [])
        holder = {}

        def fn(L, name=name, holder=holder):
            if "rig" not in holder:
                holder["rig"] = N.make_rig(pkg, op, dev, synth, name)
            holder["rig"].L = L
            return holder["rig"].run()
        book.run("subject/" + name, fn)
    X.STENCILS["reach1"] = [[0, -1], [-1, 0]]
    todo = [(f, s) for f in sorted(X.EXPECT) for s in sorted(X.EXPECT[f]) if X.EXPECT[f][s][0] == "1"] + [("f32_16", "reach1"), ("f32_32", "reach1"),
                                                                                                         ("f16_32", "reach1")]
    for family, stencil in todo:
        D, dt, dims, B = X.FAMILIES[family]
        set_env([X.ENV[family]] if family in X.ENV else [])
        for border in ((1,) if dims[0] > 1 else (0, 1)):
            c = N.A.case(D=D, B=B, dims=dims, border=border, norm=1 if border else 0, dtype=dt, mask="u8", seed=0)
            I = X.make_inputs(synth, dev, family, stencil, 11 + border)
            holder = {}

            def fn(L, c=c, I=I, holder=holder, what="%s %s %d" % (family, stencil, border)):
                if "rig" not in holder:
                    holder["rig"] = N.LossRig(pkg, op, dev, c, I, what)
                holder["rig"].L = L
                return holder["rig"].run()
            book.run("stencil/%s/%s/%s" % (family, stencil, "crop" if border else "circ"), fn, fwd=True, reach=reach(I["o3"]), dims=dims,
                     border=border, kind="march" if family == "v3_march" else ("ZF" if dims[0] > 1 else "2d"))
    set_env([])


def backwards(book, pkg, op, synth, dev):
    import cross_stencils as X
    import test_gpu_vjp as V
    X.STENCILS.setdefault("reach1", [[0, -1], [-1, 0]])
    dl = torch.full((1,), X.DLOSS, device=dev)

    def case(name, I, d, border, env=(), want_other=False, accumulate=False, raw_map=True, **tags):
        set_env(list(env))
        G, G_alt, _ = V.upstream(I, border)

        def fn(L):
            exp = X.supported(pkg, d)
            inv, raw = V.protocol(pkg, op, dev, I, d, exp, name, raw_map=raw_map)
            base = None
            if accumulate:
                base = torch.linspace(-1, 1, I["E"].numel(), device=dev).view(I["E"].shape).to(I["tdt"])
            rc, de, deo = V.launch(pkg, op, dev, I, d, G, inv, raw, dl, want_other=want_other, base=base)
            assert rc == 0, "rc %d" % rc
            return dict(inv=inv, raw=raw, de=de, de_other=deo)
        book.run("bwd/" + name, fn, reach=reach(I["o3"]), dims=I["dims"], border=border, **tags)

    def fam(family, stencil, border, other=False, **kw):
        I = V.family_inputs(synth, dev, family, stencil, border, other=other)
        flags = FLAG_ACCUMULATE if kw.get("accumulate") else 0
        d = X.fill_desc(pkg, family, stencil, border, flags=flags)
        name = "%s/%s/%s%s%s%s" % (family, stencil, "crop" if border else "circ", "/detached" if other else "",
                                    "/acc" if flags else "", "".join("/%s=%s" % e for e in kw.get("env", ())) + ("" if kw.get("raw_map", True) else "/nomap"))
        case(name, I, d, border, **kw)

    for b in (0, 1):
        for f, s in V.D16 + [("f32_16", "reach1")]:
            fam(f, s, b)
        for f, s in V.PF:
            fam(f, s, b)
            fam(f, s, b, raw_map=False)
        for s in ("pos", "two_sw32"):
            fam("f32_16", s, b, other=True)
            fam("f32_16", s, b, other=True, accumulate=True)
        for f, s in (("f32_32", "pos"), ("f32_64", "pos4")):
            fam(f, s, b, other=True)
        for f, s in V.H16 + [("f16_32", "reach1")]:
            fam(f, s, b)
            fam(f, s, b, other=True)
        fam("f16_32", "small", b, env=(("PEA_H16_HW", "1"),))
    fam("v3", "z_mixed", 1, kind="ZP")
    fam("v3", "z_neg_inplane_pos", 1, kind="ZP")
    for zseg in ("-", "2", "3"):
        fam("v3_march", "z_neg_inplane_pos", 1, env=(X.ENV["v3_march"],) + ((("PEA_ZSEG", zseg),) if zseg != "-" else ()), kind="march")
    # the pair backward
    set_env([])
    I = V.family_inputs(synth, dev, "f32_16", "pos", 0, other=True)
    d = X.fill_desc(pkg, "f32_16", "pos", 0)
    Gx = V.upstream(I, 0)[0]
    G0 = V.make_g(I, 0, I["seed"] + 1000)[0]
    dlx = torch.full((1,), 1.5, device=dev)

    def pair(L):
        inv, _ = V.protocol(pkg, op, dev, I, d, X.supported(pkg, d), "pair")
        de = V.nan(I["E"].shape, dev)
        rc = L.pea_affinity_bwd_dual_ex(ctypes.byref(d), X.P(I["E"]), X.P(I["O"]), X.P(G0), X.P(Gx), X.P(inv[0]), X.P(inv[1]), X.P(dl), X.P(dlx),
                                        X.P(de), op._stream())
        assert rc == 0, "rc %d" % rc
        torch.cuda.synchronize()
        return dict(inv=inv, de=de)
    book.run("bwd/pair/f32_16/pos/circ", pair, reach=27, dims=I["dims"], border=0)
    # the unit-box kernels: backward both ways, the forward as inference
    for cname, kernel in (("n26_crop", "box"), ("n26_crop", "boxm"), ("subset_3d", "box"), ("subset_3d", "boxm"), ("n26_circular", "box"),
                          ("diag_2d_mask", "box")):
        B, dims, o3, border, norm = V.BOX[cname]
        env = ((("PEA_BOXM", "0"),) if kernel == "box" else (("PEA_ZMARCH", "2"),)) if border else ()
        I = V.shape_inputs(synth, dev, cname, B, 16, dims, o3, 60 + len(o3))
        d = V.desc_for(pkg, I, border, norm=norm)
        case("box/%s/%s" % (cname, kernel), I, d, border, env=env, kind=kernel)

        def infer(L, I=I, d=d):
            out = V.nan((I["B"], I["K"]) + I["dims"], dev)
            rc = L.pea_affinity_infer(ctypes.byref(d), X.P(I["E"]), None, X.P(out), op._stream())
            assert rc == 0, "rc %d" % rc
            torch.cuda.synchronize()
            return dict(affs=out)
        if kernel == "box":
            book.run("fwd/box/%s" % cname, infer, kind="box")
    set_env([])


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
    book = Book(pkg, parent, change)
    dev = torch.device("cuda:0")
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    op = importlib.import_module(ge.PKG_NAME + ".affinity_op")
    try:
        forwards(book, pkg, op, synth, dev)
        backwards(book, pkg, op, synth, dev)
    finally:
        pkg._lib._lib = change
        set_env([])
        change.pea_reload_env()
    par, chg, again = book.rows["parent"], book.rows["change"], book.rows["again"]
    tags = [t for c, t in book.tags.items() if "declined" not in chg[c]]
    # what the set has to contain
    assert any(t.get("reach") == 1 for t in tags), "no stencil of reach 1"
    assert any(t.get("reach") == 27 for t in tags), "no stencil of reach 27"
    assert any(t.get("dims") and t["dims"][2] % 32 and t["dims"][1] % 16 for t in tags), "no image with X % 32 != 0 and Y % 16 != 0"
    assert {t.get("border") for t in tags} >= {0, 1}, "not both borders"
    assert {t.get("kind") for t in tags} >= {"ZF", "ZP", "march"}, "no 3D case for each of ZF, ZP and the march"
    differ = sorted("%s:%s" % (c, o) for c in par for o in set(par[c]) | set(chg[c]) if par[c].get(o) != chg[c].get(o))
    unstable = sorted("%s:%s" % (c, o) for c in chg for o in set(chg[c]) | set(again[c]) if chg[c].get(o) != again[c].get(o))
    n = sum(len(v) for v in par.values())
    declined = sorted(c for c in chg if "declined" in chg[c])
    groups = {}  # the record keeps one digest per subject: SHA-256 over its cases' output digests in sorted order, and their number
    for c in sorted(chg):
        key = "/".join(c.split("/")[:2])
        g = groups.setdefault(key, [hashlib.sha256(), 0])
        for o in sorted(chg[c]):
            g[0].update(("%s:%s=%s\n" % (c, o, chg[c][o])).encode())
            g[1] += 1
    rec = {"what": "SHA-256 of every output tensor: parent library against this tree, and this tree launched twice, one process; every digest is "
                   "compared, kept is one per subject",
           "device": torch.cuda.get_device_name(0), "cases": len(par), "digests": n, "declined_in_both": declined, "differ": differ,
           "differ_between_identical_launches": unstable, "seconds": round(time.time() - t0, 1),
           "subjects": {k: "%d %s" % (v[1], v[0].hexdigest()) for k, v in groups.items()}}
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(rec, open(os.path.join(a.out_dir, "stage_refactor_bits.json"), "w"), indent=1)
    print("bits: %d cases (%d declined by both), %d digests, %d differ from the parent, %d differ between identical launches, %.1f s"
          % (len(par), len(declined), n, len(differ), len(unstable), time.time() - t0))
    for c in differ + unstable:
        print("  differs:", c)
    return 1 if differ or unstable else 0


if __name__ == "__main__":
    sys.exit(main())
