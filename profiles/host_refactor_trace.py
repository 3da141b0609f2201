#!/usr/bin/env python3
"""What the Python layer hands the library, scenario by scenario: a record to compare two versions of the host code on ONE library file.

    python profiles/host_refactor_trace.py --root <checkout> --out trace.json

imports the package of <checkout> (default: this one), runs a fixed list of scenarios through the public entry points -- the 2D and 3D
single losses, their labels-in and *_multi forms (fused and declined), the four loss sections with batched / label_downs both ways,
cvppp_validation_section; float32 and bfloat16 embeddings; the shapes of tests/test_gpu_host_rules.py; a first and a second backward
over a retained graph -- and records per scenario
  * calls:   every library call that can launch, in order: name, then per argument the first 8 hex digits of the SHA-256 of a
             descriptor's bytes, P / 0 for a pointer that is set / NULL, the value of a number; the entries of a table likewise; the
             return code last;
  * queries: the host-only questions (pea_*_supported, pea_*_bytes, pea_desc_validate) as a sorted set: they are memoised, so when
             and how often they are asked is the memo's business, not the library's;
  * digests: SHA-256 (16 hex digits) of every returned tensor and of the gradients of both backwards.
The file holds per scenario one string, "count:SHA-256" of the calls, of the queries and of the tensor digests and whether the
second backward repeated the first one's bits, and at its head how often each function was called; --full writes the records.  Two versions of the host code agree when their files are equal.
Needs an MI355X."""
import argparse
import collections
import collections.abc
import ctypes
import hashlib
import importlib
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", required=True)
ap.add_argument("--full", action="store_true", help="write every record whole instead of its digest (to find where two versions part)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
_lib = pkg._lib
op = importlib.import_module(ge.PKG_NAME + ".affinity_op")
L = _lib.lib()
dev = torch.device("cuda:0")
CALLS, QUERIES = [], set()


def sha(b, n=16):
    return hashlib.sha256(b).hexdigest()[:n]


def show(a):
    if a is None:
        return "0"
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, ctypes.c_void_p):
        return "P" if a.value else "0"
    if isinstance(a, _lib.PeaDesc):
        return sha(bytes(a), 8)
    if hasattr(a, "_obj"):  # ctypes.byref(x)
        return show(a._obj)
    if isinstance(a, ctypes._Pointer):
        return show(a.contents) if a else "0"
    if isinstance(a, ctypes.Array):
        return "".join("P" if x else "0" for x in a) if a._type_ is ctypes.c_void_p else [show(x) for x in a]
    if isinstance(a, ctypes.Structure):  # (a void* field reads back as an int: an address, logged as set / NULL like every pointer)
        return [("P" if getattr(a, f) else "0") if t is ctypes.c_void_p else show(getattr(a, f)) for f, t in a._fields_]
    if isinstance(a, ctypes._SimpleCData):
        return show(a.value)
    return type(a).__name__


def is_query(name):
    return name.endswith(("_supported", "_supported_t", "_bytes", "_validate")) or name in ("pea_version", "pea_strerror")


for name in sorted(n for n in dir(L) if n.startswith("pea_") and callable(getattr(L, n))):
    def wrapped(*a, _real=getattr(L, name), _name=name):
        rec = [_name] + [show(x) for x in a]
        rc = _real(*a)
        rec.append(show(rc))
        if is_query(_name):
            QUERIES.add(json.dumps(rec))
        else:
            CALLS.append(rec)
        return rc
    setattr(L, name, wrapped)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def labels(seed, *shape):
    """blocky instance ids with background"""
    small = torch.randint(0, 5, tuple((s + 3) // 4 if i else s for i, s in enumerate(shape)), generator=torch.Generator().manual_seed(seed))
    for ax in range(1, len(shape)):
        small = small.repeat_interleave(4, dim=ax)
    return small[tuple(slice(0, s) for s in shape)].to(torch.int32).contiguous().to(dev)


def flatten(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, op.LossList):
        out.append(x.tensor)
    elif isinstance(x, collections.abc.Mapping):
        for k in x:
            flatten(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            flatten(v, out)
    elif hasattr(x, "__dict__") and not callable(x):  # (AffinityMetrics and the like)
        for k in sorted(vars(x)):
            flatten(vars(x)[k], out)
    return out


def digest(t):
    if t is None:
        return None
    t = t.detach().contiguous()
    return "%s%s:%s" % (str(t.dtype)[6:], list(t.shape), sha(t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""))


SCENARIOS = {}


def run(name, leaves, fn, train=True):
    """fn(*leaf tensors) -> the entry point's result; its differentiable scalars are the losses, weighted 0.25, 0.5, .. for the backward"""
    CALLS.clear()
    QUERIES.clear()
    rec = {}
    try:
        xs = [x.clone().requires_grad_(train) for x in leaves]
        outs = flatten(fn(*xs), [])
        rec["out"] = [digest(t) for t in outs]
        if train:
            loss = sum(0.25 * (i + 1) * l for i, l in enumerate(t for t in outs if t.dim() == 0 and t.requires_grad))
            for k in ("grad1", "grad2"):  # the second one over the retained graph
                rec[k] = [digest(g) for g in torch.autograd.grad(loss, xs, retain_graph=True, allow_unused=True)]
        torch.cuda.synchronize()
    except Exception as ex:  # noqa: BLE001 -- an entry point that refuses must refuse alike
        rec["error"] = "%s: %s" % (type(ex).__name__, str(ex)[:200])
    rec["calls"], rec["queries"] = [list(c) for c in CALLS], sorted(QUERIES)
    assert name not in SCENARIOS, name
    SCENARIOS[name] = rec


OFF = [[-1, 0], [0, -1], [1, 0], [0, 1]]
crit = pkg.WeightedMSE()
BC, NBX = _lib.BORDER_CIRCULAR, _lib.NORM_BX


def smallest_with_plane_and_raw(D):
    for _, Y, X in sorted((Y * X, Y, X) for Y in range(16, 72, 2) for X in range(32, 132, 4)):
        d = op.make_desc(pkg.AffinitySpec(2, OFF, None, BC, NBX), torch.empty((1, D, Y, X), device="meta"))
        if all(L.pea_cross_supported(ctypes.byref(d), mode) for mode in (1, 3)):
            return Y, X
    raise SystemExit("no image takes modes 1 and 3")


def twm(seed, K, *sp, mask=torch.uint8):
    m = rnd(seed + 2, 1, K, *sp) > -1
    return (rnd(seed, 1, K, *sp) > 0).float(), rnd(seed + 1, 1, K, *sp).abs() + 0.5, m.to(mask)


def scenarios_2d(tag, dt, D, H, W):
    sizes = [(16, 16), (12, 12), (8, 8), (6, 6)]
    e, ema = rnd(1, 1, D, H, W).to(dt), rnd(2, 1, D, H, W).to(dt)
    t, w, m = twm(3, 4, H, W)
    emds = [rnd(10 + j, 1, D, *s).to(dt) for j, s in enumerate(sizes)]
    small = [twm(20 + 3 * j, 4 - j, *s, mask=torch.float32) for j, s in enumerate(sizes)]
    downs = [torch.cat(x, dim=1) for x in small]
    offs = [OFF[:4 - j] for j in range(4)]
    lab = labels(40, 1, H, W)
    run(tag + "embedding_loss", [e], lambda x: pkg.embedding_loss(x, t, w, m, crit, OFF))
    run(tag + "embedding_loss/no_grad", [e], lambda x: pkg.embedding_loss(x, t, w, m, crit, OFF), train=False)
    run(tag + "ema_embedding_loss", [e], lambda x: pkg.ema_embedding_loss(x, ema, t, w, m, crit, OFF, affs0_weight=2))
    run(tag + "ema_embedding_loss/both", [e, ema], lambda x, y: pkg.ema_embedding_loss(x, y, t, w, m, crit, OFF))
    run(tag + "embedding2affs", [e], lambda x: pkg.embedding2affs(x, OFF, activation="relu"), train=False)
    run(tag + "embedding_loss_from_labels", [e], lambda x: pkg.embedding_loss_from_labels(x, lab, crit, OFF))
    run(tag + "ema_embedding_loss_from_labels", [e], lambda x: pkg.ema_embedding_loss_from_labels(x, ema, lab, crit, OFF))
    multi = lambda n, **kw: (lambda *xs: pkg.embedding_loss_multi(list(xs), [a[0] for a in small[:n]] + [t] * (n - 4),  # noqa: E731
                                                                  [a[1] for a in small[:n]] + [w] * (n - 4), [a[2] for a in small[:n]] + [m] * (n - 4),
                                                                  crit, offs[:n] + [OFF] * (n - 4), **kw))
    run(tag + "embedding_loss_multi", emds, multi(4))
    run(tag + "embedding_loss_multi/need_affs", emds, multi(4, need_affs=True))
    run(tag + "embedding_loss_multi/declined", emds + [e], multi(5))  # five losses: outside the fused set
    for batched in (False, True):
        run(tag + "cvppp_loss_section/batched=%d" % batched, [e] + emds,
            lambda x, *xs: pkg.cvppp_loss_section(x, list(xs), ema, t, w, m, downs, crit, OFF, 1, deep_weight=2, batched=batched))  # noqa: B023
        run(tag + "cvppp_validation_section/batched=%d" % batched, [e] + emds,
            lambda x, *xs: pkg.cvppp_validation_section(x, list(xs), t, w, m, downs, crit, OFF, 1, batched=batched), train=False)  # noqa: B023
    run(tag + "cvppp_loss_section/relu_pred", [e] + emds,
        lambda x, *xs: pkg.cvppp_loss_section(x, list(xs), ema, t, w, m, downs, crit, OFF, 1, relu_pred=True))


def scenarios_2d_labels(tag, dt, D):
    """64 x 64 with the scales 32 .. 4: label_downs=None needs sizes that divide"""
    e, ema = rnd(1, 1, D, 64, 64).to(dt), rnd(2, 1, D, 64, 64).to(dt)
    emds = [rnd(10 + j, 1, D, 32 >> j, 32 >> j).to(dt) for j in range(4)]
    offs = [OFF[:4 - j] for j in range(4)]
    lab = labels(41, 1, 64, 64)
    lds = [lab[:, ::2 << j, ::2 << j].contiguous() for j in range(4)]
    run(tag + "embedding_loss_from_labels_multi", emds, lambda *xs: pkg.embedding_loss_from_labels_multi(list(xs), lds, crit, offs))
    run(tag + "embedding_loss_from_labels_multi/steps", emds,
        lambda *xs: pkg.embedding_loss_from_labels_multi(list(xs), lab, crit, offs, need_affs=True))
    run(tag + "embedding_loss_from_labels_multi/declined", emds + [e],
        lambda *xs: pkg.embedding_loss_from_labels_multi(list(xs), lds + [lab], crit, offs + [OFF]))
    for batched in (False, True):
        for downs in (lds, None):
            name = "cvppp_loss_section_from_labels/batched=%d/label_downs=%s" % (batched, "given" if downs else "None")
            run(tag + name, [e] + emds, lambda x, *xs: pkg.cvppp_loss_section_from_labels(x, list(xs), ema, lab, downs, crit, OFF, 1,  # noqa: B023
                                                                                        batched=batched))  # noqa: B023
    tables = pkg.cvppp_label_weight_tables(lab, lds, OFF, 1)
    run(tag + "cvppp_loss_section_from_labels/weight_tables", [e] + emds,
        lambda x, *xs: pkg.cvppp_loss_section_from_labels(x, list(xs), ema, lab, lds, crit, OFF, 1, weight_tables=tables, batched=True))


def scenarios_3d(tag, dt):
    dims, sizes = (4, 32, 32), [(4, 16, 16), (4, 8, 8), (4, 4, 4), (4, 2, 2)]
    e, ema = rnd(1, 1, 16, *dims).to(dt), rnd(2, 1, 16, *dims).to(dt)
    emds = [rnd(10 + j, 1, 16, *s).to(dt) for j, s in enumerate(sizes)]
    t1, w1, _ = twm(3, 3, *dims)
    dims5 = (6, 32, 32)  # (norm5 reaches 4 slices along z)
    e5, ema5 = rnd(7, 1, 16, *dims5).to(dt), rnd(8, 1, 16, *dims5).to(dt)
    t5, w5, _ = twm(6, 12, *dims5)
    lab5 = labels(43, 1, *dims5)
    small = [twm(20 + 3 * j, 3, *s) for j, s in enumerate(sizes)]
    downs = [torch.cat(x[:2], dim=1) for x in small][::-1]  # (emd1 <-> down4 .. emd4 <-> down1)
    lab = labels(42, 1, *dims)
    lds = [lab[:, :, ::2 << j, ::2 << j].contiguous() for j in range(4)]
    run(tag + "embedding_loss_norm1", [e], lambda x: pkg.embedding_loss_norm1(x, t1, w1, crit))
    run(tag + "ema_embedding_loss_norm1", [e], lambda x: pkg.ema_embedding_loss_norm1(x, ema, t1, w1, crit, affs0_weight=2))
    run(tag + "embedding_loss_norm5", [e5], lambda x: pkg.embedding_loss_norm5(x, t5, w5, crit))
    run(tag + "ema_embedding_loss_norm5", [e5], lambda x: pkg.ema_embedding_loss_norm5(x, ema5, t5, w5, crit))
    run(tag + "inf_embedding_loss_norm1", [e], lambda x: pkg.inf_embedding_loss_norm1(x), train=False)
    run(tag + "inf_embedding_loss_norm5", [e5], lambda x: pkg.inf_embedding_loss_norm5(x), train=False)
    run(tag + "embedding_loss_norm1_from_labels", [e], lambda x: pkg.embedding_loss_norm1_from_labels(x, lab, crit))
    run(tag + "embedding_loss_norm5_from_labels", [e5], lambda x: pkg.embedding_loss_norm5_from_labels(x, lab5, crit))
    run(tag + "embedding_loss_norm1_multi", emds,
        lambda *xs: pkg.embedding_loss_norm1_multi(list(xs), [a[0] for a in small], [a[1] for a in small], crit))
    run(tag + "embedding_loss_norm1_multi/declined", emds + [e],
        lambda *xs: pkg.embedding_loss_norm1_multi(list(xs), [a[0] for a in small] + [t1], [a[1] for a in small] + [w1], crit, need_affs=False))
    run(tag + "embedding_loss_norm1_from_labels_multi", emds, lambda *xs: pkg.embedding_loss_norm1_from_labels_multi(list(xs), lds, crit))
    run(tag + "embedding_loss_norm1_from_labels_multi/steps", emds,
        lambda *xs: pkg.embedding_loss_norm1_from_labels_multi(list(xs), lab, crit, need_affs=False))
    run(tag + "embedding_loss_norm1_from_labels_multi/declined", emds + [e],
        lambda *xs: pkg.embedding_loss_norm1_from_labels_multi(list(xs), lds + [lab], crit))
    for batched in (False, True):
        for mode in (1, 5):
            full = (e, ema, t1, w1) if mode == 1 else (e5, ema5, t5, w5)
            run(tag + "ac3ac4_loss_section/mode=%d/batched=%d" % (mode, batched), [full[0]] + emds,
                lambda x, *xs: pkg.ac3ac4_loss_section(x, list(xs), full[1], full[2], full[3], downs, crit,  # noqa: B023
                                                       embedding_mode=mode, batched=batched))  # noqa: B023
        for ld in (lds[::-1], None):
            name = "ac3ac4_loss_section_from_labels/batched=%d/label_downs=%s" % (batched, "given" if ld else "None")
            run(tag + name, [e] + emds,
                lambda x, *xs: pkg.ac3ac4_loss_section_from_labels(x, list(xs), ema, lab, ld, crit, embedding_mode=1, batched=batched))  # noqa: B023
    run(tag + "ac3ac4_loss_section/finish_pred", [e5] + emds,
        lambda x, *xs: pkg.ac3ac4_loss_section(x, list(xs), ema5, t5, w5, downs, crit, embedding_mode=5, finish_pred=True))


Y, X = smallest_with_plane_and_raw(32)
for dname, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
    for D, H, W in ((32, Y, X), (32, 30, 30), (16, Y, X)):
        scenarios_2d("%s/2d/D%d/%dx%d/" % (dname, D, H, W), dt, D, H, W)
    for D in (16, 32):
        scenarios_2d_labels("%s/2d/D%d/64x64/" % (dname, D), dt, D)
    scenarios_3d("%s/3d/D16/" % dname, dt)

def brief(rec):
    """calls, queries, tensors as count:digest; whether the second backward gave the first one's bits; the refusal, if any"""
    count = lambda x: "%d:%s" % (len(x), sha(json.dumps(x).encode(), 12))  # noqa: E731
    out = "%s %s %s" % (count(rec["calls"]), count(rec["queries"]), count([rec.get(k) for k in ("out", "grad1", "grad2")]))
    if "grad1" in rec:
        out += " again=" + ("same" if rec["grad1"] == rec["grad2"] else "OTHER")
    return out + (" " + rec["error"] if "error" in rec else "")


with open(_lib.SO_PATH, "rb") as f:
    so = sha(f.read(), 64)
tally = collections.Counter(c[0] for v in SCENARIOS.values() for c in v["calls"])
out = {"library_sha256": so, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "calls_per_function": dict(sorted(tally.items()))}
ncalls = sum(len(v["calls"]) for v in SCENARIOS.values())
errors = [k for k, v in SCENARIOS.items() if "error" in v]
if not args.full:
    SCENARIOS = {k: brief(v) for k, v in SCENARIOS.items()}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("{\n")
    for k in out:
        f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(out[k])))
    f.write(' "scenarios": {\n')
    f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in SCENARIOS.items()))
    f.write("\n }\n}\n")
print("%d scenarios, %d library calls, %d refused: %s" % (len(SCENARIOS), ncalls, len(errors), errors))
