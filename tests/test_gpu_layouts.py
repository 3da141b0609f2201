"""GPU: the Python entry points on strided, expanded and permuted tensors.

The C ABI takes raw pointers and assumes dense NCHW / NCDHW blocks; the Python layer is all that stands between that and what torch
callers pass.  The contract held here, for every entry point and every layout of tests/layouts.py that applies to its arguments:

    the call on the VIEW returns the same bits as the call on .contiguous() clones of the same values

-- loss, per-offset parts and stats, the affinity map, every input gradient -- and leaves its inputs bit-unchanged.  Bit equality is
what the code promises: a copied layout is the identical call after the copy; the layouts taken without a copy (L4, L5) have batch
strides that are multiples of 4 elements, so the dispatch picks the same kernel family, and the loss accumulators are integers (order
free: tests/test_gpu_loss_reduction.py).  A gradient for a non-contiguous leaf has the leaf's shape and the dense run's values.
One float64 anchor per entry point (tests/f64_reference.py, vjp_reference.py, disc_reference.py, fgmask_reference.py,
metrics_reference.py) at the f32 bars of tests/test_gpu_parity.py keeps "both wrong alike" from passing.

The one-item sources of the broadcast layouts (L1 / L2 / L8) sit in a guard-banded tests/arena.py Arena with B * K * S pattern
elements behind them: a reader that takes a batch stride of 0 for "dense" (include/pea.h) lands in the arena's NaN pattern -- the test
fails by value and nothing is read outside the allocation.

Shapes: 2D B=3, D=16, 24 x 40 with multi_offset((1, 3), 4) (K = 4); 3D B=2, D=16, 6 x 16 x 24 for norm1.  norm5 reaches 27 voxels in y
and x and pea_desc_validate wants |offset| < dim, so its volume is 6 x 28 x 32, the smallest it accepts with X a multiple of 4.  The
five-scale sections need H / 16 and every scale larger than its reach: the shapes tests/test_gpu_parity.py runs them at, at B = 2.
"""
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import layouts as ly
from arena import Arena
from disc_reference import disc_reference
from f64_reference import BORDER_CIRCULAR, BORDER_CROP_ZERO, NORM_BX, NORM_CROPPED, cosine_loss
from fgmask_reference import fgmask_reference, mask_reference
from metrics_reference import metrics_reference
from vjp_reference import vjp

pytestmark = pytest.mark.gpu

AFFS_ATOL, LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-5, 1e-4  # the f32 bars of tests/test_gpu_parity.py
B2, D, H, W = 3, 16, 24, 40
SHIFTS2 = (1, 3)
B3, VOL1, VOL5 = 2, (6, 16, 24), (6, 28, 32)
NORM5 = (1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27)
E_LAYOUTS = ("L3", "L6", "L7")
TW_LAYOUTS = ("L1a", "L1b", "L2", "L3", "L4", "L5", "L8")
MASK_LAYOUTS = ("L1a", "L1b", "L2", "L3", "L4", "L5")
MASK_KINDS = {"u8": torch.uint8, "bool": torch.bool, "f32": "mask_f32"}
ARENA_LAYOUTS = ("L1a", "L1b", "L2", "L8")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def offs2(pkg):
    return pkg.multi_offset(list(SHIFTS2), 4)


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8) if t.numel() else t


def same(a, b):
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def val(t):
    return float(t.detach())


def relmax(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Inputs(object):
    """views by name; the broadcast layouts come out of one guard-banded arena on the device"""

    def __init__(self, dev, arena_bytes=24 << 20):
        self.dev, self.arena_bytes, self.ar, self.recs, self.views = dev, arena_bytes, None, [], {}

    def add(self, name, layout, shape, dtype, seed):
        if layout in ARENA_LAYOUTS:
            if self.ar is None:
                self.ar = Arena(self.arena_bytes, self.dev)
            v, rec = ly.make(layout, shape, dtype, seed, self.dev, arena=self.ar, name=name)
            self.recs.append(rec)
        else:
            v, _ = ly.make(layout, shape, dtype, seed, self.dev)
        assert tuple(v.shape) == tuple(shape)
        if layout != "dense" and ly.numel(shape[1:]) > 1 and shape[0] > 1:
            assert not v.is_contiguous(), "layout %s of %s is no test: it is dense" % (layout, name)
        self.views[name] = v
        return v

    def labels(self, name, layout, Bn, sp, dtype, seed):
        v = self.views[name] = ly.make_labels(layout, Bn, sp, dtype, seed, self.dev)
        return v

    def check_arena(self):
        if self.ar is not None:
            self.ar.check(untouched=self.recs)


def contract(call, inp, leaves=()):
    """call(args) -> {name: tensor} on the views and on their dense twins (it may run a backward; the .grad of every name in `leaves`
    joins the outputs): the same bits, inputs unchanged, the arena untouched.  -> (outputs of the dense run, its arguments)"""
    views = inp.views
    snaps = {k: v.clone() for k, v in views.items()}
    runs = []
    for form in ("view", "dense"):
        args = {}
        for k, v in views.items():
            t = v if form == "view" else ly.dense(v)
            args[k] = t.detach().requires_grad_(True) if k in leaves else t
        out = dict(call(args))
        for k in leaves:
            g = args[k].grad
            assert g is not None, "no gradient for %s" % k
            assert tuple(g.shape) == tuple(args[k].shape), "the gradient of %s has shape %s" % (k, tuple(g.shape))
            out["grad_" + k] = g
        runs.append((out, args))
    torch.cuda.synchronize()
    (ov, _), (od, ad) = runs
    assert sorted(ov) == sorted(od)
    for k in ov:
        assert same(ov[k], od[k]), "%s of the call on the views differs from the call on their dense twins" % k
        if k.startswith("grad_"):
            assert torch.equal(ov[k], od[k])
    for k, v in views.items():
        assert same(v, snaps[k]), "input %s was changed by the call" % k
    inp.check_arena()
    return od, ad


def off3(offsets):
    return [[0] * (3 - len(o)) + [int(v) for v in o] for o in offsets]


def as5(t):
    return None if t is None else (t.unsqueeze(2) if t.dim() == 4 else t)


def anchor_loss(out, args, offsets3, lam, border, norm, dloss, ema=False, eps=1e-12):
    """the dense run against tests/f64_reference.py::cosine_loss at the f32 bars"""
    other = args["ema"] if ema else None
    other_grad = ema and args["ema"].requires_grad
    m = args.get("m")
    ref = cosine_loss(as5(args["e"]), as5(other), as5(args["t"]), as5(args["w"]), as5(None if m is None else m.float()), offsets3, lam, eps,
                      border, norm, dloss=dloss, other_grad=other_grad)
    assert abs(val(out["loss"]) - float(ref["loss"])) <= LOSS_RTOL * abs(float(ref["loss"]))
    assert float((as5(out["affs"]).double() - ref["affs"]).abs().max()) < AFFS_ATOL
    if "parts" in out:
        assert relmax(out["parts"], ref["parts"]) < LOSS_RTOL
    assert relmax(as5(out["grad_e"]), ref["de"]) < GRAD_RTOL
    if other_grad:
        assert relmax(as5(out["grad_ema"]), ref["de_other"]) < GRAD_RTOL


# ---- embedding_loss / ema_embedding_loss ---------------------------------------------------------------------------------------------
def _cases_2d():
    """(id, layouts of e / ema / target / weightmap / mask, mask kind): the embeddings in L3 / L6 / L7 over dense tensors, then every
    mask kind in every mask layout with target and weightmap walking through theirs (each at least once in every role)"""
    cases = [("e_%s" % l, dict(e=l, ema=E_LAYOUTS[(i + 1) % 3], t="dense", w="dense", m="dense"), "u8") for i, l in enumerate(E_LAYOUTS)]
    i = 0
    for kind in MASK_KINDS:
        for ml in MASK_LAYOUTS:
            lay = dict(e="dense", ema="dense", t=TW_LAYOUTS[i % 7], w=TW_LAYOUTS[(i + 3) % 7], m=ml)
            cases.append(("t_%s-w_%s-m_%s_%s" % (lay["t"], lay["w"], kind, ml), lay, kind))
            i += 1
    cases.append(("t_L8-w_L8-nomask", dict(e="L6", ema="L3", t="L8", w="L8", m=None), "u8"))
    return cases


CASES_2D = _cases_2d()


@pytest.mark.parametrize("ema", [False, True], ids=["self", "ema"])
@pytest.mark.parametrize("name,lay,kind", CASES_2D, ids=[c[0] for c in CASES_2D])
def test_embedding_loss_2d(pkg, dev, offs2, name, lay, kind, ema):
    K = len(offs2)
    inp = Inputs(dev)
    inp.add("e", lay["e"], (B2, D, H, W), torch.float32, 1)
    if ema:
        inp.add("ema", lay["ema"], (B2, D, H, W), torch.float32, 2)
    inp.add("t", lay["t"], (B2, K, H, W), "mask_f32", 3)
    inp.add("w", lay["w"], (B2, K, H, W), "mask_f32", 4)
    if lay["m"] is not None:
        inp.add("m", lay["m"], (B2, K, H, W), MASK_KINDS[kind], 5)
    crit = pkg.WeightedMSE()
    ema_grad = ema and name.startswith("e_")  # a second operand with a gradient of its own where it is the one under test

    def call(a):
        if ema:
            loss, affs = pkg.ema_embedding_loss(a["e"], a["ema"], a["t"], a["w"], a.get("m"), crit, offs2, affs0_weight=2)
            out = dict(loss=loss, affs=affs)
        else:
            loss, affs, parts = pkg.embedding_loss(a["e"], a["t"], a["w"], a.get("m"), crit, offs2)
            out = dict(loss=loss, affs=affs, parts=parts.tensor)
        (loss * 0.75).backward()
        return out

    out, args = contract(call, inp, leaves=("e", "ema") if ema_grad else ("e",))
    assert bool(torch.isfinite(out["loss"])) and float(out["grad_e"].abs().max()) > 0
    if name in ("e_L6", "t_L1a-w_L3-m_u8_L1a"):
        lam = [2.0, 2.0] + [1.0] * (K - 2) if ema else [1.0] * K
        anchor_loss(out, args, off3(offs2), lam, BORDER_CIRCULAR, NORM_BX, 0.75, ema=ema)


def test_the_anchored_2d_cases_exist():
    assert {"e_L6", "t_L1a-w_L3-m_u8_L1a"} <= {c[0] for c in CASES_2D}


# ---- the 3D losses -----------------------------------------------------------------------------------------------------------------------
CASES_3D = [("e_%s" % l, dict(e=l, ema=E_LAYOUTS[(i + 1) % 3], t="dense", w="dense")) for i, l in enumerate(E_LAYOUTS)] + \
           [("t_%s-w_%s" % (TW_LAYOUTS[i], TW_LAYOUTS[(i + 3) % 7]), dict(e="dense", ema="dense", t=TW_LAYOUTS[i], w=TW_LAYOUTS[(i + 3) % 7]))
            for i in range(7)]


@pytest.mark.parametrize("which", ["norm1", "norm5", "ema_norm5"])
@pytest.mark.parametrize("name,lay", CASES_3D, ids=[c[0] for c in CASES_3D])
def test_embedding_loss_3d(pkg, dev, name, lay, which):
    vol, shifts, first = (VOL1, (1, 1, 1), 1) if which == "norm1" else (VOL5, NORM5, 3)
    K, ema = len(shifts), which.startswith("ema")
    inp = Inputs(dev)
    inp.add("e", lay["e"], (B3, D) + vol, torch.float32, 11)
    if ema:
        inp.add("ema", lay["ema"], (B3, D) + vol, torch.float32, 12)
    inp.add("t", lay["t"], (B3, K) + vol, "mask_f32", 13)
    inp.add("w", lay["w"], (B3, K) + vol, "mask_f32", 14)
    crit = pkg.WeightedMSE()
    ema_grad = ema and name.startswith("e_")

    def call(a):
        if which == "norm1":
            loss, affs = pkg.embedding_loss_norm1(a["e"], a["t"], a["w"], crit, affs0_weight=2)
        elif which == "norm5":
            loss, affs = pkg.embedding_loss_norm5(a["e"], a["t"], a["w"], crit, affs0_weight=2)
        else:
            loss, affs = pkg.ema_embedding_loss_norm5(a["e"], a["ema"], a["t"], a["w"], crit, affs0_weight=2)
        (loss * 0.75).backward()
        return dict(loss=loss, affs=affs)

    out, args = contract(call, inp, leaves=("e", "ema") if ema_grad else ("e",))
    assert bool(torch.isfinite(out["loss"])) and float(out["grad_e"].abs().max()) > 0
    if name in ("e_L6", "t_L1a-w_L3"):
        lam = [2.0 if i < first else 1.0 for i in range(K)]
        offsets3 = [[-s if a == i % 3 else 0 for a in range(3)] for i, s in enumerate(shifts)]
        anchor_loss(out, args, offsets3, lam, BORDER_CROP_ZERO, NORM_CROPPED, 0.75, ema=ema)


# ---- the batched tables -------------------------------------------------------------------------------------------------------------------
def test_embedding_loss_multi_mixed_layouts(pkg, dev, offs2):
    """three losses in one table, their targets / weights / masks in different layouts, one entry broadcast over the batch"""
    shapes = [(H, W), (H // 2, W // 2), (16, 24)]
    offsets = [offs2, offs2[:2], offs2]
    table = [dict(e="L6", t="L4", w="L5", m=("L1a", torch.uint8)), dict(e="dense", t="L1b", w="L2", m=("L3", "mask_f32")),
             dict(e="L3", t="dense", w="L8", m=("L4", torch.bool))]
    inp = Inputs(dev)
    for j, (sp, offs, lay) in enumerate(zip(shapes, offsets, table)):
        k = len(offs)
        inp.add("e%d" % j, lay["e"], (B2, D) + sp, torch.float32, 20 + j)
        inp.add("t%d" % j, lay["t"], (B2, k) + sp, "mask_f32", 30 + j)
        inp.add("w%d" % j, lay["w"], (B2, k) + sp, "mask_f32", 40 + j)
        inp.add("m%d" % j, lay["m"][0], (B2, k) + sp, lay["m"][1], 50 + j)
    crit = pkg.WeightedMSE()

    def call(a):
        res = pkg.embedding_loss_multi([a["e%d" % j] for j in range(3)], [a["t%d" % j] for j in range(3)], [a["w%d" % j] for j in range(3)],
                                       [a["m%d" % j] for j in range(3)], crit, offsets, need_affs=True)
        (res[0][0] * 0.5 + res[1][0] * 2.0 + res[2][0]).backward()
        out = {}
        for j, (loss, affs, parts) in enumerate(res):
            out.update({"loss%d" % j: loss, "affs%d" % j: affs, "parts%d" % j: parts.tensor})
        return out

    out, args = contract(call, inp, leaves=("e0", "e1", "e2"))
    for j, dl in enumerate((0.5, 2.0, 1.0)):
        sub = dict(e=args["e%d" % j], t=args["t%d" % j], w=args["w%d" % j], m=args["m%d" % j])
        res = dict(loss=out["loss%d" % j], affs=out["affs%d" % j], parts=out["parts%d" % j], grad_e=out["grad_e%d" % j])
        anchor_loss(res, sub, off3(offsets[j]), [1.0] * len(offsets[j]), BORDER_CIRCULAR, NORM_BX, dl)


def test_embedding_loss_norm1_multi_mixed_layouts(pkg, dev):
    vols = [VOL1, (3, 8, 12)]
    table = [dict(e="L6", t="L1a", w="L4"), dict(e="L7", t="L5", w="L2")]
    inp = Inputs(dev)
    for j, (vol, lay) in enumerate(zip(vols, table)):
        inp.add("e%d" % j, lay["e"], (B3, D) + vol, torch.float32, 60 + j)
        inp.add("t%d" % j, lay["t"], (B3, 3) + vol, "mask_f32", 62 + j)
        inp.add("w%d" % j, lay["w"], (B3, 3) + vol, "mask_f32", 64 + j)
    crit = pkg.WeightedMSE()

    def call(a):
        res = pkg.embedding_loss_norm1_multi([a["e0"], a["e1"]], [a["t0"], a["t1"]], [a["w0"], a["w1"]], crit, affs0_weight=2, need_affs=True)
        (res[0][0] + res[1][0] * 0.25).backward()
        return {"loss0": res[0][0], "affs0": res[0][1], "loss1": res[1][0], "affs1": res[1][1]}

    out, args = contract(call, inp, leaves=("e0", "e1"))
    offsets3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    for j, dl in enumerate((1.0, 0.25)):
        sub = dict(e=args["e%d" % j], t=args["t%d" % j], w=args["w%d" % j])
        res = dict(loss=out["loss%d" % j], affs=out["affs%d" % j], grad_e=out["grad_e%d" % j])
        anchor_loss(res, sub, offsets3, [2.0, 1.0, 1.0], BORDER_CROP_ZERO, NORM_CROPPED, dl)


# ---- the loss sections ----------------------------------------------------------------------------------------------------------------------
SEC_SHIFTS, SEC_NB_HALF, SEC_B, SEC_HW = [1, 3, 5, 9, 27], 2, 2, 96
SEC_VOLS = [(6, 72, 76), (6, 36, 38), (6, 36, 38), (3, 18, 20), (3, 18, 20)]  # full, emd1 .. emd4


def _section_embeddings_2d(inp, layout):
    inp.add("e", layout, (SEC_B, D, SEC_HW, SEC_HW), torch.float32, 70)
    inp.add("ema", layout, (SEC_B, D, SEC_HW, SEC_HW), torch.float32, 71)
    for j in range(4):
        inp.add("emd%d" % j, layout, (SEC_B, D, SEC_HW >> (j + 1), SEC_HW >> (j + 1)), torch.float32, 72 + j)


def _section_out(loss, pred, parts, scale):
    (loss * scale).backward()
    out = dict(loss=loss, pred=pred)
    if parts is not None:
        out.update(self_part=parts["loss_embedding"], cross_part=parts["loss_embedding_cross"])
        out.update({"emd_part%d" % j: p for j, p in enumerate(parts["loss_emd"])})
    return out


@pytest.mark.parametrize("batched", [False, True], ids=["per_scale", "batched"])
def test_cvppp_loss_section_l1_weights_l6_embeddings(pkg, dev, batched):
    offsets = pkg.multi_offset(SEC_SHIFTS, 4)
    K = len(offsets)
    inp = Inputs(dev)
    _section_embeddings_2d(inp, "L6")
    inp.add("t", "L4", (SEC_B, K, SEC_HW, SEC_HW), "mask_f32", 80)
    inp.add("w", "L1a", (SEC_B, K, SEC_HW, SEC_HW), "mask_f32", 81)
    inp.add("m", "L1b", (SEC_B, K, SEC_HW, SEC_HW), torch.uint8, 82)
    for j in range(4):  # the packed (target | weight | mask) thirds, float like the reference's; two of them broadcast over the batch
        k = SEC_NB_HALF * (4 - j)
        inp.add("down%d" % j, ("L1a", "L5", "L1b", "L3")[j], (SEC_B, 3 * k, SEC_HW >> (j + 1), SEC_HW >> (j + 1)), "mask_f32", 83 + j)
    crit = pkg.WeightedMSE()

    def call(a):
        loss, pred, parts = pkg.cvppp_loss_section(a["e"], [a["emd%d" % j] for j in range(4)], a["ema"], a["t"], a["w"], a["m"],
                                                   [a["down%d" % j] for j in range(4)], crit, offsets, SEC_NB_HALF, deep_weight=2,
                                                   self_emb=0.7, cross_emb=1.3, batched=batched)
        return _section_out(loss, pred, parts, 0.5)

    out, args = contract(call, inp, leaves=("e", "emd0", "emd1", "emd2", "emd3"))
    # float64: the six losses of scripts_cvppp/main.py:284-293 with their weights
    dwf = pkg.deep_weight_factor(2)
    o3 = off3(offsets)
    ref_s = cosine_loss(as5(args["e"]), None, as5(args["t"]), as5(args["w"]), as5(args["m"].float()), o3, [1.0] * K, 1e-12, BORDER_CIRCULAR,
                        NORM_BX, dloss=0.5 * dwf[0] * 0.7)
    ref_x = cosine_loss(as5(args["e"]), as5(args["ema"]), as5(args["t"]), as5(args["w"]), as5(args["m"].float()), o3, [1.0] * K, 1e-12,
                        BORDER_CIRCULAR, NORM_BX, dloss=0.5 * dwf[0] * 1.3)
    want = dwf[0] * (0.7 * float(ref_s["loss"]) + 1.3 * float(ref_x["loss"]))
    for j in range(4):
        k = SEC_NB_HALF * (4 - j)
        dn = args["down%d" % j]
        rj = cosine_loss(as5(args["emd%d" % j]), None, as5(dn[:, :k]), as5(dn[:, k:2 * k]), as5(dn[:, 2 * k:]), o3[:k], [1.0] * k, 1e-12,
                         BORDER_CIRCULAR, NORM_BX, dloss=0.5 * dwf[j + 1] * 0.7)
        want += dwf[j + 1] * 0.7 * float(rj["loss"])
        assert relmax(as5(out["grad_emd%d" % j]), rj["de"]) < GRAD_RTOL
    assert abs(val(out["loss"]) - want) <= LOSS_RTOL * abs(want)
    assert relmax(as5(out["grad_e"]), ref_s["de"] + ref_x["de"]) < GRAD_RTOL
    assert float((as5(out["pred"]).double() - ref_s["affs"]).abs().max()) < AFFS_ATOL


@pytest.mark.parametrize("batched", [False, True], ids=["per_scale", "batched"])
def test_cvppp_loss_section_from_labels_l9_labels(pkg, dev, batched):
    offsets = pkg.multi_offset(SEC_SHIFTS, 4)
    crit = pkg.WeightedMSE()
    res = {}
    for form, (lab_layout, down_layout, dtype) in (("plane", ("L9p", "L9s", torch.int64)), ("strided", ("L9s", "L9p", torch.int16)),
                                                   ("crop", ("L3", "L3", torch.uint8))):
        inp = Inputs(dev)
        _section_embeddings_2d(inp, "L6")
        inp.labels("lab", lab_layout, SEC_B, (SEC_HW, SEC_HW), dtype, 90)
        for j in range(4):
            inp.labels("lab%d" % j, down_layout, SEC_B, (SEC_HW >> (j + 1), SEC_HW >> (j + 1)), dtype, 91 + j)

        def call(a):
            loss, pred, parts = pkg.cvppp_loss_section_from_labels(a["e"], [a["emd%d" % j] for j in range(4)], a["ema"], a["lab"],
                                                                   [a["lab%d" % j] for j in range(4)], crit, offsets, SEC_NB_HALF,
                                                                   deep_weight=2, batched=batched)
            return _section_out(loss, pred, parts, 0.5)

        res[form], args = contract(call, inp, leaves=("e", "emd0", "emd1", "emd2", "emd3"))
    # the anchor: the labels-in section against the tensor section on the targets the label images stand for (the tensor section is
    # held to float64 above), at the bars tests/test_gpu_parity.py::test_labels_step_3d_and_section holds the two to
    t, m, w = pkg.gen_targets(args["lab"], offsets, padding=True)
    downs = []
    for j in range(4):
        k = SEC_NB_HALF * (4 - j)
        tj, mj, wj = pkg.gen_targets(args["lab%d" % j], offsets[:k], padding=True)
        downs.append(torch.cat([tj, wj, mj.float()], dim=1))
    leaves = [args[k].detach().clone().requires_grad_(True) for k in ("e", "emd0", "emd1", "emd2", "emd3")]
    loss, pred, _ = pkg.cvppp_loss_section(leaves[0], leaves[1:], args["ema"], t, w, m, downs, crit, offsets, SEC_NB_HALF, deep_weight=2)
    (loss * 0.5).backward()
    out = res["crop"]
    assert abs(val(out["loss"]) - val(loss)) <= LOSS_RTOL * abs(val(loss))
    assert float((out["pred"] - pred).abs().max()) < AFFS_ATOL
    for k, leaf in zip(("e", "emd0", "emd1", "emd2", "emd3"), leaves):
        assert relmax(out["grad_" + k], leaf.grad) < GRAD_RTOL


def _section_embeddings_3d(inp, layout):
    inp.add("e", layout, (SEC_B, D) + SEC_VOLS[0], torch.float32, 100)
    inp.add("ema", layout, (SEC_B, D) + SEC_VOLS[0], torch.float32, 101)
    for j in range(4):
        inp.add("emd%d" % j, layout, (SEC_B, D) + SEC_VOLS[1 + j], torch.float32, 102 + j)


def test_ac3ac4_loss_section_l1_weights_l6_embeddings(pkg, dev):
    inp = Inputs(dev, arena_bytes=64 << 20)
    _section_embeddings_3d(inp, "L6")
    inp.add("t", "L4", (SEC_B, 12) + SEC_VOLS[0], "mask_f32", 110)
    inp.add("w", "L1a", (SEC_B, 12) + SEC_VOLS[0], "mask_f32", 111)
    for k in range(4):  # downs[k] belongs to emd(4 - k): packed (target[:3] | weight[3:])
        inp.add("down%d" % k, ("L1b", "L5", "L3", "L1a")[k], (SEC_B, 6) + SEC_VOLS[4 - k], "mask_f32", 112 + k)
    crit = pkg.WeightedMSE()

    def call(a):
        loss, pred = pkg.ac3ac4_loss_section(a["e"], [a["emd%d" % j] for j in range(4)], a["ema"], a["t"], a["w"],
                                             [a["down%d" % k] for k in range(4)], crit, embedding_mode=5, affs0_weight=2)
        return _section_out(loss, pred, None, 0.5)

    out, args = contract(call, inp, leaves=("e", "emd0", "emd1", "emd2", "emd3"))
    o5 = [[-s if a == i % 3 else 0 for a in range(3)] for i, s in enumerate(NORM5)]
    o1 = o5[:3]
    lam5 = [2.0] * 3 + [1.0] * 9
    ref_s = cosine_loss(args["e"], None, args["t"], args["w"], None, o5, lam5, 1e-12, BORDER_CROP_ZERO, NORM_CROPPED, dloss=0.5)
    ref_x = cosine_loss(args["e"], args["ema"], args["t"], args["w"], None, o5, lam5, 1e-12, BORDER_CROP_ZERO, NORM_CROPPED, dloss=0.5)
    want = float(ref_s["loss"]) + float(ref_x["loss"])
    for j in range(4):
        dn = args["down%d" % (3 - j)]
        rj = cosine_loss(args["emd%d" % j], None, dn[:, :3], dn[:, 3:], None, o1, [2.0, 1.0, 1.0], 1e-12, BORDER_CROP_ZERO, NORM_CROPPED, dloss=0.5)
        want += float(rj["loss"])
        assert relmax(out["grad_emd%d" % j], rj["de"]) < GRAD_RTOL
    assert abs(val(out["loss"]) - want) <= LOSS_RTOL * abs(want)
    assert relmax(out["grad_e"], ref_s["de"] + ref_x["de"]) < GRAD_RTOL
    assert float((out["pred"].double() - ref_s["affs"]).abs().max()) < AFFS_ATOL


def test_ac3ac4_loss_section_from_labels_l9_labels(pkg, dev):
    crit = pkg.WeightedMSE()
    inp = Inputs(dev)
    _section_embeddings_3d(inp, "L6")
    inp.labels("lab", "L9p", SEC_B, SEC_VOLS[0], torch.int64, 120)
    for k in range(4):
        inp.labels("lab%d" % k, ("L9s", "L3", "L1a", "L9s")[k], SEC_B, SEC_VOLS[4 - k], (torch.int32, torch.int16, torch.uint8, torch.int64)[k], 121 + k)

    def call(a):
        loss, pred = pkg.ac3ac4_loss_section_from_labels(a["e"], [a["emd%d" % j] for j in range(4)], a["ema"], a["lab"],
                                                         [a["lab%d" % k] for k in range(4)], crit, embedding_mode=5, affs0_weight=2)
        return _section_out(loss, pred, None, 0.5)

    out, args = contract(call, inp, leaves=("e", "emd0", "emd1", "emd2", "emd3"))
    o5 = [[-s if a == i % 3 else 0 for a in range(3)] for i, s in enumerate(NORM5)]
    t0, _, w0 = pkg.gen_targets(args["lab"], o5, padding=False, both_foreground=True, want_mask=False)
    downs = []
    for k in range(4):
        tk, _, wk = pkg.gen_targets(args["lab%d" % k], o5[:3], padding=False, both_foreground=True, want_mask=False)
        downs.append(torch.cat([tk, wk], dim=1))
    leaves = [args[k].detach().clone().requires_grad_(True) for k in ("e", "emd0", "emd1", "emd2", "emd3")]
    loss, pred = pkg.ac3ac4_loss_section(leaves[0], leaves[1:], args["ema"], t0, w0, downs, crit, embedding_mode=5, affs0_weight=2)
    (loss * 0.5).backward()
    assert abs(val(out["loss"]) - val(loss)) <= LOSS_RTOL * abs(val(loss))
    assert float((out["pred"] - pred).abs().max()) < AFFS_ATOL
    for k, leaf in zip(("e", "emd0", "emd1", "emd2", "emd3"), leaves):
        assert relmax(out["grad_" + k], leaf.grad) < GRAD_RTOL


# ---- the labels-in entries and the target generators -------------------------------------------------------------------------------------
LABEL_CASES = [("L1a", torch.int64), ("L1b", torch.uint8), ("L3", torch.int32), ("L9s", torch.int16), ("L9p", torch.int64), ("L9s", torch.bool),
               ("L3", torch.uint8), ("L9p", torch.int32)]
LABEL_IDS = ["%s-%s" % (l, str(d).split(".")[1]) for l, d in LABEL_CASES]


@pytest.mark.parametrize("layout,dtype", LABEL_CASES, ids=LABEL_IDS)
def test_gen_targets_and_seg_to_aff(pkg, dev, offs2, layout, dtype):
    inp = Inputs(dev)
    inp.labels("lab2", layout, B2, (H, W), dtype, 130)
    inp.labels("lab3", layout, B3, VOL1, dtype, 131)

    def call(a):
        t, m, w = pkg.gen_targets(a["lab2"], offs2, padding=True)
        t3, _, w3 = pkg.gen_targets(a["lab3"], [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], padding=False, both_foreground=True, want_mask=False)
        ta, ma = pkg.gen_affs_ours(a["lab2"], offs2, padding=True)
        return dict(t=t, m=m, w=w, t3=t3, w3=w3, ta=ta, ma=ma, aff=pkg.seg_to_aff(a["lab3"]))

    out, args = contract(call, inp)
    # the anchor: gen_affs_ours(padding=True) restated on the label image (1 where the labels agree or the neighbour is outside)
    lab = args["lab2"].long()
    for i, (dy, dx) in enumerate(offs2):
        nb = torch.roll(lab, shifts=(-dy, -dx), dims=(1, 2))
        yy, xx = torch.arange(H, device=dev).view(1, H, 1) + dy, torch.arange(W, device=dev).view(1, 1, W) + dx
        inside = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).expand(B2, H, W)
        assert torch.equal(out["t"][:, i], torch.where(inside, (lab == nb).float(), torch.ones_like(out["t"][:, i])))
        assert torch.equal(out["m"][:, i].bool(), inside)
    seg = args["lab3"].long()
    assert torch.equal(out["aff"][:, 2, :, :, 1:], ((seg[..., 1:] == seg[..., :-1]) & (seg[..., 1:] > 0)).float())


@pytest.mark.parametrize("layout,dtype", LABEL_CASES, ids=LABEL_IDS)
def test_embedding_loss_from_labels(pkg, dev, offs2, layout, dtype):
    inp = Inputs(dev)
    inp.add("e", "L6", (B2, D, H, W), torch.float32, 140)
    inp.labels("lab", layout, B2, (H, W), dtype, 141)
    inp.add("e3", "L3", (B3, D) + VOL1, torch.float32, 142)
    inp.labels("lab3", layout, B3, VOL1, dtype, 143)
    crit = pkg.WeightedMSE()

    def call(a):
        loss, affs, parts = pkg.embedding_loss_from_labels(a["e"], a["lab"], crit, offs2)
        loss3, affs3 = pkg.embedding_loss_norm1_from_labels(a["e3"], a["lab3"], crit, affs0_weight=2)
        (loss * 0.75 + loss3).backward()
        return dict(loss=loss, affs=affs, parts=parts.tensor, loss3=loss3, affs3=affs3)

    out, args = contract(call, inp, leaves=("e", "e3"))
    t, m, w = pkg.gen_targets(args["lab"], offs2, padding=True)
    sub = dict(e=args["e"], t=t, w=w, m=m)
    anchor_loss(dict(loss=out["loss"], affs=out["affs"], parts=out["parts"], grad_e=out["grad_e"]), sub, off3(offs2), [1.0] * len(offs2),
                BORDER_CIRCULAR, NORM_BX, 0.75)


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "shared_image"])
@pytest.mark.parametrize("layout,dtype", LABEL_CASES[:6], ids=LABEL_IDS[:6])
def test_embedding_loss_from_labels_multi(pkg, dev, offs2, layout, dtype, shared):
    shapes = [(H, W), (H // 2, W // 2)]
    offsets = [offs2, offs2[:2]]
    inp = Inputs(dev)
    for j, sp in enumerate(shapes):
        inp.add("e%d" % j, ("L6", "L3")[j], (B2, D) + sp, torch.float32, 150 + j)
    inp.labels("lab0", layout, B2, shapes[0], dtype, 152)
    if not shared:
        inp.labels("lab1", layout, B2, shapes[1], dtype, 153)
    crit = pkg.WeightedMSE()

    def call(a):
        labels = a["lab0"] if shared else [a["lab0"], a["lab1"]]
        res = pkg.embedding_loss_from_labels_multi([a["e0"], a["e1"]], labels, crit, offsets, need_affs=True)
        (res[0][0] + res[1][0] * 0.5).backward()
        out = {}
        for j, (loss, affs, parts) in enumerate(res):
            out.update({"loss%d" % j: loss, "affs%d" % j: affs, "parts%d" % j: parts.tensor})
        return out

    out, args = contract(call, inp, leaves=("e0", "e1"))
    for j, dl in enumerate((1.0, 0.5)):
        lab = args["lab0"][:, ::2, ::2] if (shared and j) else args["lab%d" % j]
        t, m, w = pkg.gen_targets(lab, offsets[j], padding=True)
        res = dict(loss=out["loss%d" % j], affs=out["affs%d" % j], parts=out["parts%d" % j], grad_e=out["grad_e%d" % j])
        anchor_loss(res, dict(e=args["e%d" % j], t=t, w=w, m=m), off3(offsets[j]), [1.0] * len(offsets[j]), BORDER_CIRCULAR, NORM_BX, dl)


# ---- a criterion on the activated map --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", ["L1a", "L1b"])
def test_weighted_bce_on_the_activated_map_with_broadcast_weights(pkg, dev, offs2, wl):
    """WeightedBCE through loss_embedding.embedding_loss: the batch-stride decision reaches the PEA_FLAG_LOSS_* path"""
    K = len(offs2)
    inp = Inputs(dev)
    inp.add("e", "L6", (B2, D, H, W), torch.float32, 160)
    inp.add("t", "L4", (B2, K, H, W), "mask_f32", 161)
    inp.add("w", wl, (B2, K, H, W), "mask_f32", 162)
    inp.add("m", "L1a", (B2, K, H, W), torch.uint8, 163)
    crit = pkg.WeightedBCE()

    def call(a):
        loss, affs = pkg.loss_embedding.embedding_loss(a["e"], a["t"], a["w"], a["m"], crit, offs2, affs0_weight=2)
        (loss * 0.75).backward()
        return dict(loss=loss, affs=affs)

    out, args = contract(call, inp, leaves=("e",))
    # float64: u = clamp((cos + 1) / 2, 0, 1) with the norm clamp at 1e-6, F.binary_cross_entropy(u m, t m, w) per offset
    x = args["e"].detach().double().requires_grad_(True)
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-6)
    total = 0.0
    for i, (dy, dx) in enumerate(offs2):
        u = (((xn * torch.roll(xn, shifts=(-dy, -dx), dims=(2, 3))).sum(1) + 1) / 2).clamp(0, 1)
        m = args["m"][:, i].double()
        li = torch.nn.functional.binary_cross_entropy(u * m, args["t"][:, i].double() * m, args["w"][:, i].double())
        total = total + li * (2.0 if i < 2 else 1.0)
    (total * 0.75).backward()
    assert abs(val(out["loss"]) - val(total)) <= LOSS_RTOL * abs(val(total))
    assert relmax(out["grad_e"], x.grad) < GRAD_RTOL


# ---- inference and the differentiable map ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", E_LAYOUTS)
def test_affinity_infer_and_embedding2affs(pkg, dev, offs2, layout):
    inp = Inputs(dev)
    inp.add("e", layout, (B2, D, H, W), torch.float32, 170)
    inp.add("ema", E_LAYOUTS[(E_LAYOUTS.index(layout) + 1) % 3], (B2, D, H, W), torch.float32, 171)
    inp.add("e3", layout, (B3, D) + VOL5, torch.float32, 172)
    spec = pkg.AffinitySpec(2, offs2, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)

    def call(a):
        return dict(a=pkg.embedding2affs(a["e"], offs2), relu=pkg.embedding2affs(a["e"], offs2, activation="relu"),
                    cross=pkg.affinity_infer(a["e"], a["ema"], spec), n1=pkg.inf_embedding_loss_norm1(a["e3"]),
                    n5=pkg.inf_embedding_loss_norm5(a["e3"]))

    out, args = contract(call, inp)
    ref = vjp(as5(args["e"]), None, torch.zeros((B2, len(offs2), 1, H, W), device=dev), off3(offs2), 1e-12, BORDER_CIRCULAR, None)
    assert float((as5(out["a"]).double() - ref["affs"]).abs().max()) < AFFS_ATOL
    assert torch.equal(out["relu"], torch.relu(out["a"]))


def _upstream(style, out, G):
    """a scalar whose backward hands `out` the upstream gradient G in the layout of L10 `style`"""
    nd = out.dim()
    if style == "sum":        # ones, expanded: every stride 0
        return out.sum()
    if style == "perm":       # a channels-last tensor seen through permute: what a graph through permute().contiguous() sends back
        perm = (0,) + tuple(range(2, nd)) + (1,)
        return (out.permute(*perm) * G.permute(*perm).contiguous()).sum()
    if style == "cl":
        return (out * G.contiguous(memory_format=torch.channels_last if nd == 4 else torch.channels_last_3d)).sum()
    raise ValueError(style)


def _upstream_pair(style, make_out, wrt, G):
    """gradients of `wrt` for the L10 upstream of `style` and for the same values as a dense grad_output -> (strided, dense, seen):
    seen: the strides autograd handed to the node in the strided run"""
    seen = []
    out = make_out()
    out.register_hook(lambda g: seen.append((tuple(g.shape), tuple(g.stride()), g.is_contiguous())))
    strided = torch.autograd.grad(_upstream(style, out, G), wrt)
    out = make_out()
    dense = torch.autograd.grad(out, wrt, grad_outputs=(torch.ones_like(out) if style == "sum" else G.clone()))
    return strided, dense, seen


@pytest.mark.parametrize("style", ["sum", "perm", "cl"])
@pytest.mark.parametrize("ema", [False, True], ids=["self", "ema"])
def test_affinity_map_upstream_gradient_layouts(pkg, dev, offs2, style, ema):
    K = len(offs2)
    spec = pkg.AffinitySpec(2, offs2, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    e = ly.make("L6", (B2, D, H, W), torch.float32, 180, dev)[0].detach().requires_grad_(True)
    o = ly.make("L3", (B2, D, H, W), torch.float32, 181, dev)[0].detach().requires_grad_(True) if ema else None
    G = ly.values((B2, K, H, W), torch.float32, 182, dev)
    wrt = [e, o] if ema else [e]
    strided, dense, seen = _upstream_pair(style, lambda: pkg.AffinityMap.apply(e, o, spec), wrt, G)
    if style != "cl":
        assert seen and not seen[0][2], "the upstream gradient arrived contiguous: %s" % (seen,)
    for a, b, leaf in zip(strided, dense, wrt):
        assert tuple(a.shape) == tuple(leaf.shape) and same(a, b) and torch.equal(a, b)
    Gd = torch.ones_like(G) if style == "sum" else G
    ref = vjp(as5(e), as5(o), as5(Gd), off3(offs2), 1e-12, BORDER_CIRCULAR, None, other_grad=ema)
    assert relmax(as5(dense[0]), ref["de"]) < GRAD_RTOL
    if ema:
        assert relmax(as5(dense[1]), ref["de_other"]) < GRAD_RTOL


# ---- the embedding head ----------------------------------------------------------------------------------------------------------------------
HEAD_DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _head(pkg, dev, ndim, seed):
    torch.manual_seed(seed)
    head = pkg.OutConv(32, 16) if ndim == 2 else pkg.head_conv3d_block(28, 16)
    return head.to(dev)


def _head_params(head):
    conv = head.conv if hasattr(head, "conv") else head[0]
    return conv.weight, conv.bias


@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("layout", ["L6", "L7", "L3"])
def test_head_on_strided_features(pkg, dev, layout, ndim, dtype):
    head = _head(pkg, dev, ndim, 190)
    Wt, bt = _head_params(head)
    shape = (B2, 32, H, W) if ndim == 2 else (B3, 28) + VOL1
    view = ly.make(layout, shape, dtype, 191, dev)[0]
    assert not view.is_contiguous()
    snap = view.clone()
    G = ly.values((shape[0], 16) + shape[2:], dtype, 192, dev)
    res = []
    for x in (view.detach().requires_grad_(True), ly.dense(view).requires_grad_(True)):
        e = head(x)
        res.append((e,) + torch.autograd.grad(e, [x, Wt, bt], grad_outputs=G))
    for name, a, b in zip(("e", "dx", "dW", "db"), res[0], res[1]):
        assert same(a, b), name
    assert tuple(res[0][1].shape) == shape and same(view, snap)
    if dtype == torch.float32 and layout == "L6":  # the float64 anchor
        x64, W64, G64 = ly.dense(view).double(), Wt.detach().double().reshape(16, -1), G.double()
        e, dx, dW, db = res[1]
        assert relmax(e, torch.einsum("dc,bc...->bd...", W64, x64) + bt.detach().double().view((1, 16) + (1,) * ndim)) < GRAD_RTOL
        assert relmax(dx, torch.einsum("dc,bd...->bc...", W64, G64)) < GRAD_RTOL
        assert relmax(dW.reshape(16, -1), torch.einsum("bd...,bc...->dc", G64, x64)) < GRAD_RTOL
        assert relmax(db, G64.transpose(0, 1).reshape(16, -1).sum(1)) < GRAD_RTOL


@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("style", ["sum", "perm", "cl"])
def test_head_upstream_gradient_layouts(pkg, dev, style, ndim, dtype):
    head = _head(pkg, dev, ndim, 193)
    Wt, bt = _head_params(head)
    shape = (B2, 32, H, W) if ndim == 2 else (B3, 28) + VOL1
    x = ly.make("L6", shape, dtype, 194, dev)[0].detach().requires_grad_(True)
    G = ly.values((shape[0], 16) + shape[2:], dtype, 195, dev)
    strided, dense, seen = _upstream_pair(style, lambda: head(x), [x, Wt, bt], G)
    if style != "cl":
        assert seen and not seen[0][2], "the upstream gradient arrived contiguous: %s" % (seen,)
    for name, a, b in zip(("dx", "dW", "db"), strided, dense):
        assert same(a, b), name


@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("layout,tl,wl,ml", [("L6", "L1a", "L4", "L2"), ("L7", "L5", "L1b", "L1a"), ("L3", "L8", "L2", "L3")])
def test_head_embedding_loss(pkg, dev, offs2, layout, tl, wl, ml, dtype):
    """head + loss as one node: x strided, the loss operands in their layouts, and a second use of the embedding output whose
    gradient arrives with stride 0 (L10)"""
    K = len(offs2)
    head = _head(pkg, dev, 2, 196)
    Wt, bt = _head_params(head)
    inp = Inputs(dev)
    inp.add("x", layout, (B2, 32, H, W), dtype, 197)
    inp.add("t", tl, (B2, K, H, W), "mask_f32", 198)
    inp.add("w", wl, (B2, K, H, W), "mask_f32", 199)
    inp.add("m", ml, (B2, K, H, W), torch.uint8, 200)
    crit = pkg.WeightedMSE()

    def call(a):
        loss, affs, parts, emb = pkg.head_embedding_loss(a["x"], head, a["t"], a["w"], a["m"], crit, offs2)
        Wt.grad = bt.grad = None
        (loss * 0.75 + emb.sum() * 1e-3).backward()
        dW, db = Wt.grad, bt.grad
        Wt.grad = bt.grad = None
        return dict(loss=loss, affs=affs, parts=parts.tensor, emb=emb, dW=dW, db=db)

    out, args = contract(call, inp, leaves=("x",))
    if dtype == torch.float32 and layout == "L6":  # the anchor: the one node against head(x) -> float64 loss on ITS embedding
        ref = cosine_loss(as5(out["emb"]), None, as5(args["t"]), as5(args["w"]), as5(args["m"].float()), off3(offs2), [1.0] * K, 1e-12,
                          BORDER_CIRCULAR, NORM_BX, dloss=0.75)
        assert abs(val(out["loss"]) - float(ref["loss"])) <= LOSS_RTOL * abs(float(ref["loss"]))
        assert float((as5(out["affs"]).double() - ref["affs"]).abs().max()) < AFFS_ATOL
        de = ref["de"][:, :, 0] + 1e-3
        W64 = Wt.detach().double().reshape(16, 32)
        assert relmax(out["grad_x"], torch.einsum("dc,bdhw->bchw", W64, de)) < GRAD_RTOL
        assert relmax(out["dW"].reshape(16, 32), torch.einsum("bdhw,bchw->dc", de, args["x"].detach().double())) < GRAD_RTOL
        assert relmax(out["db"], de.sum((0, 2, 3))) < GRAD_RTOL


# ---- the discriminative loss ---------------------------------------------------------------------------------------------------------------------
DISC_CASES = [("L3", "L9s", torch.int64), ("L6", "L9p", torch.int32), ("L3", "L9n", torch.int16), ("L6", "L9s", torch.uint8), ("L7", "L1a", torch.int64)]


@pytest.mark.parametrize("el,ll,dtype", DISC_CASES, ids=["%s-%s-%s" % (a, b, str(c).split(".")[1]) for a, b, c in DISC_CASES])
@pytest.mark.parametrize("num_ids", [None, 8])
def test_discriminative_loss(pkg, dev, el, ll, dtype, num_ids):
    inp = Inputs(dev)
    inp.add("e", el, (B2, D, H, W), torch.float32, 210)
    inp.labels("lab", ll, B2, (H, W), dtype, 211)

    def call(a):
        loss, stats = pkg.discriminative_loss_stats(a["e"], a["lab"], background=False, num_ids=num_ids)
        (loss * 0.75).backward()
        return dict(loss=loss, stats=stats, again=pkg.discriminative_loss(a["e"].detach(), a["lab"], num_ids=num_ids))

    out, args = contract(call, inp, leaves=("e",))
    if el == "L3" and num_ids is None:
        loss, stats, de = disc_reference(args["e"].detach().cpu().numpy(), args["lab"].cpu().numpy().reshape(B2, H, W), dloss=0.75)
        assert abs(val(out["loss"]) - loss) <= LOSS_RTOL * abs(loss)
        np.testing.assert_allclose(out["stats"].cpu().numpy(), stats, rtol=LOSS_RTOL, atol=0)
        assert relmax(out["grad_e"], torch.from_numpy(de).to(dev)) < GRAD_RTOL


# ---- the foreground mask -----------------------------------------------------------------------------------------------------------------------------
FG_CASES = [("L6", "packed", torch.uint8), ("L7", "packed", torch.int32), ("L6", "L1a", torch.bool), ("L7", "L1b", torch.bool),
            ("L3", "L9s", torch.uint8), ("L2", "L9n", torch.bool)]


@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("gl,ll,ldtype", FG_CASES, ids=["%s-%s-%s" % (a, b, str(c).split(".")[1]) for a, b, c in FG_CASES])
def test_foreground_mask_entries(pkg, dev, gl, ll, ldtype, dtype):
    inp = Inputs(dev)
    inp.add("lg", gl, (B2, 2, H, W), dtype, 220)
    if ll == "packed":  # [B, 1, H, W] sliced from a packed label tensor
        inp.views["lab"] = ly.label_values((B2, 3, H, W), ldtype, 221, dev)[:, 1:2]
    else:
        inp.labels("lab", ll, B2, (H, W), ldtype, 221)

    def call(a):
        loss, stats = pkg.foreground_mask_loss(a["lg"], a["lab"])
        (loss * 0.75).backward()
        return dict(loss=loss, stats=stats, bce=pkg.BCE_loss_func(a["lg"].detach(), a["lab"]), mask=pkg.foreground_mask(a["lg"]),
                    crop=pkg.foreground_mask(a["lg"], crop=((2, 3), (4, 1))))

    out, args = contract(call, inp, leaves=("lg",))
    lg, lab = args["lg"].detach().float().cpu().numpy(), args["lab"].cpu().numpy().reshape(B2, H, W)
    assert np.array_equal(out["mask"].cpu().numpy(), mask_reference(lg)) and np.array_equal(out["crop"].cpu().numpy(), mask_reference(lg, ((2, 3), (4, 1))))
    if dtype == torch.float32 and (gl, ll) == ("L6", "packed"):
        loss, stats, dlg = fgmask_reference(lg, lab, dloss=0.75)
        assert abs(val(out["loss"]) - loss) <= LOSS_RTOL * abs(loss)
        np.testing.assert_allclose(out["stats"].cpu().numpy(), stats, rtol=LOSS_RTOL, atol=0)
        assert relmax(out["grad_lg"], torch.from_numpy(dlg).to(dev)) < GRAD_RTOL


# ---- the validation metrics and the in-place epilogues -------------------------------------------------------------------------------------------------
MET_CASES = [(t, MASK_LAYOUTS[(i + 2) % 6], k) for i, (t, k) in enumerate(zip(MASK_LAYOUTS, ("u8", "bool", "f32", "u8", "bool", "f32")))]


@pytest.mark.parametrize("tl,ml,kind", MET_CASES, ids=["t_%s-m_%s_%s" % (a, k, b) for a, b, k in MET_CASES])
def test_affinity_metrics(pkg, dev, tl, ml, kind):
    K = 4
    pred = ly.values((B2, K, H, W), torch.float32, 230, dev) * 0.5 + 0.5
    inp = Inputs(dev)
    inp.add("t", tl, (B2, K, H, W), torch.uint8, 231)
    inp.add("m", ml, (B2, K, H, W), MASK_KINDS[kind], 232)
    snap = pred.clone()

    def call(a):
        tab = pkg.affinity_metrics(pred, a["t"], a["m"], relu=True)  # (a uint8 target is converted by the entry itself)
        tab2 = pkg.affinity_metrics(pred, a["t"], None, relu=True)
        return dict(table=tab.table, nomask=tab2.table)

    out, args = contract(call, inp)
    assert same(pred, snap)
    ref = metrics_reference(pred.cpu().numpy(), args["t"].float().cpu().numpy(), args["m"].float().cpu().numpy(), relu=True)
    got = out["table"].cpu().numpy()
    np.testing.assert_allclose(got[:, :2], ref[:, :2], rtol=LOSS_RTOL, atol=0)
    assert np.array_equal(got[:, 2:], ref[:, 2:])


def test_float_targets_in_every_layout_reach_the_metrics(pkg, dev):
    K = 4
    pred = ly.values((B2, K, H, W), torch.float32, 233, dev) * 0.5 + 0.5
    for tl in TW_LAYOUTS:
        inp = Inputs(dev)
        inp.add("t", tl, (B2, K, H, W), "mask_f32", 234)
        out, args = contract(lambda a: dict(table=pkg.affinity_metrics(pred, a["t"]).table), inp)
        ref = metrics_reference(pred.cpu().numpy(), args["t"].cpu().numpy())
        np.testing.assert_allclose(out["table"].cpu().numpy()[:, :2], ref[:, :2], rtol=LOSS_RTOL, atol=0)


@pytest.mark.parametrize("layout", ["L3", "L4", "L5", "L6", "L7", "L1a"])
def test_in_place_entries_refuse_a_strided_pred(pkg, dev, layout):
    """affinity_metrics, fill_border_relu_ and relu_ write (or may write) through data_ptr(): a pred that is not dense is refused before
    anything is launched, and is left as it was"""
    pred = ly.make(layout, (B2, 4, H, W), torch.float32, 240, dev)[0]
    pred3 = ly.make(layout, (B3, 3) + VOL1, torch.float32, 241, dev)[0]
    target = ly.values((B2, 4, H, W), "mask_f32", 242, dev)
    snap, snap3 = pred.clone(), pred3.clone()
    with pytest.raises(ValueError, match="contiguous"):
        pkg.affinity_metrics(pred, target)
    with pytest.raises(ValueError, match="contiguous"):
        pkg.affinity_metrics(pred, target, store=True, relu=True)
    with pytest.raises(ValueError, match="contiguous"):
        pkg.relu_(pred)
    with pytest.raises(ValueError, match="contiguous"):
        pkg.fill_border_relu_(pred3, shift=1)
    wm = ly.make("L3", (1,) + VOL1, torch.float32, 243, dev)[0]
    dense3 = ly.values((1, 3) + VOL1, torch.float32, 244, dev)
    snapd = dense3.clone()
    with pytest.raises(ValueError, match="contiguous"):
        pkg.affinity_metrics(dense3, ly.values((1, 3) + VOL1, "mask_f32", 245, dev), weight_map=wm)
    torch.cuda.synchronize()
    assert same(pred, snap) and same(pred3, snap3) and same(dense3, snapd)


# ---- the un-flip ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("layout", ["L6", "L3", "L7"])
def test_unflip_on_strided_tensors_and_rules(pkg, dev, layout, dtype):
    inp = Inputs(dev)
    inp.add("x", layout, (4, D, 24, 24), dtype, 250)
    inp.add("x3", layout, (4, D, 3, 24, 24), dtype, 251)
    rules = torch.tensor([[1, 9, 0, 9, 0, 9, 1, 9], [0, 9, 1, 9, 1, 9, 0, 9], [1, 9, 1, 9, 1, 9, 1, 9], [0, 9, 0, 9, 1, 9, 1, 9]], device=dev)
    inp.views["r3"] = rules[:, 0:6:2]          # [B, 3] every other column of a wider table
    inp.views["r4"] = rules.t()[::2].t()       # [B, 4] through two transposes
    inp.views["rb"] = (rules[:, 0:6:2] == 1)   # bool
    assert not inp.views["r3"].is_contiguous() and not inp.views["r4"].is_contiguous()

    def call(a):
        return dict(u=pkg.unflip(a["x"], a["r3"]), ub=pkg.unflip(a["x"], a["rb"]), u3=pkg.unflip(a["x3"], a["r3"]), u4=pkg.unflip(a["x3"], a["r4"]),
                    c=pkg.convert_consistency_flip(a["x"], a["r3"]), c4=pkg.convert_consistency_flip(a["x3"], a["r4"]))

    out, args = contract(call, inp)
    assert same(out["u"], out["ub"]) and same(out["u"], out["c"]) and same(out["u4"], out["c4"])
    # the anchor: the reference's composition on views (a bit-exact copy either way)
    ts = importlib.import_module(ge.PKG_NAME + ".harness.train_step")
    assert same(out["u"], ts._torch_unflip(args["x"], args["r3"].cpu().numpy().astype(np.uint8)))
    assert same(out["u4"], ts._torch_unflip(args["x3"], args["r4"].cpu().numpy().astype(np.uint8)))
    assert out["u"].is_contiguous() and out["u4"].is_contiguous()


# ---- the stitcher ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["three_calls", "fused"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_volume_stitcher_on_strided_windows(pkg, dev, fused, dtype):
    vol, pos = (8, 24, 40), [(0, 0, 0), (2, 8, 16)]
    view = ly.make("L3", (B3, D) + VOL1, dtype, 260, dev)[0]
    snap = view.clone()
    affs_vol = ly.values(VOL1 + (3,), torch.float32, 261, dev).permute(3, 0, 1, 2)  # [C, oz, oy, ox] seen through a permute
    assert not view.is_contiguous() and not affs_vol.is_contiguous()
    res = []
    for e, av in ((view, affs_vol), (ly.dense(view), ly.dense(affs_vol))):
        st = pkg.VolumeStitcher(3, vol, VOL1, dev)
        st.add_embedding(e, pos, embedding_mode=1, fused=fused)
        st.add_vol(av, (1, 4, 8))
        res.append((st.out_affs.clone(), st.weight_map.clone(), st.get_results((0, 0, 0)).clone()))
    for name, a, b in zip(("out_affs", "weight_map", "result"), res[0], res[1]):
        assert same(a, b), name
    assert same(view, snap)
    if dtype == torch.float32:  # the anchor: the statements of scripts_ac3ac4/inference.py:150-166 in float64
        ref = vjp(ly.dense(view), None, torch.zeros((B3, 3) + VOL1, device=dev), [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], 1e-12, BORDER_CROP_ZERO, None)
        a = ref["affs"].clone()
        a[:, 0, 0], a[:, 1, :, 0], a[:, 2, :, :, 0] = a[:, 0, 1], a[:, 1, :, 1], a[:, 2, :, :, 1]
        a = a.clamp_min(0)
        wv = torch.from_numpy(importlib.import_module(ge.PKG_NAME + ".harness.stitch").get_weight(VOL1)).to(dev).double()
        acc = torch.zeros((3,) + vol, dtype=torch.float64, device=dev)
        for b, (z, y, x) in enumerate(pos):
            acc[:, z:z + 6, y:y + 16, x:x + 24] += a[b] * wv
        acc[:, 1:7, 4:20, 8:32] += ly.dense(affs_vol).double() * wv
        assert float((res[1][0].double() - acc).abs().max()) < AFFS_ATOL
