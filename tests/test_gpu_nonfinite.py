"""GPU (-m gpu): NaN / inf in an EMBEDDING, through every kernel family -- the "Non-finite embeddings" paragraph of include/pea.h.

One channel of one pixel q of sample 0 is set to NaN, +inf or -inf, in `e` or in the second operand.  Every output must then be NaN
exactly on footprint(q, ...) (tests/test_nonfinite_host.py: index arithmetic alone, itself held to the float64 restatement and to the
reference's modules on the CPU) and BIT-IDENTICAL to the same call on the clean embedding everywhere else: one bad pixel poisons the
pixels whose formulas read it and nothing more, whatever a kernel stages in LDS or reduces across a wave.  Nothing here has a
tolerance: every assertion is isnan, an exact value, or equality of the int32 / int16 views with a clean call of the same kernel.

    A  the loss path   every subject of tests/test_gpu_loss_reduction.py (the alignment CASES with their switches, c16 on the direct
                       kernels, the one-launch pair, the labels step in both forms, each entry of the multi table), forward AND backward,
                       c16_crop on the direct kernels, three more second-operand families (the 3D detached ema with z steps and
                       CROP_ZERO, the 2D cropped ema, REPLICATE with de_other) and pea_affinity_infer: value in {NaN, +inf, -inf}, q interior (on no tile boundary) and at the corner (0, 0, 0) --
                       the pixel a wrapped or clamped read of a cropped pair would land on --, in e and in the second operand; one more
                       NaN run with w = 0 on every footprint pair of one offset and m = 0 on those of another (0 * NaN is NaN: L_i stays
                       NaN); the state block zero after every call; a last clean call bit-identical to the first; inputs unchanged
    B  activations     every activation bit keeps NaN (F.relu and torch.clamp do; fmaxf / fminf would not): the forwards, the inference
                       call, the loss on the activated map (PEA_FLAG_LOSS_ACT) in the families of tests/test_gpu_act_loss.py at the
                       alignment suite's shape, the fused window stitcher, pea_fill_border_relu in its four forms and relu_
    C  the heads       pea_head_fwd / _bwd and pea_head_fwd_t / _bwd_t: a NaN, an inf or a value that overflows f16 in x, a NaN in de

Under PEA_FLAG_LOSS_ACT | PEA_FLAG_CLAMP01 g is 0 on the footprint pairs (u == v is false for NaN, as in torch.clamp's backward) and de at
the neighbours of q is not asserted; the 1 / norm plane at q is not asserted either.  A test gathers every violation of its runs before it
fails, so that one GPU run shows all of them.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_alignment as A
import test_gpu_loss_reduction as R
from f64_reference import BORDER_CROP_ZERO
from test_gpu_alignment import dev, op, synth  # noqa: F401  (fixtures)
from test_nonfinite_host import _axis, footprint

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
RELU, ONE_MINUS, HALF, CLAMP, LOSS_ACT = 1, 2, 4, 8, 64
ACTS = {"relu": RELU, "half": HALF, "clamp": CLAMP, "half_clamp": HALF | CLAMP, "one_minus": ONE_MINUS, "relu_one_minus": RELU | ONE_MINUS}
LACTS = {"half": HALF, "clamp": CLAMP, "half_clamp": HALF | CLAMP}
CHANNEL = 1  # the poisoned channel


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def P(t):
    return A.P(t)


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def interior(dims):
    """a pixel on no tile boundary: (Z // 2, 21, 37) where the image holds it"""
    Z, Y, X = dims
    return (Z // 2, 21 if Y > 23 else Y // 2 + 1, 37 if X > 39 else X // 2 + 1)


def poisoned(t, q, value):
    out = t.clone()
    out[(0, CHANNEL) + tuple(q)] = value
    return out


def full_k(mask, B, dev_):
    """[K,Z,Y,X] of sample 0 -> [B,K,Z,Y,X]"""
    out = torch.zeros((B,) + tuple(mask.shape), dtype=torch.bool)
    out[0] = mask
    return out.to(dev_)


def full_d(mask, B, D, dev_):
    """[Z,Y,X] of sample 0 -> [B,D,Z,Y,X]: all D channels"""
    out = torch.zeros((B, D) + tuple(mask.shape), dtype=torch.bool)
    out[0] = mask
    return out.to(dev_)


def loss_mask(F):
    """[1 + K]: the total, then L_i"""
    return torch.cat([F["loss"].any().view(1), F["loss"]])


def at(shape, idx, dev_):
    out = torch.zeros(tuple(shape), dtype=torch.bool, device=dev_)
    out[idx] = True
    return out


def compare(tag, clean, got, want, unspec, fails, zero=None):
    """every output `key`: NaN exactly on want[key] (none where the key is absent), the clean call's bits elsewhere; unspec[key] marks
    elements that are not asserted, zero[key] elements that must be exactly 0 (affs: zero["act0"], the activation of 0)"""
    assert set(clean) == set(got)
    for key, t in got.items():
        c = clean[key]
        w = want.get(key)
        if w is None:
            w = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
        w = w.to(t.device)
        assert w.shape == t.shape, (tag, key, w.shape, t.shape)
        care = torch.ones_like(w) if unspec.get(key) is None else ~unspec[key].to(t.device)
        isn = torch.isnan(t.float())
        missing, extra = int((w & ~isn & care).sum()), int((isn & ~w & care).sum())
        if missing or extra:
            fails.append("%s %s: %d footprint elements are not NaN (of %d), %d NaN outside the footprint" % (tag, key, missing, int(w.sum()), extra))
        changed = int(((bits(t) != bits(c)) & ~w & care).sum())
        if changed:
            fails.append("%s %s: %d elements outside the footprint differ from the clean call" % (tag, key, changed))
        if zero is not None and zero.get(key) is not None:
            z, v0 = zero[key].to(t.device), (zero.get("act0", 0.0) if key == "affs" else 0.0)
            if bool((t[z] != v0).any()):  # (NaN != v0 as well)
                fails.append("%s %s: %d elements that must be exactly %g are not" % (tag, key, int((t[z] != v0).sum()), v0))


def act_of_zero(flags):
    """what a cropped-away position of the affs output holds: the activation of 0 (include/pea.h: applied in this order)"""
    a = 0.5 if flags & HALF else 0.0
    return 1.0 - a if flags & ONE_MINUS else a


def cropped(c_border, dims, o3, B, dev_):
    """[B,K,Z,Y,X]: the positions whose pair does not exist (CROP_ZERO), else None"""
    if c_border != BORDER_CROP_ZERO:
        return None
    rows = []
    for o in o3:
        ok = [_axis(n, v, c_border)[1] for n, v in zip(dims, o)]
        rows.append(~torch.from_numpy(ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]))
    return torch.stack(rows)[None].expand(B, -1, -1, -1, -1).contiguous().to(dev_)


def state(pkg, op, dev_, d, n=1):  # noqa: F811
    return A.new_state(R.Plain(dev_), pkg, op, d, n=n)


# ---- the rigs: run(...) -> dict of freshly allocated outputs; masks(q, operand) -> (want, unspec) ------------------------------------------
class LossRig(object):
    """pea_affinity_fwd_ex + pea_affinity_bwd_ex2 of one case of tests/test_gpu_alignment.py"""

    def __init__(self, pkg, op, dev_, c, I, name, flags=0, backward=True):  # noqa: F811
        self.L, self.op, self.pkg, self.dev, self.c, self.I, self.name = pkg._lib.lib(), op, pkg, dev_, c, I, name
        self.flags, self.backward = flags, backward
        self.d = A.make_desc(pkg, c, I["o3"], I["lam"], flags | (A.FLAG_ACCUMULATE if c["accumulate"] else 0))
        self.st, self.sb = state(pkg, op, dev_, self.d)
        self.tdt = A.DTYPES[c["dtype"]][0]
        self.operands = ["e"] + (["other"] if c["other"] else [])
        self.other_mode = c["other"]
        self.base = None
        if c["accumulate"]:
            gen = torch.Generator().manual_seed(5)
            self.base = ((torch.rand(I["E"].shape, generator=gen) - 0.5) * 1e-3).to(dev_)

    def tensors(self):
        return dict(E=self.I["E"], O=self.I["O"], W=self.I["W"], M=self.I["M"])

    def run(self, E=None, O=None, W=None, M=None):
        I, c = self.I, self.c
        E, O = I["E"] if E is None else E, I["O"] if O is None else O
        W, M = I["W"] if W is None else W, I["M"] if M is None else M
        f = dict(dtype=torch.float32, device=self.dev)
        out = dict(affs=torch.zeros(I["T"].shape, **f), g=torch.zeros(I["T"].shape, **f), lv=torch.zeros(1 + I["K"], **f),
                   inv=torch.zeros((2 if O is not None else 1, c["B"]) + tuple(c["dims"]), **f))
        rc = A.launched(self.L.pea_affinity_fwd_ex(ctypes.byref(self.d), P(E), P(O), P(I["T"]), P(W), P(M), P(out["affs"]), P(out["g"]),
                                                   P(out["inv"]), P(out["lv"]), P(self.st), self.sb, self.op._stream()))
        assert rc == 0, "%s: forward rc %d" % (self.name, rc)
        A.sync()
        A.assert_state_clean(self.st, self.sb, self.name)
        if self.backward:
            out["de"] = torch.zeros(E.shape, dtype=self.tdt, device=self.dev) if self.base is None else self.base.clone()
            if c["other"] == "both":
                out["de_other"] = torch.zeros(E.shape, dtype=self.tdt, device=self.dev)
            dl = torch.tensor([A.DLOSS], **f)
            raw = out["affs"] if c["raw"] and not (self.flags & A_ACT_MASK) else None
            rc = A.launched(self.L.pea_affinity_bwd_ex2(ctypes.byref(self.d), P(E), P(O), P(out["g"]), P(out["inv"]), P(raw), P(dl), P(out["de"]),
                                                        P(out.get("de_other")), self.op._stream()))
            assert rc == 0, "%s: backward rc %d" % (self.name, rc)
            A.sync()
        return out

    def masks(self, q, operand):
        c, I = self.c, self.I
        B, D = c["B"], c["D"]
        F = footprint(q, operand, c["border"], c["dims"], I["o3"], c["other"])
        want = dict(affs=full_k(F["affs"], B, self.dev), g=full_k(F["g"], B, self.dev), lv=loss_mask(F), de=full_d(F["de"], B, D, self.dev))
        if F["de_other"] is not None:
            want["de_other"] = full_d(F["de_other"], B, D, self.dev)
        plane = (1 if operand == "other" else 0, 0) + tuple(q)
        unspec = dict(inv=at((2 if c["other"] else 1, B) + tuple(c["dims"]), plane, self.dev))
        gone = cropped(c["border"], c["dims"], I["o3"], B, self.dev)
        return F, want, unspec, dict(affs=gone, g=gone, act0=act_of_zero(self.flags))

    def states_clean(self, what):
        A.assert_state_clean(self.st, self.sb, "%s %s" % (self.name, what))


A_ACT_MASK = RELU | ONE_MINUS | HALF | CLAMP


class InferRig(object):
    """pea_affinity_infer"""
    operands, other_mode = ["e"], None

    def __init__(self, pkg, op, dev_, c, I, name, flags=RELU):  # noqa: F811
        self.L, self.op, self.dev, self.c, self.I, self.name = pkg._lib.lib(), op, dev_, c, I, name
        self.flags = flags
        self.d = A.make_desc(pkg, dict(c, mask=None), I["o3"], I["lam"], flags)

    def tensors(self):
        return dict(E=self.I["E"], O=None, W=None, M=None)

    def run(self, E=None, O=None, W=None, M=None):
        E = self.I["E"] if E is None else E
        out = dict(affs=torch.zeros(self.I["T"].shape, dtype=torch.float32, device=self.dev))
        rc = A.launched(self.L.pea_affinity_infer(ctypes.byref(self.d), P(E), None, P(out["affs"]), self.op._stream()))
        assert rc == 0, "%s: rc %d" % (self.name, rc)
        A.sync()
        return out

    def masks(self, q, operand):
        c = self.c
        F = footprint(q, "e", c["border"], c["dims"], self.I["o3"], None)
        return F, dict(affs=full_k(F["affs"], c["B"], self.dev)), {}, dict(affs=cropped(c["border"], c["dims"], self.I["o3"], c["B"], self.dev),
                                                                           act0=act_of_zero(self.flags))

    def states_clean(self, what):
        pass


class PairRig(object):
    """pea_affinity_fwd_dual_ex + pea_affinity_bwd_dual_ex: the self loss (affs, g, lv) and the cross loss with the detached ema (gx, lvx)"""
    operands, other_mode = ["e", "other"], "detached"

    def __init__(self, pkg, op, dev_, synth, name):  # noqa: F811
        self.L, self.op, self.dev, self.name = pkg._lib.lib(), op, dev_, name
        self.c, self.I = A.PAIR, A.pair_inputs(synth, dev_)
        I = self.I
        self.d, self.dc = A.make_desc(pkg, self.c, I["o3"], I["lam"]), A.make_desc(pkg, self.c, I["o3"], I["lam_cross"])
        assert self.L.pea_cross_supported(ctypes.byref(self.d), 5) == 1
        self.st, self.sb = state(pkg, op, dev_, self.d, 2)

    def tensors(self):
        return dict(E=self.I["E"], O=self.I["O"], W=self.I["W"], M=self.I["M"])

    def run(self, E=None, O=None, W=None, M=None):
        I, c = self.I, self.c
        E, O = I["E"] if E is None else E, I["O"] if O is None else O
        W, M = I["W"] if W is None else W, I["M"] if M is None else M
        f = dict(dtype=torch.float32, device=self.dev)
        plane = (c["B"],) + tuple(c["dims"])
        out = dict(affs=torch.zeros(I["T"].shape, **f), g=torch.zeros(I["T"].shape, **f), gx=torch.zeros(I["T"].shape, **f),
                   inv=torch.zeros(plane, **f), invo=torch.zeros(plane, **f), lv=torch.zeros(1 + I["K"], **f), lvx=torch.zeros(1 + I["K"], **f),
                   de=torch.zeros(E.shape, **f))
        rc = A.launched(self.L.pea_affinity_fwd_dual_ex(
            ctypes.byref(self.d), ctypes.byref(self.dc), P(E), P(O), P(I["T"]), P(W), P(M), P(out["affs"]), P(out["g"]), P(out["gx"]),
            P(out["inv"]), P(out["invo"]), P(out["lv"]), P(out["lvx"]), P(self.st), ctypes.c_void_p(self.st.data_ptr() + self.sb), self.sb,
            self.op._stream()))
        assert rc == 0, "pair forward rc %d" % rc
        A.sync()
        A.assert_state_clean(self.st, self.sb, self.name)
        dl = torch.tensor([A.DLOSS], **f)
        rc = A.launched(self.L.pea_affinity_bwd_dual_ex(ctypes.byref(self.d), P(E), P(O), P(out["g"]), P(out["gx"]), P(out["inv"]), P(out["invo"]),
                                                        P(dl), P(dl), P(out["de"]), self.op._stream()))
        assert rc == 0, "pair backward rc %d" % rc
        A.sync()
        return out

    def masks(self, q, operand):
        """each loss on its own: a poisoned ema leaves the self loss' outputs alone"""
        c, I = self.c, self.I
        B, D = c["B"], c["D"]
        Fx = footprint(q, operand, c["border"], c["dims"], I["o3"], "detached")
        want = dict(gx=full_k(Fx["g"], B, self.dev), lvx=loss_mask(Fx))
        de = Fx["de"]
        unspec = {}
        if operand == "e":
            Fs = footprint(q, "e", c["border"], c["dims"], I["o3"], None)
            want.update(affs=full_k(Fs["affs"], B, self.dev), g=full_k(Fs["g"], B, self.dev), lv=loss_mask(Fs))
            de = de | Fs["de"]
            unspec["inv"] = at((B,) + tuple(c["dims"]), (0,) + tuple(q), self.dev)
        else:
            unspec["invo"] = at((B,) + tuple(c["dims"]), (0,) + tuple(q), self.dev)
        want["de"] = full_d(de, B, D, self.dev)
        return Fx, want, unspec, {}

    def states_clean(self, what):
        A.assert_state_clean(self.st, self.sb, "%s %s" % (self.name, what))


class LabRig(object):
    """pea_affinity_fwd_bwd_labels_ex, with the scratch (two launches) and without (one)"""
    operands, other_mode = ["e"], None

    def __init__(self, pkg, op, dev_, synth, name):  # noqa: F811
        self.L, self.op, self.dev, self.name = pkg._lib.lib(), op, dev_, name
        self.c, self.I = A.LAB, A.lab_inputs(pkg, op, synth, dev_)
        self.d = A.make_desc(pkg, dict(self.c, mask=None), self.I["o3"], self.I["lam"])
        self.st, self.sb = state(pkg, op, dev_, self.d)
        self.scratch, self.nsc = None, 0
        if name.endswith("scratch"):
            self.nsc = int(self.L.pea_labels_scratch_bytes(ctypes.byref(self.d)))
            assert self.nsc > 0 and self.nsc % 16 == 0, "lab16 is not in the two-launch set"
            self.scratch = torch.empty(self.nsc // 4, dtype=torch.float32, device=dev_)

    def tensors(self):
        return dict(E=self.I["E"], O=None, W=None, M=None)

    def run(self, E=None, O=None, W=None, M=None):
        I = self.I
        E = I["E"] if E is None else E
        f = dict(dtype=torch.float32, device=self.dev)
        out = dict(affs=torch.zeros(I["T"].shape, **f), lv=torch.zeros(1 + I["K"], **f), de=torch.zeros(E.shape, **f))
        dl = torch.tensor([A.DLOSS], **f)
        rc = A.launched(self.L.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(self.d), P(E), None, P(I["labels"]), P(I["wtab"]), R.TGT, P(out["affs"]),
                                                              P(out["lv"]), P(dl), P(out["de"]), P(self.st), self.sb, P(self.scratch), self.nsc,
                                                              self.op._stream()))
        assert rc == 0, "labels step rc %d" % rc
        A.sync()
        return out

    def masks(self, q, operand):
        c = self.c
        F = footprint(q, "e", c["border"], c["dims"], self.I["o3"], None)
        return F, dict(affs=full_k(F["affs"], c["B"], self.dev), lv=loss_mask(F), de=full_d(F["de"], c["B"], c["D"], self.dev)), {}, {}

    def states_clean(self, what):
        A.assert_state_clean(self.st, self.sb, "%s %s" % (self.name, what))


class MultiRig(object):
    """pea_affinity_fwd_multi + pea_affinity_bwd_multi on the whole table; entry j carries the poisoned pixel, the others must not notice"""
    operands, other_mode = ["e"], None

    def __init__(self, pkg, op, dev_, synth, name):  # noqa: F811
        self.L, self.op, self.pkg, self.dev, self.name = pkg._lib.lib(), op, pkg, dev_, name
        self.j = int(name.rsplit("_", 1)[1])
        self.ents = A.multi_inputs(synth, dev_)
        self.I = self.ents[self.j]
        self.c = self.I["c"]
        self.descs = [A.make_desc(pkg, I["c"], I["o3"], I["lam"]) for I in self.ents]
        n = len(self.ents)
        arr = (ctypes.POINTER(pkg._lib.PeaDesc) * n)(*[ctypes.pointer(x) for x in self.descs])
        assert self.L.pea_multi_supported(arr, n) == 1
        self.st, self.sb = state(pkg, op, dev_, self.descs[0], n)

    def tensors(self):
        return dict(E=self.I["E"], O=None, W=self.I["W"], M=self.I["M"])

    def run(self, E=None, O=None, W=None, M=None):
        n = len(self.ents)
        f = dict(dtype=torch.float32, device=self.dev)
        ft, bt = (self.pkg._lib.PeaMultiFwd * n)(), (self.pkg._lib.PeaMultiBwd * n)()
        out, keep = {}, []
        for i, I in enumerate(self.ents):
            mine = i == self.j
            Ei, Wi, Mi = (E if mine and E is not None else I["E"]), (W if mine and W is not None else I["W"]), (M if mine and M is not None else I["M"])
            if I["want_affs"]:
                out["affs@%d" % i] = torch.zeros(I["T"].shape, **f)
            out["g@%d" % i], out["lv@%d" % i], out["de@%d" % i] = torch.zeros(I["T"].shape, **f), torch.zeros(1 + I["K"], **f), torch.zeros(I["E"].shape, **f)
            dl = None if I["dloss"] is None else torch.tensor([I["dloss"]], **f)
            keep += [Ei, Wi, Mi, dl]
            a, b = ft[i], bt[i]
            a.desc, a.e, a.target, a.weight = ctypes.pointer(self.descs[i]), Ei.data_ptr(), I["T"].data_ptr(), Wi.data_ptr()
            a.mask = None if Mi is None else Mi.data_ptr()
            a.affs = out["affs@%d" % i].data_ptr() if I["want_affs"] else None
            a.g_out, a.loss_out = out["g@%d" % i].data_ptr(), out["lv@%d" % i].data_ptr()
            b.desc, b.e, b.g, b.de = ctypes.pointer(self.descs[i]), Ei.data_ptr(), out["g@%d" % i].data_ptr(), out["de@%d" % i].data_ptr()
            b.dloss = None if dl is None else dl.data_ptr()
        rc = A.launched(self.L.pea_affinity_fwd_multi(ft, n, P(self.st), n * self.sb, self.op._stream()))
        assert rc == 0, "multi forward rc %d" % rc
        A.sync()
        A.assert_state_clean(self.st, self.sb, self.name)
        rc = A.launched(self.L.pea_affinity_bwd_multi(bt, n, self.op._stream()))
        assert rc == 0, "multi backward rc %d" % rc
        A.sync()
        return out

    def masks(self, q, operand):
        c, j = self.c, self.j
        F = footprint(q, "e", c["border"], c["dims"], self.I["o3"], None)
        want = {"g@%d" % j: full_k(F["g"], c["B"], self.dev), "lv@%d" % j: loss_mask(F), "de@%d" % j: full_d(F["de"], c["B"], c["D"], self.dev)}
        if self.I["want_affs"]:
            want["affs@%d" % j] = full_k(F["affs"], c["B"], self.dev)
        return F, want, {}, {}

    def states_clean(self, what):
        A.assert_state_clean(self.st, self.sb, "%s %s" % (self.name, what))


# second-operand families beyond the alignment suite's 2D circular ones: the 3D detached ema on zm5's volume (CROP_ZERO, z steps: the
# role-A LDS-DMA backward with z gathers), the 2D cropped ema, a REPLICATE stencil with a second operand that has a gradient
EXTRA = {
    "zm5_ema": A.case(other="detached", modes=(2,), seed=31, **A.V3),
    "ema16_crop": A.case(other="detached", border=1, norm=1, seed=32),
    "rep6_both": A.case(B=1, dims=(4, 40, 72), offs="rep6", border=2, norm=2, mask=None, other="both", seed=33),
}
_EXTRA_INPUTS = {}


def make_rig(pkg, op, dev_, synth, name):  # noqa: F811
    if name == "pair16":
        return PairRig(pkg, op, dev_, synth, name)
    if name.startswith("lab16"):
        return LabRig(pkg, op, dev_, synth, name)
    if name.startswith("multi4"):
        return MultiRig(pkg, op, dev_, synth, name)
    if name in A.INFER:
        c = A.INFER[name]
        I = A.make_inputs(synth, dev_, c)
        return InferRig(pkg, op, dev_, c, I, name)
    if name in EXTRA:
        c = EXTRA[name]
        if name not in _EXTRA_INPUTS:
            _EXTRA_INPUTS[name] = A.make_inputs(synth, dev_, c)
        rig = LossRig(pkg, op, dev_, c, _EXTRA_INPUTS[name], name)
        for mode in c["modes"]:
            assert rig.L.pea_cross_supported(ctypes.byref(rig.d), mode) == 1, "%s is not in the fast set of mode %d" % (name, mode)
        return rig
    cname = name[:-len("_direct")] if name.endswith("_direct") else name
    c = A.CASES[cname]
    rig = LossRig(pkg, op, dev_, c, A.loss_inputs(synth, dev_, cname), name)
    if cname == name:  # (the precondition of the alignment test's aligned variant: the case reaches its family)
        for mode in c["modes"]:
            assert rig.L.pea_cross_supported(ctypes.byref(rig.d), mode) == 1, "%s is not in the fast set of mode %d" % (name, mode)
    return rig


def poison_run(rig, clean, q, operand, value, fails, tag, zero_w_m=False, relaxed=None):
    """one poisoned call against the clean one; zero_w_m: w = 0 on every footprint pair of one offset, m = 0 on those of another"""
    T = rig.tensors()
    key = "O" if operand == "other" else "E"
    bad = poisoned(T[key], q, value)
    F, want, unspec, zero = rig.masks(q, operand)
    kw = {key: bad}
    if zero_w_m:
        ks = [int(k) for k in torch.nonzero(F["loss"]).flatten()]
        assert len(ks) >= 2, tag
        k1, k2 = ks[len(ks) // 2], ks[0]
        W = T["W"].clone()
        W[0, k1][F["affs"][k1].to(W.device)] = 0.0
        kw["W"] = W
        if T["M"] is not None:
            M = T["M"].clone()
            M[0, k2][F["affs"][k2].to(M.device)] = 0
            kw["M"] = M
    if zero_w_m:  # the clean call on the same weights and mask (the pair's self loss reads them too)
        clean = rig.run(**{k: v for k, v in kw.items() if k in ("W", "M")})
    ins = dict(T, **kw)  # every input of the call: both operands, weight, mask, target (the labels and their table)
    ins.update({k: rig.I[k] for k in ("T", "labels", "wtab") if k in rig.I})
    before = {k: v.clone() for k, v in ins.items() if v is not None}
    got = rig.run(**kw)
    if relaxed is not None:
        relaxed(F, want, unspec, zero, q)
    compare(tag, clean, got, want, unspec, fails, zero)
    for k, v in before.items():
        if not torch.equal(ins[k].contiguous().view(torch.uint8), v.view(torch.uint8)):
            fails.append("%s: the call changed its input %s" % (tag, k))
    rig.states_clean(tag)
    return got


# ---- A: the loss path ------------------------------------------------------------------------------------------------------------
# (c16_crop once more on the direct kernels: the one forward that reads no staged zeros for a cropped pair but skips it)
SUBJECTS_A = R.SUBJECTS + ["c16_crop_direct"] + list(EXTRA) + list(A.INFER)
ENV = dict(R.ENV, c16_crop_direct=("PEA_FORCE_DIRECT", "1"))


@pytest.mark.parametrize("name", SUBJECTS_A)
def test_a_one_bad_pixel_poisons_its_footprint_and_nothing_else(pkg, op, dev, synth, monkeypatch, name):  # noqa: F811
    if name in ENV:
        monkeypatch.setenv(*ENV[name])
    rig = make_rig(pkg, op, dev, synth, name)
    clean = rig.run()
    for k, t in clean.items():
        assert not bool(torch.isnan(t.float()).any()), "%s: the clean call has NaN in %s" % (name, k)
    fails = []
    qi, qc = interior(rig.c["dims"]), (0, 0, 0)
    for operand in rig.operands:
        for value, vname, places in ((NAN, "nan", (qi, qc)), (INF, "+inf", (qi, qc)), (-INF, "-inf", (qi,))):
            for q in places:
                poison_run(rig, clean, q, operand, value, fails, "%s %s in %s at %s" % (name, vname, operand, q))
        if rig.tensors()["W"] is not None:
            poison_run(rig, clean, qi, operand, NAN, fails, "%s nan in %s at %s, w = 0 / m = 0 on the footprint" % (name, operand, qi), zero_w_m=True)
    again = rig.run()
    for k in clean:
        if not torch.equal(bits(again[k]), bits(clean[k])):
            fails.append("%s: the clean call after the poisoned ones differs in %s" % (name, k))
    rig.states_clean("at the end")
    assert not fails, "\n".join(fails)


def test_a_rep6_footprint_holds_every_clamped_pair():
    """the precondition of the rep6 runs above: at the corner the footprint of a REPLICATE stencil holds every pixel that the clamp
    folds onto q, more pairs than the cropped stencil has"""
    c = A.CASES["rep6"]
    o3 = A.offsets3(c)
    rep = footprint((0, 0, 0), "e", 2, c["dims"], o3, None)["affs"]
    crop = footprint((0, 0, 0), "e", 1, c["dims"], o3, None)["affs"]
    assert bool((rep | crop).eq(rep).all()) and int(rep.sum()) > int(crop.sum())
    assert int(rep[o3.index([0, 9, 0])].sum()) == 1   # nothing is folded onto row 0 by a step of +9: only q's own pair
    assert int(rep[o3.index([0, -3, 0])].sum()) == 4  # rows 0 .. 3 of q's column read row 0 (q's own pair is one of them)


# ---- B: activations ----------------------------------------------------------------------------------------------------------------
FWD_ACT = ["c16", "c32", "h32_f16", "diag16", "diag64", "c16_direct", "zm5", "n26", "infer16", "infer32_f16"]


@pytest.mark.parametrize("name", FWD_ACT)
def test_b_every_activation_bit_keeps_nan(pkg, op, dev, synth, monkeypatch, name):  # noqa: F811
    if name in R.ENV:
        monkeypatch.setenv(*R.ENV[name])
    fails = []
    for aname, act in ACTS.items():
        if name in A.INFER:
            c = A.INFER[name]
            if name not in A._CACHE:
                A._CACHE[name] = A.make_inputs(synth, dev, c)
            rig = InferRig(pkg, op, dev, c, A._CACHE[name], name, flags=act)
        else:
            cname = "c16" if name == "c16_direct" else name
            rig = LossRig(pkg, op, dev, A.CASES[cname], A.loss_inputs(synth, dev, cname), name, flags=act, backward=False)
        clean = rig.run()
        for q in (interior(rig.c["dims"]), (0, 0, 0)):
            poison_run(rig, clean, q, "e", NAN, fails, "%s %s nan at %s" % (name, aname, q))
        poison_run(rig, clean, interior(rig.c["dims"]), "e", INF, fails, "%s %s +inf" % (name, aname))
    assert not fails, "\n".join(fails)


# the families of tests/test_gpu_act_loss.py's CASES at the alignment suite's shape (B = 2, 48 x 96): (D, storage, stencil, switch)
LACT_CASES = {
    "xdma_d16": (16, "f32", "cross", None), "xdma_d32": (32, "f32", "cross", None), "xdma_h_d32_f16": (32, "f16", "cross", None),
    "xdma_h_d32_bf16": (32, "bf16", "cross", None), "xdma_h_d64_f16": (64, "f16", "cross8", None), "xdma_h_d64_bf16": (64, "bf16", "cross8", None),
    "tiled_d16": (16, "f32", "diag", None), "chunked_d64": (64, "f32", "diag", None), "direct_d16": (16, "f32", "cross", ("PEA_FORCE_DIRECT", "1")),
    "xdma_d64": (64, "f32", "cross8", None), "tiled_d32": (32, "f32", "diag", None), "tiled_d16_bf16": (16, "bf16", "diag", None),
}
_LACT = {}


@pytest.mark.parametrize("other", [None, "detached"], ids=["self", "ema"])
@pytest.mark.parametrize("case", sorted(LACT_CASES))
def test_b_loss_on_the_activated_map_keeps_nan(pkg, op, dev, synth, monkeypatch, case, other):  # noqa: F811
    D, dtype, offs, env = LACT_CASES[case]
    if env:
        monkeypatch.setenv(*env)
    c = A.case(D=D, dtype=dtype, offs=offs, other=other, seed=60 + sorted(LACT_CASES).index(case))
    if (case, other) not in _LACT:
        _LACT[(case, other)] = A.make_inputs(synth, dev, c)
    I = _LACT[(case, other)]
    fails = []
    qi = interior(c["dims"])
    for aname, act in LACTS.items():
        rig = LossRig(pkg, op, dev, c, I, "%s %s" % (case, aname), flags=act | LOSS_ACT)
        # the name still says which family runs at this shape: the LDS-DMA kernels take the xdma cases and decline the others
        lds_dma = case.startswith("xdma")
        modes = (0, 1) if not other else ((4,) if case in ("xdma_d32", "xdma_d64") else (2,))
        # (the second-operand queries are made without the activation bits: they answer for forward AND backward, and the
        # projection-first role-A backward of D > 16 / 16-bit storage steps aside for any activation -- the forward, where the loss
        # is taken, does not)
        dq = A.make_desc(pkg, c, I["o3"], I["lam"]) if other else rig.d
        if not env:
            for mode in modes:
                assert rig.L.pea_cross_supported(ctypes.byref(dq), mode) == int(lds_dma), "%s: pea_cross_supported(mode %d)" % (case, mode)
        clean = rig.run()

        def relaxed(F, want, unspec, zero, q, act=act):
            """with the clamp: g is exactly 0 on the footprint pairs, de is asserted at q only (NaN) and outside the footprint"""
            if not act & CLAMP:
                return
            pairs = want.pop("g")
            zero["g"], unspec["g"] = pairs, pairs
            de = want["de"]
            own = at(de.shape, (0, slice(None)) + tuple(q), de.device)
            want["de"] = de & own
            unspec["de"] = de & ~own

        for operand in rig.operands:
            for value, vname in ((NAN, "nan"), (INF, "+inf")):
                tag = "%s %s %s %s in %s" % (case, "ema" if other else "self", aname, vname, operand)
                poison_run(rig, clean, qi, operand, value, fails, tag, relaxed=relaxed)
            poison_run(rig, clean, (0, 0, 0), operand, NAN, fails, "%s %s %s nan at the corner in %s" % (case, "ema" if other else "self", aname, operand),
                       relaxed=relaxed)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("win,pos,vol", [((5, 20, 24), (1, 3, 4), (7, 26, 32)), ((5, 20, 22), (1, 3, 5), (7, 26, 31))], ids=["quads", "elementwise"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_b_stitched_window_with_a_nan_voxel(pkg, op, dev, synth, win, pos, vol, dtype):  # noqa: F811
    """pea_affinity_infer_stitch (fill 1, relu): the volume is NaN exactly at the window's footprint voxels, the border-fill copies of
    channels 0 .. 2 among them (q lies on the source slices z = 1 and x = 1), also where the blend weight is 0; the rest of the volume
    and the weight map keep the clean call's bits"""
    L = pkg._lib.lib()
    o3 = [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [-2, 0, 0], [0, -3, 0], [0, 0, -3], [0, -9, 0], [0, 0, -9], [1, 2, -2]]
    K, D = len(o3), 16
    c = A.case(D=D, B=1, dims=win, border=1, norm=1, dtype=dtype, mask=None)
    d = A.make_desc(pkg, c, o3, [1.0] * K, RELU)
    assert L.pea_infer_stitch_supported(ctypes.byref(d), 1) == 1
    gen = torch.Generator().manual_seed(81)
    E = torch.from_numpy(synth.synth_embedding((1, D) + win, 82)).float().to(A.DTYPES[dtype][0]).to(dev)
    wv = torch.rand(win, generator=gen)
    wv[1, 4:7, 0:3] = 0.0
    wv = wv.to(dev)
    out0, wm0 = torch.rand((K,) + vol, generator=gen).to(dev), (torch.rand(vol, generator=gen) + 0.5).to(dev)

    def run(e):
        out, wm = out0.clone(), wm0.clone()
        rc = A.launched(L.pea_affinity_infer_stitch(ctypes.byref(d), P(e), 1, P(wv), P(out), P(wm), vol[0], vol[1], vol[2], pos[0], pos[1], pos[2],
                                                    op._stream()))
        assert rc == 0
        A.sync()
        return dict(out=out, wmap=wm)

    clean = run(E)
    assert not bool(torch.isnan(clean["out"]).any())
    fails = []
    for q in ((1, 5, 1), (0, 0, 0), (2, 11, 13)):
        m = footprint(q, "e", 1, win, o3, None)["affs"].clone()
        m[1, :, :1, :] = m[1, :, 1:2, :]
        m[2, :, :, :1] = m[2, :, :, 1:2]
        m[0, :1, :, :] = m[0, 1:2, :, :]
        want = torch.zeros((K,) + vol, dtype=torch.bool)
        want[:, pos[0]:pos[0] + win[0], pos[1]:pos[1] + win[1], pos[2]:pos[2] + win[2]] = m
        got = run(poisoned(E, q, NAN))
        compare("stitch %s q=%s" % (dtype, q), clean, got, dict(out=want.to(dev)), {}, fails)
    assert not fails, "\n".join(fails)


FILL_FORMS = [((2, 12, 6, 20, 24), 1, True), ((2, 12, 6, 20, 24), 2, True), ((1, 3, 5, 9, 16), 1, True), ((2, 12, 6, 20, 24), 1, False),
              ((1, 12, 7, 12, 20), 3, False), ((2, 3, 4, 10, 22), 1, True), ((1, 2, 4, 6, 8), 1, False), ((1, 1, 4, 6, 8), 2, True),
              ((1, 1, 4, 3, 3), 2, True), ((1, 1, 4, 3, 3), 2, False),  # K = 1: only Z has to hold 2 * shift
              ((2, 10, 1, 40, 48), 0, True), ((1, 3, 1, 9, 11), 0, True)]  # relu_: quads, and a ragged tail


def _torch_fill_relu(pred, shift, relu):
    """scripts_ac3ac4/main.py:233-237 as tests/test_gpu_parity.py restates it"""
    ref = pred.clone()
    K = pred.shape[1]
    if shift:
        if K > 1:
            ref[:, 1, :, :shift, :] = ref[:, 1, :, shift:shift * 2, :]
        if K > 2:
            ref[:, 2, :, :, :shift] = ref[:, 2, :, :, shift:shift * 2]
        ref[:, 0, :shift, :, :] = ref[:, 0, shift:shift * 2, :, :]
    return torch.nn.functional.relu(ref) if relu else ref


@pytest.mark.parametrize("shape,shift,relu", FILL_FORMS)
def test_b_fill_border_relu_keeps_nan_like_torch(pkg, dev, shape, shift, relu):  # noqa: F811
    """NaN, +-inf and -0.0 in the source slices, the border slices and the interior: the isnan mask of the torch statements, their
    values wherever the result is not NaN"""
    gen = torch.Generator().manual_seed(sum(shape) + shift)
    pred = torch.randn(shape, generator=gen)
    pick = torch.randint(0, 16, shape, generator=gen)
    for k, v in enumerate((NAN, INF, -INF, -0.0)):
        pred[pick == k] = v
    s = max(shift, 1)
    for b, v in [(0, NAN)] + ([(shape[0] - 1, -INF)] if shape[0] > 1 else []):  # whole border and source rows of one kind, in every filled channel
        pred[b, 0, 0, 1 % shape[3], :] = v
        pred[b, 0, min(s, shape[2] - 1), 0, :] = v
        pred[b, min(1, shape[1] - 1), :, min(s, shape[3] - 1), 0] = v
        pred[b, min(2, shape[1] - 1), 0, :, min(s, shape[4] - 1)] = v
    pred = pred.to(dev)
    ref = _torch_fill_relu(pred, shift, relu)
    got = pkg.fill_border_relu_(pred, shift=shift, relu=relu) if shift else pkg.relu_(pred)
    nan = torch.isnan(ref)
    assert bool(nan.any()) and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], ref[~nan])


# ---- C: the heads --------------------------------------------------------------------------------------------------------------------
HEAD_CD = [(32, 16), (36, 16), (256, 16), (64, 32)]
HEAD_S = [(17, 19), (24, 40)]  # S = 323 (odd: the one-element form) and S = 960 (the packed form)
HEAD_T = [("f32", "f32"), ("f16", "f16"), ("f16", "f32"), ("bf16", "bf16"), ("bf16", "f32")]
TORCH_T = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f32": 0, "f16": 1, "bf16": 2}


class Head(object):
    def __init__(self, pkg, dev_, C, D, sp, xt, et):
        self.L, self.dev, self.xt, self.et = pkg._lib.lib(), dev_, xt, et
        self.B, self.C, self.D, self.S = 2, C, D, sp[0] * sp[1]
        gen = torch.Generator().manual_seed(7 * C + D)
        self.x = torch.randn((self.B, C, self.S), generator=gen).to(TORCH_T[xt]).to(dev_)
        W = torch.randn((D, C), generator=gen) * 0.2
        self.cs, self.d0, self.d1 = C // 2 + 1, 3, 5  # the poisoned column c*, the row whose W[d0, c*] is 0, a row with a large weight
        W[self.d0, self.cs] = 0.0
        W[self.d1, self.cs] = -4.0
        self.W, self.bias = W.to(dev_), torch.randn(D, generator=gen).to(dev_)
        self.de = torch.randn((self.B, D, self.S), generator=gen).to(TORCH_T[et]).to(dev_)
        self.wsb = int(self.L.pea_head_workspace_bytes(C, D))
        self.ws = torch.zeros(max(self.wsb // 4, 1), dtype=torch.float32, device=dev_)
        if xt != "f32":
            assert self.L.pea_head_supported_t(C, D, CODE[xt], CODE[et]) == 1
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(self, x):
        e = torch.zeros((self.B, self.D, self.S), dtype=TORCH_T[self.et], device=self.dev)
        if self.xt == "f32":
            rc = self.L.pea_head_fwd(self.B, self.C, self.D, self.S, P(x), P(self.W), P(self.bias), P(e), self.st)
        else:
            rc = self.L.pea_head_fwd_t(self.B, self.C, self.D, self.S, P(x), CODE[self.xt], P(self.W), P(self.bias), P(e), CODE[self.et], self.st)
        assert A.launched(rc) == 0
        A.sync()
        return dict(e=e)

    def bwd(self, x, de):
        dx = torch.zeros(x.shape, dtype=x.dtype, device=self.dev)
        dW, db = torch.zeros_like(self.W), torch.zeros_like(self.bias)
        if self.xt == "f32":
            rc = self.L.pea_head_bwd(self.B, self.C, self.D, self.S, P(x), P(self.W), P(de), P(dx), P(dW), P(db), P(self.ws), self.wsb, self.st)
        else:
            rc = self.L.pea_head_bwd_t(self.B, self.C, self.D, self.S, P(x), CODE[self.xt], P(self.W), P(de), CODE[self.et], P(dx), P(dW), P(db),
                                       P(self.ws), self.wsb, self.st)
        assert A.launched(rc) == 0
        A.sync()
        return dict(dx=dx, dW=dW, db=db)


@pytest.mark.parametrize("xt,et", HEAD_T, ids=["%s_e%s" % t for t in HEAD_T])
@pytest.mark.parametrize("sp", HEAD_S, ids=["S323", "S960"])
@pytest.mark.parametrize("C,D", HEAD_CD)
def test_c_heads(pkg, dev, C, D, sp, xt, et):  # noqa: F811
    H = Head(pkg, dev, C, D, sp, xt, et)
    S = H.S
    ps = 200 if S % 2 else 201  # p*: even in the one-element form, odd in the packed one
    fails = []
    e0, b0 = H.fwd(H.x), H.bwd(H.x, H.de)
    for k, t in list(e0.items()) + list(b0.items()):
        assert bool(torch.isfinite(t.float()).all()), k
    col = at(e0["e"].shape, (0, slice(None), ps), dev)

    def xp(v):
        x = H.x.clone()
        x[0, H.cs, ps] = v
        return x

    # forward: NaN in x
    compare("head fwd nan", e0, H.fwd(xp(NAN)), dict(e=col), {}, fails)
    # forward: +inf in x -> sign(W[d, c*]) inf, NaN where W[d0, c*] == 0
    got = H.fwd(xp(INF))["e"]
    want = torch.sign(H.W[:, H.cs]) * INF
    want[H.d0] = NAN
    column = got[0, :, ps].float()
    if not (torch.equal(torch.isnan(column), torch.isnan(want)) and torch.equal(column[~torch.isnan(want)], want[~torch.isnan(want)])):
        fails.append("head fwd +inf: e[0, :, p*] = %s, wanted %s" % (column.tolist(), want.tolist()))
    if int(((bits(got) != bits(e0["e"])) & ~col).sum()):
        fails.append("head fwd +inf: an element outside the column changed")
    # forward: a finite x whose f32 sum leaves the f16 range (x = 60000, W[d1, c*] = -4: about -240000)
    if xt == "f16":
        got = H.fwd(xp(60000.0))["e"]
        v = float(got[0, H.d1, ps])
        if et == "f16" and v != -INF:
            fails.append("head fwd overflow: the f16 e is %r, wanted -inf" % v)
        if et == "f32" and not (np.isfinite(v) and v < -65504.0):
            fails.append("head fwd overflow: the f32 e is %r, wanted a finite value below -65504" % v)
        if bool(torch.isnan(got.float()).any()) or int(((bits(got) != bits(e0["e"])) & ~col).sum()):
            fails.append("head fwd overflow: NaN, or an element outside the column changed")
    # backward: NaN in x -> dW[:, c*]
    compare("head bwd, nan in x", b0, H.bwd(xp(NAN), H.de), dict(dW=at(H.W.shape, (slice(None), H.cs), dev)), {}, fails)
    # backward: NaN in de at (0, d*, p*) -> dx[0, :, p*] (the column whose W is 0 as well), dW[d*, :], db[d*]
    de = H.de.clone()
    de[0, H.d0, ps] = NAN
    compare("head bwd, nan in de", b0, H.bwd(H.x, de), dict(dx=at(H.x.shape, (0, slice(None), ps), dev), dW=at(H.W.shape, (H.d0, slice(None)), dev),
                                                            db=at(H.bias.shape, (H.d0,), dev)), {}, fails)
    compare("head: a clean backward afterwards", b0, H.bwd(H.x, H.de), {}, {}, fails)
    assert not fails, "\n".join(fails)
