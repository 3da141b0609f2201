"""GPU (-m gpu): the numeric contract of the loss reduction (csrc/pea_loss.h) in every forward family, through the C ABI.

Every training forward ends in loss_accumulate / loss_value / k_loss_finish: the workgroup's f32 partial becomes a 128-bit fixed-point
number (LSB 2^-64), three digits are added into 64-bit integer words, one flag word per offset remembers non-finite and too large
partials, and the finish turns the words into loss_out and zeroes them.  The rest of the suite reaches that code with positive O(1)
weights only.  Here every case of tests/test_gpu_alignment.py (its CASES with their switches, c16 again under PEA_FORCE_DIRECT=1, the
one-launch pair, the labels step in both forms, each entry of the multi table) is driven, forward only, through

    A  repeat       the same call three more times on one state, once on a fresh one: loss_out bit for bit, the state zero again
    B  scale up     W = 2^s W0, s in {1, 20, 40} capped so that max_i S_i 2^s < 2^58 (S_i = sum w r^2 of the float64 reference; with
                    positive weights no partial exceeds S_i, so none reaches the 2^60 saturation point): 2^s lv0 within ONE f32 ulp.
                    (Not a measured tolerance: the finish rounds twice, 128 bits -> f64 -> f32; a digit, carry or dropped-word error is
                    many orders larger.)
    C  sign         W = -W0: bit for bit -lv0;  W = sigma W0, sigma = +-1 per (pixel, offset): the float64 reference within
                    LOSS_RTOL * L_i(|W0|) (relative to the sum of absolute terms: the signed sum cancels);  a batch of two copies of
                    one sample with W[1] = -W[0]: every L_i and the total exactly 0
    D  non-finite   NaN, +inf, -inf, +inf with -inf elsewhere, 2^70 at one pixel of offset k*: that offset and the total NaN / inf as
                    include/pea.h says, every other offset bit for bit; then a clean call bit for bit and the state zero (a flag on the
                    wrong offset, or one that the finish does not clear, fails here).  k* is a middle offset, never offset 0.  One more
                    weight, chosen from the reference, puts the term of p* just below 2^60 (summed) and just above (+inf)
    E  scale down   s in {-20, -40, -60}:  2^s ref_i (1 - LOSS_RTOL) - npix 2^-64 / N_i <= L_i <= 2^s ref_i (1 + LOSS_RTOL)  (bits below
                    2^-64 are dropped toward zero, at most once per partial, and there are at most npix partials);  s = -90, where every
                    S_i 2^s < 2^-64: exactly +0.0
    F  all NaN      every workgroup sets a flag and none adds a digit: every L_i NaN, then a clean call bit for bit

"bit for bit" compares int32 views.  lv0 is loss_out for the case's own positive weights W0 on a fresh state and is itself held to the
float64 reference (tests/f64_reference.py) with the suite's LOSS_RTOL.  The reference's per-pixel r^2 is computed once per case and
every reweighted L_i is sum W r^2 / N_i in float64 from it; it reproduces cosine_loss's parts for W0 (asserted).  Nothing restates the
fixed-point code on the host.

Exactly 0 in C holds for every family: each forward kernel derives ONE sample b per workgroup from its tile id (b = tile / chunks in
pea_direct.h and pea_k_multi.hip; b = plane / Z or lin / per_b in xdma_tile / march_tile of pea_xdma.h, which the cross, pair, 16-bit,
box and z-march kernels share; b = plane / Z in pea_tiled.h, pea_chunked.h and pea_fused_labels.h), the tile geometry does not depend on
b, and f32 arithmetic is odd in w -- so the partials of sample 1 are the exact negatives of sample 0's.  No family needs the relaxed
bound.

The pair shares ONE weight tensor between its two losses, so a weight poisons both; each state is then checked on its own.  That a
flag stays in its own state block is shown with a NaN in the EMA operand instead, which only the cross loss reads
(test_pair_nan_in_ema_stays_in_the_cross_state).  The labels step has no weight tensor: wtab[B, K, 2] is scaled and poisoned.  An
infinite table entry multiplies EVERY pixel of its (sample, offset, class), so the class must hold no pixel with r = 0 (inf * 0 is
NaN in any arithmetic): the "different label" class of an offset whose every such pair has |a| > 1e-4 is taken (asserted from the
reference; the suite's affs bound is 1e-5, so the kernel's a is not 0 either).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_alignment as A
from arena import PATTERN
from f64_reference import normaliser, shifted
from test_gpu_alignment import dev, op, synth  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LOSS_RTOL = A.LOSS_RTOL
UP, DOWN, GONE = (1, 20, 40), (-20, -40, -60), -90
NAN, INF = float("nan"), float("inf")
TGT = A.TGT_PADDING | A.TGT_MASK_INSIDE
kBlock = 256  # pixels of one workgroup of the multi kernels (csrc/pea_k_multi.hip: p = chunk * kBlock + threadIdx.x)

SUBJECTS = list(A.CASES) + ["c16_direct", "pair16", "lab16_scratch", "lab16_one_launch"] + ["multi4_%d" % j for j in range(len(A.MULTI))]
ENV = {"c16_direct": ("PEA_FORCE_DIRECT", "1")}
ENV.update({n: c["env"] for n, c in A.CASES.items() if c["env"]})


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
class Plain(object):
    """what new_state() needs of a Run: plain tensors (no guard bands are needed for a forward whose outputs nobody reads)"""

    def __init__(self, dev):
        self.dev = dev

    def out(self, name, shape, dtype=torch.float32, skew=0):
        return torch.empty(tuple(shape), dtype=dtype, device=self.dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def two_of(t):
    """a batch of two copies of sample 0"""
    return None if t is None else torch.cat([t[0:1], t[0:1]]).contiguous()


class View(object):
    """what the float64 reference says about ONE loss of a call: r^2 per (pixel, offset), the normalisers, lambda"""

    def __init__(self, c, T, M, o3, lam, ref_affs):
        B, dims, self.K = T.shape[0], tuple(T.shape[2:]), len(o3)
        probe = torch.zeros((1, 1) + dims, dtype=torch.float64, device=T.device)
        ok = torch.stack([shifted(probe, o, c["border"])[1] for o in o3])[None]  # [1,K,Z,Y,X]: the pair exists
        a, t = ref_affs.view(T.shape).double(), T.double()
        m = torch.ones_like(t) if M is None else M.double()
        r = (a * m - t * m) * ok
        self.r2 = r * r
        self.cand = ok & (m != 0) & ((a - t).abs() > 0.1)  # D: pixels whose term is surely not 0
        self.a, self.t, self.m = a, t, m
        self.N = torch.tensor([float(normaliser(c["norm"], B, dims, o)) for o in o3], dtype=torch.float64)
        self.lam = torch.tensor([float(v) for v in lam], dtype=torch.float64)
        self.npix = B * dims[0] * dims[1] * dims[2]

    def parts(self, W):
        """[K] float64: L_i for the full-size weights W"""
        return (W.double() * self.r2).sum(dim=(0, 2, 3, 4)).cpu() / self.N

    def total(self, parts):
        return float((self.lam * parts).sum())


class Subject(object):
    """One case: rig (the tensors, the descriptor(s), the call), the views of the losses under test, W0, lv0.

    rig.call(w, st, sb) -> one [1 + K] f32 CPU tensor per state block; self.targets: the states whose loss reads w."""

    def finish_init(self, pkg, op, dev):
        self.pkg, self.op, self.dev = pkg, op, dev
        self.reset()
        self.lv0 = self.call(self.W0)
        Wfull = self.expand(self.W0)
        assert bool((Wfull > 0).all()), "the cases' own weights are positive"
        for s in self.targets:
            v, lv = self.views[s], self.lv0[s].double()
            parts = v.parts(Wfull)
            if self.refs[s] is not None:  # the r^2 form IS cosine_loss's sum
                assert bool(((parts - self.refs[s]["parts"].cpu()).abs() <= 1e-12 * parts.abs()).all()), self.name
            assert bool(((lv[1:] - parts).abs() <= LOSS_RTOL * parts).all()), "%s: lv0 per-offset %s ref %s" % (self.name, lv[1:], parts)
            assert abs(float(lv[0]) - v.total(parts)) <= LOSS_RTOL * v.total(parts), self.name
        self.clean("after lv0")

    def reset(self):
        self.st, self.sb = A.new_state(Plain(self.dev), self.pkg, self.op, self.rig.d, n=self.rig.nstates)

    def call(self, w, fresh=False, rig=None):
        rig = rig or self.rig
        st, sb = A.new_state(Plain(self.dev), self.pkg, self.op, rig.d, n=rig.nstates) if fresh else (self.st, self.sb)
        out = rig.call(w.contiguous(), st, sb)
        if fresh:
            A.assert_state_clean(st, sb, self.name + " (fresh state)")
        return out

    def clean(self, what):
        A.assert_state_clean(self.st, self.sb, "%s %s" % (self.name, what))

    def expand(self, w):
        return w

    def is_lv0(self, out, what, but=None):
        """every state's loss_out is lv0 bit for bit; but = (state, k*): that offset and that state's total are someone else's to judge"""
        for s, (lv, l0) in enumerate(zip(out, self.lv0)):
            keep = torch.ones(lv.numel(), dtype=torch.bool)
            if but is not None and s in but[0]:
                keep[0] = keep[1 + but[1]] = False
            assert torch.equal(bits(lv)[keep], bits(l0)[keep]), "%s %s: state %d is not lv0 bit for bit: %s vs %s" % (
                self.name, what, s, lv.tolist(), l0.tolist())

    def bystanders_are_lv0(self, out, what):
        """the states whose loss does not read w (the other entries of a multi table)"""
        self.is_lv0([l if s in self.targets else o for s, (o, l) in enumerate(zip(out, self.lv0))], what + " (the other states)")

    # the sums of the reference for the cap of B and the s of E: max over the losses under test of S_i = parts_i N_i
    def max_sum(self):
        Wfull = self.expand(self.W0)
        return max(float((self.views[s].parts(Wfull) * self.views[s].N).max()) for s in self.targets)

    def pick(self):
        """k*, index of p* and of q* into w (D).  The candidates satisfy the conditions in every loss under test."""
        cand, lo, hi = None, None, None
        for s in self.targets:
            v = self.views[s]
            cand = v.cand if cand is None else cand & v.cand
            lo, hi = (v.r2, v.r2) if lo is None else (torch.minimum(lo, v.r2), torch.maximum(hi, v.r2))
        cand = cand & (hi < 1.9 * lo)  # (the pair: one weight must put both losses' terms on the same side of 2^60)
        B, Z = cand.shape[0], cand.shape[2]
        lam = self.views[self.targets[0]].lam
        K = cand.shape[1]
        for k in list(range(K // 2, K)) + list(range(K // 2)):  # (not offset 0 first: a flag that lands on flags[0] must show)
            if float(lam[k]) <= 0:
                continue
            P0 = torch.nonzero(cand[0, k]).cpu()
            if not len(P0):
                continue
            p = P0[len(P0) // 2]
            if B >= 2:  # q* in the other sample: another workgroup whatever the family
                Q = torch.nonzero(cand[1, k]).cpu()
            else:
                Q = P0[self.far(P0, p, Z, cand.shape[3], cand.shape[4])]
            if not len(Q):
                continue
            q = Q[len(Q) // 2]
            ip, iq = (0, k) + tuple(int(v) for v in p), (min(1, B - 1), k) + tuple(int(v) for v in q)
            for s in self.targets:
                v = self.views[s]
                for i in (ip, iq):  # the stated conditions, from the reference
                    assert float(v.m[i]) != 0 and abs(float(v.a[i]) - float(v.t[i])) > 0.1 and float(v.r2[i]) > 0, (self.name, i)
            assert ip != iq
            return k, ip, iq
        raise AssertionError("%s: no offset with two usable pixels" % self.name)

    def far(self, P0, p, Z, Y, X):
        """B = 1: q* two planes away in 3D, 32 rows away in 2D"""
        if Z > 1:
            return (P0[:, 0] - p[0]).abs() >= 2
        return (P0[:, 1] - p[1]).abs() >= 32

    def signs(self, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randint(0, 2, tuple(self.W0.shape), generator=g).float() * 2 - 1).to(self.dev)


# ---- the rigs --------------------------------------------------------------------------------------------------------------------
def P(t):
    return A.P(t)


class SelfRig(object):
    nstates = 1

    def __init__(self, pkg, op, dev, c, E, O, T, M, o3, lam):
        self.L, self.op = pkg._lib.lib(), op
        self.d = A.make_desc(pkg, c, o3, lam, A.FLAG_ACCUMULATE if c["accumulate"] else 0, B=E.shape[0])
        self.t = (E, O, T, M)
        f = dict(dtype=torch.float32, device=dev)
        self.affs, self.g = torch.empty(T.shape, **f), torch.empty(T.shape, **f)
        self.inv = torch.empty((2 if O is not None else 1, E.shape[0]) + tuple(E.shape[2:]), **f)
        self.lv = torch.empty(1 + len(o3), **f)

    def call(self, w, st, sb):
        E, O, T, M = self.t
        bits(self.lv).fill_(PATTERN)
        rc = A.launched(self.L.pea_affinity_fwd_ex(ctypes.byref(self.d), P(E), P(O), P(T), P(w), P(M), P(self.affs), P(self.g), P(self.inv),
                                                   P(self.lv), P(st), sb, self.op._stream()))
        assert rc == 0, "forward rc %d" % rc
        A.sync()
        return [written(self.lv)]


def written(lv):
    out = lv.cpu()
    assert not bool((bits(out) == PATTERN).any()), "loss_out was not written"
    return out


class PairRig(object):
    nstates = 2

    def __init__(self, pkg, op, dev, c, E, O, T, M, o3, lam, lam_cross):
        self.L, self.op = pkg._lib.lib(), op
        self.d, self.dc = A.make_desc(pkg, c, o3, lam, B=E.shape[0]), A.make_desc(pkg, c, o3, lam_cross, B=E.shape[0])
        self.t = (E, O, T, M)
        f = dict(dtype=torch.float32, device=dev)
        self.affs, self.g, self.gx = (torch.empty(T.shape, **f) for _ in range(3))
        plane = (E.shape[0],) + tuple(E.shape[2:])
        self.inv, self.invo = torch.empty(plane, **f), torch.empty(plane, **f)
        self.lv, self.lvx = torch.empty(1 + len(o3), **f), torch.empty(1 + len(o3), **f)

    def call(self, w, st, sb, ema=None):
        E, O, T, M = self.t
        bits(self.lv).fill_(PATTERN)
        bits(self.lvx).fill_(PATTERN)
        rc = A.launched(self.L.pea_affinity_fwd_dual_ex(
            ctypes.byref(self.d), ctypes.byref(self.dc), P(E), P(O if ema is None else ema), P(T), P(w), P(M), P(self.affs), P(self.g),
            P(self.gx), P(self.inv), P(self.invo), P(self.lv), P(self.lvx), P(st), ctypes.c_void_p(st.data_ptr() + sb), sb, self.op._stream()))
        assert rc == 0, "pair forward rc %d" % rc
        A.sync()
        return [written(self.lv), written(self.lvx)]


class LabRig(object):
    nstates = 1

    def __init__(self, pkg, op, dev, c, E, labels, o3, lam, form):
        self.L, self.op = pkg._lib.lib(), op
        self.d = A.make_desc(pkg, dict(c, mask=None), o3, lam, B=E.shape[0])
        self.t = (E, labels)
        f = dict(dtype=torch.float32, device=dev)
        self.affs = torch.empty((E.shape[0], len(o3)) + tuple(E.shape[2:]), **f)
        self.de, self.lv = torch.empty(E.shape, **f), torch.empty(1 + len(o3), **f)
        self.dl = torch.tensor([A.DLOSS], **f)
        self.scratch, self.nsc = None, 0
        if form == "scratch":
            self.nsc = int(self.L.pea_labels_scratch_bytes(ctypes.byref(self.d)))
            assert self.nsc > 0 and self.nsc % 16 == 0, "lab16 is not in the two-launch set"
            self.scratch = torch.empty(self.nsc // 4, **f)

    def call(self, wtab, st, sb):
        E, labels = self.t
        bits(self.lv).fill_(PATTERN)
        rc = A.launched(self.L.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(self.d), P(E), None, P(labels), P(wtab), TGT, P(self.affs), P(self.lv),
                                                              P(self.dl), P(self.de), P(st), sb, P(self.scratch), self.nsc, self.op._stream()))
        assert rc == 0, "labels step rc %d" % rc
        A.sync()
        return [written(self.lv)]


class MultiRig(object):
    """the whole table; w replaces the weights of entry j"""

    def __init__(self, pkg, op, dev, ents, j):
        self.L, self.op, self.pkg, self.j, self.nstates = pkg._lib.lib(), op, pkg, j, len(ents)
        self.ents, self.descs, self.bufs = ents, [], []
        f = dict(dtype=torch.float32, device=dev)
        for I in ents:
            self.descs.append(A.make_desc(pkg, I["c"], I["o3"], I["lam"], B=I["E"].shape[0]))
            self.bufs.append(dict(g=torch.empty(I["T"].shape, **f), lv=torch.empty(1 + I["K"], **f)))
        self.d = self.descs[0]
        arr = (ctypes.POINTER(pkg._lib.PeaDesc) * self.nstates)(*[ctypes.pointer(x) for x in self.descs])
        assert self.L.pea_multi_supported(arr, self.nstates) == 1

    def call(self, w, st, sb):
        n = self.nstates
        ft = (self.pkg._lib.PeaMultiFwd * n)()
        for i, (I, b) in enumerate(zip(self.ents, self.bufs)):
            a, wi = ft[i], (w if i == self.j else I["W"])
            assert wi.shape == I["T"].shape
            a.desc, a.e, a.target, a.weight = ctypes.pointer(self.descs[i]), I["E"].data_ptr(), I["T"].data_ptr(), wi.data_ptr()
            a.mask = None if I["M"] is None else I["M"].data_ptr()
            a.affs, a.g_out, a.loss_out = None, b["g"].data_ptr(), b["lv"].data_ptr()
            bits(b["lv"]).fill_(PATTERN)
        rc = A.launched(self.L.pea_affinity_fwd_multi(ft, n, P(st), n * sb, self.op._stream()))
        assert rc == 0, "multi forward rc %d" % rc
        A.sync()
        return [written(b["lv"]) for b in self.bufs]


# ---- the subjects ----------------------------------------------------------------------------------------------------------------
class SelfSubject(Subject):
    def __init__(self, pkg, op, dev, synth, name):
        self.name = name
        cname = "c16" if name == "c16_direct" else name
        c, I = A.CASES[cname], A.loss_inputs(synth, dev, cname)
        self.c, self.I = c, I
        self.rig = SelfRig(pkg, op, dev, c, I["E"], I["O"], I["T"], I["M"], I["o3"], I["lam"])
        if name != "c16_direct":  # (the precondition of the alignment test's aligned variant)
            for mode in c["modes"]:
                assert self.rig.L.pea_cross_supported(ctypes.byref(self.rig.d), mode) == 1, "%s is not in the fast set of mode %d" % (name, mode)
        self.W0, self.targets = I["W"], [0]
        self.views, self.refs = [View(c, I["T"], I["M"], I["o3"], I["lam"], I["ref"]["affs"])], [I["ref"]]
        self.finish_init(pkg, op, dev)

    def antisym(self):
        I = self.I
        rig = SelfRig(self.pkg, self.op, self.dev, self.c, two_of(I["E"]), two_of(I["O"]), two_of(I["T"]), two_of(I["M"]), I["o3"], I["lam"])
        return self.call(torch.cat([self.W0[0:1], -self.W0[0:1]]), fresh=True, rig=rig)


class PairSubject(Subject):
    def __init__(self, pkg, op, dev, synth, name):
        self.name = name
        c, I = A.PAIR, A.pair_inputs(synth, dev)
        self.c, self.I = c, I
        self.rig = PairRig(pkg, op, dev, c, I["E"], I["O"], I["T"], I["M"], I["o3"], I["lam"], I["lam_cross"])
        assert self.rig.L.pea_cross_supported(ctypes.byref(self.rig.d), 5) == 1
        self.W0, self.targets = I["W"], [0, 1]  # one weight tensor, two losses
        self.views = [View(c, I["T"], I["M"], I["o3"], I["lam"], I["ref"]["affs"]),
                      View(c, I["T"], I["M"], I["o3"], I["lam_cross"], I["ref_cross"]["affs"])]
        self.refs = [I["ref"], I["ref_cross"]]
        self.finish_init(pkg, op, dev)

    def antisym(self):
        I = self.I
        rig = PairRig(self.pkg, self.op, self.dev, self.c, two_of(I["E"]), two_of(I["O"]), two_of(I["T"]), two_of(I["M"]), I["o3"], I["lam"],
                      I["lam_cross"])
        return self.call(torch.cat([self.W0[0:1], -self.W0[0:1]]), fresh=True, rig=rig)


class LabSubject(Subject):
    """w is wtab[B, K, 2]: {same label or padding, different label} -- index (b, k, class)"""

    def __init__(self, pkg, op, dev, synth, name):
        self.name, self.form = name, name[len("lab16_"):]
        c, I = A.LAB, A.lab_inputs(pkg, op, synth, dev)
        self.c, self.I = c, I
        self.rig = LabRig(pkg, op, dev, c, I["E"], I["labels"], I["o3"], I["lam"], self.form)
        self.W0, self.targets = I["wtab"], [0]
        self.views, self.refs = [View(c, I["T"], I["M"], I["o3"], I["lam"], I["ref"]["affs"])], [I["ref"]]
        self.finish_init(pkg, op, dev)
        assert same_bits(self.expand(I["wtab"]), I["W"])

    def expand(self, w):
        T, (B, K) = self.I["T"], self.I["T"].shape[:2]
        return torch.where(T == 1, w[:, :, 0].view(B, K, 1, 1, 1), w[:, :, 1].view(B, K, 1, 1, 1)).expand_as(T).contiguous()

    def pick(self):
        v, T = self.views[0], self.I["T"]
        for k in list(range(v.K // 2, v.K)) + list(range(v.K // 2)):
            good = float(v.lam[k]) > 0
            for b in (0, 1):
                cls = T[b, k] == 0  # the "different label" class: inside pairs only, m = 1
                good = good and bool(cls.any()) and bool((v.m[b, k][cls] == 1).all()) and float(v.a[b, k][cls].abs().min()) > 1e-4 \
                    and bool(v.cand[b, k][cls].any())
            if good:
                return k, (0, k, 1), (1, k, 1)
        raise AssertionError("lab16: no offset whose different-label class is free of r = 0 in both samples")

    def antisym(self):
        I = self.I
        rig = LabRig(self.pkg, self.op, self.dev, self.c, two_of(I["E"]), two_of(I["labels"]), I["o3"], I["lam"], self.form)
        return self.call(torch.cat([self.W0[0:1], -self.W0[0:1]]), fresh=True, rig=rig)


class MultiSubject(Subject):
    def __init__(self, pkg, op, dev, synth, name):
        self.name, self.j = name, int(name.rsplit("_", 1)[1])
        self.ents = A.multi_inputs(synth, dev)
        I = self.ents[self.j]
        self.rig = MultiRig(pkg, op, dev, self.ents, self.j)
        self.W0, self.targets = I["W"], [self.j]
        self.views, self.refs = [None] * len(self.ents), [None] * len(self.ents)
        self.views[self.j], self.refs[self.j] = View(I["c"], I["T"], I["M"], I["o3"], I["lam"], I["ref"]["affs"]), I["ref"]
        self.finish_init(pkg, op, dev)

    def far(self, P0, p, Z, Y, X):
        """B = 1 (19 x 33: no two rows are 32 apart): another 256-pixel chunk of the flat plane is another workgroup"""
        return (P0[:, 1] * X + P0[:, 2]) // kBlock != (p[1] * X + p[2]) // kBlock

    def antisym(self):
        I = dict(self.ents[self.j])
        for key in ("E", "T", "M", "W"):
            I[key] = two_of(I[key])
        ents = list(self.ents)
        ents[self.j] = I
        rig = MultiRig(self.pkg, self.op, self.dev, ents, self.j)
        return self.call(torch.cat([self.W0[0:1], -self.W0[0:1]]), fresh=True, rig=rig)


_SUBJECTS = {}


@pytest.fixture
def S(request, pkg, op, dev, synth, monkeypatch):  # noqa: F811
    name = request.param
    if name in ENV:
        monkeypatch.setenv(*ENV[name])
    if name not in _SUBJECTS:
        cls = PairSubject if name == "pair16" else LabSubject if name.startswith("lab16") else MultiSubject if name.startswith("multi4") \
            else SelfSubject
        _SUBJECTS[name] = cls(pkg, op, dev, synth, name)
    s = _SUBJECTS[name]
    s.reset()  # one state per test: the calls of a test share it, a failed test does not reach into the next
    return s


every_subject = pytest.mark.parametrize("S", SUBJECTS, indirect=True)


def ulp32(x):
    """one unit in the last place of the f32 value x, as float64"""
    return float(np.spacing(np.abs(np.float32(x))))


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@every_subject
def test_a_repeat_is_bit_identical(S):
    for i in range(3):
        S.is_lv0(S.call(S.W0), "repeat %d" % i)
        S.clean("repeat %d" % i)
    S.is_lv0(S.call(S.W0, fresh=True), "on a second state")


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@every_subject
def test_b_scaling_up_by_powers_of_two(S):
    top = S.max_sum()
    cap = int(np.floor(58 - np.log2(top)))
    while top * 2.0 ** cap >= 2.0 ** 58:
        cap -= 1
    assert cap >= 1, "%s: max S_i = %g leaves no room below 2^58" % (S.name, top)
    for s in sorted(set(min(s, cap) for s in UP)):
        assert top * 2.0 ** s < 2.0 ** 58
        out = S.call(S.W0 * 2.0 ** s)
        for st in S.targets:
            lv, l0 = out[st].double(), S.lv0[st].double()
            for i in range(lv.numel()):
                want = float(l0[i]) * 2.0 ** s
                assert abs(float(lv[i]) - want) <= ulp32(float(l0[i])) * 2.0 ** s, "%s s=%d state %d entry %d: %.9g, 2^s lv0 = %.9g" % (
                    S.name, s, st, i, float(lv[i]), want)
        S.bystanders_are_lv0(out, "s=%d" % s)
        S.clean("s=%d" % s)
    S.is_lv0(S.call(S.W0), "after scaling up")


# ---- C ---------------------------------------------------------------------------------------------------------------------------
@every_subject
def test_c_negated_weights_negate_the_bits(S):
    out = S.call(-S.W0)
    for st in S.targets:
        assert same_bits(out[st], -S.lv0[st]), "%s state %d: %s vs -%s" % (S.name, st, out[st].tolist(), S.lv0[st].tolist())
    S.clean("-W0")
    S.is_lv0(S.call(S.W0), "after -W0")


@every_subject
def test_c_random_signs_against_the_reference(S):
    sg = S.signs(77)
    assert bool((sg == 1).any()) and bool((sg == -1).any())
    out = S.call(S.W0 * sg)
    Wabs, Wsg = S.expand(S.W0), S.expand(S.W0 * sg)
    for st in S.targets:
        v, lv = S.views[st], out[st].double()
        ref, mag = v.parts(Wsg), v.parts(Wabs)
        assert bool(((lv[1:] - ref).abs() <= LOSS_RTOL * mag).all()), "%s state %d: %s ref %s (|.| %s)" % (S.name, st, lv[1:], ref, mag)
        assert abs(float(lv[0]) - v.total(ref)) <= LOSS_RTOL * v.total(mag), "%s state %d total" % (S.name, st)
    S.clean("signs")


@every_subject
def test_c_opposite_samples_cancel_exactly(S):
    out = S.antisym()
    for st in S.targets:
        assert bool((out[st] == 0).all()), "%s state %d: %s" % (S.name, st, out[st].tolist())


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def poisoned(S, edits):
    w = S.W0.clone()
    for idx, val in edits:
        w[idx] = val
    return w


def expect(x, want):
    x = float(x)
    return np.isnan(x) if np.isnan(want) else x == want


@every_subject
def test_d_non_finite_and_saturating_weights(S):
    k, ip, iq = S.pick()
    assert k > 0, "k* = 0 would not notice a flag that lands on offset 0"
    lines = [("NaN", [(ip, NAN)], NAN), ("+inf", [(ip, INF)], INF), ("-inf", [(ip, -INF)], -INF), ("+inf and -inf", [(ip, INF), (iq, -INF)], NAN),
             ("2^70", [(ip, 2.0 ** 70)], INF)]
    for what, edits, want in lines:
        out = S.call(poisoned(S, edits))
        for st in S.targets:
            assert expect(out[st][1 + k], want) and expect(out[st][0], want), "%s %s state %d: L_k* %r total %r, wanted %r" % (
                S.name, what, st, float(out[st][1 + k]), float(out[st][0]), want)
        S.is_lv0(out, what + " (the other offsets)", but=(S.targets, k))
        S.is_lv0(S.call(S.W0), "the clean call after " + what)
        S.clean("after " + what)


WEIGHTED = [n for n in SUBJECTS if not n.startswith("lab16")]
# |a - a_ref| <= AFFS_ATOL (the suite's bound) and |a - t| > 0.1 at p*: r^2 = ((a - t) m)^2 is within 2 * 1e-5 / 0.1 + (1e-5 / 0.1)^2 of the reference's
EDGE_RTOL = 2.1e-4


@pytest.mark.parametrize("S", WEIGHTED, indirect=True)
def test_d_saturation_starts_at_two_to_the_60(S):
    """Both sides of the saturation point, with ONE weight chosen from the reference's r^2(p*): a term in [2^58, 0.95 * 2^60) is summed
    (finite, the reference's value), eight times the weight puts it in [2^61, 2^63) and the offset reads +inf -- where a float sum
    would stay finite.  (W[p*] = 2^70 of the table above lands beyond 2^63 for every |a - t| > 0.1: it cannot tell a threshold of 2^60
    from one of 2^64.)  The labels forms are left out: a table entry scales a whole class, so no single partial can be placed."""
    k, ip, _ = S.pick()
    r2 = [float(S.views[s].r2[ip]) for s in S.targets]
    w_hi = 2.0 ** int(np.ceil(61 - np.log2(min(r2))))
    w_lo = w_hi / 8
    rest = S.max_sum()  # what else the workgroup of p* can hold
    assert w_lo * min(r2) >= 2.0 ** 58 and w_lo * max(r2) * (1 + EDGE_RTOL) + rest < 2.0 ** 60, (S.name, r2)
    assert w_hi * min(r2) * (1 - EDGE_RTOL) >= 2.0 ** 60 and w_hi * max(r2) * (1 + EDGE_RTOL) + rest < 2.0 ** 63, (S.name, r2)
    w = poisoned(S, [(ip, w_lo)])
    out = S.call(w)
    for st in S.targets:
        v, lv = S.views[st], out[st].double()
        ref, ref0 = v.parts(S.expand(w)), v.parts(S.expand(S.W0))
        tol = EDGE_RTOL * w_lo * float(v.r2[ip]) / float(v.N[k]) + LOSS_RTOL * float(ref0[k])
        assert abs(float(lv[1 + k]) - float(ref[k])) <= tol, "%s state %d below 2^60: L_k* %.9g ref %.9g" % (S.name, st, float(lv[1 + k]), float(ref[k]))
        assert abs(float(lv[0]) - v.total(ref)) <= float(v.lam[k]) * tol + LOSS_RTOL * v.total(ref0), "%s state %d below 2^60: total" % (S.name, st)
    S.is_lv0(out, "below 2^60 (the other offsets)", but=(S.targets, k))
    S.clean("below 2^60")
    out = S.call(poisoned(S, [(ip, w_hi)]))
    for st in S.targets:
        assert expect(out[st][1 + k], INF) and expect(out[st][0], INF), "%s state %d above 2^60: L_k* %r total %r" % (
            S.name, st, float(out[st][1 + k]), float(out[st][0]))
    S.is_lv0(out, "above 2^60 (the other offsets)", but=(S.targets, k))
    S.is_lv0(S.call(S.W0), "the clean call after saturation")
    S.clean("after saturation")


# ---- E ---------------------------------------------------------------------------------------------------------------------------
@every_subject
def test_e_scaling_down_truncates_toward_zero(S):
    top = S.max_sum()
    Wfull = S.expand(S.W0)
    for s in DOWN:
        out = S.call(S.W0 * 2.0 ** s)
        for st in S.targets:
            v, lv = S.views[st], out[st].double()
            ref = v.parts(Wfull) * 2.0 ** s
            lo, hi = ref * (1 - LOSS_RTOL) - v.npix * 2.0 ** -64 / v.N, ref * (1 + LOSS_RTOL)
            assert bool((lv[1:] >= lo).all()) and bool((lv[1:] <= hi).all()), "%s s=%d state %d: %s not in [%s, %s]" % (S.name, s, st, lv[1:], lo, hi)
            assert v.total(lo) <= float(lv[0]) <= v.total(hi), "%s s=%d state %d total" % (S.name, s, st)
        S.clean("s=%d" % s)
    assert top * 2.0 ** GONE < 2.0 ** -64, "%s: max S_i = %g does not vanish at s = %d" % (S.name, top, GONE)
    out = S.call(S.W0 * 2.0 ** GONE)
    for st in S.targets:
        assert not bool(bits(out[st]).any()), "%s s=%d state %d: %s is not +0.0 everywhere" % (S.name, GONE, st, out[st].tolist())
    S.clean("s=%d" % GONE)
    S.is_lv0(S.call(S.W0), "after scaling down")


# ---- F ---------------------------------------------------------------------------------------------------------------------------
@every_subject
def test_f_all_nan_weights(S):
    out = S.call(torch.full_like(S.W0, NAN))
    for st in S.targets:
        assert bool(torch.isnan(out[st]).all()), "%s state %d: %s" % (S.name, st, out[st].tolist())
    S.bystanders_are_lv0(out, "all-NaN")
    S.is_lv0(S.call(S.W0), "the clean call after all-NaN")
    S.clean("after all-NaN")


# ---- the pair's two states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ["pair16"], indirect=True)
def test_pair_nan_in_ema_stays_in_the_cross_state(S):
    """The pair's losses share their weights, so no weight poisons one of them alone.  The EMA operand is read by the cross loss only:
    a NaN vector at p* + o_k* (CIRCULAR: every offset reaches it from some pixel) makes every cross L_i NaN and leaves the self loss'
    bits alone; afterwards both states are zero and a clean call returns lv0."""
    k, ip, _ = S.pick()
    o, dims = S.I["o3"][k], S.c["dims"]
    q = tuple((ip[2 + a] + o[a]) % dims[a] for a in range(3))
    ema = S.I["O"].clone()
    ema[(0, slice(None)) + q] = NAN
    out = S.rig.call(S.W0, S.st, S.sb, ema=ema)
    assert same_bits(out[0], S.lv0[0]), "the self loss changed: %s vs %s" % (out[0].tolist(), S.lv0[0].tolist())
    assert bool(torch.isnan(out[1]).all()), "the cross loss: %s" % out[1].tolist()
    S.is_lv0(S.call(S.W0), "the clean call after a NaN in ema")
    S.clean("after a NaN in ema")
