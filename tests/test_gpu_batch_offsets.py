"""GPU (-m gpu): the WHOLE tensor past 4 GiB and past 2^31 elements while every batch item is small.

Here the per-item blocks are small (64 MiB, 32 MiB), so the fast families serve -- pea_cross_supported is asserted -- and what crosses
a power of two is the batch rebase `(size_t)b * ...` in front of every kernel's addressing.  For each case: two runs bit for bit;
item 0 and the LAST item each run alone as B = 1 must give the in-batch affs within 2e-6 and their gradient / B the in-batch gradient
within rel-to-max 1e-5 (f16 2e-3, bf16 8e-3: the stored gradient is rounded) -- the batch-additivity identity of
test_gpu_fullsize.py:118-121: an item addressed 2^32 bytes too low or too high reads another item's pixels --; the CPU oracle on one
window of the last item (affs 1e-5, grads rel-to-max 1e-4; 16-bit as above).  Inputs are generated on the device.

Cases (limits: 2^32 = 4 294 967 296 bytes, 2^31 = 2 147 483 648 elements):

  e65     f32 D=16 1024 x 1024, the first two offsets of the BBBC stencil (K=2), u8 mask, B=65: the EMBEDDING-side crossing
          e, de: 65 * 16 * 2^20 * 4 = 4 362 076 160 bytes > 2^32 (B=64 is exactly 2^32).  self loss, EMA cross loss, labels-in step
  k103    f32 D=16 1024 x 1024, BBBC stencil (K=10), u8 mask, B=103: the K-side crossing
          t, w, g, affs: 103 * 10 * 2^20 * 4 = 4 320 133 120 bytes > 2^32 (B=102: 4 278 190 080 < 2^32); e, de 6.4 GiB each.
          With affs, g, de and a second run alive the case passes 40 GiB through the Python entry points (e 6.4 + its clone 6.4 + de 6.4
          + t, w, affs, g 4 x 4.02 + m 1.0 = 36.3 GiB for ONE run), so it is split as the issue allows: e65 above through the Python
          entry points, and here the self loss and the EMA cross loss through the C ABI with `affs` NOT requested in the two
          bit-compared runs (a third forward writes affs alone), and the labels-in step, which needs no t / w / m
  h129    f16 and bf16 D=64 512 x 512, K=8 (configs[4]'s stencil), B=129: the ELEMENT-index crossing
          e, de: 129 * 64 * 2^18 = 2 164 260 864 elements = 2^31 + 2^24, 4.03 GiB.  self loss, the batch run at dloss = 128: under the
          normaliser B * W = 66 048 the stored f16 gradient would otherwise lie among the f16 subnormals, coarser than the 2e-3 bound
  multi   pea_affinity_fwd_multi / _bwd_multi and pea_affinity_fwd_bwd_labels_multi on a two-entry table: e65 and its half-resolution
          sibling (B=65, 512 x 512), held to the single calls as test_gpu_gather_families.py holds them: affs and de bit for bit against
          the forced-direct single calls (tensor form) and against the tensor-form table on pea_gen_targets' output (labels form)
  head    pea_head_fwd / pea_head_bwd (f32, C=32, D=16) and pea_head_fwd_t / pea_head_bwd_t (f16 in and out: C=64, D=16 at the same S,
          and the largest supported pair C=256, D=32 at S = 2^23 + 4099), B=2, S = 2^25 + 4099: ONE item's x block is 4 295 491 968
          (4 297 065 984) bytes > 2^32.  e and dx against a float64 einsum on the first 4096, the last 4099 and the 8192 pixels around
          byte offset 2^32 of each item's x; dW / db against float64 sums over the whole tensor (f32 e / dx 1e-5, 16-bit e / dx and
          dW / db as test_gpu_head16.py)
  dist    pea_dist_affinity and its vjp, f32 D=16 1024 x 1024, K=8, B=129: affs, g: 129 * 8 * 2^20 * 4 = 4 328 521 728 bytes > 2^32
          (B=128 is exactly 2^32).  Window reference from dist_reference.py on the last item; items 0 and 128 against their B=1 runs

Every case prints its shape, the crossed limit, its peak device memory and its run time.

Measured on an MI355X (case, shape, peak device memory of the case, run time inside the case; in some runs one or two cases,
not the same ones each time, took 5 to 6 s instead):

  batch f32 D=16 K=2 B=65 self                   65x16x1024x1024           19.68 GiB   0.71 s
  batch f32 D=16 K=2 B=65 cross                  65x16x1024x1024           23.99 GiB   0.87 s
  batch f32 D=16 K=2 B=65 labels                 65x16x1024x1024           16.01 GiB   0.97 s
  batch f32 D=16 K=10 B=103 self                 103x10x1024x1024          37.22 GiB   0.68 s
  batch f32 D=16 K=10 B=103 cross                103x10x1024x1024          33.57 GiB   0.31 s
  batch f32 D=16 K=10 B=103 labels-in            103x10x1024x1024          32.19 GiB   1.49 s
  batch float16 D=64 K=8 B=129 self              129x64x512x512            33.51 GiB   1.52 s
  batch bfloat16 D=64 K=8 B=129 self             129x64x512x512            33.51 GiB   1.48 s
  multi f32 D=16 K=2 B=65, 1024^2 + 512^2        65x16x1024x1024           21.36 GiB   0.02 s
  multi labels f32 D=16 K=2 B=65, 1024^2 + 512^2 65x16x1024x1024           19.20 GiB   0.02 s
  dist f32 D=16 K=8 B=129 replicate              129x8x1024x1024           34.27 GiB   2.77 s
  dist f32 D=16 K=8 B=129 zero                   129x8x1024x1024           34.27 GiB   1.40 s
  head f32 C=32 D=16 B=2                         2x32x33558531             38.01 GiB   1.53 s
  head f16 C=64 D=16 B=2                         2x64x33558531             34.01 GiB   0.15 s
  head f16 C=256 D=32 B=2                        2x256x8392707             31.05 GiB   2.44 s
"""
import ctypes

import numpy as np
import pytest
import torch

from dist_reference import dist_reference, dist_vjp_reference
from test_gpu_block_edges import BBBC, GRAD_16BIT, block_labels, case_report, cross_answers, dev_relmax, ema_of, spec_2d
from test_gpu_dist_affinity import DD, DV, EDGE, TOL_AFFS, TOL_DE, c_fwd, c_vjp
from test_gpu_fullsize import AFFS_ATOL, GRAD_RTOL, gpu_inputs, run
from test_gpu_fullsize2 import npy, relmax, window_oracle_2d
from test_gpu_parity import LOSS_RTOL

pytestmark = pytest.mark.gpu
P32, E31 = 1 << 32, 1 << 31
H = W = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def window_of_last_item(orc, offsets, lam, reach, B, e, eo, t, w, m, affs, grad, dloss, gtol=GRAD_RTOL, b=None, tb=None):
    """the oracle on the far window (rows H-96.., columns W-128..) of item b (the last one) against the in-batch result; interior only.
    tb: the item of t / w / m to cut (they may hold the last item alone)"""
    b = B - 1 if b is None else b
    tb = b if tb is None else tb
    Hh, Ww = e.shape[2], e.shape[3]
    hh, ww, y0, x0 = 96, 128, Hh - 96, Ww - 128
    cut = lambda x, i: None if x is None else x[i:i + 1, :, y0:y0 + hh, x0:x0 + ww]
    oa, og = window_oracle_2d(orc, offsets, lam, float(B * Ww), 0, 0, 0, hh, ww, cut(e, b), cut(eo, b), cut(t, tb), cut(w, tb), cut(m, tb), dloss)
    inner = (slice(None), slice(reach, hh - reach), slice(reach, ww - reach))
    if affs is not None:
        ea = float(np.abs(npy(cut(affs, b))[0][inner] - oa[inner]).max())
        assert ea < AFFS_ATOL, "window of item %d: affs differ from the oracle by %.3g" % (b, ea)
    eg = relmax(npy(cut(grad, b))[0][inner], og[inner])
    print("window of item %d vs oracle: de rel-to-max %.3g" % (b, eg))
    assert eg < gtol, "window of item %d: de differs from the oracle by rel-to-max %.3g" % (b, eg)


def items_alone(B, affs, grad, alone, gtol, scale=1.0):
    """alone(b) -> (affs, grad) of item b run as B = 1: the in-batch affs within 2e-6, grad / B within rel-to-max gtol.
    scale: the in-batch run's dloss over the single run's"""
    for b in (0, B - 1):
        a1, g1 = alone(b)
        if affs is not None:
            da = (a1[0] - affs[b]).abs().max().item()
            assert da < 2e-6, "item %d alone: affs differ by %.3g" % (b, da)
        dg = dev_relmax(g1[0].float() * (scale / B), grad[b])
        print("item %d alone vs in batch: de rel-to-max %.3g" % (b, dg))
        assert dg < gtol, "item %d alone: de / B differs by rel-to-max %.3g" % (b, dg)


# ----------------------------------------------------------------------------------------------------------------------------
# e65: the embedding side, f32, through the Python entry points
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["self", "cross", "labels"])
def test_embedding_side_past_4gib_b65(pkg, dev, orc, loss):
    """e and de of 4.06 GiB.  Peak 16.0 to 24.0 GiB over its cases (measured)"""
    B, D = 65, 16
    offsets = pkg.multi_offset(BBBC, 4)[:2]
    K = len(offsets)
    lam = [2.0, 2.0] if loss == "cross" else [1.0] * K
    spec = spec_2d(pkg, offsets, lam)
    nbytes = B * D * H * W * 4
    assert nbytes > P32 and (B - 1) * D * H * W * 4 <= P32
    crit = pkg.WeightedMSE()
    with case_report("batch f32 D=16 K=2 B=65 %s" % loss, (B, D, H, W), "e bytes = %d vs 2^32", nbytes):
        e, t, w, m = gpu_inputs(dev, B, D, [H, W], K, 5100)
        eo = ema_of(dev, e, 5200) if loss == "cross" else None
        assert cross_answers(pkg, spec, e, (0, 1, 2)) == [1, 1, 1]
        if loss == "labels":
            lab = torch.cat([block_labels(dev, H, W, 5300 + (b % 5)) for b in range(B)])  # (items 0 and 64 differ)
            del t, w, m

            def step(ee, ll):
                et = ee.detach().requires_grad_(True)
                ls, affs, _ = pkg.embedding_loss_from_labels(et, ll, crit, offsets)
                (ls * 0.5).backward()
                return ls.detach().clone(), affs, et.grad

            full = lambda: step(e, lab)
            alone = lambda b: step(e[b:b + 1], lab[b:b + 1])[1:]
            t, m, w = pkg.gen_targets(lab[B - 1:B], offsets, padding=True)  # the last item's targets, for the oracle's window
            tb = 0
        else:
            full = lambda: [run(pkg, spec, e, t, w, m, 0.5, eo)[i] for i in (0, 1, 3)]
            alone = lambda b: [run(pkg, spec, e[b:b + 1], t[b:b + 1], w[b:b + 1], m[b:b + 1], 0.5, None if eo is None else eo[b:b + 1])[i] for i in (1, 3)]
            tb = None
        l1, a1, g1 = full()
        l2, a2, g2 = full()
        assert torch.equal(l1, l2) and torch.equal(a1, a2) and torch.equal(g1, g2)
        del l2, a2, g2
        assert torch.isfinite(g1).all()
        items_alone(B, a1, g1, alone, 1e-5)
        window_of_last_item(orc, offsets, lam, 1, B, e, eo, t, w, m, a1, g1, 0.5, tb=tb)
        del e, eo, t, w, m, l1, a1, g1


# ----------------------------------------------------------------------------------------------------------------------------
# k103: the K side, f32, through the C ABI (affs not requested in the bit-compared runs)
# ----------------------------------------------------------------------------------------------------------------------------
def equal_in_chunks(a, b, chunk=8):
    """torch.equal over the batch a few items at a time (its temporary is a byte per element)"""
    return all(torch.equal(a[i:i + chunk], b[i:i + chunk]) for i in range(0, a.shape[0], chunk))


def bit_digest(x):
    """per batch item two exact 64-bit sums over the elements' bit patterns, the second weighted by the element's place (1 .. 65521
    repeating): equal tensors give equal digests, and a changed, moved or swapped element changes one of them"""
    out = []
    for b in range(x.shape[0]):
        bits = x[b].reshape(-1).view(torch.int32).to(torch.int64)
        wgt = torch.arange(bits.numel(), device=x.device, dtype=torch.int64).remainder_(65521).add_(1)
        out.append(torch.stack([bits.sum(), (bits * wgt).sum()]))
    return torch.stack(out)


@pytest.mark.parametrize("loss", ["self", "cross"])
def test_k_side_past_4gib_b103(pkg, dev, orc, loss):
    """t, w, g and affs of 4.02 GiB, e (cross: and the EMA operand) and de of 6.4 GiB, through the C ABI.  self: two runs with g and de
    alive, compared bit for bit.  cross (the detached-EMA cross forward and its role-A backward, mode 2): a second g and de do not
    fit beside two operands, so the second run writes over the first (the buffers refilled with -3 in between) and its loss row and
    the exact per-item digests of g and de (bit_digest) must be the first run's.  Then a forward that writes affs alone, items 0 and
    102 against their B = 1 runs, the oracle on the last item's window.  Peak 33.6 to 37.2 GiB over its cases (measured)"""
    B, D = 103, 16
    offsets = pkg.multi_offset(BBBC, 4)
    K = len(offsets)
    cross = loss == "cross"
    lam = [2.0, 2.0] + [1.0] * (K - 2) if cross else [1.0] * K
    spec = spec_2d(pkg, offsets, lam)
    nbytes = B * K * H * W * 4
    assert nbytes > P32 and (B - 1) * K * H * W * 4 <= P32
    op, L = pkg.affinity_op, pkg._lib.lib()
    P = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    with case_report("batch f32 D=16 K=10 B=103 %s" % loss, (B, K, H, W), "t / w / g / affs bytes = %d vs 2^32", nbytes):
        g0 = torch.Generator(device=dev).manual_seed(5400)
        e = torch.randn([B, D, H, W], generator=g0, device=dev)
        eo = torch.randn([B, D, H, W], generator=g0, device=dev) if cross else None
        t = torch.rand([B, K, H, W], generator=g0, device=dev).lt_(0.6)          # (in place: no second 4 GiB block)
        w = torch.rand([B, K, H, W], generator=g0, device=dev).add_(0.5)
        m = torch.empty([B, K, H, W], dtype=torch.uint8, device=dev)
        for b0 in range(0, B, 26):
            m[b0:b0 + 26] = torch.rand([min(26, B - b0), K, H, W], generator=g0, device=dev) < 0.9
        assert cross_answers(pkg, spec, e, (1, 2) if cross else (0, 1)) == [1, 1]
        d, t, w, m, kshape = op._loss_operands(spec, e, t, w, m, dev)
        work, wsb = op.workspace(dev, d)
        dl = torch.full((), 0.5, device=dev)
        st = op._stream()

        def step(g, inv, de):
            lv = torch.empty(1 + K, device=dev)
            assert L.pea_affinity_fwd_ex(ctypes.byref(d), P(e), P(eo), P(t), P(w), P(m), None, P(g), P(inv), P(lv), P(work), wsb, st) == 0
            assert L.pea_affinity_bwd_ex2(ctypes.byref(d), P(e), P(eo), P(g), P(inv), None, P(dl), P(de), None, st) == 0
            torch.cuda.synchronize()
            return lv

        def mem(what):
            print("  allocated after %s: %.2f GiB" % (what, torch.cuda.memory_allocated() / 2.0 ** 30))

        inv_shape = (2, B, H, W) if cross else (B, H, W)
        mem("the inputs")
        g1, inv1 = torch.empty(kshape, device=dev), torch.empty(inv_shape, device=dev)
        de1 = torch.empty_like(e)
        lv1 = step(g1, inv1, de1)
        mem("run 1")
        if cross:  # run 2 writes over run 1: its loss row and the digests of its g and de must be run 1's
            dig1 = (bit_digest(g1), bit_digest(de1))
            g1.fill_(-3.0), de1.fill_(-3.0)
            lv2 = step(g1, inv1, de1)
            assert torch.equal(lv1, lv2) and all(torch.equal(a, b) for a, b in zip(dig1, (bit_digest(g1), bit_digest(de1))))
        else:
            g2, de2 = torch.empty(kshape, device=dev), torch.empty_like(e)
            lv2 = step(g2, torch.empty(inv_shape, device=dev), de2)
            assert torch.equal(lv1, lv2) and equal_in_chunks(g1, g2) and equal_in_chunks(de1, de2)
            del g2, de2
        mem("run 2")
        del lv2, inv1
        assert all(torch.isfinite(de1[i:i + 8]).all() for i in range(0, B, 8))  # (in chunks: isfinite takes |x| and three masks)
        affs = g1  # g has served: the same block takes the map
        lv3 = torch.empty(1 + K, device=dev)
        assert L.pea_affinity_fwd_ex(ctypes.byref(d), P(e), P(eo), P(t), P(w), P(m), P(affs), None, None, P(lv3), P(work), wsb, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(lv3, lv1)
        alone = lambda b: [run(pkg, spec, e[b:b + 1], t[b:b + 1], w[b:b + 1], m[b:b + 1], 0.5, None if eo is None else eo[b:b + 1])[i] for i in (1, 3)]
        items_alone(B, affs, de1, alone, 1e-5)
        window_of_last_item(orc, offsets, lam, max(BBBC), B, e, eo, t, w, m, affs, de1, 0.5)
        del e, eo, t, w, m, affs, g1, de1, work


def test_k_side_past_4gib_b103_labels_in(pkg, dev, orc):
    """the labels-in step at B = 103: affs of 4.02 GiB, e and de of 6.4 GiB, the g scratch of the two-launch form 4.4 GiB.  Peak 32.2 GiB (measured)"""
    B, D = 103, 16
    offsets = pkg.multi_offset(BBBC, 4)
    K = len(offsets)
    crit = pkg.WeightedMSE()
    with case_report("batch f32 D=16 K=10 B=103 labels-in", (B, K, H, W), "affs bytes = %d vs 2^32", B * K * H * W * 4):
        e = torch.randn([B, D, H, W], generator=torch.Generator(device=dev).manual_seed(5500), device=dev)
        lab = torch.cat([block_labels(dev, H, W, 5600 + (b % 7)) for b in range(B)])

        def step(ee, ll):
            et = ee.detach().requires_grad_(True)
            ls, affs, _ = pkg.embedding_loss_from_labels(et, ll, crit, offsets)
            (ls * 0.5).backward()
            return ls.detach().clone(), affs, et.grad

        l1, a1, g1 = step(e, lab)
        l2, a2, g2 = step(e, lab)
        assert torch.equal(l1, l2) and torch.equal(a1, a2) and torch.equal(g1, g2)
        del l2, a2, g2
        assert torch.isfinite(g1).all()
        items_alone(B, a1, g1, lambda b: step(e[b:b + 1], lab[b:b + 1])[1:], 1e-5)
        t, m, w = pkg.gen_targets(lab[B - 1:B], offsets, padding=True)
        window_of_last_item(orc, offsets, [1.0] * K, max(BBBC), B, e, None, t, w, m, a1, g1, 0.5, tb=0)
        del e, lab, t, m, w, l1, a1, g1


# ----------------------------------------------------------------------------------------------------------------------------
# h129: the element index, 16-bit storage
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_element_index_past_2_31_b129(pkg, dev, orc, dtype):
    """e and de of 2^31 + 2^24 elements (4.03 GiB).  Peak 33.5 GiB (measured)"""
    B, D, Hh, Ww = 129, 64, 512, 512
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8]
    K = len(offsets)
    spec = spec_2d(pkg, offsets)
    n = B * D * Hh * Ww
    assert n > E31 and (B - 1) * D * Hh * Ww <= E31
    gtol = GRAD_16BIT[dtype]
    with case_report("batch %s D=64 K=8 B=129 self" % str(dtype)[6:], (B, D, Hh, Ww), "e elements = %d vs 2^31", n):
        e, t, w, m = gpu_inputs(dev, B, D, [Hh, Ww], K, 5700)
        e = e.to(dtype)
        assert cross_answers(pkg, spec, e, (0, 1)) == [1, 1]
        # dloss = 128 for the batch: the normaliser B * W = 66 048 would put the stored f16 gradient (about 1e-5) among the f16
        # subnormals, whose spacing (6e-8) is coarser than the 2e-3 bound; the single-item runs (dloss 1) carry 129 / 128 of it
        l1, a1, _, g1 = run(pkg, spec, e, t, w, m, 128.0)
        l2, a2, _, g2 = run(pkg, spec, e, t, w, m, 128.0)
        assert g1.dtype == dtype
        assert torch.equal(l1, l2) and torch.equal(a1, a2) and torch.equal(g1, g2)
        del l2, a2, g2
        assert torch.isfinite(g1.float()).all()
        alone = lambda b: [run(pkg, spec, e[b:b + 1], t[b:b + 1], w[b:b + 1], m[b:b + 1])[i] for i in (1, 3)]
        items_alone(B, a1, g1, alone, gtol, scale=128.0)
        window_of_last_item(orc, offsets, [1.0] * K, 9, B, e, None, t, w, m, a1, g1, 128.0, gtol=gtol)
        del e, t, w, m, l1, a1, g1


# ----------------------------------------------------------------------------------------------------------------------------
# multi: the batched forms on a two-entry table
# ----------------------------------------------------------------------------------------------------------------------------
def same_loss(a, b):
    return abs(a.item() - b.item()) <= LOSS_RTOL * abs(b.item())


def test_multi_table_past_4gib(pkg, dev, monkeypatch):
    """pea_affinity_fwd_multi + pea_affinity_bwd_multi: entry 0 is e65 (e, de of 4.06 GiB), entry 1 its half-resolution sibling.  affs
    and de bit for bit against the forced-direct single calls, the loss at LOSS_RTOL (test_gpu_gather_families.py).  Peak 21.4 GiB (measured)"""
    B, D = 65, 16
    op = pkg.affinity_op
    offsets = pkg.multi_offset(BBBC, 4)[:2]
    K = len(offsets)
    specs = [spec_2d(pkg, offsets), spec_2d(pkg, offsets)]
    with case_report("multi f32 D=16 K=2 B=65, 1024^2 + 512^2", (B, D, H, W), "e bytes = %d vs 2^32", B * D * H * W * 4):
        ins = [gpu_inputs(dev, B, D, [H >> j, W >> j], K, 5800 + j) for j in range(2)]
        descs = [op.make_desc(sp, x[0]) for sp, x in zip(specs, ins)]
        assert op.multi_supported(descs)
        xs = [x[0].detach().requires_grad_(True) for x in ins]
        out = op.MultiAffinityMSE.apply(specs, [(x[1], x[2], x[3]) for x in ins], True, *xs)
        (out[0] * 0.5 + out[1] * 2.0).backward()
        monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
        try:
            for j, dloss in enumerate((0.5, 2.0)):
                l, a, _, g = run(pkg, specs[j], *ins[j], dloss)
                assert same_loss(out[j], l), j
                assert torch.equal(out[2 + j], a), "entry %d: affs of the table vs the single call" % j
                assert torch.equal(xs[j].grad, g), "entry %d: de of the table vs the single call" % j
                assert torch.equal(xs[j].grad[B - 1], g[B - 1]) and g[B - 1].abs().max() > 0
                del l, a, g
        finally:
            monkeypatch.delenv("PEA_FORCE_DIRECT", raising=False)
        del ins, xs, out


def test_multi_labels_table_past_4gib(pkg, dev):
    """pea_affinity_fwd_bwd_labels_multi on the same two-entry geometry, both entries sampling ONE label image (steps 1 and 2), against
    the tensor-form table fed with pea_gen_targets' output for the materialised label images: affs and de bit for bit, the loss at
    LOSS_RTOL (test_gpu_gather_families.py).  Peak 19.2 GiB (measured)"""
    B, D = 65, 16
    op = pkg.affinity_op
    offsets = pkg.multi_offset(BBBC, 4)[:2]
    specs = [spec_2d(pkg, offsets), spec_2d(pkg, offsets)]
    flags = pkg._lib.TGT_PADDING | pkg._lib.TGT_MASK_INSIDE
    with case_report("multi labels f32 D=16 K=2 B=65, 1024^2 + 512^2", (B, D, H, W), "e bytes = %d vs 2^32", B * D * H * W * 4):
        g0 = torch.Generator(device=dev).manual_seed(5900)
        es = [torch.randn([B, D, H >> j, W >> j], generator=g0, device=dev) for j in range(2)]
        lab = torch.cat([block_labels(dev, H, W, 5950 + (b % 5)) for b in range(B)])
        xs = [x.detach().requires_grad_(True) for x in es]
        sources = op.label_sources(xs, 2, lab, None)
        out = op.MultiLabelsAffinityMSE.apply(specs, sources, flags, True, None, *xs)
        (out[0] * 0.5 + out[1] * 2.0).backward()
        tens = []
        for j, (lb, step) in enumerate(sources):
            t, m, w = pkg.gen_targets(op.materialise_labels(lb, es[j], 2, step), offsets, padding=True)
            tens.append((t, w, m))
        ys = [x.detach().requires_grad_(True) for x in es]
        ref = op.MultiAffinityMSE.apply(specs, tens, True, *ys)
        (ref[0] * 0.5 + ref[1] * 2.0).backward()
        for j in range(2):
            assert same_loss(out[j], ref[j]), j
            assert torch.equal(out[2 + j], ref[2 + j]), "entry %d: affs of the labels table vs the tensor table" % j
            assert torch.equal(xs[j].grad, ys[j].grad), "entry %d: de of the labels table vs the tensor table" % j
            assert xs[j].grad[B - 1].abs().max() > 0
        del es, lab, xs, ys, out, ref, tens


# ----------------------------------------------------------------------------------------------------------------------------
# dist: the distance-form affinities
# ----------------------------------------------------------------------------------------------------------------------------
DIST_OFFS = [[-1, 0], [0, -1], [0, -1], [2, -3], [0, 0], [0, 9], [-27, 0], [5, 5]]


def dist_embedding(dev, B, D, seed):
    """per-label mean + noise over blocky labels (blocks of 4, 12 ids) on the f16 grid: the recipe of test_gpu_dist_affinity.embedding,
    on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    coarse = torch.randint(0, 12, (B, H // 4, W // 4), generator=g, device=dev)
    means = 2.1 / np.sqrt(D) * torch.randn(B, 12, D, generator=g, device=dev)
    e = torch.gather(means, 1, coarse.reshape(B, -1, 1).expand(-1, -1, D)).reshape(B, H // 4, W // 4, D).permute(0, 3, 1, 2)
    e = e.repeat_interleave(4, 2).repeat_interleave(4, 3)
    e += 0.24 / np.sqrt(D) * torch.randn(e.shape, generator=g, device=dev)
    return e.half().float().contiguous()


@pytest.mark.parametrize("border", ["replicate", "zero"])
def test_dist_affinity_past_4gib_b129(pkg, dev, border):
    """affs and g of 4.03 GiB, e and de of 8.06 GiB.  Peak 34.3 GiB (measured)"""
    B, D, K = 129, 16, len(DIST_OFFS)
    nbytes = B * K * H * W * 4
    assert nbytes > P32 and (B - 1) * K * H * W * 4 <= P32
    with case_report("dist f32 D=16 K=8 B=129 %s" % border, (B, K, H, W), "affs bytes = %d vs 2^32", nbytes):
        e = dist_embedding(dev, B, D, 6000)
        a1 = c_fwd(pkg, e, DIST_OFFS, border=border)
        a2 = c_fwd(pkg, e, DIST_OFFS, border=border)
        assert torch.equal(a1, a2)
        del a2
        # the window of the last item: the far corner of the image, so the border rule is part of it
        hh, ww, y0, x0 = 96, 128, H - 96, W - 128
        ew = e[B - 1:, :, y0:, x0:].cpu().numpy()
        a64, d64 = dist_reference(ew, DIST_OFFS, DV, DD, border)
        keep = np.abs(d64 - DV) >= EDGE
        inner = (slice(None), slice(None), slice(27, hh), slice(27, ww))  # the window's own near faces are not the image's
        err = float((np.abs(a1[B - 1:, :, y0:, x0:].cpu().numpy() - a64) * keep)[inner].max())
        assert err <= TOL_AFFS and 1 - keep.mean() < 1e-3, err
        # the vjp: g zero outside the window's kept pairs would not test the batch; a dense g, zero only at the left-out pairs
        g = torch.randn(a1.shape, generator=torch.Generator(device=dev).manual_seed(6001), device=dev)
        gw = g[B - 1:, :, y0:, x0:].cpu().numpy() * keep
        g[B - 1:, :, y0:, x0:] = torch.from_numpy(gw).to(dev)
        de1 = c_vjp(pkg, e, DIST_OFFS, g, border=border)
        de2 = c_vjp(pkg, e, DIST_OFFS, g, border=border)
        assert torch.equal(de1, de2)
        del de2
        de64 = dist_vjp_reference(ew, DIST_OFFS, gw, DV, DD, border)
        # de(p) sums the pairs (p, p + o) and (p - o, p): past the near margin every such pair lies in the window or, at the far faces,
        # outside the image itself, where window and image apply the same border rule
        inn = inner
        dw = de1[B - 1:, :, y0:, x0:].cpu().numpy()
        top = float(np.abs(de64[inn]).max())
        err_g = float(np.abs(dw[inn] - de64[inn]).max()) / top
        print("dist window of item %d: affs %.3g  de rel-to-max %.3g" % (B - 1, err, err_g))
        assert top > 0.1 and err_g <= TOL_DE["f32"]
        for b in (0, B - 1):
            ab = c_fwd(pkg, e[b:b + 1].contiguous(), DIST_OFFS, border=border)
            db = c_vjp(pkg, e[b:b + 1].contiguous(), DIST_OFFS, g[b:b + 1].contiguous(), border=border)
            da = (ab[0] - a1[b]).abs().max().item()
            dg = dev_relmax(db[0], de1[b])
            print("dist item %d alone vs in batch: affs %.3g  de rel-to-max %.3g" % (b, da, dg))
            assert da <= TOL_AFFS and dg <= TOL_DE["f32"]
        del e, a1, g, de1


# ----------------------------------------------------------------------------------------------------------------------------
# head: one item's x block past 4 GiB
# ----------------------------------------------------------------------------------------------------------------------------
HEAD_S = (1 << 25) + 4099


def head_ranges(x_elem_bytes, S):
    """the pixel ranges compared per item: the first 4096, the last 4099, and 8192 around byte offset 2^32 of the item's x block"""
    p = (P32 // x_elem_bytes) % S  # the pixel (of some channel's plane) at which the block's byte offset passes 2^32
    lo = max(0, min(p - 4096, S - 8192))
    return [(0, 4096), (S - 4099, S), (lo, lo + 8192)]


HEAD_CASES = [("f32", 32, 16, HEAD_S), ("f16", 64, 16, HEAD_S), ("f16", 256, 32, (1 << 23) + 4099)]


@pytest.mark.parametrize("family,C,D,S", HEAD_CASES, ids=["f32_32to16", "f16_64to16", "f16_256to32"])
def test_head_item_block_past_4gib(pkg, dev, family, C, D, S):
    """pea_head_fwd / pea_head_bwd (f32, C = 32, D = 16) and pea_head_fwd_t / pea_head_bwd_t (f16 in and out: C = 64, D = 16, and the
    largest pair pea_head_supported_t accepts, C = 256, D = 32, on the channel-chunked heads) at B = 2 and an odd S (the element
    forms).  One item's x block is C * S * bytes per element: 32 * 33 558 531 * 4 = 64 * 33 558 531 * 2 = 4 295 491 968 and
    256 * 8 392 707 * 2 = 4 297 065 984 bytes, all > 2^32; x and dx are 8 GiB each, and two dx are alive for the bit comparison (at
    S = 2^25 + 4099 the pair (256, 32) would need 34 GiB for x alone, hence its smaller S).  e and dx against a float64 einsum on
    three pixel ranges of each item, dW / db against float64 sums over the whole tensor taken on the device in chunks.  Tolerances:
    f32 e / dx 1e-5 max|ref| (test_gpu_head16.py, test_gpu_fullsize2.py), a 16-bit e / dx half an ulp + 2e-5 max|ref|, dW / db 2e-5
    max|ref| (test_gpu_head16.py).  Two runs bit for bit.  Peak 31.1 to 38.0 GiB over its cases (measured)"""
    import test_gpu_head16 as h16
    L = pkg._lib.lib()
    B = 2
    dt = torch.float32 if family == "f32" else torch.float16
    es = 4 if family == "f32" else 2
    block = C * S * es
    assert block > P32
    if family == "f16":
        assert L.pea_head_supported_t(C, D, h16.CODE[dt], h16.CODE[dt]) == 1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with case_report("head %s C=%d D=%d B=2" % (family, C, D), (B, C, S), "x block of one item = %d bytes vs 2^32", block):
        g = torch.Generator(device=dev).manual_seed(6100)
        X = torch.randn(B, C, S, generator=g, device=dev, dtype=dt)
        UP = torch.randn(B, D, S, generator=g, device=dev, dtype=dt)
        Wt = torch.randn(D, C, generator=g, device=dev) * (0.2 if C <= 64 else 0.1)
        Bt = torch.randn(D, generator=g, device=dev)
        wsb = L.pea_head_workspace_bytes(C, D)
        outs = []
        for _ in range(2):
            E = torch.empty(B, D, S, device=dev, dtype=dt)
            dX = torch.empty_like(X)
            dW, dB = torch.empty(D, C, device=dev), torch.empty(D, device=dev)
            work = torch.empty(wsb // 4, device=dev)
            if family == "f32":
                assert L.pea_head_fwd(B, C, D, S, p(X), p(Wt), p(Bt), p(E), st) == 0
                assert L.pea_head_bwd(B, C, D, S, p(X), p(Wt), p(UP), p(dX), p(dW), p(dB), p(work), wsb, st) == 0
            else:
                code = h16.CODE[dt]
                assert L.pea_head_fwd_t(B, C, D, ctypes.c_size_t(S), p(X), code, p(Wt), p(Bt), p(E), code, st) == 0
                assert L.pea_head_bwd_t(B, C, D, ctypes.c_size_t(S), p(X), code, p(Wt), p(UP), code, p(dX), p(dW), p(dB), p(work), wsb, st) == 0
            torch.cuda.synchronize()
            if outs:  # the second run: bit for bit, then gone (two dx of 8 GiB do not stay)
                for name, a, b in zip(("e", "dx", "dW", "db"), (E, dX, dW, dB), outs[0]):
                    assert torch.equal(a, b), name
            else:
                outs.append((E, dX, dW, dB))
            del E, dX, dW, dB
        E, dX, dW, dB = outs[0]
        W64 = Wt.double()
        for b in range(B):
            for lo, hi in head_ranges(es, S):
                e_ref = torch.einsum("dc,cp->dp", W64, X[b, :, lo:hi].double()) + Bt.double()[:, None]
                dx_ref = torch.einsum("dc,dp->cp", W64, UP[b, :, lo:hi].double())
                tag = "item %d pixels %d..%d" % (b, lo, hi)
                if family == "f32":
                    h16.check32(tag + " e", h16.npf(E[b, :, lo:hi]), e_ref.cpu().numpy(), 1e-5)
                    h16.check32(tag + " dx", h16.npf(dX[b, :, lo:hi]), dx_ref.cpu().numpy(), 1e-5)
                else:
                    h16.check16(tag + " e", h16.npf(E[b, :, lo:hi]), e_ref.cpu().numpy(), h16.UNIT[dt])
                    h16.check16(tag + " dx", h16.npf(dX[b, :, lo:hi]), dx_ref.cpu().numpy(), h16.UNIT[dt])
        dw_ref = torch.zeros(D, C, dtype=torch.float64, device=dev)
        db_ref = torch.zeros(D, dtype=torch.float64, device=dev)
        step = (1 << 27) // C  # 1 GiB of float64 x per chunk
        for b in range(B):
            for lo in range(0, S, step):
                u = UP[b, :, lo:lo + step].double()
                dw_ref += u @ X[b, :, lo:lo + step].double().t()
                db_ref += u.sum(1)
        h16.check32("dW", h16.npf(dW), dw_ref.cpu().numpy(), 2e-5)
        h16.check32("db", h16.npf(dB), db_ref.cpu().numpy(), 2e-5)
        del X, UP, E, dX, outs
