"""GPU (-m gpu): ONE batch item's [D or K, Z, Y, X] block on either side of 2 GiB.

The LDS-tiled, LDS-DMA (cross) and unit-box kernels select a channel plane through the scalar offset of a raw buffer whose
num_records is 2^31, and the gfx9 range check counts that scalar offset (csrc/pea_plan.h:33-43): once the block of one batch item
reaches 2^31 bytes the planes past it read zeros and drop their stores without an error.  plan_tiles (pea_plan.h:39-43), plan_xdma
(pea_xdma.h:997-998) and plan_box (pea_k_box.hip:82, pea_box.h:350) therefore refuse such blocks and the direct kernels (64-bit
pointers) run.  Every case here runs at two shapes four columns apart: UNDER, the largest block the fast families accept, and AT,
the smallest they must refuse.  Each loss case runs with the default dispatch (twice: bit for bit) and with PEA_FORCE_DIRECT=1; the
whole affs, loss and de of the two are compared on the device (loss rel 1e-5, affs 2e-6, grads rel-to-max 1e-5; the stored gradient
of f16 storage 2e-3, of bf16 storage 8e-3 as in test_gpu_bf16.py): that covers every channel, the last row and the last pixel.  AT
the limit the default dispatch IS the direct kernels, so there the two runs must agree bit for bit: a block of exactly 2^31 bytes is
still addressable through one resource (the last byte lies at offset 2^31 - 1), so a guard moved by one plane computes the right
numbers on this shape and only the bits tell which family ran.  The CPU oracle then runs on two windows of the default result
(affs abs 1e-5, grads rel-to-max 1e-4; 16-bit storage as above): an interior one and, for the circular 2D problems, the SEAM window
-- rows H-48..H-1 then 0..47, columns W-64..W-1 then 0..63, concatenated on the device; on the torus that is a contiguous window
whose interior holds the last row, column and pixel of every plane, the highest addresses of the block -- or, for 3D CROP_ZERO,
the FAR-CORNER window (the mirror of test_gpu_fullsize.py:155-166).  pea_cross_supported is asserted on each side, so a pass cannot
come from the fall-back having served both; where no query exists the bits tell (default_vs_direct).  The pair and the labels-in
cases are held to the calls they replace (and, at the limit, to their refusal) instead of a forced-direct run; the labels-in cases
have no oracle window of their own.  Inputs are generated on the device; only windows travel to the host.

Cases (S = pixels of the item; the limit is 2^31 = 2 147 483 648 bytes in every one):

  d16     2D f32 D=16 circular NORM_BX, multi_offset([1,3,5,9,11], 4) (K=10), u8 mask
          4096 x 8188: D S 4 = 16 * 33 538 048 * 4 = 2 146 435 072 = 2^31 - 2^20;  4096 x 8192: 16 * 2^25 * 4 = 2^31
          self loss; EMA cross loss; the one-launch pair (pea_affinity_fwd_dual_ex / _bwd_dual_ex); the labels-in step
          cross modes 0, 1, 2, 5 answer 1 under, 0 at
  d32     2D f32 D=32, the same stencil: 4096 x 4092: 32 * 16 760 832 * 4 = 2 145 386 496 = 2^31 - 2^21;  4096 x 4096: 2^31
          self loss and cross loss on the projection-first backward (modes 0 .. 4 answer 1 under, 0 at)
  d64     2D f16 / bf16 storage D=64, K=8 (configs[4]'s stencil): 2048 x 4092: 64 * 8 380 416 * 4 = 2 145 386 496;  2048 x 4096: 2^31
          the planners multiply by 4 whatever the storage: the tensor is 1 GiB, the fast families already step aside.  The 16-bit
          cross kernels also need X % 8 == 0, so 2048 x 4092 is theirs at no size (the tiled kernels serve it); 2048 x 4088
          (64 * 8 372 224 * 4 = 2 143 289 344) is the largest block they accept and runs as a third shape (f16, self and cross)
  3d      3D f32 D=16 CROP_ZERO NORM_CROPPED, norm5's 12 offsets: 32 x 1024 x 1020: 16 * 33 423 360 * 4 = 2 139 095 040;
          32 x 1024 x 1024: 2^31.  training forward + backward (z-march, 3D cross kernels; modes 0 .. 3 answer 1 under, 0 at), the
          cross loss, pea_affinity_infer, and pea_affinity_infer_stitch into a volume of its own size against pea_affinity_infer +
          pea_fill_border_relu + pea_stitch_add: bit for bit where pea_affinity_infer runs the direct kernels (PEA_FORCE_DIRECT=1),
          whose arithmetic the fused kernel states; against the default dispatch, whose LDS kernels sum in another order under the
          limit, within 1e-5 after pea_stitch_finalize (test_gpu_infer_stitch.py).  pea_infer_stitch_supported answers 1 on BOTH
          sides: that kernel is a gather through 64-bit pointers (csrc/pea_k_infer_stitch.hip) and has no block limit
  k20     2D f32 D=16 K=20 (multi_offset([1,3,5,9,11], 8)), u8 mask and once an f32 mask
          4096 x 6552: K S 4 = 20 * 26 836 992 * 4 = 2 146 959 360 < 2^31;  4096 x 6556: 20 * 26 853 376 * 4 = 2 148 270 080 >= 2^31
          there the tiled kernels take the second resource (ksplit = 10: 10 * 26 853 376 * 4 = 1 074 135 040 per half) and the cross
          kernels refuse on both sides (K = 20 > their 10 offsets).  D S 4 = 1.72e9 stays under the limit on both sides

Peak device memory (torch.cuda.max_memory_allocated above the case's start) and run time are printed by every case and listed below.
Every case stays under 40 GiB and frees its tensors.  tests/test_block_edges_host.py pins the planner's answers without a device.

Measured on an MI355X (case, shape, peak device memory of the case, run time inside the case; in some runs one or two cases,
not the same ones each time, took 5 to 6 s instead):

  2d f32 D=16 self under                         1x16x4096x8188            15.31 GiB   0.75 s
  2d f32 D=16 self at                            1x16x4096x8192            15.31 GiB   0.05 s
  2d f32 D=16 cross under                        1x16x4096x8188            17.31 GiB   1.11 s
  2d f32 D=16 cross at                           1x16x4096x8192            17.31 GiB   0.04 s
  2d f32 D=32 self under                         1x32x4096x4092            12.65 GiB   0.04 s
  2d f32 D=32 self at                            1x32x4096x4096            12.66 GiB   1.63 s
  2d f32 D=32 cross under                        1x32x4096x4092            14.64 GiB   0.04 s
  2d f32 D=32 cross at                           1x32x4096x4096            14.66 GiB   0.04 s
  2d f32 D=16 pair under                         1x16x4096x8188            18.94 GiB   1.37 s
  2d f32 D=16 pair at                            1x16x4096x8192            16.94 GiB   0.03 s
  2d f32 D=16 labels-in two_launch under         1x16x4096x8188            17.44 GiB   1.41 s
  2d f32 D=16 labels-in two_launch at            1x16x4096x8192            17.94 GiB   0.04 s
  2d f32 D=16 labels-in one_launch under         1x16x4096x8188            17.44 GiB   1.28 s
  2d f32 D=16 labels-in one_launch at            1x16x4096x8192            17.94 GiB   0.04 s
  2d float16 D=64 self under                     1x64x2048x4092            10.06 GiB   0.04 s
  2d float16 D=64 self at                        1x64x2048x4096            10.06 GiB   0.04 s
  2d float16 D=64 cross under                    1x64x2048x4092            11.06 GiB   1.87 s
  2d float16 D=64 cross at                       1x64x2048x4096            11.06 GiB   0.04 s
  2d float16 D=64 self under8                    1x64x2048x4088            10.04 GiB   0.04 s
  2d float16 D=64 cross under8                   1x64x2048x4088            11.04 GiB   0.04 s
  2d bfloat16 D=64 self under                    1x64x2048x4092            10.06 GiB   0.04 s
  2d bfloat16 D=64 self at                       1x64x2048x4096            10.06 GiB   0.04 s
  2d f32 D=16 K=20 u8 mask under                 1x20x4096x6552            17.30 GiB   2.06 s
  2d f32 D=16 K=20 u8 mask at                    1x20x4096x6556            17.31 GiB   0.05 s
  2d f32 D=16 K=20 f32 mask at                   1x20x4096x6556            18.81 GiB   1.31 s
  3d f32 D=16 self under                         1x16x32x1024x1020         15.94 GiB   0.17 s
  3d f32 D=16 self at                            1x16x32x1024x1024         16.00 GiB   0.15 s
  3d f32 D=16 cross under                        1x16x32x1024x1020         17.93 GiB   0.15 s
  3d f32 D=16 cross at                           1x16x32x1024x1024         18.00 GiB   2.03 s
  3d f32 D=16 infer + stitch under               1x16x32x1024x1020          8.22 GiB   0.30 s
  3d f32 D=16 infer + stitch at                  1x16x32x1024x1024          8.25 GiB   0.23 s
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest
import torch

from test_gpu_fullsize import AFFS_ATOL, GRAD_RTOL, full_norms, gpu_inputs, run
from test_gpu_fullsize2 import npy, relmax, window_oracle_2d

pytestmark = pytest.mark.gpu
LIMIT = 1 << 31
SIDES = ["under", "at"]
BBBC = [1, 3, 5, 9, 11]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@contextlib.contextmanager
def case_report(name, shape, limit, value):
    """prints the case's shape, the limit it crosses and the value, its peak device memory (above what was allocated when it began: an
    earlier test that failed may still hold its tensors) and its run time; frees the cache; holds the case to the 40 GiB budget"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 30
    print("\n[edge] %s shape=%s %s peak=%.2f GiB time=%.2f s" % (name, "x".join(str(v) for v in shape), limit % value, peak, dt))
    torch.cuda.empty_cache()
    assert peak < 40.0, "the case must stay under 40 GiB"


def dev_relmax(a, b):
    """max |a - b| / max |b| on the device"""
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30)).item()


def cross_answers(pkg, spec, e, modes):
    d = pkg.affinity_op.make_desc(spec, e)
    return [int(pkg._lib.lib().pea_cross_supported(ctypes.byref(d), mo)) for mo in modes]


def default_vs_direct(pkg, spec, e, t, w, m, monkeypatch, dloss, eo=None, gtol=1e-5, direct_serves=False):
    """two default runs bit for bit; the default run against PEA_FORCE_DIRECT=1 over the WHOLE tensors -> the default run.
    direct_serves: the block is at the limit, where the default dispatch IS the direct kernels (csrc/pea_plan.h: "larger blocks take
    the direct kernels"): the two runs must then agree bit for bit -- a planner that let a fast family through shows here even where
    its kernel still happens to be right.  Otherwise a fast family must serve (the LDS kernels sum in another order: some bits of
    affs, loss or de differ from the direct kernels'), which is the only witness where no query exists: the tiled kernels on the
    16-bit 2048 x 4092 shape, and their second resource (ksplit) on the far side of the K block"""
    monkeypatch.delenv("PEA_FORCE_DIRECT", raising=False)
    l1, a1, p1, g1 = run(pkg, spec, e, t, w, m, dloss, eo)
    l2, a2, p2, g2 = run(pkg, spec, e, t, w, m, dloss, eo)
    assert torch.equal(l1, l2) and torch.equal(p1, p2), "two default runs: loss differs"
    assert torch.equal(a1, a2), "two default runs: affs differ"
    assert torch.equal(g1, g2), "two default runs: de differs"
    del l2, a2, p2, g2
    assert torch.isfinite(g1.float()).all()
    monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
    try:
        l0, a0, _, g0 = run(pkg, spec, e, t, w, m, dloss, eo)
    finally:
        monkeypatch.delenv("PEA_FORCE_DIRECT", raising=False)
    dl = abs(l1.item() - l0.item()) / abs(l0.item())
    da = (a1 - a0).abs().max().item()
    last = (a1[0, :, -1].reshape(a1.shape[1], -1)[:, -1] - a0[0, :, -1].reshape(a0.shape[1], -1)[:, -1]).abs().max().item()
    dg = dev_relmax(g1, g0)
    print("default vs direct: loss rel %.3g  affs max %.3g (last pixel of every channel %.3g)  de rel-to-max %.3g" % (dl, da, last, dg))
    assert dl <= 1e-5, "default vs PEA_FORCE_DIRECT=1: loss differs by rel %.3g" % dl
    assert da < 2e-6, "default vs PEA_FORCE_DIRECT=1: affs differ by %.3g" % da
    assert dg < gtol, "default vs PEA_FORCE_DIRECT=1: de differs by rel-to-max %.3g" % dg
    same = torch.equal(a1, a0) and torch.equal(g1, g0) and torch.equal(l1, l0)
    if direct_serves:
        assert same, "at the limit the direct kernels must serve: affs differ from PEA_FORCE_DIRECT=1 by %.3g, de by rel-to-max %.3g" % (da, dg)
    else:
        assert not same, "a fast family must serve this shape, but the default run has the direct kernels' bits"
    return l1, a1, p1, g1


def seam(x):
    """[B, C, H, W] -> [B, C, 96, 128]: rows H-48..H-1, 0..47 and columns W-64..W-1, 0..63 -- contiguous on the torus"""
    if x is None:
        return None
    r = torch.cat([x[:, :, -48:], x[:, :, :48]], dim=2)
    return torch.cat([r[..., -64:], r[..., :64]], dim=3).contiguous()


def windows_2d(orc, offsets, lam, reach, W, e, eo, t, w, m, affs, grad, dloss, gtol=GRAD_RTOL, og_extra=None):
    """the oracle on the seam window and on an interior window of image 0 (B = 1: N_i = W under NORM_BX); interior compared.
    og_extra(view) -> a second oracle gradient to add (the pair's cross half)"""
    H = e.shape[2]
    hh, ww = 96, 128
    inner = (slice(None), slice(reach, hh - reach), slice(reach, ww - reach))
    cut = lambda x, y0, x0: None if x is None else x[:, :, y0:y0 + hh, x0:x0 + ww]
    views = {"seam": seam, "interior": lambda x: cut(x, (H // 2) & ~7, (W // 2 + 40) & ~7)}
    for name, view in views.items():
        ev, ov, tv, wv, mv = (view(x) for x in (e, eo, t, w, m))
        oa, og = window_oracle_2d(orc, offsets, lam, float(W), 0, 0, 0, hh, ww, ev, ov, tv, wv, mv, dloss)
        if og_extra is not None:
            og = og + og_extra(view)
        if affs is not None:
            ea = float(np.abs(npy(view(affs))[0][inner] - oa[inner]).max())
            assert ea < AFFS_ATOL, "%s window: affs differ from the oracle by %.3g" % (name, ea)
        eg = relmax(npy(view(grad))[0][inner], og[inner])
        print("%s window vs oracle: de rel-to-max %.3g" % (name, eg))
        assert eg < gtol, "%s window: de differs from the oracle by rel-to-max %.3g" % (name, eg)


def spec_2d(pkg, offsets, lam=None):
    return pkg.AffinitySpec(2, offsets, lam, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)


def ema_of(dev, e, seed):
    eo = torch.randn(e.shape, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
    return eo.to(e.dtype)


# ----------------------------------------------------------------------------------------------------------------------------
# 2D, f32, D = 16 and D = 32: the D block
# ----------------------------------------------------------------------------------------------------------------------------
D_SHAPES = {(16, "under"): (4096, 8188), (16, "at"): (4096, 8192), (32, "under"): (4096, 4092), (32, "at"): (4096, 4096)}
D_MODES = {16: (0, 1, 2, 5), 32: (0, 1, 2, 3, 4)}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("loss", ["self", "cross"])
@pytest.mark.parametrize("D", [16, 32])
def test_2d_f32_d_block(pkg, dev, orc, monkeypatch, D, loss, side):
    """self loss / EMA cross loss (detached second operand), f32, BBBC stencil, u8 mask.  Peak 12.7 to 17.3 GiB over its cases (measured)"""
    H, W = D_SHAPES[(D, side)]
    offsets = pkg.multi_offset(BBBC, 4)
    K = len(offsets)
    lam = [2.0 if i < 2 else 1.0 for i in range(K)] if loss == "cross" else [1.0] * K
    spec = spec_2d(pkg, offsets, lam)
    block = D * H * W * 4
    assert (block < LIMIT) == (side == "under") and abs(block - LIMIT) <= 1 << 21
    with case_report("2d f32 D=%d %s %s" % (D, loss, side), (1, D, H, W), "D*S*4 = %d vs 2^31", block):
        e, t, w, m = gpu_inputs(dev, 1, D, [H, W], K, 4100 + D)
        eo = ema_of(dev, e, 4200 + D) if loss == "cross" else None
        want = 1 if side == "under" else 0
        assert cross_answers(pkg, spec, e, D_MODES[D]) == [want] * len(D_MODES[D])
        l, a, _, g = default_vs_direct(pkg, spec, e, t, w, m, monkeypatch, 0.5, eo, direct_serves=side == "at")
        windows_2d(orc, offsets, lam, max(BBBC), W, e, eo, t, w, m, a, g, 0.5)
        del e, t, w, m, eo, l, a, g


@pytest.mark.parametrize("side", SIDES)
def test_2d_d16_pair_in_one_launch(pkg, dev, orc, side):
    """pea_affinity_fwd_dual_ex: every output bit-identical to the two pea_affinity_fwd_ex calls it replaces (include/pea.h), which
    test_2d_f32_d_block holds to the oracle; pea_affinity_bwd_dual_ex against the two pea_affinity_bwd_ex2 calls (rel-to-max 2e-5, the
    bound of test_gpu_cross.py between the pair's kernels) and against the oracle's self + cross gradient on both windows.  AT the
    limit the forward pair and the backward pair must answer PEA_E_UNSUPPORTED before anything is launched.  Peak 16.9 to 18.9 GiB over its cases (measured)"""
    H, W = D_SHAPES[(16, side)]
    D, B = 16, 1
    offsets = pkg.multi_offset(BBBC, 4)
    K = len(offsets)
    lamx = [2.0, 2.0] + [1.0] * (K - 2)
    op, L = pkg.affinity_op, pkg._lib.lib()
    with case_report("2d f32 D=16 pair %s" % side, (1, D, H, W), "D*S*4 = %d vs 2^31", D * H * W * 4):
        E, T, Wt, M = gpu_inputs(dev, 1, D, [H, W], K, 4116)
        EO = ema_of(dev, E, 4216)
        d0 = op.make_desc(spec_2d(pkg, offsets), E)
        dx = op.make_desc(spec_2d(pkg, offsets, lamx), E)
        P = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        wsb = L.pea_workspace_bytes(ctypes.byref(d0))
        work = torch.empty(2, max(wsb, 8) // 4, device=dev)
        assert L.pea_workspace_init(P(work), 2 * wsb, None) == 0
        affs, g0, gx = (torch.empty(B, K, H, W, device=dev) for _ in range(3))
        inv0, inv2 = torch.empty(B, H, W, device=dev), torch.empty(2, B, H, W, device=dev)
        l0, lx = torch.empty(1 + K, device=dev), torch.empty(1 + K, device=dev)
        assert L.pea_affinity_fwd_ex(ctypes.byref(d0), P(E), None, P(T), P(Wt), P(M), P(affs), P(g0), P(inv0), P(l0), P(work[0]), wsb, st) == 0
        assert L.pea_affinity_fwd_ex(ctypes.byref(dx), P(E), P(EO), P(T), P(Wt), P(M), None, P(gx), P(inv2), P(lx), P(work[1]), wsb, st) == 0
        affs_d, g0_d, gx_d = (torch.full((B, K, H, W), -3.0, device=dev) for _ in range(3))
        inv0_d, invo_d = torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev)
        l0_d, lx_d = torch.empty(1 + K, device=dev), torch.empty(1 + K, device=dev)
        rc = L.pea_affinity_fwd_dual_ex(ctypes.byref(d0), ctypes.byref(dx), P(E), P(EO), P(T), P(Wt), P(M), P(affs_d), P(g0_d), P(gx_d),
                                        P(inv0_d), P(invo_d), P(l0_d), P(lx_d), P(work[0]), P(work[1]), wsb, st)
        torch.cuda.synchronize()
        assert L.pea_cross_supported(ctypes.byref(d0), 5) == (1 if side == "under" else 0)
        if side == "under":
            assert rc == 0
            for name, x, y in (("affs", affs_d, affs), ("g", g0_d, g0), ("g_cross", gx_d, gx), ("inv", inv0_d, inv0), ("inv_own_of_pair", inv0_d, inv2[0]),
                               ("inv_other", invo_d, inv2[1]), ("loss", l0_d, l0), ("loss_cross", lx_d, lx)):
                assert torch.equal(x, y), name
        else:
            assert rc == pkg._lib.E_UNSUPPORTED
            assert (affs_d == -3.0).all() and (g0_d == -3.0).all() and (gx_d == -3.0).all()  # nothing was launched
        del affs_d, g0_d, gx_d, inv0_d, invo_d
        # the pair's backward against the two single backwards and the oracle
        dl0, dlx = torch.full((), 0.6, device=dev), torch.full((), 1.7, device=dev)
        de_s, de_x, de_p = torch.empty_like(E), torch.empty_like(E), torch.full_like(E, -3.0)
        assert L.pea_affinity_bwd_ex2(ctypes.byref(d0), P(E), None, P(g0), P(inv0), None, P(dl0), P(de_s), None, st) == 0
        assert L.pea_affinity_bwd_ex2(ctypes.byref(dx), P(E), P(EO), P(gx), P(inv2), None, P(dlx), P(de_x), None, st) == 0
        rc = L.pea_affinity_bwd_dual_ex(ctypes.byref(d0), P(E), P(EO), P(g0), P(gx), P(inv0), P(inv2[1]), P(dl0), P(dlx), P(de_p), st)
        torch.cuda.synchronize()
        de_s += de_x
        del de_x
        assert rc == (0 if side == "under" else pkg._lib.E_UNSUPPORTED)  # at the limit plan_xdma refuses the pair's backward too
        if rc == 0:
            dg = dev_relmax(de_p, de_s)
            print("pair backward vs the two single backwards: rel-to-max %.3g" % dg)
            assert dg < 2e-5
        if rc != 0:
            assert (de_p == -3.0).all()  # nothing was launched
        grad = de_p if rc == 0 else de_s
        cross_half = lambda view: window_oracle_2d(orc, offsets, lamx, float(W), 0, 0, 0, 96, 128, view(E), view(EO), view(T), view(Wt), view(M), 1.7)[1]
        windows_2d(orc, offsets, [1.0] * K, max(BBBC), W, E, None, T, Wt, M, affs, grad, 0.6, og_extra=cross_half)
        del E, EO, T, Wt, M, affs, g0, gx, inv0, inv2, de_s, de_p, grad


def block_labels(dev, H, W, seed):
    """a random id image, ids 0..200, drawn as blocks of 16 x 16"""
    g = torch.Generator(device=dev).manual_seed(seed)
    ids = torch.randint(0, 201, (1, (H + 15) // 16, (W + 15) // 16), generator=g, device=dev, dtype=torch.int32)
    return ids.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W].contiguous()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("form", ["two_launch", "one_launch"])
def test_2d_d16_labels_in_step(pkg, dev, monkeypatch, form, side):
    """pea_affinity_fwd_bwd_labels_ex (two launches through the scratch buffer; the one-launch kernel) against the tensor form fed
    with pea_gen_targets' output (loss 2e-6, affs 2e-6, grads 1e-5: test_gpu_fullsize2.py).  UNDER the limit the entry must
    serve; AT it it must answer PEA_E_UNSUPPORTED with nothing written (the wrapper then generates the targets and takes the tensor
    path: there the comparison only holds the fall-back to itself).  No oracle window here: the tensor form is held to the oracle by
    test_2d_f32_d_block.  Peak 17.4 to 17.9 GiB over its cases (measured)"""
    H, W = D_SHAPES[(16, side)]
    D = 16
    op = pkg.affinity_op
    monkeypatch.setattr(op, "LABELS_TWO_LAUNCH_MIN_PX", 0 if form == "two_launch" else 1 << 62)
    offsets = pkg.multi_offset(BBBC, 4)
    crit = pkg.WeightedMSE()
    with case_report("2d f32 D=16 labels-in %s %s" % (form, side), (1, D, H, W), "D*S*4 = %d vs 2^31", D * H * W * 4):
        lab = block_labels(dev, H, W, 4316)
        e = torch.randn([1, D, H, W], generator=torch.Generator(device=dev).manual_seed(4317), device=dev)
        d = op.make_desc(spec_2d(pkg, offsets), e)
        sb = int(pkg._lib.lib().pea_labels_scratch_bytes(ctypes.byref(d)))
        assert (sb > 0) == (side == "under"), "the two-launch form's scratch: %d bytes" % sb
        # the entry itself: UNDER the limit it serves, AT it PEA_E_UNSUPPORTED before anything is launched (try_fused_labels ->
        # plan_tiles and xdma_labels_supported -> plan_xdma both refuse), so the wrapper's fall-back cannot stand in for it
        L, K = pkg._lib.lib(), len(offsets)
        flags = pkg._lib.TGT_PADDING | pkg._lib.TGT_MASK_INSIDE
        P = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        wtab, _, _ = op.label_weight_table(d, lab, flags, 1, K)
        work, wsb = op.workspace(dev, d)
        scratch = torch.empty(sb // 4, device=dev) if (form == "two_launch" and sb) else None
        affs_c, de_c = torch.full((1, K, H, W), -3.0, device=dev), torch.full_like(e, -3.0)
        lv_c = torch.full((1 + K,), -3.0, device=dev)
        rc = L.pea_affinity_fwd_bwd_labels_ex(ctypes.byref(d), P(e), None, P(lab), P(wtab), flags, P(affs_c), P(lv_c), None, P(de_c), P(work), wsb,
                                              P(scratch), sb if scratch is not None else 0, op._stream())
        torch.cuda.synchronize()
        print("pea_affinity_fwd_bwd_labels_ex rc = %d" % rc)
        if side == "under":
            assert rc == 0 and torch.isfinite(de_c).all() and de_c.abs().max() > 0
        else:
            assert rc == pkg._lib.E_UNSUPPORTED
            assert (de_c == -3.0).all() and (affs_c == -3.0).all() and (lv_c == -3.0).all()  # nothing was launched
        unit_de = de_c if rc == 0 else None
        del affs_c, lv_c, scratch, wtab

        def step(labels_in, t=None, w=None, m=None):
            et = e.clone().requires_grad_(True)
            loss, affs, _ = (pkg.embedding_loss_from_labels(et, lab, crit, offsets) if labels_in else pkg.embedding_loss(et, t, w, m, crit, offsets))
            (loss * 0.5).backward()
            return loss.detach().clone(), affs, et.grad

        l1, a1, g1 = step(True)
        l2, a2, g2 = step(True)
        assert torch.equal(l1, l2) and torch.equal(a1, a2) and torch.equal(g1, g2)
        del l2, a2, g2
        t, m, w = pkg.gen_targets(lab, offsets, padding=True)
        l0, a0, g0 = step(False, t, w, m)
        assert abs(l1.item() - l0.item()) <= 2e-6 * abs(l0.item())
        assert (a1 - a0).abs().max().item() < 2e-6
        dg = dev_relmax(g1, g0)
        print("labels-in vs tensor form: de rel-to-max %.3g" % dg)
        assert dg < 1e-5
        if unit_de is not None:  # the wrapper ran this entry: its gradient is the entry's for dloss = 1, times 0.5 (exact)
            assert torch.equal(g1, unit_de * 0.5)
        del lab, e, t, m, w, l1, a1, g1, l0, a0, g0, unit_de, de_c


# ----------------------------------------------------------------------------------------------------------------------------
# 2D, 16-bit storage, D = 64: the planners count 4 bytes per element whatever the storage
# ----------------------------------------------------------------------------------------------------------------------------
# the stored gradient is rounded to its storage type: f16 2e-3 (test_gpu_fullsize.py), bf16 8e-3 (test_gpu_bf16.py: three bits fewer)
GRAD_16BIT = {torch.float16: 2e-3, torch.bfloat16: 8e-3}
H64 = {"under": (2048, 4092), "at": (2048, 4096), "under8": (2048, 4088)}


@pytest.mark.parametrize("dtype,loss,side", [(torch.float16, "self", "under"), (torch.float16, "self", "at"), (torch.float16, "cross", "under"),
                                             (torch.float16, "cross", "at"), (torch.float16, "self", "under8"), (torch.float16, "cross", "under8"),
                                             (torch.bfloat16, "self", "under"), (torch.bfloat16, "self", "at")],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_2d_16bit_d64_block(pkg, dev, orc, monkeypatch, dtype, loss, side):
    """f16 / bf16 storage, D = 64, K = 8: D S 4 on either side of 2^31 although the tensor is 1 GiB.  The 16-bit cross kernels take rows
    of whole 8-element quads: they answer 1 at 2048 x 4088 (under8), 0 at 2048 x 4092 (the tiled kernels run) and 0 at 2048 x 4096.
    Peak 10.0 to 11.1 GiB over its cases (measured)"""
    H, W = H64[side]
    D = 64
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8]
    K = len(offsets)
    lam = [2.0 if i < 2 else 1.0 for i in range(K)] if loss == "cross" else [1.0] * K
    spec = spec_2d(pkg, offsets, lam)
    block = D * H * W * 4
    assert (block < LIMIT) == (side != "at")
    with case_report("2d %s D=64 %s %s" % (str(dtype)[6:], loss, side), (1, D, H, W), "D*S*4 = %d vs 2^31 (tensor: 2 bytes per element)", block):
        e, t, w, m = gpu_inputs(dev, 1, D, [H, W], K, 4164)
        e = e.to(dtype)
        eo = ema_of(dev, e, 4264) if loss == "cross" else None
        want = 1 if side == "under8" else 0
        assert cross_answers(pkg, spec, e, (0, 1, 2, 3, 4)) == [want] * 5
        gtol = GRAD_16BIT[dtype]
        l, a, _, g = default_vs_direct(pkg, spec, e, t, w, m, monkeypatch, 1.0, eo, gtol=gtol, direct_serves=side == "at")
        assert g.dtype == dtype
        windows_2d(orc, offsets, lam, 9, W, e, eo, t, w, m, a, g, 1.0, gtol=gtol)
        del e, t, w, m, eo, l, a, g


# ----------------------------------------------------------------------------------------------------------------------------
# the K block, 2D, f32, D = 16, K = 20
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,side", [("u8", "under"), ("u8", "at"), ("f32", "at")])
def test_2d_k20_block(pkg, dev, orc, monkeypatch, mask, side):
    """self loss, K = 20: under the limit one resource serves the K block; at it the tiled kernels reach channels 10 .. 19 of target,
    weight, mask, affs and g through the second resource (ksplit = 10).  The 2D counterpart of test_config3[n26], and the first case
    whose mask block is addressed at that size.  Peak 17.3 to 18.8 GiB over its cases (measured)"""
    H, W = (4096, 6552) if side == "under" else (4096, 6556)
    D = 16
    offsets = pkg.multi_offset(BBBC, 8)
    K = len(offsets)
    assert K == 20
    spec = spec_2d(pkg, offsets)
    block = K * H * W * 4
    assert (block < LIMIT) == (side == "under") and D * H * W * 4 < LIMIT and (K // 2) * H * W * 4 < LIMIT
    with case_report("2d f32 D=16 K=20 %s mask %s" % (mask, side), (1, K, H, W), "K*S*4 = %d vs 2^31", block):
        e, t, w, m = gpu_inputs(dev, 1, D, [H, W], K, 4120)
        if mask == "f32":
            m = m.float() * 0.75
        assert cross_answers(pkg, spec, e, (0, 1, 2, 5)) == [0] * 4  # K > the cross kernels' 10 offsets, on both sides
        l, a, _, g = default_vs_direct(pkg, spec, e, t, w, m, monkeypatch, 0.5)
        if mask == "f32":  # the oracle takes u8 masks: r = a m - t m under weight w is r = a - t under weight w m^2 (include/pea.h)
            w, m = w * m * m, None
        windows_2d(orc, offsets, [1.0] * K, max(BBBC), W, e, None, t, w, m, a, g, 0.5)
        del e, t, w, m, l, a, g


# ----------------------------------------------------------------------------------------------------------------------------
# 3D, f32, D = 16, CROP_ZERO, norm5
# ----------------------------------------------------------------------------------------------------------------------------
DIMS_3D = {"under": [32, 1024, 1020], "at": [32, 1024, 1024]}


def spec_3d(pkg, lam):
    ao = pkg.utils.affinity_ours
    offs = [list(o) for o in ao.axis_offsets_3d(ao.NORM5_SHIFTS)]
    return pkg.AffinitySpec(3, offs, lam, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_CROPPED), offs


def far_corner_vs_oracle(pkg, orc, spec, dims, e, eo, t, w, affs, grad, dloss):
    """the window that IS the far corner of the volume on three faces (all of z, the last 96 rows, the last 128 columns): compared
    wherever the window's own near faces do not matter (the mirror of test_gpu_fullsize.py:155-166)"""
    Z, Y, X = dims
    size = [Z, 96, 128]
    sl = (slice(0, 1), slice(None), slice(0, Z), slice(Y - 96, Y), slice(X - 128, X))
    cut = lambda x: None if x is None else np.ascontiguousarray(x[sl].cpu().numpy())
    ew, ow, tw, ww = cut(e), cut(eo), cut(t), cut(w)
    offs = [list(o) for o in spec.offsets]
    reach = [max(abs(o[a]) for o in offs) for a in range(3)]
    lam_w = [spec.lam[i] * float(np.prod(size)) / n for i, n in enumerate(full_norms(pkg, spec, 1, dims))]
    d = orc.make_desc(1, ew.shape[1], size, offs, lam_w, spec.border, orc.NORM_FULL, ndim=3)
    o_affs, _ = orc.c_fwd(d, ew, ow, tw, ww, None)
    o_grad, _ = orc.c_bwd(d, ew, ow, tw, ww, None, dloss=dloss)
    inner = (slice(None), slice(0, Z), slice(reach[1], 96), slice(reach[2], 128))
    ea = float(np.abs(affs[sl][0].cpu().numpy()[inner] - o_affs.reshape([len(offs)] + size)[inner]).max())
    eg = relmax(grad[sl][0].cpu().numpy()[inner], o_grad.reshape([ew.shape[1]] + size)[inner])
    print("far-corner window vs oracle: affs %.3g  de rel-to-max %.3g" % (ea, eg))
    assert ea < AFFS_ATOL, "far-corner window: affs differ from the oracle by %.3g" % ea
    assert eg < GRAD_RTOL, "far-corner window: de differs from the oracle by rel-to-max %.3g" % eg


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("loss", ["self", "cross"])
def test_3d_d16_block_training(pkg, dev, orc, monkeypatch, loss, side):
    """the training forward and backward (z-march, 3D cross kernels) and the cross loss on either side of the block limit.  Peak 15.9 to 18.0 GiB over its cases (measured)"""
    from test_gpu_fullsize import window_vs_oracle
    dims = DIMS_3D[side]
    D, K = 16, 12
    spec, offs = spec_3d(pkg, [2.0] * 3 + [1.0] * 9)
    block = D * int(np.prod(dims)) * 4
    assert (block < LIMIT) == (side == "under")
    with case_report("3d f32 D=16 %s %s" % (loss, side), [1, D] + dims, "D*S*4 = %d vs 2^31", block):
        e, t, w, _ = gpu_inputs(dev, 1, D, dims, K, 4303, mask=False)
        eo = ema_of(dev, e, 4403) if loss == "cross" else None
        want = 1 if side == "under" else 0
        assert cross_answers(pkg, spec, e, (0, 1, 2, 3)) == [want] * 4
        l, a, _, g = default_vs_direct(pkg, spec, e, t, w, None, monkeypatch, 2.0, eo, direct_serves=side == "at")
        window_vs_oracle(pkg, orc, spec, 1, dims, e, t, w, None, a, g, b=0, lo=[0, 480, 640], size=[dims[0], 80, 96], dloss=2.0, eo=eo)
        far_corner_vs_oracle(pkg, orc, spec, dims, e, eo, t, w, a, g, 2.0)
        del e, t, w, eo, l, a, g


@pytest.mark.parametrize("side", SIDES)
def test_3d_d16_block_inference_and_stitch(pkg, dev, orc, monkeypatch, side):
    """pea_affinity_infer (default against PEA_FORCE_DIRECT=1 over the whole map, twice bit for bit, the far corner against the oracle)
    and pea_affinity_infer_stitch into a stitched volume of the window's own size against pea_affinity_infer + pea_fill_border_relu +
    pea_stitch_add on the same window: bit for bit where pea_affinity_infer runs the direct kernels, whose arithmetic the fused kernel
    states, and within 1e-5 after pea_stitch_finalize on the default dispatch.  Peak 8.2 GiB (measured)"""
    dims = DIMS_3D[side]
    D, K = 16, 12
    spec, offs = spec_3d(pkg, None)
    with case_report("3d f32 D=16 infer + stitch %s" % side, [1, D] + dims, "D*S*4 = %d vs 2^31", D * int(np.prod(dims)) * 4):
        e = torch.randn([1, D] + dims, generator=torch.Generator(device=dev).manual_seed(4503), device=dev)
        monkeypatch.delenv("PEA_FORCE_DIRECT", raising=False)
        a1 = pkg.affinity_op.affinity_infer(e, None, spec)
        a2 = pkg.affinity_op.affinity_infer(e, None, spec)
        assert torch.equal(a1, a2)
        del a2
        monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
        try:
            a0 = pkg.affinity_op.affinity_infer(e, None, spec)
        finally:
            monkeypatch.delenv("PEA_FORCE_DIRECT", raising=False)
        da = (a1 - a0).abs().max().item()
        assert da < 2e-6, "infer, default vs PEA_FORCE_DIRECT=1: affs differ by %.3g" % da
        del a0
        Z, Y, X = dims
        sl = (slice(0, 1), slice(None), slice(0, Z), slice(Y - 96, Y), slice(X - 128, X))
        ew = np.ascontiguousarray(e[sl].cpu().numpy())
        d = orc.make_desc(1, D, [Z, 96, 128], offs, None, spec.border, orc.NORM_FULL, ndim=3)
        o_affs, _ = orc.c_fwd(d, ew, want_affs=True)
        inner = (slice(None), slice(0, Z), slice(27, 96), slice(27, 128))
        ea = float(np.abs(a1[sl][0].cpu().numpy()[inner] - o_affs.reshape(K, Z, 96, 128)[inner]).max())
        assert ea < AFFS_ATOL, "infer, far-corner window: affs differ from the oracle by %.3g" % ea
        del a1
        dd = pkg.affinity_op.make_desc(pkg.harness.stitch._with_relu(spec), e)
        assert pkg._lib.lib().pea_infer_stitch_supported(ctypes.byref(dd), 1) == 1  # a 64-bit gather: no block limit, on either side
        st = pkg.VolumeStitcher(K, dims, dims, dev)
        st.add_embedding(e, (0, 0, 0), spec=spec, shift=1, relu=True, fused=True)
        fused, fused_w = st.out_affs, st.weight_map
        # the fused kernel states the direct kernels' arithmetic (csrc/pea_k_infer_stitch.hip): the composition on them gives its bits
        st.reset_output()
        monkeypatch.setenv("PEA_FORCE_DIRECT", "1")
        try:
            st.add_embedding(e, (0, 0, 0), spec=spec, shift=1, relu=True, fused=False)
        finally:
            monkeypatch.delenv("PEA_FORCE_DIRECT", raising=False)
        assert torch.equal(st.weight_map, fused_w)
        assert torch.equal(st.out_affs, fused), "fused window vs infer (direct) + fill_border_relu + stitch_add"
        # the composition on the default dispatch (under the limit: the LDS kernels, which sum in another order), finalized: the bound
        # of test_gpu_infer_stitch.py::test_fused_vs_composed
        st.reset_output()
        st.add_embedding(e, (0, 0, 0), spec=spec, shift=1, relu=True, fused=False)
        assert torch.equal(st.weight_map, fused_w)
        composed = st.get_results((0, 0, 0))
        st.out_affs, st.weight_map = fused, fused_w
        err = (st.get_results((0, 0, 0)) - composed).abs().max().item()
        print("fused vs composed (default dispatch), finalized: max |difference| = %.3g" % err)
        assert err < AFFS_ATOL
        del e, st, fused, fused_w, composed
