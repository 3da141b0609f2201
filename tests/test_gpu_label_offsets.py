"""GPU (-m gpu): the integer and element-wise kernels past 4 GiB and past 2^31 elements.

The label kernels are exact, which allows a reference-free identity: ONE plane (or one small volume) from the existing case generators
is replicated B times on the device with expand(...).contiguous(); every item of every output must equal item 0 under torch.equal on
the device, and item 0 must equal the restatement's result for the one plane.  An item whose batch rebase `(size_t)b * ...` wrapped
at 2^32 bytes or 2^31 elements would read or write another item's place and break the identity.  Planes are 1024 x 1024, or the ragged
1021 x 1027 where a kernel's tile suggests it.  B is the one at which some B * S * elements array passes 2^31 ELEMENTS where that fits
under 40 GiB, else the smallest at which one array passes 2^32 BYTES (the docstring of the case says which).  The element-wise helpers
are compared, whole tensor, with the torch expression their existing tests use, on the device.

Cases (limits: 2^32 = 4 294 967 296 bytes, 2^31 = 2 147 483 648 elements; S = 1021 * 1027 = 1 048 567 or 2^20):

  targets   pea_gen_targets + pea_label_weights, K=10, with mask, 1021 x 1027, B=205:
            target, weight: 205 * 10 * 1 048 567 * 4 = 8 598 249 400 bytes > 2^32 (and 2 149 562 350 elements > 2^31);
            mask (u8): 2 149 562 350 elements > 2^31 (B=204: 2 139 076 680 < 2^31)
  cc        pea_cc_label, u8 in, labels and mask out, connectivity 2, min_size 25, 1024 x 1024, B=2049:
            B * S = 2 148 532 224 > 2^31 (B=2048 is exactly 2^31): 2 GiB in, 8 GiB labels, 2 GiB mask, the workspace about 16 GiB
  ws        pea_ws_seeds + pea_ws_flood, 171 planes of 1024 x 1024, with and without PEA_WS_STACK_IDS: past 2^31 pixels the workspaces
            alone would take 74 GiB, so N is the smallest at which an array passes 2^32 BYTES -- the workspace of pea_ws_flood
            (24.0 MiB a plane: 4.008 GiB; that of pea_ws_seeds is then 6.2 GiB)
  rag       pea_rag_build, K=3, boundary, capacity 1024, images of 1 x 1024 x 1024, B=683: affs 683 * 3 * 2^20 = 2 148 532 224 > 2^31;
            pea_rag_project, n = 2^31 + 4099 voxels in one call, then once with seg aliasing fragments
  scores    pea_seg_scores and pea_inst_scores, B=2049 pairs of 1024 x 1024 nuclei images: 2 148 532 224 > 2^31 pixels
  fgmask    pea_fgmask_loss_fwd / _bwd / _argmax, B=1025: logits 2 * 1025 * 2^20 = 2 149 580 800 > 2^31 elements
  disc      pea_disc_loss_fwd / _bwd, D=16, B=129: e 129 * 16 * 2^20 = 2 164 260 864 > 2^31 elements
  metrics   pea_affs_metrics, C=3, u8 mask, B=683: pred 2 148 532 224 > 2^31 elements
  scale     pea_scale_inplace, f32 and f16, n = 2^31 + 4099 elements (8 GiB / 4 GiB): a body of quads and a tail of three
  border    pea_fill_border_relu on [1, 3, 44, 4096, X]: each of its four launch routes (relu alone; the border alone; quads, X = 4096:
            3 * 44 * 2^24 = 2 214 592 512 elements; per voxel, X = 4094: 2 213 511 168 elements), all > 2^31
  crop      pea_affs_crop_zero on [1, 12, 46, 2048, 2050], norm5's offsets: 12 * 193 126 400 = 2 317 516 800 elements > 2^31
  unflip    pea_consistency_unflip, f16 [130, 16, 1024, 1024]: 2 181 038 080 elements > 2^31 (B=128 is exactly 2^31), all eight rules
  stitch    pea_stitch_add + pea_stitch_finalize at C = 12, a volume of 2^28 + 4099 voxels (1 x 1 x voxels: the AC3 volume's size class):
            out_affs 12 * 268 439 555 * 4 = 12 885 098 640 bytes, c * S + i passes 2^31 from channel 8 on

Every case prints its shape, the crossed limit, its peak device memory and its run time.

Measured on an MI355X (case, shape, peak device memory of the case, run time inside the case; in some runs one or two cases,
not the same ones each time, took 5 to 6 s instead):

  gen_targets + label_weights K=10 B=205         205x10x1021x1027          18.97 GiB   0.05 s
  cc_label conn 2 min_size 25 B=2049             2049x1024x1024            28.28 GiB   1.77 s
  scale_inplace float32                          2147487747                18.00 GiB   0.01 s
  scale_inplace float16                          2147487747                20.00 GiB   0.02 s
  fill_border_relu relu_alone                    1x3x44x4096x4096          18.56 GiB   0.03 s
  fill_border_relu border_alone                  1x3x44x4096x4096          18.56 GiB   2.73 s
  fill_border_relu quads                         1x3x44x4096x4096          18.56 GiB   0.02 s
  fill_border_relu per_voxel                     1x3x44x4096x4094          18.55 GiB   0.02 s
  affs_crop_zero norm5                           1x12x46x2048x2050         19.43 GiB   0.01 s
  consistency_unflip f16                         130x16x1024x1024          15.22 GiB   0.06 s
  stitch_add + stitch_finalize C=12              12x268439555              35.50 GiB   0.07 s
  ws_seeds + ws_flood N=171                      171x1024x1024             17.20 GiB   1.68 s
  rag_build K=3 B=683                            683x3x1x1024x1024         13.40 GiB   0.04 s
  rag_project                                    2147487747                22.25 GiB   0.22 s
  seg_scores B=2049                              2049x1024x1024            16.17 GiB   0.08 s
  inst_scores B=2049                             2049x1024x1024            16.11 GiB   0.08 s
  fgmask loss + argmax B=1025                    1025x2x1024x1024          21.17 GiB   0.02 s
  disc loss B=129                                129x16x1024x1024          16.82 GiB   4.22 s
  affs_metrics B=683                             683x3x1024x1024           18.04 GiB   0.01 s
"""
import ctypes

import numpy as np
import pytest
import torch

import cc_reference as ccr
import targets_reference as tr
from test_gpu_block_edges import BBBC, case_report

pytestmark = pytest.mark.gpu
P32, E31 = 1 << 32, 1 << 31


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def every_item_is_item_0(name, x, chunk=16):
    """x[b] == x[0] for every b, on the device, a few items at a time (no temporary of x's size)"""
    for b0 in range(0, x.shape[0], chunk):
        part = x[b0:b0 + chunk]
        assert torch.equal(part, x[:1].expand_as(part)), "%s: an item in %d..%d differs from item 0" % (name, b0, b0 + part.shape[0] - 1)


def drop_stream_workspaces(pkg, family):
    """forget the per-stream scratch block of `family` (affinity_op.stream_workspace keeps one per stream for reuse: here 16 GiB)"""
    ws = pkg.affinity_op._WS
    for k in [k for k in ws if k[0] == family]:
        del ws[k]


def same_bits(a, b):
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ----------------------------------------------------------------------------------------------------------------------------
# pea_gen_targets + pea_label_weights
# ----------------------------------------------------------------------------------------------------------------------------
def test_gen_targets_and_label_weights_past_2_31(pkg, dev):
    """target / weight past 2^32 bytes and 2^31 elements, the u8 mask past 2^31 elements.  Peak 19.0 GiB (measured)"""
    B, Y, X = 205, 1021, 1027
    offsets = pkg.multi_offset(BBBC, 4)
    K = len(offsets)
    S = Y * X
    assert B * K * S > E31 and (B - 1) * K * S <= E31 and B * K * S * 4 > P32
    flags = pkg._lib.TGT_PADDING
    synth = tr._synth()
    plane = synth.synth_labels(1, (1, Y, X), 7100, cell=37, n=40).astype(np.int32)  # [1, 1, Y, X]
    t_ref, m_ref, w_ref, wtab_ref, _ = tr.targets_reference(plane, offsets, flags)
    with case_report("gen_targets + label_weights K=10 B=205", (B, K, Y, X), "mask elements = %d vs 2^31", B * K * S):
        lab = torch.from_numpy(plane[0]).to(dev).expand(B, Y, X).contiguous()
        t, m, w = pkg.gen_targets(lab, offsets, padding=True)
        for name, x, ref in (("target", t, t_ref), ("mask", m, m_ref), ("weight", w, w_ref)):
            every_item_is_item_0(name, x)
            assert np.array_equal(x[0].cpu().numpy(), ref[0, :, 0]), name
        del t, m, w
        op = pkg.affinity_op
        spec = op.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_FULL)
        d = pkg.utils.targets._targets_desc(spec, lab)
        wtab, _, _ = op.label_weight_table(d, lab, flags, B, K)
        wtab = wtab.reshape(B, K, 2)
        every_item_is_item_0("wtab", wtab, chunk=B)
        assert np.array_equal(wtab[0].cpu().numpy(), wtab_ref[0])
        del lab, wtab


# ----------------------------------------------------------------------------------------------------------------------------
# pea_cc_label
# ----------------------------------------------------------------------------------------------------------------------------
def cc_plane():
    """1024 x 1024 from the named 2D cases (70 x 150 each), tiled with gaps, plus a strip of random pixels: components
    inside one 32 x 32 tile, across tile borders, of fewer and of more than 25 pixels"""
    cases = ccr.cases_2d()
    names = ["sized", "serpentine", "spiral", "rings", "comb", "u_shape", "random_0.3", "random_0.59", "checkerboard", "random_0.8"]
    plane = np.zeros((1024, 1024), np.uint8)
    k = 0
    for y0 in range(3, 1024 - 70, 77):
        for x0 in range(5, 1024 - 150, 161):
            plane[y0:y0 + 70, x0:x0 + 150] = cases[names[k % len(names)]]
            k += 1
    plane[:, 980:] = ccr.random_mask(41, 0.45, (1024, 44))
    return plane


def test_cc_label_past_2_31_pixels(pkg, dev):
    """B * S past 2^31 pixels: labels (int32) past 2^33 bytes.  Peak 28.3 GiB (measured)"""
    B, Y, X = 2049, 1024, 1024
    assert B * Y * X > E31 and (B - 1) * Y * X <= E31
    plane = cc_plane()
    lab_ref, cnt_ref = ccr.cc_reference_batch(plane[None], 2, 25)
    assert cnt_ref[0, 0] > cnt_ref[0, 1] > 100  # min_size drops some, keeps many
    with case_report("cc_label conn 2 min_size 25 B=2049", (B, Y, X), "pixels = %d vs 2^31", B * Y * X):
        x = torch.from_numpy(plane).to(dev).expand(B, Y, X).contiguous()
        cc = pkg.harness.cc.connected_components(x, connectivity=2, min_size=25, mask=True)
        torch.cuda.synchronize()
        every_item_is_item_0("labels", cc.labels, chunk=64)
        every_item_is_item_0("mask", cc.mask, chunk=256)
        every_item_is_item_0("counts", cc.counts, chunk=B)
        assert np.array_equal(cc.labels[0].cpu().numpy(), lab_ref[0])
        assert np.array_equal(cc.counts[0].cpu().numpy(), cnt_ref[0])
        assert torch.equal(cc.mask[B - 1], (cc.labels[B - 1] != 0).to(torch.uint8))
        del x, cc
        drop_stream_workspaces(pkg, "cc")


# ----------------------------------------------------------------------------------------------------------------------------
# the element-wise helpers
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_scale_inplace_past_2_31(pkg, dev, dtype):
    """buf *= scale over 2^31 + 4099 elements against (x.float() * sc).to(dtype), bit for bit (test_gpu_helpers.py).  Peak 18.0 to 20.0 GiB over its cases (measured)"""
    n = E31 + 4099
    code = {torch.float32: 0, torch.float16: 1}[dtype]
    sc = -3.5
    with case_report("scale_inplace %s" % str(dtype)[6:], (n,), "elements = %d vs 2^31", n):
        x = torch.randn(n, generator=torch.Generator(device=dev).manual_seed(7200), device=dev, dtype=dtype)
        want = (x.float() * sc).to(dtype) if dtype != torch.float32 else x * sc
        s = torch.tensor([sc], device=dev)
        pkg._lib.check(pkg._lib.lib().pea_scale_inplace(vp(x), code, ctypes.c_size_t(n), vp(s), stream()), "pea_scale_inplace")
        torch.cuda.synchronize()
        assert same_bits(x, want)
        assert x[-1].item() == want[-1].item() and want[-1].item() != 0
        del x, want


def torch_fill_border_relu(pred, shift, relu):
    if shift:
        K = pred.shape[1]
        pred[:, 0, :shift] = pred[:, 0, shift:2 * shift]
        if K > 1:
            pred[:, 1, :, :shift] = pred[:, 1, :, shift:2 * shift]
        if K > 2:
            pred[:, 2, :, :, :shift] = pred[:, 2, :, :, shift:2 * shift]
    return torch.relu_(pred) if relu else pred


@pytest.mark.parametrize("route,X,shift,relu", [("relu_alone", 4096, 0, True), ("border_alone", 4096, 1, False), ("quads", 4096, 1, True),
                                                ("per_voxel", 4094, 1, True)])
def test_fill_border_relu_past_2_31(pkg, dev, route, X, shift, relu):
    """each launch route of pea_fill_border_relu (csrc/pea_k_direct.hip) on a map of more than 2^31 elements, against the three slice
    statements and F.relu on the device.  Peak 18.6 GiB (measured)"""
    B, K, Z, Y = 1, 3, 44, 4096
    n = B * K * Z * Y * X
    assert n > E31
    with case_report("fill_border_relu %s" % route, (B, K, Z, Y, X), "elements = %d vs 2^31", n):
        a = torch.randn([B, K, Z, Y, X], generator=torch.Generator(device=dev).manual_seed(7300), device=dev)
        want = torch_fill_border_relu(a.clone(), shift, relu)
        assert pkg.utils.postproc.fill_border_relu_(a, shift=shift, relu=relu) is a
        torch.cuda.synchronize()
        assert same_bits(a, want)
        if relu:
            assert a[0, K - 1, Z - 1, Y - 1].min().item() == 0.0 and a[0, K - 1, Z - 1, Y - 1].max().item() > 0
        del a, want


def test_affs_crop_zero_past_2_31(pkg, dev):
    """+0.0 on every cropped-away pair of norm5's twelve offsets, nothing else touched, on a map of 2.3 G elements.  Peak 19.4 GiB (measured)"""
    ao = pkg.utils.affinity_ours
    offs = [list(o) for o in ao.axis_offsets_3d(ao.NORM5_SHIFTS)]
    B, K, Z, Y, X = 1, len(offs), 46, 2048, 2050
    n = B * K * Z * Y * X
    assert n > E31
    with case_report("affs_crop_zero norm5", (B, K, Z, Y, X), "elements = %d vs 2^31", n):
        a = torch.randn([B, K, Z, Y, X], generator=torch.Generator(device=dev).manual_seed(7400), device=dev)
        want = a.clone()
        for k, o in enumerate(offs):
            for ax in range(3):
                if o[ax]:
                    sl = [slice(None)] * 3
                    sl[ax] = slice(0, -o[ax]) if o[ax] < 0 else slice(want.shape[2 + ax] - o[ax], None)
                    want[(0, k) + tuple(sl)] = 0.0
        assert pkg.affs_crop_zero_(a, offs) is a
        torch.cuda.synchronize()
        assert same_bits(a, want)
        assert (a[0, K - 1, :, :, :27] == 0).all() and a[0, K - 1, Z - 1, Y - 1, X - 1].item() != 0
        del a, want


def test_consistency_unflip_past_2_31(pkg, dev):
    """all eight rule triples over a batch of 2.18 G f16 elements against the reference's composition on views.  Peak 15.2 GiB (measured)"""
    B, C, Hh, Ww = 130, 16, 1024, 1024
    n = B * C * Hh * Ww
    assert n > E31
    with case_report("consistency_unflip f16", (B, C, Hh, Ww), "elements = %d vs 2^31", n):
        x = torch.randn([B, C, Hh, Ww], generator=torch.Generator(device=dev).manual_seed(7500), device=dev, dtype=torch.float16)
        rules = np.array([[(b >> 0) & 1, (b >> 1) & 1, (b >> 2) & 1] for b in range(B)], np.uint8)
        rules[B - 1] = (1, 1, 1)
        out = pkg.affinity_op.unflip(x, torch.from_numpy(rules).to(dev))
        want = pkg.harness.train_step._torch_unflip(x, rules)
        torch.cuda.synchronize()
        assert same_bits(out, want)
        del x, out, want


def test_stitch_add_and_finalize_at_the_ac3_size_class(pkg, dev):
    """C = 12, 2^28 + 4099 voxels: out_affs of 12.9 GB.  A window over the far half of the volume, off every 16-byte boundary, and a
    second, ragged one over its last voxels: the highest addresses of every channel.  out += vol * w and wmap += w with product and sum
    rounded separately, then out / wmap: the torch statements on the device, channel by channel, bit for bit (test_gpu_helpers.py).
    Peak 35.5 GiB (measured)"""
    L = pkg._lib.lib()
    C, V = 12, (1 << 28) + 4099
    assert C * V > E31 and C * V * 4 > P32
    with case_report("stitch_add + stitch_finalize C=12", (C, V), "out_affs elements = %d vs 2^31", C * V):
        g = torch.Generator(device=dev).manual_seed(7600)
        out = torch.randn([C, 1, 1, V], generator=g, device=dev)
        wmap = torch.rand([1, 1, V], generator=g, device=dev) + 0.1
        want, want_w = out.clone(), wmap.clone()
        for x0 in ((1 << 27) - 5, V - 4099 - 777):
            n = V - x0
            vol = torch.randn([C, 1, 1, n], generator=g, device=dev)
            wv = torch.rand([1, 1, n], generator=g, device=dev) + 0.05
            for c in range(C):  # (torch rounds the product and the sum separately)
                want[c, ..., x0:] = want[c, ..., x0:] + vol[c] * wv
            want_w[..., x0:] = want_w[..., x0:] + wv
            pkg._lib.check(L.pea_stitch_add(vp(out), vp(wmap), vp(vol), vp(wv), C, 1, 1, V, 1, 1, n, 0, 0, x0, stream()), "pea_stitch_add")
            torch.cuda.synchronize()
            assert same_bits(out, want) and same_bits(wmap, want_w), x0
            del vol, wv
        del want_w
        for c in range(C):
            want[c] = want[c] / wmap
        pkg._lib.check(L.pea_stitch_finalize(vp(out), vp(wmap), C, ctypes.c_size_t(V), stream()), "pea_stitch_finalize")
        torch.cuda.synchronize()
        assert same_bits(out, want)
        assert torch.isfinite(out[C - 1, 0, 0, -4099:]).all()
        del out, want, wmap


# ----------------------------------------------------------------------------------------------------------------------------
# pea_ws_seeds + pea_ws_flood
# ----------------------------------------------------------------------------------------------------------------------------
def test_watershed_workspaces_past_4gib(pkg, dev):
    """N = 171 planes of 1024 x 1024.  B * S past 2^31 elements would need 37 MB of workspace per plane times 2049 planes (74 GiB), so N
    is the smallest at which an array passes 2^32 bytes: the WORKSPACE of pea_ws_flood (24.0 MiB a plane: 171 planes = 4.008 GiB; that
    of pea_ws_seeds, 36.1 MiB a plane, is then 6.2 GiB).  Every plane of seeds / dt2 / dts / hmap / labels equals plane 0; plane 0
    against the restatement as test_gpu_ws.py holds it (dt2, seeds, labels exact; dts, hmap within the arithmetic's bounds); with
    PEA_WS_STACK_IDS plane n = plane 0 + n * kept.  Peak 17.2 GiB (measured)"""
    import test_gpu_ws as tw
    import ws_reference as R
    N, Y, X = 171, 1024, 1024
    synth = tr._synth()
    b, _ = synth.synth_membranes(1, Y, X, 240, seed=21, gap=2, gaps_per_plane=6)
    L = pkg._lib.lib()
    hw = pkg.harness.ws
    L.pea_ws_seeds_workspace_bytes.restype = L.pea_ws_flood_workspace_bytes.restype = ctypes.c_size_t
    with case_report("ws_seeds + ws_flood N=171", (N, Y, X), "flood workspace bytes = %d vs 2^32",
                     int(L.pea_ws_flood_workspace_bytes(ctypes.byref(hw._desc(torch.empty((N, Y, X), device="meta"), min_size=20))))):
        Bd = torch.from_numpy(b[0]).to(dev).expand(N, Y, X).contiguous()
        d = hw._desc(Bd, .25, 2., 2., .9)
        assert int(L.pea_ws_seeds_workspace_bytes(ctypes.byref(d))) > P32
        assert int(L.pea_ws_flood_workspace_bytes(ctypes.byref(hw._desc(Bd, min_size=20)))) > P32
        s = pkg.watershed_seeds(Bd, .25, 2., 2., .9)
        for name in ("seeds", "dt2", "dts", "hmap", "counts"):
            every_item_is_item_0(name, getattr(s, name), chunk=32)
        dt2 = R.dt2_reference(b, .25)
        assert np.array_equal(s.dt2[0].cpu().numpy(), dt2[0])
        tol_s, tol_w = tw.tolerances(b, dt2, 2., 2., .9)
        dts0, hmap0 = s.dts[:1].cpu().numpy(), s.hmap[:1].cpu().numpy()
        assert (np.abs(dts0.astype(np.float64) - R.dts_reference(dt2, 2.)) <= tol_s).all()
        assert (np.abs(hmap0.astype(np.float64) - R.hmap_reference(b, dt2, 2., .9)) <= tol_w).all()
        rs, rc = R.seeds_reference(dts0, 2, 1)  # on the device's own dts
        assert np.array_equal(s.seeds[0].cpu().numpy(), rs[0]) and s.counts[0].item() == rc[0] > 100
        w = pkg.seeded_watershed(s.hmap, s.seeds, min_size=20)
        for name in ("labels", "counts", "stats"):
            every_item_is_item_0(name, getattr(w, name), chunk=32)
        ref_l, ref_c, _ = R.flood_reference(hmap0, rs, 20)
        assert np.array_equal(w.labels[0].cpu().numpy(), ref_l[0]) and w.counts[0].tolist() == ref_c[0].tolist()
        kept = int(ref_c[0, 1])
        ws = pkg.seeded_watershed(s.hmap, s.seeds, min_size=20, stack_ids=True)
        assert torch.equal(ws.counts, w.counts)
        step = (torch.arange(N, device=dev, dtype=torch.int32) * kept)[:, None, None]
        assert torch.equal(ws.labels, torch.where(w.labels > 0, w.labels + step, torch.zeros_like(w.labels)))
        assert int(ws.labels[N - 1].max()) == N * kept
        del Bd, s, w, ws
        drop_stream_workspaces(pkg, "ws_seeds")
        drop_stream_workspaces(pkg, "ws_flood")


# ----------------------------------------------------------------------------------------------------------------------------
# pea_rag_build + pea_rag_project
# ----------------------------------------------------------------------------------------------------------------------------
def test_rag_build_past_2_31_samples(pkg, dev):
    """K = 3, boundary, capacity 1024, images of 1 x 1024 x 1024, B = 683: affs holds 683 * 3 * 2^20 = 2 148 532 224 samples > 2^31
    (B=682: 2 145 386 496), 8 GiB.  Every row of every table equals image 0's; image 0 against the restatement (test_gpu_rag.compare).
    Peak 13.4 GiB (measured)"""
    import rag_reference as rr
    import test_gpu_rag as tg
    B, Y, X, K = 683, 1024, 1024, 3
    assert B * K * Y * X > E31 and (B - 1) * K * Y * X <= E31
    offs = [[0, -1, 0], [0, 0, -1], [0, -3, 0]]
    rng = np.random.default_rng(7700)
    frag = tr._synth().synth_labels(1, (1, Y, X), 7701, cell=37, n=20).astype(np.int32)  # [1, 1, Y, X]
    affs = rng.random((1, K, 1, Y, X), dtype=np.float32)
    bnd = rng.random((1, 1, Y, X), dtype=np.float32)
    M = int(frag.max())
    ref = rr.rag_reference_batch(frag, affs, offs, bnd, max_id=M)
    assert 50 < len(ref[0]["uv"]) < 512
    with case_report("rag_build K=3 B=683", (B, K, 1, Y, X), "affs samples = %d vs 2^31", B * K * Y * X):
        F = torch.from_numpy(frag).to(dev).expand(B, 1, Y, X).contiguous()
        A = torch.from_numpy(affs).to(dev).expand(B, K, 1, Y, X).contiguous()
        Bd = torch.from_numpy(bnd).to(dev).expand(B, 1, Y, X).contiguous()
        t = pkg.region_adjacency(F, A, offs, Bd, max_id=M, capacity=1024, max_edges=512, batched=True).tensors
        torch.cuda.synchronize()
        for name, x in t.items():
            every_item_is_item_0(name, x, chunk=B)
        tg.compare("image 0 of 683", {k: v[:1].cpu().numpy() for k, v in t.items()}, ref)
        del F, A, Bd, t
        drop_stream_workspaces(pkg, "rag")


def test_rag_project_past_2_31_voxels(pkg, dev):
    """seg[p] = node_labels[fragments[p]] over n = 2^31 + 4099 voxels in ONE call (8 GiB in, 8 GiB out), against torch's gather in
    chunks; ids that are no node give 0 and are counted; then once more with seg aliasing fragments.  Peak 22.2 GiB (measured)"""
    L = pkg._lib.lib()
    n, M = E31 + 4099, 1000
    with case_report("rag_project", (n,), "voxels = %d vs 2^31", n):
        g = torch.Generator(device=dev).manual_seed(7800)
        F = torch.randint(-2, M + 3, (n,), generator=g, device=dev, dtype=torch.int32)
        N = torch.randint(1, 1 << 30, (M,), generator=g, device=dev, dtype=torch.int32)
        seg = torch.full((n,), -9, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        pkg._lib.check(L.pea_rag_project(n, vp(F), vp(N), M, vp(seg), vp(bad), stream()), "pea_rag_project")
        torch.cuda.synchronize()
        n_bad = 0
        for lo in range(0, n, 1 << 28):
            f = F[lo:lo + (1 << 28)].long()
            ok = (f >= 0) & (f < M)
            want = torch.where(ok, N[f.clamp(0, M - 1)], torch.zeros_like(N[:1]))
            assert torch.equal(seg[lo:lo + (1 << 28)], want), lo
            n_bad += int((~ok).sum())
        assert int(bad) == n_bad > 0 and seg[-1].item() == (N[F[-1]].item() if 0 <= F[-1].item() < M else 0)
        pkg._lib.check(L.pea_rag_project(n, vp(F), vp(N), M, vp(F), None, stream()), "pea_rag_project")  # in place
        torch.cuda.synchronize()
        assert torch.equal(F, seg)
        del F, seg


# ----------------------------------------------------------------------------------------------------------------------------
# pea_seg_scores, pea_inst_scores
# ----------------------------------------------------------------------------------------------------------------------------
def nuclei_pair():
    synth = tr._synth()
    gt = synth.synth_nuclei(1, 1024, 1024, 70, 30, 7900)
    pred = synth.synth_nuclei(1, 1024, 1024, 66, 30, 7900, specks=12)  # the same centres, two fewer discs, some specks
    return pred.astype(np.int32), gt.astype(np.int32)


@pytest.mark.parametrize("which", ["seg", "inst"])
def test_scores_past_2_31_pixels(pkg, dev, which):
    """pea_seg_scores / pea_inst_scores on B = 2049 copies of one 1024 x 1024 pair of nuclei images: pred and gt hold B * S =
    2 148 532 224 > 2^31 pixels (8 GiB each).  The headers promise per-image rows: every row (and every row of the match tables) equals
    row 0 bit for bit, and row 0 meets the restatement at the bars of test_gpu_segscore.py / test_gpu_instscore.py.  Peak 16.1 to 16.2 GiB over its cases (measured)"""
    B = 2049
    pred, gt = nuclei_pair()
    assert B * pred[0].size > E31
    with case_report("%s_scores B=2049" % which, (B, 1024, 1024), "pixels = %d vs 2^31", B * pred[0].size):
        P = torch.from_numpy(pred).to(dev).expand(B, 1024, 1024).contiguous()
        G = torch.from_numpy(gt).to(dev).expand(B, 1024, 1024).contiguous()
        if which == "seg":
            import test_gpu_segscore as ts
            from segscore_reference import seg_reference
            sc = pkg.harness.segscore.segmentation_scores(P, G, capacity=1024, batched=True)
            torch.cuda.synchronize()
            assert same_bits(sc.table, sc.table[:1].expand_as(sc.table).contiguous())
            ts.close("image 0 of 2049", sc.table[:1], seg_reference(pred.reshape(1, -1), gt.reshape(1, -1)))
            drop_stream_workspaces(pkg, "seg")
        else:
            import test_gpu_instscore as ti
            from instscore_reference import inst_reference
            out, match = pkg.harness.instscore._launch(P.reshape(B, -1), G.reshape(B, -1), 1024, 128, 0.5)
            torch.cuda.synchronize()
            assert same_bits(out, out[:1].expand_as(out).contiguous())
            every_item_is_item_0("aji_match", match[0], chunk=B)
            every_item_is_item_0("pq_match", match[1], chunk=B)
            ref, ram, rpm = inst_reference(pred.reshape(1, -1), gt.reshape(1, -1), 128)
            ti.close("image 0 of 2049", out[:1], ref)
            assert np.array_equal(match[0, :1].cpu().numpy(), ram) and np.array_equal(match[1, :1].cpu().numpy(), rpm)
            drop_stream_workspaces(pkg, "inst")
        del P, G


# ----------------------------------------------------------------------------------------------------------------------------
# the losses and metrics that give a BATCH MEAN: equal to their B = 1 value within the bound of the kernel's own GPU test
# ----------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_fgmask_loss_and_argmax_past_2_31(pkg, dev):
    """pea_fgmask_loss_fwd / _bwd / _argmax on B = 1025 copies of one 1024 x 1024 image: logits and dlogits hold 2 * 1025 * 2^20 =
    2 149 580 800 > 2^31 elements (8 GiB each).  The loss is a batch mean of class means: B copies give the B = 1 loss (rel 1e-5,
    test_gpu_fgmask.py); dlogits of every image equals image 0's bit for bit and, times B, the B = 1 gradient (1e-4 of its maximum);
    the argmax mask of every image equals image 0's and [l1 > l0].  Peak 21.2 GiB (measured)"""
    B, Y, X = 1025, 1024, 1024
    n = B * 2 * Y * X
    assert n > E31 and (B - 1) * 2 * Y * X <= E31
    fg = pkg.harness.fgmask
    lab1 = torch.from_numpy(nuclei_pair()[1]).to(dev)
    with case_report("fgmask loss + argmax B=1025", (B, 2, Y, X), "logits elements = %d vs 2^31", n):
        lg1 = torch.randn([1, 2, Y, X], generator=torch.Generator(device=dev).manual_seed(8000), device=dev)
        x1 = lg1.clone().requires_grad_(True)
        loss1, stats1 = fg.foreground_mask_loss(x1, lab1)
        loss1.backward()
        x = lg1.expand(B, 2, Y, X).contiguous().requires_grad_(True)
        lab = lab1.expand(B, Y, X).contiguous()
        loss, stats = fg.foreground_mask_loss(x, lab)
        loss.backward()
        torch.cuda.synchronize()
        print("fgmask loss B=1025 %.9g, B=1 %.9g" % (loss.item(), loss1.item()))
        assert rel(loss, loss1) <= 1e-5 and rel(stats[1], stats1[1]) <= 1e-5 and rel(stats[2], stats1[2]) <= 1e-5
        assert stats[3].item() == B * stats1[3].item() and stats[4].item() == B * stats1[4].item()
        every_item_is_item_0("dlogits", x.grad, chunk=32)
        top = x1.grad.abs().max().item()
        assert ((x.grad[B - 1] * B - x1.grad[0]).abs().max().item()) <= 1e-4 * top and top > 0
        m = fg.foreground_mask(x.detach())
        every_item_is_item_0("argmax", m, chunk=128)
        assert torch.equal(m[B - 1], (lg1[0, 1] > lg1[0, 0]).to(torch.uint8))
        del x, lab, m
        drop_stream_workspaces(pkg, "fgmask")


def test_disc_loss_past_2_31(pkg, dev):
    """pea_disc_loss_fwd / _bwd on B = 129 copies of one 1024 x 1024 image at D = 16: e and de hold 129 * 16 * 2^20 = 2 164 260 864 >
    2^31 elements (8 GiB each).  The per-image stats (var_b, dist_b, reg_b, C_b) of every image equal image 0's bit for bit, and so does
    de; the loss, a batch mean, equals the B = 1 loss (rel 1e-5, test_gpu_disc.py) and de times B the B = 1 gradient (1e-4 of its
    maximum).  Peak 16.8 GiB (measured)"""
    B, D, Y, X = 129, 16, 1024, 1024
    n = B * D * Y * X
    assert n > E31 and (B - 1) * D * Y * X <= E31
    hd = pkg.harness.disc
    lab1 = torch.from_numpy(nuclei_pair()[1]).to(dev)
    with case_report("disc loss B=129", (B, D, Y, X), "e elements = %d vs 2^31", n):
        e1 = torch.randn([1, D, Y, X], generator=torch.Generator(device=dev).manual_seed(8100), device=dev)
        x1 = e1.clone().requires_grad_(True)
        loss1, stats1 = hd.discriminative_loss_stats(x1, lab1, num_ids=128)
        loss1.backward()
        x = e1.expand(B, D, Y, X).contiguous().requires_grad_(True)
        loss, stats = hd.discriminative_loss_stats(x, lab1.expand(B, Y, X).contiguous(), num_ids=128)
        loss.backward()
        torch.cuda.synchronize()
        print("disc loss B=129 %.9g, B=1 %.9g" % (loss.item(), loss1.item()))
        assert stats[4].item() == 0 and rel(loss, loss1) <= 1e-5
        for c in (1, 2, 3):
            assert rel(stats[c], stats1[c]) <= 1e-5, c
        per = stats[5:].reshape(B, 4)
        assert torch.equal(per, per[:1].expand_as(per)) and torch.equal(per[0], stats1[5:9]) and per[0, 3].item() > 10
        every_item_is_item_0("de", x.grad, chunk=8)
        top = x1.grad.abs().max().item()
        assert ((x.grad[B - 1] * B - x1.grad[0]).abs().max().item()) <= 1e-4 * top and top > 0
        del x
        drop_stream_workspaces(pkg, "disc")


def test_affs_metrics_past_2_31(pkg, dev):
    """pea_affs_metrics on B = 683 copies of one [3, 1024, 1024] map with a u8 mask: pred and target hold 2 148 532 224 > 2^31 elements
    (8 GiB each).  mse and bce are means over the batch: the B = 1 values within rel 1e-5 (test_gpu_metrics.py); tp, fp, fn are exact
    counts: B times those of the one map.  Peak 18.0 GiB (measured)"""
    B, C, Y, X = 683, 3, 1024, 1024
    n = B * C * Y * X
    assert n > E31 and (B - 1) * C * Y * X <= E31
    hm = pkg.harness.metrics
    with case_report("affs_metrics B=683", (B, C, Y, X), "pred elements = %d vs 2^31", n):
        g = torch.Generator(device=dev).manual_seed(8200)
        p1 = torch.rand([1, C, Y, X], generator=g, device=dev) * 1.2 - 0.1
        t1 = (torch.rand([1, C, Y, X], generator=g, device=dev) < 0.7).float()
        m1 = (torch.rand([1, C, Y, X], generator=g, device=dev) < 0.9).to(torch.uint8)
        one = hm.affinity_metrics(p1, t1, m1, relu=True).table.clone()
        many = hm.affinity_metrics(p1.expand(B, C, Y, X).contiguous(), t1.expand(B, C, Y, X).contiguous(), m1.expand(B, C, Y, X).contiguous(),
                                   relu=True).table
        torch.cuda.synchronize()
        a, b = many.cpu().numpy(), one.cpu().numpy()
        print("affs_metrics B=683", a[0].tolist(), "B=1", b[0].tolist())
        assert (np.abs(a[:, :2] - b[:, :2]) <= 1e-5 * np.abs(b[:, :2])).all() and (b[:, :2] > 0).all()
        assert np.array_equal(a[:, 2:], B * b[:, 2:]) and (b[0, 2:] > 0).all()
        drop_stream_workspaces(pkg, "metrics")
