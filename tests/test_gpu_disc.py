"""GPU: the discriminative instance loss (include/pea_disc.h, csrc/pea_k_disc.hip) through the C ABI and through discriminative_loss /
discriminative_loss_stats / CvpppTrainStep(disc_weight=..), against the reference's own numbers (tests/golden/gdisc_*.npz) and the
float64 restatement tests/disc_reference.py (which test_disc_host.py holds to those numbers).

Tolerances are the project's f32 bars (tests/test_gpu_parity.py): the loss and each of var / dist / reg 1e-5 relative, the gradient
1e-4 of the largest reference magnitude.  C_b, n_bad and everything called bit-identical are compared exactly.  The loss is C^1 (a
squared hinge), so no pixel is left out of any comparison.  Every C call of this file also checks that the workspace is all zero
afterwards but for its magic word, and starts from a ctx, stats and loss filled with a pattern."""
import copy
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from arena import Arena
from disc_reference import disc_reference, load_disc_golden

pytestmark = pytest.mark.gpu
RTOL_LOSS, RTOL_GRAD = 1e-5, 1e-4
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
BACKGROUND, NEED_GRAD = 1, 2
GOLDENS = ("gdisc_2d_b3_37x53", "gdisc_2d_b3_37x53_bg", "gdisc_3d_b2_5x20x24", "gdisc_d5")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


def all_same(x, y):
    return all(same_bits(a, b) for a, b in zip(x, y))


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_desc(pkg, e, num_ids, flags=NEED_GRAD, params=(0.5, 1.5, 1.0, 1.0, 0.001)):
    d = pkg._lib.PeaDiscDesc()
    d.B, d.D, d.S = e.shape[0], e.shape[1], e[0, 0].numel()
    d.num_ids, d.flags = num_ids, flags
    d.dtype = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[e.dtype]
    d.delta_v, d.delta_d, d.alpha, d.beta, d.gamma = params
    return d


def new_state(pkg, dev, d):
    L = pkg._lib.lib()
    nb = L.pea_disc_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    pkg._lib.check(L.pea_disc_workspace_init(vp(ws), nb, None), "pea_disc_workspace_init")
    return ws, nb


def is_clean(ws):
    words = ws.view(torch.int32)
    return int((words != 0).sum()) == 1 and int(words[0]) != 0


def raw_step(pkg, dev, e, labels, num_ids, flags=NEED_GRAD, params=(0.5, 1.5, 1.0, 1.0, 0.001), dloss=None, state=None, de=None, bufs=None,
             poison=-7.0):
    """the two C calls on device tensors -> (loss f32 [1], stats f64 [5 + 4 B], de, ctx); dloss: None (NULL) or a device scalar;
    bufs: (loss, stats, ctx) views lent by the caller (an arena)"""
    L = pkg._lib.lib()
    d = raw_desc(pkg, e, num_ids, flags, params)
    ws, nb = state if state is not None else new_state(pkg, dev, d)
    nctx = L.pea_disc_context_bytes(ctypes.byref(d)) // 8
    if bufs is None:
        bufs = (torch.empty(1, dtype=torch.float32, device=dev), torch.empty(5 + 4 * d.B, dtype=torch.float64, device=dev),
                torch.empty(nctx, dtype=torch.float64, device=dev))
    loss, stats, ctx = bufs
    assert ctx.numel() == nctx
    for t in bufs:
        t.fill_(poison)
    if de is None:
        de = torch.empty_like(e)
    lab = labels.reshape(d.B, -1)
    pkg._lib.check(L.pea_disc_loss_fwd(ctypes.byref(d), vp(e), vp(lab), vp(loss), vp(stats), vp(ctx), vp(ws), nb, None), "pea_disc_loss_fwd")
    if flags & NEED_GRAD:
        pkg._lib.check(L.pea_disc_loss_bwd(ctypes.byref(d), vp(e), vp(lab), vp(ctx), vp(dloss), vp(de), None), "pea_disc_loss_bwd")
    torch.cuda.synchronize()
    assert is_clean(ws[:nb // 8]), "the workspace is not clean after the call"
    return loss, stats, de, ctx


def close(what, loss, stats, de, ref, uncounted=None):
    """device results against (loss, stats, de) of the restatement: the bars of the module docstring; uncounted: bool [B, *spatial],
    the pixels of no counted id, whose gradient is exactly 0"""
    rl, rs, rg = ref
    gl, gs = float(loss.detach().reshape(-1)[0]), stats.cpu().numpy()
    B = (len(rs) - 5) // 4
    assert gs.shape == rs.shape
    print("%s: loss %.9g ref %.17g | var dist reg %s ref %s | C_b %s" % (what, gl, rl, gs[1:4], rs[1:4], gs[8::4]))
    assert gs[4] == rs[4], (what, "n_bad", gs[4], rs[4])
    assert np.array_equal(gs[8::4], rs[8::4]), (what, "C_b", gs[8::4], rs[8::4])
    if np.isnan(rl):
        assert np.isnan(gl) and np.isnan(gs[:4]).all(), what
    else:
        assert abs(gl - rl) <= RTOL_LOSS * abs(rl) and gl == np.float32(gs[0]), (what, gl, gs[0], rl)
        for c in range(4):
            assert abs(gs[c] - rs[c]) <= RTOL_LOSS * abs(rs[c]), (what, c, gs[c], rs[c])
    for b in range(B):
        for c in range(3):
            i = 5 + 4 * b + c
            assert abs(gs[i] - rs[i]) <= RTOL_LOSS * abs(rs[i]), (what, "image", b, c, gs[i], rs[i])
    if de is not None:
        gg = de.float().cpu().numpy().astype(np.float64).reshape(rg.shape)
        top = np.abs(rg).max()
        err = np.abs(gg - rg).max()
        print("%s: gradient err %.3g of top %.3g" % (what, err, top))
        assert np.isfinite(gg).all() and err <= RTOL_GRAD * top, (what, err, top)
        if uncounted is not None:
            assert uncounted.any() and not gg[np.broadcast_to(uncounted[:, None], gg.shape)].any(), what


def blocky(rng, B, Y, X, block, n_ids, zero=0.25):
    by, bx = (Y + block - 1) // block, (X + block - 1) // block
    coarse = rng.integers(1, n_ids, (B, by, bx))
    coarse = np.where(rng.random(coarse.shape) < zero, 0, coarse)
    lab = np.repeat(np.repeat(coarse, block, axis=1), block, axis=2)[:, :Y, :X]
    return np.ascontiguousarray(lab.astype(np.int32))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (e f32 [B, D, Y, X], labels i32 [B, Y, X], num_ids): seeded, shared by the tests (never modified: copy first)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "run_boundary":        # S = 70 * 61 is no multiple of a wave's or a workgroup's run; ids on both sides of a boundary
        B, D, Y, X = 2, 16, 70, 61
        labels = blocky(rng, B, Y, X, 9, 12)
        assert set(labels[0].reshape(-1)[:4096].tolist()) & set(labels[0].reshape(-1)[4096:].tolist()) - {0}
    elif name == "cache_overflow":    # 400 distinct ids in 1600 pixels: a wave meets more than a hundred of them
        B, D, Y, X = 1, 16, 40, 40
        labels = (1 + np.arange(400, dtype=np.int32).reshape(20, 20)).repeat(2, axis=0).repeat(2, axis=1)[None]
    elif name == "table_ceiling":     # num_ids = 4096 with only ids 1 and 4095 present
        B, D, Y, X = 2, 16, 33, 17
        labels = np.where(blocky(rng, B, Y, X, 5, 3, zero=0.0) == 1, 1, 4095).astype(np.int32)
    elif name.startswith("d"):        # the channel count is a run-time value
        B, D, Y, X = 2, int(name[1:]), 33, 17
        labels = blocky(rng, B, Y, X, 6, 9)
    else:
        B, D, Y, X = 2, 16, 37, 53
        labels = blocky(rng, B, Y, X, 8, 12)
    e = rng.standard_normal((B, D, Y, X)).astype(np.float32)
    num_ids = 4096 if name == "table_ceiling" else int(labels.max()) + 1
    return e, labels, num_ids


@functools.lru_cache(maxsize=None)
def case_ref(name, background=False, dloss=1.0):
    e, labels, num_ids = case(name)
    return disc_reference(e, labels, background=background, dloss=dloss, num_ids=num_ids)


# ---- 1. the reference's numbers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_through_the_c_abi_and_discriminative_loss(pkg, dev, name):
    g = load_disc_golden(name)
    bg = g["background"]
    num_ids = int(g["labels"].max()) + 1
    E, Lb = cu(g["e"], dev), cu(g["labels"], dev)
    loss, stats, de, _ = raw_step(pkg, dev, E, Lb, num_ids, flags=NEED_GRAD | (BACKGROUND if bg else 0))
    close(name + " C ABI", loss, stats, de, disc_reference(g["e"], g["labels"], background=bg), None if bg else g["labels"] == 0)
    # the reference's own numbers: float64, and float32 with its autograd gradient
    top = np.abs(g["de64"]).max()
    for l_ref, g_ref in ((g["loss64"], g["de64"]), (g["loss"], g["de"])):
        assert abs(float(loss[0]) - float(l_ref)) <= RTOL_LOSS * abs(float(l_ref))
        assert np.abs(de.cpu().numpy() - g_ref).max() <= RTOL_GRAD * top
    # the Python name with the reference's call: int64 labels, the label range read on the host
    x = E.clone().requires_grad_(True)
    l2 = pkg.discriminative_loss(x, Lb.long(), background=bg)
    assert l2.shape == () and l2.dtype == torch.float32 and l2.requires_grad
    l2.backward()
    assert same_bits(l2.detach().reshape(1), loss) and same_bits(x.grad, de)
    x = E.clone().requires_grad_(True)
    l3, st3 = pkg.discriminative_loss_stats(x, Lb[:, None].to(torch.int16), bg, num_ids=num_ids + 3)  # a wider table: the same bits
    pkg.backward(l3)
    assert same_bits(l3.detach().reshape(1), loss) and same_bits(st3, stats) and same_bits(x.grad, de)
    with torch.no_grad():  # only the loss is wanted: the sums of h u are skipped, the loss has the same bits
        l4, st4 = pkg.discriminative_loss_stats(E, Lb, bg, num_ids=num_ids)
    assert same_bits(l4.reshape(1), loss) and same_bits(st4, stats)


def test_python_refuses_ids_outside_the_table(pkg, dev):
    e, labels, _ = case("base")
    E = cu(e, dev)
    for bad in (-1, 4096):
        lab = labels.copy()
        lab[1, 5, 5] = bad
        with pytest.raises(ValueError, match=r"\[0, 4096\)"):
            pkg.discriminative_loss(E, cu(lab, dev))


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["run_boundary", "cache_overflow", "table_ceiling", "d1", "d5", "d16", "d32", "d64"])
@pytest.mark.parametrize("background", [False, True], ids=["drop0", "keep0"])
def test_shapes(pkg, dev, name, background):
    e, labels, num_ids = case(name)
    if name == "cache_overflow":
        assert len(np.unique(labels)) == 400
    if name == "table_ceiling":
        assert num_ids == 4096 and set(np.unique(labels).tolist()) == {1, 4095}
    got = raw_step(pkg, dev, cu(e, dev), cu(labels, dev), num_ids, flags=NEED_GRAD | (BACKGROUND if background else 0))
    zero = None if background or not (labels == 0).any() else labels == 0
    close("%s background=%s" % (name, background), *got[:3], case_ref(name, background), zero)


# ---- 3. the upstream gradient ----------------------------------------------------------------------------------------------------------------
def test_upstream_dloss(pkg, dev):
    e, labels, num_ids = case("base")
    E, Lb = cu(e, dev), cu(labels, dev)
    null = raw_step(pkg, dev, E, Lb, num_ids, dloss=None)
    one = raw_step(pkg, dev, E, Lb, num_ids, dloss=torch.tensor(1.0, device=dev))
    assert all_same(one, null)  # NULL is 1
    for s in (2.5, -1.0):
        got = raw_step(pkg, dev, E, Lb, num_ids, dloss=torch.tensor(s, dtype=torch.float32, device=dev))
        close("dloss %g" % s, *got[:3], case_ref("base", False, s))
        assert same_bits(got[0], one[0]) and same_bits(got[1], one[1]) and same_bits(got[3], one[3])
        x = E.clone().requires_grad_(True)
        (s * pkg.discriminative_loss(x, Lb, num_ids=num_ids)).backward()
        assert same_bits(x.grad, got[2])


def test_loss_weights_and_margins(pkg, dev):
    e, labels, num_ids = case("base")
    params = (0.25, 2.0, 0.5, 3.0, 0.1)
    got = raw_step(pkg, dev, cu(e, dev), cu(labels, dev), num_ids, params=params)
    close("params", *got[:3], disc_reference(e, labels, False, *params, num_ids=num_ids))
    x = cu(e, dev).requires_grad_(True)
    l = pkg.discriminative_loss(x, cu(labels, dev), False, *params, num_ids=num_ids)
    l.backward()
    assert same_bits(l.detach().reshape(1), got[0]) and same_bits(x.grad, got[2])


# ---- 4. labels outside the table -------------------------------------------------------------------------------------------------------------
def test_bad_labels_touch_nothing_and_leave_the_workspace_clean(pkg, dev):
    e, labels, num_ids = case("base")
    L = pkg._lib.lib()
    bad = labels.copy()
    bad[0, 0, 0], bad[0, 36, 52], bad[1, 7, 7], bad[1, 20, 20] = num_ids, -1, 2 ** 31 - 1, -2 ** 31
    ref = disc_reference(e, bad, num_ids=num_ids)
    assert ref[1][4] == 4 and np.isnan(ref[0])
    ar = Arena(4 << 20, dev)
    d = raw_desc(pkg, cu(e, dev), num_ids)
    nb, nctx = L.pea_disc_workspace_bytes(ctypes.byref(d)), L.pea_disc_context_bytes(ctypes.byref(d))
    E = ar.fill(ar.carve(e.shape, torch.float32, 4, name="e"), e)
    Lb = ar.fill(ar.carve(bad.shape, torch.int32, 4, name="labels"), bad)
    De = ar.carve(e.shape, torch.float32, 4, name="de")
    loss, stats = ar.carve((1,), torch.float32, 4, name="loss"), ar.carve((5 + 4 * d.B,), torch.float64, 8, name="stats")
    ctx, ws = ar.carve((nctx // 8,), torch.float64, 8, name="ctx"), ar.carve((nb // 8,), torch.float64, 8, name="workspace")
    pkg._lib.check(L.pea_disc_workspace_init(vp(ws), nb, None), "pea_disc_workspace_init")
    got = raw_step(pkg, dev, E, Lb, num_ids, state=(ws, nb), de=De, bufs=(loss, stats, ctx))
    ar.check(written=[De, loss, stats, ctx, ws], untouched=[E, Lb])
    close("bad labels", *got[:3], ref, (bad < 0) | (bad >= num_ids) | (bad == 0))
    assert bool(torch.isnan(got[0]).all()) and float(got[1][4]) == 4.0
    # the next call on the same workspace gives the bits of a fresh one
    again = raw_step(pkg, dev, E, cu(labels, dev), num_ids, state=(ws, nb))
    fresh = raw_step(pkg, dev, E, cu(labels, dev), num_ids)
    assert all_same(again, fresh) and bool(torch.isfinite(again[0]).all())
    close("after bad labels", *again[:3], case_ref("base"))


def test_uninitialised_workspace_gives_nan(pkg, dev):
    e, labels, num_ids = case("base")
    E, Lb = cu(e, dev), cu(labels, dev)
    d = raw_desc(pkg, E, num_ids)
    nb = pkg._lib.lib().pea_disc_workspace_bytes(ctypes.byref(d))
    raw = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    L = pkg._lib.lib()
    loss, stats = torch.zeros(1, device=dev), torch.zeros(5 + 4 * d.B, dtype=torch.float64, device=dev)
    ctx = torch.zeros(L.pea_disc_context_bytes(ctypes.byref(d)) // 8, dtype=torch.float64, device=dev)
    pkg._lib.check(L.pea_disc_loss_fwd(ctypes.byref(d), vp(E), vp(Lb.reshape(2, -1)), vp(loss), vp(stats), vp(ctx), vp(raw), nb, None), "fwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(stats).all())


# ---- 5. the same bits ------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_every_alignment_give_the_same_bits(pkg, dev):
    e, labels, num_ids = case("run_boundary")
    E, Lb = cu(e, dev), cu(labels, dev)
    d = raw_desc(pkg, E, num_ids)
    state = new_state(pkg, dev, d)
    a = raw_step(pkg, dev, E, Lb, num_ids, state=state, poison=-7.0)
    b = raw_step(pkg, dev, E, Lb, num_ids, state=state, poison=3.0)  # ctx, stats and loss start from another pattern: all of it is written
    assert all_same(a, b)
    close("run 1", *a[:3], case_ref("run_boundary"))
    for skew in (1, 3):  # odd element offsets: no quad of e, labels or de is 16-byte aligned
        ar = Arena(4 << 20, dev)
        Es = ar.fill(ar.carve(e.shape, torch.float32, 4 * skew, name="e"), e)
        Ls = ar.fill(ar.carve(labels.shape, torch.int32, 4 * skew, name="labels"), labels)
        Ds = ar.carve(e.shape, torch.float32, 4 * skew, name="de")
        assert Es.data_ptr() % 16 == 4 * skew and Ls.data_ptr() % 16 == 4 * skew and Ds.data_ptr() % 16 == 4 * skew
        c = raw_step(pkg, dev, Es, Ls, num_ids, de=Ds)
        ar.check(written=[Ds], untouched=[Es, Ls])
        assert all_same(a, c), skew


def test_graphed_call_replays_the_eager_bits(pkg, dev):
    e, labels, num_ids = case("base")
    E, Lb = cu(e, dev).requires_grad_(True), cu(labels, dev)

    def step(E, Lb):
        E.grad = None
        loss, stats = pkg.discriminative_loss_stats(E, Lb, num_ids=num_ids)
        pkg.backward(2.0 * loss)
        return loss, stats, E.grad

    def snap(outs):
        return [o.detach().clone() for o in outs]

    eager = snap(step(E, Lb))
    g = pkg.graphed(step, E, Lb)
    first = snap(g.replay())
    assert all_same(first, eager)
    close("graphed", first[0], first[1], first[2], case_ref("base", False, 2.0))
    # refill the static inputs: the replay follows, and equals the eager call on the new data
    e2, labels2, n2 = case("d16")
    assert n2 <= num_ids
    lab2 = np.zeros_like(labels)
    lab2[:, :33, :17] = labels2
    with torch.no_grad():
        E.mul_(0.5)
        Lb.copy_(cu(lab2, dev))
    second = snap(g.replay())
    eager2 = snap(step(E, Lb))
    assert all_same(second, eager2) and not same_bits(second[0], first[0])


# ---- 6. 16-bit embeddings ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_16bit_embeddings_are_the_f32_call_on_the_widened_values(pkg, dev, dt):
    e, labels, num_ids = case("base")
    Lb = cu(labels, dev)
    E16 = cu(e, dev).to(TDT[dt])
    dl = torch.tensor(3.0, dtype=torch.float32, device=dev)
    r16 = raw_step(pkg, dev, E16, Lb, num_ids, dloss=dl)
    r32 = raw_step(pkg, dev, E16.float(), Lb, num_ids, dloss=dl)
    assert r16[2].dtype == TDT[dt] and same_bits(r16[0], r32[0]) and same_bits(r16[1], r32[1]) and same_bits(r16[3], r32[3])
    assert same_bits(r16[2], r32[2].to(TDT[dt]))  # rounded once, to nearest even
    close(dt, r16[0], r16[1], r32[2], disc_reference(E16.float().cpu().numpy(), labels, dloss=3.0, num_ids=num_ids))
    for skew in (1, 3):  # element-aligned 16-bit pointers
        ar = Arena(1 << 20, dev)
        Es = ar.fill(ar.carve(e.shape, TDT[dt], 2 * skew, name="e"), E16)
        Ds = ar.carve(e.shape, TDT[dt], 2 * skew, name="de")
        c = raw_step(pkg, dev, Es, Lb, num_ids, dloss=dl, de=Ds)
        ar.check(written=[Ds], untouched=[Es])
        assert all_same(r16, c), skew
    x = E16.clone().requires_grad_(True)
    (3.0 * pkg.discriminative_loss(x, Lb, num_ids=num_ids)).backward()
    assert x.grad.dtype == TDT[dt] and same_bits(x.grad, r16[2])


# ---- 7. non-finite embeddings ------------------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_stay_in_their_image(pkg, dev):
    e, labels, num_ids = case("base")
    two = [int(c) for c in np.unique(labels[0]) if c > 0][:2]  # a pixel of each of two counted clusters of image 0
    (y1, x1), (y2, x2) = (tuple(int(v) for v in np.argwhere(labels[0] == c)[-1]) for c in two)
    p_nan, p_inf = (0, 3, y1, x1), (0, 9, y2, x2)
    E, Lb = cu(e, dev), cu(labels, dev)
    state = new_state(pkg, dev, raw_desc(pkg, E, num_ids))
    fin = raw_step(pkg, dev, E, Lb, num_ids, state=state)
    bad_in = E.clone()
    bad_in[p_nan], bad_in[p_inf] = float("nan"), float("inf")
    bad = raw_step(pkg, dev, bad_in, Lb, num_ids, state=state)  # (raw_step: the workspace is clean afterwards)
    assert bool(torch.isnan(bad[0]).all()) and bool(torch.isnan(bad[1][0])) and bool(torch.isnan(bad[1][1])) and bool(torch.isnan(bad[1][5]))
    assert bool(torch.isnan(bad[2][0, :, y1, x1]).all()) and bool(torch.isnan(bad[2][0, :, y2, x2]).all())
    # image 1: the bits of the finite run
    assert same_bits(bad[2][1], fin[2][1]) and same_bits(bad[1][9:13], fin[1][9:13]) and bool(torch.isfinite(bad[2][1]).all())
    assert float(bad[1][4]) == 0.0 and float(bad[1][8]) == float(fin[1][8])
    again = raw_step(pkg, dev, E, Lb, num_ids, state=state)  # the next call on the same workspace is finite again
    assert all_same(again, fin) and bool(torch.isfinite(again[0]).all())


# ---- 8. the train step -----------------------------------------------------------------------------------------------------------------------------
def test_train_step_with_disc_weight(pkg, dev):
    """one step at 2 x 3 x 64 x 64 with disc_weight=0.1, disc_num_ids=64: the loss is the loss of the step without the term plus
    0.1 * discriminative_loss on the full-resolution embedding of a copy of the net (BatchNorm runs on batch statistics, so the copy
    sees the same activations).  disc_weight=None is the step as it was: the loss bits of a step built without the keyword (the
    parameter gradients are not compared: the convolutions' backward is not bit-reproducible from run to run)."""
    mod = importlib.import_module(ge.PKG_NAME + ".model.unet2d_residual")
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    torch.manual_seed(7)
    net = mod.ResidualUNet2D_deep(in_channels=3, out_channels=2, nfeatures=[4, 8, 8, 16, 16], emd=16).to(dev)
    none_net, old_net, ref_net = copy.deepcopy(net), copy.deepcopy(net), copy.deepcopy(net)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 64, 64, generator=gen).to(dev)
    x_ema = (x.cpu() + 0.1 * torch.randn(2, 3, 64, 64, generator=gen)).to(dev)
    labels = torch.from_numpy(synth.synth_labels(2, (1, 64, 64), 5)[:, 0].copy()).to(torch.int32).to(dev)
    assert 0 <= int(labels.min()) and int(labels.max()) < 64 and int((labels > 0).sum()) > 0
    kw = dict(shifts=(1, 2, 3, 5, 9), neighbor=4)

    loss = pkg.CvpppTrainStep(net, torch.optim.SGD(net.parameters(), lr=0.0), disc_weight=0.1, disc_num_ids=64, **kw).step(x, x_ema, labels)
    loss0 = pkg.CvpppTrainStep(none_net, torch.optim.SGD(none_net.parameters(), lr=0.0), disc_weight=None, **kw).step(x, x_ema, labels)
    loss_old = pkg.CvpppTrainStep(old_net, torch.optim.SGD(old_net.parameters(), lr=0.0), **kw).step(x, x_ema, labels)
    ref_net.train()
    with torch.no_grad():
        term, stats = pkg.discriminative_loss_stats(ref_net(x)[4], labels, num_ids=64)
    torch.cuda.synchronize()
    print("step loss %.9g, without the term %.9g, the term %.9g (C_b %s)" % (float(loss), float(loss0), float(term), stats[8::4].tolist()))
    assert float(term) > 0 and float(stats[4]) == 0 and float(stats[8]) > 0
    assert abs(float(loss) - (float(loss0) + 0.1 * float(term))) <= 1e-5 * abs(float(loss))
    assert same_bits(loss0.reshape(1), loss_old.reshape(1))
