"""GPU: the foreground-mask loss and the validation mask (include/pea_fgmask.h, csrc/pea_k_fgmask.hip) through the C ABI and through
BCE_loss_func / foreground_mask_loss / foreground_mask / CvpppTrainStep(mask_weight=..), against the reference's own numbers
(tests/golden/gfg_*.npz) and the float64 restatement tests/fgmask_reference.py (which test_fgmask_host.py holds to those numbers).

Tolerances are the project's f32 bars (tests/test_gpu_parity.py): loss 1e-5 relative, gradient 1e-4 of the largest reference
magnitude.  Counts and everything called bit-identical are compared exactly."""
import copy
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from arena import Arena
from conftest import load_golden
from fgmask_reference import fgmask_reference, mask_reference

pytestmark = pytest.mark.gpu
RTOL_LOSS, RTOL_GRAD = 1e-5, 1e-4
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SKIP = 1  # PEA_FG_SKIP_EMPTY_CLASS


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


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def new_state(pkg, dev):
    L = pkg._lib.lib()
    nb = L.pea_fgmask_workspace_bytes()
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    pkg._lib.check(L.pea_workspace_init(vp(ws), nb, None), "pea_workspace_init")
    return ws, nb


def raw_desc(pkg, logits, labels, flags=0):
    d = pkg._lib.PeaFgDesc()
    d.B, d.Y, d.X = logits.shape[0], logits.shape[2], logits.shape[3]
    d.logits_dtype = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[logits.dtype]
    d.labels_type = 0 if labels is None or labels.dtype == torch.int32 else 1
    d.flags = flags
    return d


def raw_step(pkg, dev, logits, labels, flags=0, dloss=None, dlogits=None, state=None):
    """the two C calls on device tensors -> (loss f32 [1], stats f64 [5], dlogits); dloss: None (NULL) or a device scalar"""
    L = pkg._lib.lib()
    d = raw_desc(pkg, logits, labels, flags)
    ws, nb = state if state is not None else new_state(pkg, dev)
    loss = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    stats = torch.full((5,), -7.0, dtype=torch.float64, device=dev)
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    pkg._lib.check(L.pea_fgmask_loss_fwd(ctypes.byref(d), vp(logits), vp(labels), vp(loss), vp(stats), vp(ws), nb, None), "pea_fgmask_loss_fwd")
    pkg._lib.check(L.pea_fgmask_loss_bwd(ctypes.byref(d), vp(logits), vp(labels), vp(stats), vp(dloss), vp(dlogits), None), "pea_fgmask_loss_bwd")
    torch.cuda.synchronize()
    return loss, stats, dlogits


def close(what, loss, stats, dlogits, ref, check_stats=True):
    """device results against (loss, stats, dlogits) of the restatement: the bars of the module docstring, NaN where it is NaN"""
    rl, rs, rg = ref
    gl, gs, gg = float(loss.detach().reshape(-1)[0]), stats.cpu().numpy(), dlogits.float().cpu().numpy().astype(np.float64)
    top = np.nanmax(np.abs(rg)) if np.isfinite(rg).any() else 0.0
    with np.errstate(invalid="ignore"):
        err = np.nanmax(np.abs(gg - rg)) if np.isfinite(rg).any() else 0.0
    print("%s: loss %.9g ref %.17g | stats %s | grad err %.3g of top %.3g" % (what, gl, rl, gs, err, top))
    if np.isnan(rl):
        assert np.isnan(gl) and np.isnan(gs[0]), what
    else:
        assert abs(gl - rl) <= RTOL_LOSS * abs(rl) and abs(gs[0] - rl) <= RTOL_LOSS * abs(rl), (what, gl, gs[0], rl)
        assert gl == np.float32(gs[0]), what  # loss[0] = (float)stats[0]
    if check_stats:
        for c in (1, 2):
            assert (np.isnan(gs[c]) and np.isnan(rs[c])) or abs(gs[c] - rs[c]) <= RTOL_LOSS * abs(rs[c]), (what, c, gs[c], rs[c])
        assert gs[3] == rs[3] and gs[4] == rs[4], (what, gs, rs)
    assert np.array_equal(np.isnan(gg), np.isnan(rg)), what
    assert err <= RTOL_GRAD * top, (what, err, top)


def make(seed, B, Y, X, fg=0.35):
    """seeded logits (float32, N(0, 2)) and int32 labels with negatives and large ids; both classes present unless fg is 0 or 1"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, 2, Y, X)) * 2.0).astype(np.float32)
    pos = rng.random((B, Y, X)) < fg
    ids = np.where(rng.random((B, Y, X)) < 0.2, 2 ** 31 - 1 - rng.integers(0, 9, (B, Y, X)), rng.integers(1, 50, (B, Y, X)))
    neg = np.where(rng.random((B, Y, X)) < 0.3, -rng.integers(1, 2 ** 31, (B, Y, X)), 0)
    labels = np.where(pos, ids, neg).astype(np.int32)
    if 0.0 < fg < 1.0:
        flat = labels.reshape(-1)
        flat[0], flat[-1] = 5, -3  # at least one pixel of each class
    return logits, labels


# ---- 1. the reference's numbers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gfg_b2_37x53", "gfg_b3_64x80"])
def test_goldens_through_the_c_abi_and_bce_loss_func(pkg, dev, name):
    g = load_golden(name)
    top = np.abs(g["dlogits64"]).max()
    ref64 = (float(g["loss64"]), fgmask_reference(g["logits"], g["labels"])[1], g["dlogits64"].astype(np.float64))
    loss, stats, dl = raw_step(pkg, dev, cu(g["logits"], dev), cu(g["labels"], dev))
    close(name + " C ABI", loss, stats, dl, ref64)
    # the reference's own float32 loss and autograd gradient
    assert abs(float(loss[0]) - float(g["loss"])) <= RTOL_LOSS * abs(float(g["loss"]))
    assert np.abs(dl.cpu().numpy() - g["dlogits"]).max() <= RTOL_GRAD * top
    # the Python name, as main.py:289 calls it
    out = cu(g["logits"], dev).requires_grad_(True)
    target_ins = cu(g["labels"], dev)[:, None]
    l2 = pkg.BCE_loss_func(out, torch.gt(target_ins[:, 0], 0), weight_rate=[10, 1])
    assert l2.shape == () and l2.dtype == torch.float32 and l2.requires_grad
    pkg.backward(l2)
    assert same_bits(l2.detach().reshape(1), loss) and same_bits(out.grad, dl)  # bool labels, the bits of the int32 call


def test_all_background_golden_is_nan_like_the_reference(pkg, dev):
    g = load_golden("gfg_allbg")
    assert np.isnan(g["loss"]) and np.isnan(g["dlogits"]).all()
    loss, stats, dl = raw_step(pkg, dev, cu(g["logits"], dev), cu(g["labels"], dev))
    close("gfg_allbg", loss, stats, dl, fgmask_reference(g["logits"], g["labels"]))
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dl).all()) and float(stats[4]) == 0.0 and float(stats[3]) == g["labels"].size
    out = cu(g["logits"], dev).requires_grad_(True)
    l2 = pkg.BCE_loss_func(out, cu(g["labels"], dev))
    pkg.backward(l2)
    assert bool(torch.isnan(l2)) and bool(torch.isnan(out.grad).all())


# ---- 2. shapes and pointers ----------------------------------------------------------------------------------------------------------
SHAPES = [("1px_per_image", 2, 1, 1), ("3px", 1, 1, 3), ("5px", 1, 5, 1), ("4095px", 1, 63, 65), ("4097px", 1, 17, 241), ("37x53", 2, 37, 53),
          ("3x64x80", 3, 64, 80)]


@pytest.mark.parametrize("ltype", ["i32", "u8"])
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes_and_element_aligned_pointers(pkg, dev, case, ltype):
    """every shape 16-byte aligned and one element off, inside a guard-banded arena: the restatement's numbers, the same bits both
    ways, every element of dlogits written and nothing else"""
    name, B, Y, X = case
    logits, labels = make(sum(map(ord, name)), B, Y, X)
    if name == "1px_per_image":
        labels[:] = np.array([7, -2], np.int32).reshape(2, 1, 1)  # one pixel of each class
    ref = fgmask_reference(logits, labels)
    lt = torch.int32 if ltype == "i32" else torch.uint8
    lab = labels if ltype == "i32" else (labels > 0).astype(np.uint8)
    runs = []
    for skew in (0, 1):
        ar = Arena(1 << 20, dev)
        Lg = ar.fill(ar.carve(logits.shape, torch.float32, 4 * skew, name="logits"), logits)
        Lb = ar.fill(ar.carve(labels.shape, lt, (4 if ltype == "i32" else 1) * skew, name="labels"), lab)
        Dg = ar.carve(logits.shape, torch.float32, 4 * skew, name="dlogits")
        assert Lg.data_ptr() % 16 == 4 * skew and Dg.data_ptr() % 16 == 4 * skew and Lb.data_ptr() % 4 == (0 if ltype == "i32" else skew)
        loss, stats, dl = raw_step(pkg, dev, Lg, Lb, dlogits=Dg)
        ar.check(written=[Dg], untouched=[Lg, Lb])
        runs.append((loss.clone(), stats.clone(), dl.clone()))
    close("%s %s" % (name, ltype), *runs[0], ref)
    for a, b in zip(runs[0], runs[1]):
        assert same_bits(a, b), name


def test_16bit_pointers_one_element_off(pkg, dev):
    logits, labels = make(21, 2, 37, 53)
    for dt in (torch.float16, torch.bfloat16):
        runs = []
        for skew in (0, 1, 3):
            ar = Arena(1 << 18, dev)
            Lg = ar.fill(ar.carve(logits.shape, dt, 2 * skew, name="logits"), logits)
            Lb = ar.fill(ar.carve(labels.shape, torch.uint8, skew, name="labels"), (labels > 0))
            Dg = ar.carve(logits.shape, dt, 2 * skew, name="dlogits")
            runs.append(tuple(t.clone() for t in raw_step(pkg, dev, Lg, Lb, dlogits=Dg)))
            ar.check(written=[Dg], untouched=[Lg, Lb])
        for r in runs[1:]:
            assert all(same_bits(a, b) for a, b in zip(runs[0], r)), dt


# ---- 3. label types ------------------------------------------------------------------------------------------------------------------
def test_label_types_give_the_same_bits(pkg, dev):
    logits, labels = make(31, 2, 37, 53)
    assert (labels < 0).any()
    outs = []
    for lab in (cu(labels, dev), cu((labels > 0).astype(np.uint8), dev), cu(labels > 0, dev), cu(labels > 0, dev)[:, None]):
        x = cu(logits, dev).requires_grad_(True)
        loss, stats = pkg.foreground_mask_loss(x, lab)
        pkg.backward(loss)
        outs.append((loss.detach().reshape(1), stats, x.grad))
    close("int32 labels", *outs[0], fgmask_reference(logits, labels))
    for o in outs[1:]:
        assert all(same_bits(a, b) for a, b in zip(outs[0], o))
    # uint8 values above 1 are foreground too (value > 0)
    big = cu(((labels > 0) * 200).astype(np.uint8), dev)
    loss, stats = pkg.foreground_mask_loss(cu(logits, dev), big)
    assert same_bits(loss.reshape(1), outs[0][0]) and same_bits(stats, outs[0][1])


# ---- 4. reproducibility and the state contract -----------------------------------------------------------------------------------------
def test_two_runs_agree_and_the_state_serves_a_later_call(pkg, dev):
    L, op = pkg._lib.lib(), pkg.affinity_op
    logits, labels = make(41, 3, 64, 80)
    Lg, Lb = cu(logits, dev), cu(labels, dev)
    state = new_state(pkg, dev)
    a = raw_step(pkg, dev, Lg, Lb, state=state)
    b = raw_step(pkg, dev, Lg, Lb, state=state)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    close("run 1", *a, fgmask_reference(logits, labels))
    # the block is zero again (but for the magic word): an embedding_loss forward on it gives the bits of a fresh block
    words = state[0].view(torch.int32)
    assert int((words != 0).sum()) == 1 and int(words[0]) != 0
    spec = pkg.AffinitySpec(2, [(0, 1), (1, 0), (3, -2)], None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX, 1e-6)
    gen = torch.Generator(device=dev).manual_seed(9)
    e = torch.randn((2, 16, 40, 56), generator=gen, device=dev)
    t = (torch.rand((2, 3, 40, 56), generator=gen, device=dev) < 0.5).float()
    w = torch.rand((2, 3, 40, 56), generator=gen, device=dev) + 0.5
    pd = op.make_desc(spec, e)
    one = L.pea_workspace_bytes(ctypes.byref(pd))
    assert state[1] >= one
    rows = []
    for block in (state[0], new_state(pkg, dev)[0]):
        affs, loss = torch.empty_like(t), torch.empty(4, dtype=torch.float32, device=dev)
        pkg._lib.check(L.pea_affinity_fwd(ctypes.byref(pd), vp(e), None, vp(t), vp(w), None, vp(affs), None, vp(loss), vp(block), one, None),
                       "pea_affinity_fwd")
        torch.cuda.synchronize()
        rows.append((loss, affs))
    assert same_bits(rows[0][0], rows[1][0]) and same_bits(rows[0][1], rows[1][1]) and bool(torch.isfinite(rows[0][0]).all())
    # a block that was never initialised: NaN, not a wrong number
    raw = torch.zeros(state[1] // 8, dtype=torch.float64, device=dev)
    loss, stats, _ = raw_step(pkg, dev, Lg, Lb, state=(raw, state[1]))
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(stats).all())


# ---- 5. 16-bit logits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("ltype", ["i32", "u8"])
def test_16bit_logits_are_the_f32_call_on_the_widened_values(pkg, dev, dt, ltype):
    logits, labels = make(51, 2, 37, 53)
    Lb = cu(labels, dev) if ltype == "i32" else cu((labels > 0).astype(np.uint8), dev)
    L16 = cu(logits, dev).to(TDT[dt])
    dl_s = torch.tensor(3.0, dtype=torch.float32, device=dev)
    loss16, stats16, d16 = raw_step(pkg, dev, L16, Lb, dloss=dl_s)
    loss32, stats32, d32 = raw_step(pkg, dev, L16.float(), Lb, dloss=dl_s)
    assert d16.dtype == TDT[dt] and same_bits(loss16, loss32) and same_bits(stats16, stats32)
    assert same_bits(d16, d32.to(TDT[dt]))  # rounded once, to nearest even
    close("%s %s" % (dt, ltype), loss16, stats16, d32, fgmask_reference(L16.float().cpu().numpy(), labels, dloss=3.0))
    # through autograd: the gradient has the logits' dtype
    x = L16.clone().requires_grad_(True)
    loss, _ = pkg.foreground_mask_loss(x, Lb)
    (loss * 3.0).backward()
    assert x.grad.dtype == TDT[dt] and same_bits(x.grad, d16) and same_bits(loss.detach().reshape(1), loss16)


# ---- 6. the upstream gradient ----------------------------------------------------------------------------------------------------------
def test_upstream_dloss(pkg, dev):
    logits, labels = make(61, 2, 37, 53)
    Lg, Lb = cu(logits, dev), cu(labels, dev)
    one = raw_step(pkg, dev, Lg, Lb, dloss=torch.tensor(1.0, device=dev))
    null = raw_step(pkg, dev, Lg, Lb, dloss=None)
    assert all(same_bits(a, b) for a, b in zip(one, null))  # NULL is 1
    for s in (0.5, 1000.0):
        got = raw_step(pkg, dev, Lg, Lb, dloss=torch.tensor(s, dtype=torch.float32, device=dev))
        close("dloss %g" % s, *got, fgmask_reference(logits, labels, dloss=s))
        assert same_bits(got[0], one[0]) and same_bits(got[1], one[1])
        x = Lg.clone().requires_grad_(True)
        pkg.backward(s * pkg.BCE_loss_func(x, Lb))
        close("autograd dloss %g" % s, got[0], got[1], x.grad, fgmask_reference(logits, labels, dloss=s))


# ---- 7. an absent class ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fg", [0.0, 1.0], ids=["all_background", "all_foreground"])
def test_an_absent_class(pkg, dev, fg):
    logits, labels = make(71, 2, 12, 20, fg=fg)
    assert ((labels > 0).all() if fg else ((labels <= 0).all() and (labels < 0).any()))
    Lg, Lb = cu(logits, dev), cu(labels, dev)
    got = raw_step(pkg, dev, Lg, Lb)
    close("default", *got, fgmask_reference(logits, labels))
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[2]).all())
    got = raw_step(pkg, dev, Lg, Lb, flags=SKIP, dloss=torch.tensor(2.0, device=dev))
    ref = fgmask_reference(logits, labels, dloss=2.0, skip_empty=True)
    close("skip_empty", *got, ref)
    assert np.isfinite(ref[0]) and bool(torch.isfinite(got[2]).all()) and float(got[1][2 if fg == 0.0 else 1]) == 0.0
    x = Lg.clone().requires_grad_(True)
    loss, stats = pkg.foreground_mask_loss(x, Lb, skip_empty=True)
    pkg.backward(loss)
    close("skip_empty, Python", loss, stats, x.grad, fgmask_reference(logits, labels, skip_empty=True))
    # with both classes present the flag changes nothing
    logits, labels = make(72, 2, 12, 20)
    a, b = raw_step(pkg, dev, cu(logits, dev), cu(labels, dev)), raw_step(pkg, dev, cu(logits, dev), cu(labels, dev), flags=SKIP)
    assert all(same_bits(p, q) for p, q in zip(a, b))


# ---- 8. non-finite logits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_one_nan_logit(pkg, dev, dt):
    logits, labels = make(81, 2, 37, 53)
    Lb = cu(labels, dev)
    fin_in = cu(logits, dev).to(TDT[dt])
    state = new_state(pkg, dev)
    fin = raw_step(pkg, dev, fin_in, Lb, state=state)
    bad_in = fin_in.clone()
    bad_in[1, 0, 20, 11] = float("nan")
    bad = raw_step(pkg, dev, bad_in, Lb, state=state)
    assert bool(torch.isnan(bad[0]).all()) and bool(torch.isnan(bad[1][0]))
    cls = 2 if labels[1, 20, 11] > 0 else 1
    assert bool(torch.isnan(bad[1][cls])) and same_bits(bad[1][3 - cls:4 - cls], fin[1][3 - cls:4 - cls]) and same_bits(bad[1][3:], fin[1][3:])
    nan = torch.isnan(bad[2])
    assert int(nan.sum()) == 2 and bool(nan[1, :, 20, 11].all())  # that pixel, both channels, and nothing else
    keep = ~nan
    assert same_bits(bad[2][keep], fin[2][keep])
    again = raw_step(pkg, dev, fin_in, Lb, state=state)  # the next call on the same state is finite again
    assert all(same_bits(a, b) for a, b in zip(again, fin)) and bool(torch.isfinite(again[0]).all())


# ---- 9. the validation mask --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_foreground_mask(pkg, dev, dt):
    g = load_golden("gfg_valid_200x24")
    crop = tuple(tuple(int(v) for v in r) for r in g["crop"])
    L = cu(g["logits"], dev).to(TDT[dt])
    widened = L.float().cpu().numpy()  # (a 16-bit cast makes new ties: the rule is applied to the values the kernel sees)
    m = pkg.foreground_mask(L, crop)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (1, 16, 16) and m.is_cuda
    assert np.array_equal(m.cpu().numpy(), mask_reference(widened, crop))
    if dt == "f32":
        assert np.array_equal(m.cpu().numpy()[0], g["mask"])  # main.py:406-410 run as written
    full = pkg.foreground_mask(L)
    assert tuple(full.shape) == (1, 200, 24) and np.array_equal(full.cpu().numpy(), mask_reference(widened))
    # a batch, odd crops, an output that is no multiple of four and spans workgroups; the output inside guard bands
    logits, _ = make(91, 3, 37, 53)
    logits[1, 1, 5, 7:11] = logits[1, 0, 5, 7:11]
    logits[2, 0, 30, 50] = np.nan
    Lb = cu(logits, dev).to(TDT[dt])
    wb = Lb.float().cpu().numpy()
    for c in (((0, 0), (0, 0)), ((3, 1), (2, 4)), ((0, 36), (52, 0)), ((36, 0), (0, 52))):
        assert np.array_equal(pkg.foreground_mask(Lb, c).cpu().numpy(), mask_reference(wb, c)), c
    for skew in (0, 1, 3):
        ar = Arena(1 << 16, dev)
        out = ar.carve((3, 33, 47), torch.uint8, skew, name="mask")
        d = raw_desc(pkg, Lb, None)
        d.origin[:], d.out_dims[:] = (3, 2), (33, 47)
        pkg._lib.check(pkg._lib.lib().pea_fgmask_argmax(ctypes.byref(d), vp(Lb), vp(out), None), "pea_fgmask_argmax")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), mask_reference(wb, ((3, 1), (2, 4)))), skew
        ar.check(scratch=[out])
    with pytest.raises(ValueError):
        pkg.foreground_mask(Lb, ((20, 17), (0, 0)))


# ---- 10. graph capture -------------------------------------------------------------------------------------------------------------------
def test_graphed_step_replays_the_eager_bits(pkg, dev):
    """embedding_loss + 1000 * BCE_loss_func + pea.backward on 2 x 64 x 64: capturable (no host synchronisation), bit-identical to eager"""
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    offsets = pkg.multi_offset([1, 3, 5], neighbor=4)
    crit = pkg.WeightedMSE()
    e, t, w, m = synth.synth_inputs_2d(2, 16, 64, 64, offsets, seed=101)
    logits, labels = make(102, 2, 64, 64)
    E, Lg = cu(e, dev).requires_grad_(True), cu(logits, dev).requires_grad_(True)
    T, W, M, Lb = cu(t, dev), cu(w, dev), cu(m, dev), cu(labels, dev)

    def step(E, Lg, T, W, M, Lb):
        E.grad, Lg.grad = None, None
        loss, affs, _ = pkg.embedding_loss(E, T, W, M, crit, offsets)
        loss_mask = pkg.BCE_loss_func(Lg, torch.gt(Lb, 0), weight_rate=[10, 1])
        total = loss + 1000.0 * loss_mask
        pkg.backward(total)
        return total, loss_mask, E.grad, Lg.grad

    def snap(outs):
        return [o.detach().clone() for o in outs]

    eager = snap(step(E, Lg, T, W, M, Lb))
    g = pkg.graphed(step, E, Lg, T, W, M, Lb)
    first = snap(g.replay())
    assert all(same_bits(a, b) for a, b in zip(first, eager))
    ref = fgmask_reference(logits, labels, dloss=1000.0)
    assert abs(float(first[1]) - ref[0]) <= RTOL_LOSS * abs(ref[0])
    assert np.abs(first[3].cpu().numpy() - ref[2]).max() <= RTOL_GRAD * np.abs(ref[2]).max()
    # refill the static inputs: the replay follows, and equals the eager call on the new data
    logits2, labels2 = make(103, 2, 64, 64, fg=0.6)
    with torch.no_grad():
        Lg.copy_(cu(logits2, dev))
        Lb.copy_(cu(labels2, dev))
        E.mul_(0.5)
    second = snap(g.replay())
    eager2 = snap(step(E, Lg, T, W, M, Lb))
    assert all(same_bits(a, b) for a, b in zip(second, eager2)) and not same_bits(second[1], first[1])
    ref2 = fgmask_reference(logits2, labels2, dloss=1000.0)
    assert abs(float(second[1]) - ref2[0]) <= RTOL_LOSS * abs(ref2[0])


# ---- 11. the BBBC step -------------------------------------------------------------------------------------------------------------------
def test_train_step_with_mask_weight(pkg, dev):
    """one step at 2 x 3 x 64 x 64 with mask_weight=1000: the binary_seg parameters receive the gradients of the reference's term,
    1000 * nn.CrossEntropyLoss(weight from two .item())(pred_mask, labels > 0), taken in eager on a copy of the net (the head's
    parameters are reached by that term alone; BatchNorm runs on batch statistics, so the copy sees the same activations).  With
    mask_weight=None they receive none."""
    mod = importlib.import_module(ge.PKG_NAME + ".model.unet2d_residual")
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    torch.manual_seed(7)
    net = mod.ResidualUNet2D_deep(in_channels=3, out_channels=2, nfeatures=[4, 8, 8, 16, 16], emd=16).to(dev)
    ref_net, none_net = copy.deepcopy(net), copy.deepcopy(net)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 64, 64, generator=gen).to(dev)
    x_ema = (x.cpu() + 0.1 * torch.randn(2, 3, 64, 64, generator=gen)).to(dev)
    labels = torch.from_numpy(synth.synth_labels(2, (1, 64, 64), 5)[:, 0].copy()).to(torch.int32).to(dev)
    n1 = int((labels > 0).sum())
    assert 0 < n1 < labels.numel()
    kw = dict(shifts=(1, 2, 3, 5, 9), neighbor=4)

    st = pkg.CvpppTrainStep(net, torch.optim.SGD(net.parameters(), lr=0.0), mask_weight=1000, **kw)
    loss = st.step(x, x_ema, labels)
    st0 = pkg.CvpppTrainStep(none_net, torch.optim.SGD(none_net.parameters(), lr=0.0), mask_weight=None, **kw)
    loss0 = st0.step(x, x_ema, labels)
    torch.cuda.synchronize()
    seg0 = [p for n, p in none_net.named_parameters() if n.startswith("binary_seg.")]
    assert seg0 and all(p.grad is None for p in seg0)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(loss0))

    # the reference's term in eager (scripts_bbbc039v1/loss/loss.py:187-194)
    ref_net.train()
    pred_mask = ref_net(x)[5]
    target = torch.gt(labels, 0)
    weight = torch.tensor([float(torch.sum(target == 1).item()), float(torch.sum(target == 0).item())], device=dev)
    loss_mask = 1000.0 * torch.nn.CrossEntropyLoss(weight=weight)(pred_mask, target.long())
    loss_mask.backward()
    loss_mask = loss_mask.detach()
    print("step loss %.6g, without the mask term %.6g, the term in eager %.6g" % (float(loss), float(loss0), float(loss_mask)))
    assert abs((float(loss) - float(loss0)) - float(loss_mask)) <= 1e-4 * abs(float(loss))
    got = {n: p.grad for n, p in net.named_parameters() if n.startswith("binary_seg.")}
    want = {n: p.grad for n, p in ref_net.named_parameters() if n.startswith("binary_seg.")}
    assert set(got) == set(want) and len(got) >= 4
    # The largest reference magnitude is taken per LAYER (weight and bias of one module share their upstream gradient): the bias of
    # the first convolution feeds a BatchNorm on batch statistics, its gradient is zero analytically and both sides hold rounding noise
    # of the sums that make the weight's gradient -- noise has no magnitude of its own to be measured against.
    layers = sorted(set(n.rsplit(".", 1)[0] for n in want))
    for layer in layers:
        names = sorted(n for n in want if n.rsplit(".", 1)[0] == layer)
        top = max(float(want[n].abs().max()) for n in names)
        for n in names:
            assert got[n] is not None, n
            err = float((got[n] - want[n]).abs().max())
            print("%s: err %.3g of the layer's top %.3g" % (n, err, top))
            assert top > 0 and err <= RTOL_GRAD * top, (n, err, top)
