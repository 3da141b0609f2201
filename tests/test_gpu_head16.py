"""GPU (-m gpu): the embedding head on 16-bit features -- pea_head_fwd_t / pea_head_bwd_t (include/pea_head16.h, csrc/pea_head.h) and
the Python layer on top of them (model/head.py, harness/head_loss.py).

The C ABI runs on all twelve (C, D) pairs, both 16-bit types, the embedding in the same type and in f32, B = 2, inside a guard-banded
arena (tests/arena.py) at three sets of pointer residues, against oracle.np_head_fwd / np_head_bwd (float64) on the inputs AS ROUNDED to
the 16-bit type.  The shapes are small on purpose: every one still has more than one workgroup or a ragged / short last chunk, S odd
and even, C not a multiple of 16, the channel-chunked heads.

Tolerances (derived, not tuned; u = 2^-11 for f16, 2^-8 for bf16 -- half an ulp, relative):
  a 16-bit e / dx   |got - ref| <= u |ref| + 2e-5 max|ref|   one rounding to nearest even of an f32 sum, plus the slack the f32 head tests
                                                             allow for the f32 sum itself
  an f32 e          1e-5 max|ref|                            as test_head_wide_and_3d_channel_pairs_vs_oracle
  dW, db            2e-5 max|ref|                            as there: 16-bit inputs are exact in f32, the sums are the f32 head's
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from arena import Arena

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
CODE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
B = 2
# (C, D), spatial
SHAPES = [((32, 16), (40, 56)),      # ragged last chunk
          ((32, 16), (17, 19)),      # S = 323: odd, more than one chunk, the planes of odd channels 2 bytes off
          ((64, 32), (9, 11)),       # S = 99: less than a chunk
          ((28, 16), (5, 16, 24)),
          ((36, 16), (5, 16, 24)),   # C not a multiple of 16
          ((48, 16), (40, 40)),
          ((64, 16), (16, 24)),
          ((80, 16), (3, 20, 20)),
          ((128, 16), (17, 40)),
          ((256, 16), (34, 34)),     # channel-chunked
          ((128, 32), (17, 40)),
          ((256, 32), (9, 11))]
# pointer residues modulo 256, in bytes: (x, W, bias, e / de as 16-bit, e / de as f32, dx, dW, db, workspace)
RESIDUES = {
    "aligned": dict(x=0, W=0, bias=0, e16=0, e32=0, dx=0, dW=0, db=0, ws=0),           # the packed form wherever S is even
    "element": dict(x=2, W=4, bias=12, e16=6, e32=4, dx=10, dW=4, db=12, ws=4),        # element-aligned, no 16-bit tensor on a dword
    "dword": dict(x=4, W=4, bias=12, e16=12, e32=8, dx=12, dW=12, db=4, ws=12),        # 4 (f32 e: 8) but not 16 bytes: packed, no wider
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def npf(t):
    return t.detach().float().cpu().numpy()


def check16(name, got, ref, u):
    """a 16-bit result: u |ref| + 2e-5 max|ref| element-wise (module docstring); prints the worst ratio before it asserts"""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    bound = u * np.abs(ref) + 2e-5 * np.abs(ref).max()
    ratio = float((np.abs(got - ref) / bound).max())
    print("%s: worst |got - ref| / bound = %.3f" % (name, ratio))
    assert np.isfinite(got).all() and ratio <= 1.0, (name, ratio)


def check32(name, got, ref, rel):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("%s: max |got - ref| / max|ref| = %.3g (bound %.0e)" % (name, err, rel))
    assert np.isfinite(got).all() and err <= rel, (name, err)


def make_inputs(C, D, sp, dtype, e_dtype, seed):
    """x, de ~ N(0, 1) rounded to their storage types; W ~ 0.2 N (0.1 for C > 64) and bias ~ N in f32"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C) + sp, generator=gen).to(dtype)
    W = torch.randn((D, C), generator=gen) * (0.2 if C <= 64 else 0.1)
    bias = torch.randn(D, generator=gen)
    de = torch.randn((B, D) + sp, generator=gen).to(e_dtype)
    return x, W, bias, de


def run_in_arena(pkg, dev, res, x, W, bias, de):
    """forward, backward, the backward again, and the backward without dx / db through the C ABI inside a guard-banded arena at
    the residues `res`; asserts the arena's invariants after every call and returns the outputs on the device"""
    L = pkg._lib.lib()
    (_, C), D = x.shape[:2], W.shape[0]
    S = x[0, 0].numel()
    dt, et = x.dtype, de.dtype
    eres = res["e32"] if et == torch.float32 else res["e16"]
    wsb = L.pea_head_workspace_bytes(C, D)
    total = wsb + 3 * x.numel() * x.element_size() + 4 * de.numel() * de.element_size() + 5 * W.numel() * 4 + 64 * 1024
    ar = Arena(total, dev)
    xv = ar.fill(ar.carve(x.shape, dt, res["x"], name="x"), x)
    Wv = ar.fill(ar.carve(W.shape, torch.float32, res["W"], name="W"), W)
    bv = ar.fill(ar.carve(bias.shape, torch.float32, res["bias"], name="bias"), bias)
    dev_ = ar.fill(ar.carve(de.shape, et, eres, name="de"), de)
    e1, e2 = (ar.carve(de.shape, et, eres, name="e%d" % i) for i in (1, 2))
    dx1, dx2 = (ar.carve(x.shape, dt, res["dx"], name="dx%d" % i) for i in (1, 2))
    dW1, dW2, dW3 = (ar.carve(W.shape, torch.float32, res["dW"], name="dW%d" % i) for i in (1, 2, 3))
    db1, db2 = (ar.carve(bias.shape, torch.float32, res["db"], name="db%d" % i) for i in (1, 2))
    ws = ar.carve((1, wsb // 4), torch.float32, res["ws"], name="workspace")  # one batch item: the arena walks a view per item
    for v, r in ((xv, res["x"]), (e1, eres), (dx1, res["dx"]), (dW1, res["dW"]), (ws, res["ws"])):
        assert v.data_ptr() % 256 == r
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xt, ec = CODE[dt], CODE[et]
    assert L.pea_head_supported_t(C, D, xt, ec) == 1
    ro = [xv, Wv, bv, dev_]
    done = []

    def fwd(e):
        assert L.pea_head_fwd_t(B, C, D, S, p(xv), xt, p(Wv), p(bv), p(e), ec, st) == 0
        torch.cuda.synchronize()
        done.append(e)
        ar.check(written=done, untouched=ro, scratch=[ws])

    def bwd(dx, dW, db):
        assert L.pea_head_bwd_t(B, C, D, S, p(xv), xt, p(Wv), p(dev_), ec, p(dx), p(dW), p(db), p(ws), wsb, st) == 0
        torch.cuda.synchronize()
        done.extend(t for t in (dx, dW, db) if t is not None)
        ar.check(written=done, untouched=ro, scratch=[ws])

    fwd(e1)
    fwd(e2)
    bwd(dx1, dW1, db1)
    bwd(dx2, dW2, db2)
    bwd(None, dW3, None)
    # two runs are bit-identical; dW does not depend on the optional outputs
    assert same_bits(e1, e2) and same_bits(dx1, dx2) and same_bits(dW1, dW2) and same_bits(db1, db2)
    assert same_bits(dW1, dW3)
    return e1, dx1, dW1, db1


@pytest.mark.parametrize("e_f32", [False, True], ids=["e16", "e32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cd,sp", SHAPES, ids=["%dto%d_%s" % (c, d, "x".join(map(str, sp))) for (c, d), sp in SHAPES])
def test_c_abi_vs_oracle_at_every_residue(pkg, dev, orc, cd, sp, dtype, e_f32):
    C, D = cd
    e_dtype = torch.float32 if e_f32 else dtype
    x, W, bias, de = make_inputs(C, D, sp, dtype, e_dtype, 1000 * C + D + len(sp))
    xn, Wn, bn, den = x.float().numpy(), W.numpy(), bias.numpy(), de.float().numpy()
    e_ref = orc.np_head_fwd(xn, Wn, bn)              # float64 inside, on the rounded inputs; computed once for the three residues
    dx_ref, dW_ref, db_ref = orc.np_head_bwd(xn, Wn, den)
    assert np.abs(e_ref).max() < 100                 # far below the f16 maximum
    u = UNIT[dtype]
    S = int(np.prod(sp))
    for name, res in RESIDUES.items():
        tag = "%s S=%d %s" % (name, S, "odd" if S % 2 else "even")
        e, dx, dW, db = run_in_arena(pkg, dev, res, x, W, bias, de)
        assert e.dtype == e_dtype and dx.dtype == dtype
        if e_f32:
            check32(tag + " e", npf(e), e_ref, 1e-5)
        else:
            check16(tag + " e", npf(e), e_ref, u)
        check16(tag + " dx", npf(dx), dx_ref, u)
        check32(tag + " dW", npf(dW), dW_ref, 2e-5)
        check32(tag + " db", npf(db), db_ref, 2e-5)


def _head(pkg, dev, C, D, three_d, seed):
    head = (pkg.head_conv3d_block(C, D) if three_d else pkg.OutConv(C, D)).to(dev)
    conv = head[0] if three_d else head.conv
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=gen) * 0.2).to(dev))
        conv.bias.copy_(torch.randn(D, generator=gen).to(dev))
    return head, conv


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("three_d", [False, True], ids=["OutConv", "conv3d_block"])
def test_modules_on_16bit_features(pkg, dev, dtype, three_d):
    """OutConv / head_conv3d_block on f16 / bf16 x with the f32 master weight, inside and outside torch.autocast: bit-equal to
    EmbeddingHead.apply; e and x.grad in x.dtype, weight.grad / bias.grad in f32; out_dtype = torch.float32 gives an f32 e; a 16-bit
    weight (model.half()) goes to torch's convolution"""
    C, D = (28, 16) if three_d else (32, 16)
    sp = (3, 10, 14) if three_d else (17, 19)
    head, conv = _head(pkg, dev, C, D, three_d, 3)
    gen = torch.Generator().manual_seed(4)
    x0 = torch.randn((B, C) + sp, generator=gen).to(dtype).to(dev)
    up = torch.randn((B, D) + sp, generator=gen).to(dev)

    def run(fn, out_dtype=None):
        x = x0.clone().requires_grad_(True)
        conv.weight.grad = conv.bias.grad = None
        e = fn(x)
        assert e.dtype == (out_dtype or dtype)
        (e.float() * up).sum().backward()
        assert x.grad.dtype == dtype and conv.weight.grad.dtype == torch.float32 and conv.bias.grad.dtype == torch.float32
        assert conv.weight.grad.shape == conv.weight.shape
        return e.detach(), x.grad, conv.weight.grad.clone(), conv.bias.grad.clone()

    ref = run(lambda x: pkg.EmbeddingHead.apply(x, conv.weight, conv.bias, None))
    plain = run(head)
    with torch.autocast("cuda", dtype=dtype):
        cast = run(head)
    for got in (plain, cast):
        assert all(same_bits(a, b) for a, b in zip(got, ref))
    # the f32 embedding from the same features: the same sums, not rounded
    head.out_dtype = torch.float32
    ref32 = run(lambda x: pkg.EmbeddingHead.apply(x, conv.weight, conv.bias, torch.float32), torch.float32)
    got32 = run(head, torch.float32)
    with torch.autocast("cuda", dtype=dtype):
        cast32 = run(head, torch.float32)
    assert all(same_bits(a, b) for a, b in zip(got32, ref32)) and all(same_bits(a, b) for a, b in zip(cast32, ref32))
    assert same_bits(ref32[0].to(dtype), ref[0])     # rounding the f32 embedding once gives the 16-bit one
    head.out_dtype = None
    # a 16-bit weight stays with torch
    half = head.to(dtype)
    e_t = half(x0)
    conv_t = torch.nn.functional.conv3d if three_d else torch.nn.functional.conv2d
    assert same_bits(e_t, conv_t(x0, conv.weight, conv.bias))
    with pytest.raises(RuntimeError):
        pkg.OutConv(32, 16)(torch.zeros(1, 32, 8, 8, dtype=dtype))  # CPU tensors are refused, no fallback


@pytest.mark.parametrize("dtype,with_other_loss", [(torch.bfloat16, False), (torch.float16, False), (torch.bfloat16, True)],
                         ids=["bf16", "f16", "bf16_other_loss"])
def test_head_embedding_loss_on_16bit_features(pkg, dev, synth, dtype, with_other_loss):
    """head_embedding_loss on f16 / bf16 x is, bit for bit, head(x) + embedding_loss(...) + backward() of the same package: loss, affs,
    per-offset losses, embedding, x.grad, weight.grad, bias.grad; with_other_loss: a gradient from outside into `embedding`"""
    C, D, H, W = 32, 16, 72, 96
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], neighbor=4)
    _, t, w, m = synth.synth_inputs_2d(B, D, H, W, offsets, 5)
    T, Wm, M = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (t, w, m))
    gen = torch.Generator().manual_seed(12)
    x0 = torch.randn((B, C, H, W), generator=gen).to(dtype).to(dev)
    R = (torch.randn((B, D, H, W), generator=gen) * 1e-3).to(dev)
    crit = pkg.WeightedMSE()

    def run(fused):
        head, conv = _head(pkg, dev, C, D, False, 8)
        x = x0.clone().requires_grad_(True)
        if fused:
            loss, affs, parts, emb = pkg.head_embedding_loss(x, head, T, Wm, M, crit, offsets)
        else:
            emb = head(x)
            loss, affs, parts = pkg.embedding_loss(emb, T, Wm, M, crit, offsets)
        assert emb.dtype == dtype and loss.dtype == torch.float32
        total = loss * 0.5
        if with_other_loss:
            total = total + (emb * R.to(dtype)).sum().float()
        total.backward()
        assert x.grad.dtype == dtype and conv.weight.grad.dtype == torch.float32 and conv.bias.grad.dtype == torch.float32
        return (loss.detach(), affs, torch.tensor(list(parts)), emb.detach(), x.grad, conv.weight.grad, conv.bias.grad)

    fused, separate = run(True), run(False)
    names = ("loss", "affs", "per-offset losses", "embedding", "x.grad", "weight.grad", "bias.grad")
    for name, a, b in zip(names, fused, separate):
        assert same_bits(a, b), name
    assert bool(torch.isfinite(fused[4].float()).all()) and float(fused[4].float().abs().max()) > 0
    with pytest.raises(RuntimeError):
        pkg.head_embedding_loss(x0.cpu(), _head(pkg, "cpu", C, D, False, 8)[0], T.cpu(), Wm.cpu(), M.cpu(), crit, offsets)
