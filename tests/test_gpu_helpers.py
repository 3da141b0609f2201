"""GPU: the small helpers of csrc/pea_k_direct.hip through the C ABI, each call in a guard-banded arena (arena.py) -- pea_scale_inplace
and pea_scale_inplace_multi (the gradient's grad_output), pea_weighted_sum (the total of a loss section), pea_stitch_add and
pea_stitch_finalize (the 3D inference stitcher).  tests/test_helpers_host.py pins their refusals.

Scaling.  The reference is (x.float() * sc).to(dtype) on the CPU, compared by bits: an IEEE f32 product and one rounding are fully
determined (for the 16-bit types the chosen scales make the f32 product exact, so the conversion is the only rounding whether or not the
compiler fuses the two).  What IEEE 754 leaves open is the sign and payload of a NaN result -- x86 answers inf * 0 with 0xffc00000, the
GPU with 0x7fc00000 -- so where the reference holds a NaN the result must be a NaN, and everywhere else the bits must agree.  With a scale
of exactly 1 the kernels return without touching the buffer: every bit, NaN payloads included, is the input's.

Case sizing.  k_scale_inplace<float> has a body of n / 4 quads and a tail of n % 4 elements that shares the first workgroup; the 16-bit
form takes four elements per lane.  k_scale_multi runs a grid-stride loop on at most 512 workgroups of 256 lanes: the vector route (an
f32 buffer on 16 bytes) takes a second stride above 524 288 elements, the scalar route (every other buffer) above 131 072; the one large
buffer holds 600 000 elements.

pea_weighted_sum promises a fixed order of additions, not separately rounded products (the compiler may fuse each step): each of the n
steps rounds at most twice, on magnitudes no larger than sum_j |w_j r_j|, so |got - float64 sum| <= n * 2^-23 * sum_j |w_j r_j| -- derived,
not measured; the observed error is printed beside it.

The stitcher promises a separate f32 multiply, add and divide: bit-equal to the numpy statements (NaN for NaN, as above)."""
import ctypes

import numpy as np
import pytest
import torch

from arena import Arena

pytestmark = pytest.mark.gpu
DTYPES = {"f32": (torch.float32, 0), "f16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}
SCALES = {"one": 1.0, "zero": 0.0, "m3.5": -3.5, "2^-20": 2.0 ** -20}
INT_OF = {4: torch.int32, 2: torch.int16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bits(t):
    return t.contiguous().view(INT_OF[t.element_size()])


def same_ieee(got, want):
    """bit for bit where `want` is a number; a NaN (of any sign and payload) where it is a NaN"""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    return bool(torch.isnan(got[nan]).all()) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def scale_data(n, dtype, seed):
    """n values of mixed magnitude; from 16 elements on also NaN, +-inf, the largest finite value of either sign and +-0, the last
    element among them (the tail of the f32 kernel); two NaNs carry a payload, one of them signalling"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)).to(dtype)
    if n >= 16:
        big = torch.finfo(dtype).max
        for k, v in enumerate((float("inf"), float("nan"), float("-inf"), big, -0.0, -big, 0.0, float("nan"), float("nan"))):
            x[(n - 1 - k * (n // 9)) % n] = v
        payload = {torch.float32: (0x7FC12345, 0x7F800001), torch.float16: (0x7E01, 0x7C01), torch.bfloat16: (0x7FC1, 0x7F81)}[dtype]
        bits(x)[(n - 1 - 7 * (n // 9)) % n] = payload[0]
        bits(x)[(n - 1 - 8 * (n // 9)) % n] = payload[1]
        assert int(torch.isnan(x).sum()) == 3
    return x


def scaled(x, sc):
    return x.clone() if sc == 1.0 else (x.float() * sc).to(x.dtype)


# ---- pea_scale_inplace ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_scale_inplace(pkg, dev, dtype, scale):
    L = pkg._lib.lib()
    tdt, code = DTYPES[dtype]
    sc = SCALES[scale]
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099):
        x = scale_data(n, tdt, 100 + n)
        want = scaled(x, sc)
        for skew in ((0, 16, 48) if tdt == torch.float32 else (0, 2, 6)):  # f32 on its 16 bytes; the 16-bit types on their element
            ar = Arena(n * 4 + (1 << 14), dev)
            view = ar.fill(ar.carve((1, n), tdt, skew, name="buf+%d" % skew), x[None])  # (one batch item: the arena walks a batch in Python)
            buf = view[0]
            s = ar.fill(ar.carve((1,), torch.float32, 4, name="scale"), torch.tensor([sc]))
            pkg._lib.check(L.pea_scale_inplace(vp(buf), code, ctypes.c_size_t(n), vp(s), None), "pea_scale_inplace")
            torch.cuda.synchronize()
            if sc == 1.0:
                ar.check(untouched=[view, s])  # not a bit moves, NaN payloads included
                assert torch.equal(bits(buf.cpu()), bits(x))
            else:
                ar.check(untouched=[s], scratch=[view])
                assert same_ieee(buf, want), (dtype, scale, n, skew)
        if n == 1025 and sc == 0.0:  # what the zero scale makes: signed zeros, and NaN from inf
            w = want.float()
            assert bool(torch.isnan(w[torch.isinf(x.float())]).all()) and bool((bits(want)[(x.float() < 0) & torch.isfinite(x.float())] != 0).all())
        if n == 4099 and sc == 2.0 ** -20 and dtype == "f16":  # subnormal results, not flushed
            w = want.float().abs()
            assert int(((w > 0) & (w < 2.0 ** -14)).sum()) > 100


# ---- pea_scale_inplace_multi ------------------------------------------------------------------------------------------------------------------
BIG = 600000
# (count, skew in f32 elements past 16 bytes) per buffer.  An f32 buffer with skew 0 takes the vector route, any other the scalar one.
MULTI = {
    "one_buffer": [(5, 0)],
    "three": [(4099, 1), (0, 0), (1, 0)],
    "eight_big_aligned": [(BIG, 0), (5, 1), (0, 0), (1, 3), (4099, 0), (3, 2), (1025, 1), (4, 0)],
    "big_skewed": [(BIG, 1), (4099, 0)],
}


@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("config", sorted(MULTI))
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_scale_inplace_multi(pkg, dev, dtype, config, scale):
    L = pkg._lib.lib()
    tdt, code = DTYPES[dtype]
    item = torch.empty((), dtype=tdt).element_size()
    sc = SCALES[scale]
    cfg = MULTI[config]
    ar = Arena(sum(max(c, 8) for c, _ in cfg) * item + len(cfg) * 4096 + (1 << 14), dev)
    bufs, data = [], []
    for k, (count, skew) in enumerate(cfg):
        m = count or 8  # a count-0 buffer still has eight elements behind its pointer
        x = scale_data(max(m, 8), tdt, 7 * k + count)[:m]
        data.append(x)
        bufs.append(ar.fill(ar.carve((1, m), tdt, skew * item, name="buf%d" % k), x[None]))  # (one batch item, as above)
        assert bufs[-1].data_ptr() % 16 == (skew * item) % 16
    s = ar.fill(ar.carve((1,), torch.float32, 8, name="scale"), torch.tensor([sc]))
    ptrs = (ctypes.c_void_p * len(cfg))(*[b.data_ptr() for b in bufs])
    counts = (ctypes.c_size_t * len(cfg))(*[c for c, _ in cfg])
    pkg._lib.check(L.pea_scale_inplace_multi(ptrs, counts, len(cfg), code, vp(s), None), "pea_scale_inplace_multi")
    torch.cuda.synchronize()
    idle = [b for b, (c, _) in zip(bufs, cfg) if c == 0 or sc == 1.0]
    ar.check(untouched=[s] + idle, scratch=[b for b in bufs if not any(b is i for i in idle)])  # guard bands, and a count-0 buffer's own bytes
    for b, x, (count, _) in zip(bufs, data, cfg):
        if count and sc != 1.0:
            assert same_ieee(b[0], scaled(x[:count], sc)), (dtype, config, scale, count)


# ---- pea_weighted_sum --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", (1, 11))
@pytest.mark.parametrize("n", (1, 2, 11, 64))
def test_weighted_sum(pkg, dev, n, stride):
    L = pkg._lib.lib()
    rng = np.random.default_rng(1000 + 64 * stride + n)
    mixed = lambda k: (rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-6, 4, k)).astype(np.float32)
    r, w = mixed(n), mixed(n)
    rows = np.full(((n - 1) * stride + 1,), np.nan, np.float32)  # NaN between the rows: read one and the sum is NaN
    rows[::stride] = r
    ref = float(np.sum(w.astype(np.float64) * r.astype(np.float64)))
    bound = n * 2.0 ** -23 * float(np.sum(np.abs(w.astype(np.float64) * r.astype(np.float64))))
    ar = Arena(1 << 14, dev)
    R = ar.fill(ar.carve(rows.shape, torch.float32, 4, name="rows"), torch.from_numpy(rows))
    W = ar.fill(ar.carve((n,), torch.float32, 12, name="w"), torch.from_numpy(w))
    before = torch.tensor([3.0, -7.0, float("nan"), 11.0])
    out = ar.fill(ar.carve((4,), torch.float32, 8, name="out"), before)
    seen = []
    for _ in range(10):
        pkg._lib.check(L.pea_weighted_sum(vp(R), stride, vp(W), n, vp(out), None), "pea_weighted_sum")
        torch.cuda.synchronize()
        seen.append(out.cpu().clone())
    ar.check(untouched=[R, W], scratch=[out])
    got = float(seen[0][0])
    print("n %d stride %d: got %.9g float64 %.17g |error| %.3e bound %.3e" % (n, stride, got, ref, abs(got - ref), bound))
    assert abs(got - ref) <= bound
    assert all(torch.equal(bits(s), bits(seen[0])) for s in seen), "ten calls, ten answers"
    assert torch.equal(bits(seen[0])[1:], bits(before)[1:]), "only out[0] may change"


# ---- the stitcher -----------------------------------------------------------------------------------------------------------------------------
VOL = (5, 9, 11)
WINDOWS = {  # name -> the adds in order: (window size, origin)
    "one_voxel": [((1, 1, 1), (2, 4, 5))],
    "origin": [((2, 3, 5), (0, 0, 0))],
    "far_corner": [((2, 3, 5), (3, 6, 6))],
    "whole": [(VOL, (0, 0, 0))],
    "two_overlapping": [((2, 3, 5), (1, 2, 3)), ((3, 5, 7), (2, 3, 4))],
}


def np_stitch_add(out, wmap, vol, wv, at):
    """provider_valid.add_vol: a separate f32 multiply and add"""
    z0, y0, x0 = at
    oz, oy, ox = wv.shape
    prod = (vol * wv[None]).astype(np.float32)
    out[:, z0:z0 + oz, y0:y0 + oy, x0:x0 + ox] = out[:, z0:z0 + oz, y0:y0 + oy, x0:x0 + ox] + prod
    wmap[z0:z0 + oz, y0:y0 + oy, x0:x0 + ox] = wmap[z0:z0 + oz, y0:y0 + oy, x0:x0 + ox] + wv
    return prod


@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_stitch_add(pkg, dev, name, C):
    L = pkg._lib.lib()
    rng = np.random.default_rng(31 * C + len(name))
    Z, Y, X = VOL
    out0 = rng.standard_normal((C, Z, Y, X)).astype(np.float32)
    wmap0 = rng.uniform(0.1, 3.0, (Z, Y, X)).astype(np.float32)
    ar = Arena(1 << 16, dev)
    O = ar.fill(ar.carve(out0.shape, torch.float32, 4, name="out_affs"), torch.from_numpy(out0))
    Wm = ar.fill(ar.carve(wmap0.shape, torch.float32, 12, name="weight_map"), torch.from_numpy(wmap0))
    want_o, want_w = out0.copy(), wmap0.copy()
    fused_differs, read_only = 0, []
    for k, (win, at) in enumerate(WINDOWS[name]):
        assert int(np.prod(win)) % 256 != 0
        vol = rng.standard_normal((C,) + tuple(win)).astype(np.float32)
        wv = rng.uniform(0.05, 1.0, win).astype(np.float32)
        V = ar.fill(ar.carve(vol.shape, torch.float32, 8, name="affs_vol%d" % k), torch.from_numpy(vol))
        Wv = ar.fill(ar.carve(wv.shape, torch.float32, 4, name="weight_vol%d" % k), torch.from_numpy(wv))
        read_only += [V, Wv]
        sl = (slice(None),) + tuple(slice(a, a + s) for a, s in zip(at, win))
        fused = (vol.astype(np.float64) * wv[None].astype(np.float64) + want_o[sl].astype(np.float64)).astype(np.float32)  # one rounding
        np_stitch_add(want_o, want_w, vol, wv, at)
        fused_differs += int((fused != want_o[sl]).sum())
        pkg._lib.check(L.pea_stitch_add(vp(O), vp(Wm), vp(V), vp(Wv), C, Z, Y, X, *win, *at, None), "pea_stitch_add")
    torch.cuda.synchronize()
    ar.check(untouched=read_only, scratch=[O, Wm])
    print("%s C=%d: %d of the touched voxels would differ under a fused multiply-add" % (name, C, fused_differs))
    if name in ("whole", "two_overlapping"):
        assert fused_differs > 0  # the data can tell a * b + c in one rounding from two
    assert torch.equal(bits(O.cpu()), bits(torch.from_numpy(want_o))), "out_affs: inside the window the numpy statement, outside it the old bits"
    assert torch.equal(bits(Wm.cpu()), bits(torch.from_numpy(want_w))), "weight_map"
    outside = np.ones(VOL, bool)
    for win, at in WINDOWS[name]:
        outside[tuple(slice(a, a + s) for a, s in zip(at, win))] = False
    assert np.array_equal(want_o[:, outside].view(np.int32), out0[:, outside].view(np.int32)) and outside.any() == (name != "whole")


@pytest.mark.parametrize("C", (1, 3))
def test_stitch_finalize(pkg, dev, C):
    L = pkg._lib.lib()
    rng = np.random.default_rng(77 + C)
    S = int(np.prod(VOL))
    out0 = rng.standard_normal((C, S)).astype(np.float32)
    wmap = rng.uniform(0.05, 4.0, S).astype(np.float32)
    wmap[[0, 3, 100, 255, 256, S - 1]] = 0.0  # never covered by a window: numpy divides by zero there, and so must the kernel
    out0[:, 3] = 0.0
    out0[0, 100] = -0.0
    out0[:, 255] = -np.abs(out0[:, 255]) - 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        want = (out0 / wmap[None]).astype(np.float32)
    assert np.isnan(want[:, 3]).all() and np.isposinf(want[:, 0]).sum() + np.isneginf(want[:, 0]).sum() == C and np.isneginf(want[:, 255]).all()
    for voxels in (S, 300, 1):
        ar = Arena(1 << 16, dev)
        O = ar.fill(ar.carve(out0.shape, torch.float32, 12, name="out_affs"), torch.from_numpy(out0))
        Wm = ar.fill(ar.carve(wmap.shape, torch.float32, 4, name="weight_map"), torch.from_numpy(wmap))
        # with voxels < S the call sees C planes of `voxels` elements at the head of the buffer
        pkg._lib.check(L.pea_stitch_finalize(vp(O), vp(Wm), C, ctypes.c_size_t(voxels), None), "pea_stitch_finalize")
        torch.cuda.synchronize()
        ar.check(untouched=[Wm], scratch=[O])
        flat0 = out0.reshape(-1).copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            flat0[:C * voxels] = (flat0[:C * voxels].reshape(C, voxels) / wmap[None, :voxels]).reshape(-1)
        assert same_ieee(O.reshape(-1), torch.from_numpy(flat0)), voxels
        if voxels == S:
            assert same_ieee(O, torch.from_numpy(want))
