"""GPU (-m gpu): pea_consistency_unflip (include/pea_flip.h, csrc/pea_k_unflip.hip) -- the per-sample un-flip of the EMA embedding in
one launch, rules read on the device.

Every comparison is EXACT, on bit patterns (int16 / int32 views), against the torch composition convert_consistency_flip takes for
CPU tensors, which tests/test_unflip_host.py holds to the reference's 2D and 3D functions (goldens gflip_rules, gflip_rules_3d).
The inputs carry NaNs of distinct payloads, +-inf and -0: the call moves data and does no arithmetic.

The cases of the tile edges, the non-square planes and the NaN fill run through the C ABI inside a guard-banded arena (tests/arena.py)
with src and dst each ONE ELEMENT past a 256-byte boundary: any element-aligned pointer is served, every output element is written
and no byte outside dst changes."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from arena import Arena
from conftest import load_golden

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
NAN_BITS = {torch.float32: 0x7FC00000, torch.float16: 0x7E00, torch.bfloat16: 0x7FC0}  # what pea_flip.h fills a refused sample with
RULES3 = [[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
RULES4 = [[z] + r for z in (0, 1) for r in RULES3]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


def ibits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ibits(a.cpu()), ibits(b.cpu()))


def special_input(shape, dtype, seed):
    """normal values with, at random places, 16 NaNs of distinct payloads (quiet and signalling, both signs), +-inf and -0"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen).to(dtype)
    flat = ibits(x).view(-1)
    quiet, sign = (0x7FC00000, -0x80000000) if dtype == torch.float32 else ((0x7E00, -0x8000) if dtype == torch.float16 else (0x7FC0, -0x8000))
    snan = {torch.float32: 0x7F800000, torch.float16: 0x7C00, torch.bfloat16: 0x7F80}[dtype]
    vals = [quiet | k for k in range(1, 9)] + [snan | k for k in range(1, 5)] + [(quiet | k) + sign for k in range(9, 13)]
    inf = snan
    vals += [inf, inf + sign, sign, sign]  # +inf, -inf, -0, -0
    n = min(len(vals), flat.numel())
    where = torch.randperm(flat.numel(), generator=gen)[:n]
    flat[where] = torch.tensor(vals[:n], dtype=torch.int64).to(flat.dtype)
    return x


def run_in_arena(pkg, dev, x, rules, skew_elems=1):
    """pea_consistency_unflip on x (CPU tensor) / rules (uint8 list) through the C ABI, src and dst skew_elems elements past a
    256-byte boundary of a guard-banded arena; checks the guards, that src and the rules are unchanged and that every element of dst
    was written; returns dst on the host"""
    es = x.element_size()
    r = torch.tensor(rules, dtype=torch.uint8)
    ar = Arena(2 * x.numel() * es + 16 * 1024, dev)
    src = ar.carve(x.shape, x.dtype, skew_bytes=skew_elems * es, name="src")
    dst = ar.carve(x.shape, x.dtype, skew_bytes=skew_elems * es, name="dst")
    rv = ar.carve(r.shape, torch.uint8, skew_bytes=3, name="rules")
    ar.fill(src, x)
    ar.fill(rv, r)
    assert src.data_ptr() % 256 == skew_elems * es and dst.data_ptr() % 256 == skew_elems * es
    Z = x.shape[2] if x.dim() == 5 else 1
    code = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[x.dtype]
    rc = pkg._lib.lib().pea_consistency_unflip(x.shape[0], x.shape[1], Z, x.shape[-2], x.shape[-1], code, ctypes.c_void_p(src.data_ptr()),
                                                ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(rv.data_ptr()), 0, r.shape[1],
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    ar.check(written=[dst], untouched=[src, rv])
    return dst.cpu()


# ---- 1. the reference's own vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gflip_rules", "gflip_rules_3d"])
def test_goldens(pkg, dev, name):
    g = load_golden(name)
    x = torch.from_numpy(g["gt"]).to(dev)
    out = pkg.unflip(x, torch.from_numpy(g["rules"]).to(dev))
    assert not out.requires_grad and out.is_contiguous() and out.data_ptr() != x.data_ptr()
    assert same_bits(out, torch.from_numpy(g["out"]))
    assert same_bits(x, torch.from_numpy(g["gt"]))  # the source is only read


# ---- 2. tile edges: one full and one ragged 64-tile each way (70), a single ragged tile (5), a one-element second tile (65) ------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [70, 5, 65])
@pytest.mark.parametrize("ndim", [2, 3])
def test_tile_edges_every_rule(pkg, dev, ndim, n, dtype):
    rules = RULES3 if ndim == 2 else RULES4
    shape = (8, 3, n, n) if ndim == 2 else (16, 2, 3, n, n)
    x = special_input(shape, dtype, 100 * n + ndim)
    want = pkg.convert_consistency_flip(x, rules)
    assert same_bits(run_in_arena(pkg, dev, x, rules), want)
    assert same_bits(pkg.unflip(x.to(dev), torch.tensor(rules, dtype=torch.uint8, device=dev)), want)  # (an allocator-aligned pointer)


# ---- 3. non-square planes, no transpose -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(37, 70), (70, 37)])
def test_non_square_without_transpose(pkg, dev, hw, dtype):
    rules = [[rx, ry, 0] for rx in (0, 1) for ry in (0, 1)]
    x = special_input((4, 3) + hw, dtype, 7 + hw[0])
    assert same_bits(run_in_arena(pkg, dev, x, rules), pkg.convert_consistency_flip(x, rules))
    rules4 = [[rz, rx, ry, 0] for rz in (0, 1) for rx in (0, 1) for ry in (0, 1)]
    v = special_input((8, 2, 3) + hw, dtype, 11 + hw[0])
    assert same_bits(run_in_arena(pkg, dev, v, rules4), pkg.convert_consistency_flip(v, rules4))


# ---- 4. a transpose bit on a non-square plane: that sample NaN, the others served ----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(37, 70), (70, 37)])
@pytest.mark.parametrize("ndim", [2, 3])
def test_transpose_of_a_non_square_sample_is_nan(pkg, dev, ndim, hw, dtype):
    rules = [[1, 0, 0], [0, 1, 1], [1, 1, 0]] if ndim == 2 else [[1, 1, 0, 0], [1, 0, 1, 1], [0, 1, 1, 0]]
    x = special_input((3, 3) + ((3,) if ndim == 3 else ()) + hw, dtype, 23 + ndim + hw[0])
    out = run_in_arena(pkg, dev, x, rules)
    assert bool(torch.isnan(out[1]).all())
    assert bool((ibits(out[1]) == torch.tensor(NAN_BITS[dtype]).to(ibits(out).dtype)).all())
    keep = [0, 2]
    assert same_bits(out[keep], pkg.convert_consistency_flip(x[keep].contiguous(), [rules[i] for i in keep]))


# ---- 5. (the arena cases above: src and dst one element in, f32 / f16 / bf16); further skews of a 16-byte line -----------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_element_aligned_pointers(pkg, dev, dtype):
    x = special_input((8, 2, 70, 70), dtype, 31)
    want = pkg.convert_consistency_flip(x, RULES3)
    for skew in (0, 1, 2, 3):
        assert same_bits(run_in_arena(pkg, dev, x, RULES3, skew_elems=skew), want), skew


# ---- 6. every form the rules may come in ----------------------------------------------------------------------------------------------
def test_rules_dtypes(pkg, dev):
    g = load_golden("gflip_rules_3d")
    x = torch.from_numpy(g["gt"]).to(dev)
    r = torch.from_numpy(g["rules"])
    want = torch.from_numpy(g["out"])
    for dt in (torch.uint8, torch.int32, torch.int64, torch.float32, torch.bool, torch.int16, torch.float64, torch.float16):
        assert same_bits(pkg.unflip(x, r.to(dt).to(dev)), want), dt
        assert same_bits(pkg.convert_consistency_flip(x, r.to(dt).to(dev)), want), dt
        assert same_bits(pkg.convert_consistency_flip(x, r.to(dt)), want), dt          # a CPU tensor: uploaded
    assert same_bits(pkg.convert_consistency_flip(x, g["rules"].tolist()), want)      # a host list
    assert same_bits(pkg.convert_consistency_flip(x, g["rules"].astype(np.int64)), want)
    assert same_bits(pkg.convert_consistency_flip(x, None), torch.from_numpy(g["gt"]))
    # a device tensor of a dtype the kernel does not move keeps the torch composition, as before pea_consistency_unflip
    for dt in (torch.float64, torch.int32):
        out = pkg.convert_consistency_flip(x.to(dt), r.to(dev))
        assert out.is_cuda and out.dtype == dt and torch.equal(out.cpu(), want.to(dt))
    with pytest.raises(ValueError):
        pkg.unflip(x[:, :, 0].contiguous(), r.to(dev))
    with pytest.raises(ValueError):
        pkg.unflip(x, r[:8].to(dev))
    with pytest.raises(TypeError):
        pkg.unflip(x.double(), r.to(dev))
    with pytest.raises(RuntimeError):
        pkg.unflip(x, r)


# ---- 7. the training shape, against the function this call replaces ------------------------------------------------------------------
def parent_convert_consistency_flip(ema_embedding, rules):
    """harness/train_step.convert_consistency_flip as it was before pea_consistency_unflip"""
    out = ema_embedding.detach().clone()
    r = rules.detach().cpu().numpy().astype(np.uint8)
    parts = []
    for b in range(out.shape[0]):
        t = out[b]
        if r[b][2]:
            t = t.transpose(-1, -2)
        if r[b][1]:
            t = t.flip(-2)
        if r[b][0]:
            t = t.flip(-1)
        parts.append(t)
    return torch.stack(parts, dim=0)


def test_training_shape(pkg, dev):
    gen = torch.Generator().manual_seed(544)
    x = torch.randn((2, 16, 544, 544), generator=gen).to(dev)
    drawn = torch.randint(0, 2, (3, 2, 3), generator=gen).tolist()  # random rules, as the data provider draws them
    for rules in drawn + [[[1, 0, 1], [0, 1, 0]], [[0, 0, 0], [1, 1, 1]]]:  # .. and two sets that take both paths whatever was drawn
        r = torch.tensor(rules, dtype=torch.float32, device=dev)
        assert same_bits(pkg.convert_consistency_flip(x, r), parent_convert_consistency_flip(x, r))


# ---- 8. graph capture: the replay reads the rules afresh -----------------------------------------------------------------------------
def test_graphed_unflip_and_cross_loss_follow_the_rules(pkg, dev, synth):
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    crit = pkg.WeightedMSE()
    e, t, w, m = synth.synth_inputs_2d(2, 16, 96, 96, offsets, seed=81)
    E, T, W, M = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (e, t, w, m))
    ema = torch.from_numpy(synth.synth_embedding((2, 16, 96, 96), 82)).to(dev)
    rules_dev = torch.tensor([[0, 0, 0], [1, 0, 1]], dtype=torch.float32, device=dev)

    def fn(ema, rules_dev):
        un = pkg.convert_consistency_flip(ema, rules_dev)
        loss, affs = pkg.ema_embedding_loss(E, un, T, W, M, crit, offsets)
        return un, loss, affs

    g = pkg.graphed(fn, ema, rules_dev)
    seen = []
    for rules in ([[1, 1, 0], [0, 1, 1]], [[1, 0, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 0]]):
        rules_dev.copy_(torch.tensor(rules, dtype=torch.float32))
        un, loss, affs = g.replay()
        u0, l0, a0 = fn(ema, rules_dev.clone())
        assert same_bits(un, pkg.convert_consistency_flip(ema.cpu(), rules))
        assert same_bits(un, u0) and torch.equal(loss, l0) and torch.equal(affs, a0)
        seen.append(float(loss))
    assert len(set(seen)) == 3  # (the three rule sets do give three different losses)


# ---- 9. the 3D form through the package's function -----------------------------------------------------------------------------------
def test_convert_consistency_flip_3d_on_the_device(pkg, dev):
    g = load_golden("gflip_rules_3d")
    x = torch.from_numpy(g["gt"]).to(dev).requires_grad_(True)
    out = pkg.convert_consistency_flip(x, torch.from_numpy(g["rules"]).to(dev))
    assert out.is_cuda and not out.requires_grad and same_bits(out, torch.from_numpy(g["out"]))
