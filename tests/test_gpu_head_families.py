"""GPU (-m gpu): the two entry families of the embedding head carry each other's bits (csrc/pea_head.h).

pea_head_fwd / pea_head_bwd (f32 features) and pea_head_fwd_t / pea_head_bwd_t (f16 / bf16 features, here with an f32 embedding) are
the same arithmetic: f32 products and sums with the f32 W, bias first, then c ascending; dW on the same MFMA tiles.  x and de are drawn
in the 16-bit type, so they are exact in f32, and the f32 head runs on the upcast tensors.  Then, for every (C, D) pair:

  e         bit-equal, at every form (the two forwards share the order of additions per accumulator)
  dx        the 16-bit dx is the f32 dx rounded once to nearest even (torch's .to(dtype)), bit for bit, at every form
  dW, db    bit-equal wherever the 16-bit call takes the element form for dW -- one pixel per lane, the f32 head's assignment of pixels
            to MFMA k slots, the same chunks, the same number of workgroups --: the "element" residues, an odd S, and C > 64 (the
            channel-chunked heads keep the element form).  In the packed form (the "aligned" residues, S even, C <= 64) a lane holds two
            pixels and the chunks are 512 pixels, so the sums are taken in another order: there dW and db are held to the 2e-5 max|ref|
            that tests/test_gpu_head16.py derives for them.

Shapes, inputs, the arena and its residue sets are those of tests/test_gpu_head16.py."""
import ctypes

import pytest
import torch

import test_gpu_head16 as h16

pytestmark = pytest.mark.gpu

dev = h16.dev  # module-scoped fixture


def f32_head(pkg, dev, x, W, bias, de):
    """pea_head_fwd / pea_head_bwd on f32 tensors -> e, dx, dW, db"""
    L = pkg._lib.lib()
    (B, C), D = x.shape[:2], W.shape[0]
    S = x[0, 0].numel()
    xd, Wd, bd, ded = (t.to(dev).contiguous() for t in (x, W, bias, de))
    e, dx, dW, db = torch.empty_like(ded), torch.empty_like(xd), torch.empty_like(Wd), torch.empty_like(bd)
    wsb = L.pea_head_workspace_bytes(C, D)
    ws = torch.empty(wsb // 4, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.pea_head_fwd(B, C, D, S, p(xd), p(Wd), p(bd), p(e), st) == 0
    assert L.pea_head_bwd(B, C, D, S, p(xd), p(Wd), p(ded), p(dx), p(dW), p(db), p(ws), wsb, st) == 0
    torch.cuda.synchronize()
    return e, dx, dW, db


@pytest.mark.parametrize("dtype", h16.DTYPES, ids=h16.IDS)
@pytest.mark.parametrize("cd,sp", h16.SHAPES, ids=["%dto%d_%s" % (c, d, "x".join(map(str, sp))) for (c, d), sp in h16.SHAPES])
def test_f32_head_and_16bit_head_agree(pkg, dev, cd, sp, dtype):
    C, D = cd
    x, W, bias, de = h16.make_inputs(C, D, sp, dtype, dtype, 2000 * C + D + len(sp))
    de = de.float()                                    # an f32 de holding 16-bit values
    e32, dx32, dW32, db32 = f32_head(pkg, dev, x.float(), W, bias, de)
    assert bool(torch.isfinite(dx32).all()) and float(dW32.abs().max()) > 0
    dx_rounded = dx32.to(dtype)                        # round to nearest even, once
    S = x[0, 0].numel()
    for name in ("element", "aligned"):
        packed_dw = name == "aligned" and S % 2 == 0 and C <= 64
        tag = "%s S=%d dW %s" % (name, S, "packed" if packed_dw else "element")
        e, dx, dW, db = h16.run_in_arena(pkg, dev, h16.RESIDUES[name], x, W, bias, de)
        assert e.dtype == torch.float32 and dx.dtype == dtype
        assert h16.same_bits(e, e32), tag + " e"
        assert h16.same_bits(dx, dx_rounded), tag + " dx"
        if packed_dw:
            h16.check32(tag + " dW", h16.npf(dW), h16.npf(dW32), 2e-5)
            h16.check32(tag + " db", h16.npf(db), h16.npf(db32), 2e-5)
        else:
            assert h16.same_bits(dW, dW32), tag + " dW"
            assert h16.same_bits(db, db32), tag + " db"
