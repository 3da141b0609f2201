"""CPU: the batched self losses on f16 / bf16 embeddings (include/pea_multi.h, include/pea_multi_labels.h) -- the support queries
answer 1 for tables whose entries are ALL f16 or ALL bf16 and are otherwise in the fused set, 0 where the storage types are mixed or
a 16-bit table leaves the set for another reason; and the three calls hold `e` / `de` of a 16-bit table to the alignment of a 16-bit
element: an odd address is PEA_E_ALIGN, a 2-byte-aligned one that is not 4-byte aligned goes on to the next check (dummy device
pointers, no GPU: every case ends in an error code before anything is launched).  The helpers are those of tests/test_multi_host.py
and tests/test_multi_labels_host.py."""
import pytest

import test_multi_host as mh
import test_multi_labels_host as lh

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
REPLICATE = 2
FLAG_HALF_SHIFT, FLAG_CLAMP01, FLAG_LOSS_ACT = 4, 8, 64
SIXTEEN = [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16")]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def norm1_deep(pkg, **kw):
    return [mh.desc3d(pkg, dims, **kw) for dims in ((18, 80, 80), (18, 40, 40), (18, 20, 20), (18, 10, 10))]


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_tensor_form_query_takes_tables_of_one_16_bit_type(pkg, lib, dtype):
    q = lambda descs: mh.supported(pkg, lib, descs)
    assert q(mh.cvppp_deep(pkg, dtype=dtype)) == 1
    assert q(mh.cvppp_deep(pkg, dtype=dtype, B=8)) == 1
    assert q(norm1_deep(pkg, dtype=dtype)) == 1
    assert q(mh.cvppp_deep(pkg, dtype=dtype)[:1]) == 1 and q(mh.cvppp_deep(pkg, dtype=dtype)[:2]) == 1
    assert q([mh.desc2d(pkg, D=32, dtype=dtype), mh.desc3d(pkg, dtype=dtype)]) == 1  # entries may differ in every OTHER field
    base = mh.cvppp_deep(pkg, dtype=dtype)[:3]
    other = F16 if dtype == BF16 else BF16
    assert q(base + [mh.desc2d(pkg, dtype=other)]) == 0                              # f16 + bf16
    assert q([mh.desc2d(pkg, dtype=other)] + base) == 0
    assert q(base + [mh.desc2d(pkg, dtype=F32)]) == 0 and q([mh.desc2d(pkg, dtype=F32)] + base) == 0
    assert q(base + [mh.desc2d(pkg, dtype=dtype, D=64)]) == 0
    assert q(base + [mh.desc2d(pkg, dtype=dtype, border=REPLICATE)]) == 0
    assert q(base + [mh.desc2d(pkg, dtype=dtype, flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT | FLAG_CLAMP01)]) == 0
    assert q(base + [mh.desc2d(pkg, dtype=dtype, flags=FLAG_HALF_SHIFT | FLAG_CLAMP01)]) == 1


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_labels_form_query_takes_tables_of_one_16_bit_type(pkg, lib, dtype):
    q = lambda ents, flags=lh.FLAGS_2D: lh.supported(pkg, lib, ents, flags)
    assert q(lh.cvppp_steps(pkg, dtype=dtype)) == 1 and q(lh.cvppp_steps(pkg, dtype=dtype, B=8)) == 1
    assert q([lh.entry(mh.desc2d(pkg, 272 >> j, 272 >> j, mh.CROSS[:2 * (4 - j)], dtype=dtype)) for j in range(4)]) == 1
    steps3 = [lh.entry(lh.desc3d(pkg, (18, 160 >> (j + 1), 160 >> (j + 1)), dtype=dtype), (18, 160, 160), (1, 2 << j, 2 << j))
              for j in range(4)]
    assert q(steps3, lh.FLAGS_3D) == 1
    assert q([lh.entry(d) for d in norm1_deep(pkg, dtype=dtype)], lh.FLAGS_3D) == 1
    base = lh.cvppp_steps(pkg, dtype=dtype)[:3]
    other = F16 if dtype == BF16 else BF16
    assert q(base + [lh.entry(lh.desc2d(pkg, dtype=other))]) == 0                    # f16 + bf16
    assert q([lh.entry(lh.desc2d(pkg, dtype=other))] + base) == 0
    assert q(base + [lh.entry(lh.desc2d(pkg, dtype=F32))]) == 0
    assert q(base + [lh.entry(lh.desc2d(pkg, dtype=dtype, D=64))]) == 0
    assert q(base + [lh.entry(lh.desc2d(pkg, dtype=dtype, border=REPLICATE))]) == 0
    assert q(base + [lh.entry(lh.desc2d(pkg, dtype=dtype, flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT | FLAG_CLAMP01))]) == 0
    assert q(base + [lh.entry(lh.desc2d(pkg, dtype=dtype, flags=FLAG_HALF_SHIFT | FLAG_CLAMP01))]) == 1


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_tensor_form_calls_hold_e_and_de_to_two_bytes(pkg, lib, dtype):
    """odd: PEA_E_ALIGN.  0x10002 (2-byte, not 4-byte aligned) passes the alignment check: the forward goes on to the workspace
    check, which refuses (no workspace given); the backward has no later harmless refusal of a fused table, so its table carries one
    entry outside the fused set and the call ends in PEA_E_UNSUPPORTED -- which comes after the alignment check of EVERY entry."""
    four = mh.cvppp_deep(pkg, dtype=dtype)
    for j in (0, 3):
        assert mh.fwd(pkg, lib, four, {j: {"e": 0x10001}}) == E_ALIGN, j
        assert mh.fwd(pkg, lib, four, {j: {"e": 0x10002}}, ws=None) == E_WORKSPACE, j
        for field in ("e", "de"):
            assert mh.bwd(pkg, lib, four, {j: {field: 0x10001}}) == E_ALIGN, (field, j)
    # the f32 pointers of a 16-bit table keep their four bytes
    for field in ("target", "weight", "affs", "g_out", "loss_out"):
        assert mh.fwd(pkg, lib, four, {1: {field: 0x60002}}) == E_ALIGN, field
    for field in ("g", "dloss"):
        assert mh.bwd(pkg, lib, four, {1: {field: 0x70002}}) == E_ALIGN, field
    outside = four[:3] + [mh.desc2d(pkg, dtype=dtype, D=64)]
    assert mh.bwd(pkg, lib, outside, {0: {"e": 0x10002, "de": 0x30002}, 3: {"e": 0x10002, "de": 0x30002}}) == E_UNSUPPORTED
    assert mh.bwd(pkg, lib, outside, {3: {"de": 0x30001}}) == E_ALIGN
    # an f32 table still wants four bytes
    assert mh.fwd(pkg, lib, mh.cvppp_deep(pkg), {0: {"e": 0x10002}}, ws=None) == E_ALIGN
    assert mh.bwd(pkg, lib, mh.cvppp_deep(pkg), {0: {"de": 0x30002}}) == E_ALIGN


@pytest.mark.parametrize("dtype", SIXTEEN)
def test_labels_form_call_holds_e_and_de_to_two_bytes(pkg, lib, dtype):
    four = lh.cvppp_steps(pkg, dtype=dtype)
    over = lambda j, **kw: [e if i != j else (e[0], e[1], e[2], kw) for i, e in enumerate(four)]
    for j in (0, 3):
        for field in ("e", "de"):
            assert lh.call(pkg, lib, over(j, **{field: 0x10001})) == E_ALIGN, (field, j)
        assert lh.call(pkg, lib, over(j, e=0x10002, de=0x60002), ws=None) == E_WORKSPACE, j
        assert lh.call(pkg, lib, over(j, e=0x10002, de=0x60002), scratch=None) == E_WORKSPACE, j
    for field in ("labels", "wtab", "affs", "loss_out", "dloss"):
        assert lh.call(pkg, lib, over(2, **{field: 0x70002})) == E_ALIGN, field
    assert lh.call(pkg, lib, [(e[0], e[1], e[2], dict(e=0x10002)) if i == 0 else e for i, e in enumerate(lh.cvppp_steps(pkg))],
                   ws=None) == E_ALIGN  # an f32 table still wants four bytes


def test_python_layer_leaves_large_16_bit_tensor_tables_to_the_single_calls(pkg):
    """affinity_op.multi16_pays: the size rule of the Python wrappers (not of the C query, which answers for what the kernels can
    do).  Counted in tiles of 256 voxels of one batch item; f32 tables are taken at every size, as before."""
    op = pkg.affinity_op
    limit = op.MULTI16_MAX_TILES
    tiles = lambda descs: sum(d.B * ((d.dims[0] * d.dims[1] * d.dims[2] + 255) // 256) for d in descs)
    assert tiles(mh.cvppp_deep(pkg)) == 772 and tiles(mh.cvppp_deep(pkg, B=8)) == 3088
    assert 772 <= limit < 3088  # between the size measured to gain and the size measured to lose (profiles/multi16_ab.json)
    for dtype in (F16, BF16):
        assert op.multi16_pays(mh.cvppp_deep(pkg, dtype=dtype)) is True
        assert op.multi16_pays(mh.cvppp_deep(pkg, dtype=dtype, B=8)) is False
        one = lambda B, H: [mh.desc2d(pkg, H, 256, B=B, dtype=dtype)]  # H tiles per batch item
        assert tiles(one(1, limit)) == limit and op.multi16_pays(one(1, limit)) is True
        assert op.multi16_pays(one(1, limit + 1)) is False
    assert op.multi16_pays(mh.cvppp_deep(pkg, B=8)) is True and op.multi16_pays(mh.cvppp_deep(pkg, B=64)) is True
