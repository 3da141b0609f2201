"""CPU: the guard-banded arena of tests/arena.py on a CPU buffer -- skews honoured, every kind of damage caught and named."""
import pytest
import torch

from arena import ALIGN, PATTERN, Arena, ArenaError

DTYPES = [(torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2), (torch.uint8, 1)]


@pytest.mark.parametrize("dtype,item", DTYPES)
def test_skews_are_honoured(dtype, item):
    a = Arena(1 << 16)
    assert a.raw.data_ptr() % ALIGN == 0
    for skew in (0, item, 3 * item, 8, 16 + item, 252):
        if skew % item:
            continue
        v = a.carve((3, 5, 7), dtype, skew_bytes=skew)
        assert v.data_ptr() % ALIGN == skew and v.is_contiguous() and v.shape == (3, 5, 7) and v.dtype == dtype
        if dtype.is_floating_point:
            assert bool(torch.isnan(v.float()).all())  # the pattern reads as NaN
    a.check()
    with pytest.raises(ValueError):
        a.carve((4,), torch.float32, skew_bytes=2)  # not a multiple of the element size


def test_guards_surround_every_view():
    a = Arena(1 << 16)
    v = a.carve((10,), torch.float32, skew_bytes=4, guard=1024)
    w = a.carve((10,), torch.float32, guard=1024)
    lo = v.data_ptr() - a.raw.data_ptr()
    assert lo >= 1024 and (w.data_ptr() - v.data_ptr() - 40) >= 1024
    assert (w.data_ptr() - a.raw.data_ptr()) + 40 + 1024 <= a.nbytes
    assert bool((a.raw.view(torch.int32) == PATTERN).all())
    with pytest.raises(ValueError):
        Arena(4096).carve((1 << 12,), torch.float32)  # no room for the trailing guard


def _arena():
    a = Arena(1 << 16)
    x = a.carve((2, 3, 8), torch.float32, skew_bytes=4, name="input")
    y = a.carve((2, 3, 8), torch.float32, skew_bytes=12, name="output")
    a.fill(x, torch.arange(48, dtype=torch.float32).view(2, 3, 8))
    return a, x, y


def test_a_clean_run_passes():
    a, x, y = _arena()
    y.copy_(x * 2)
    a.check(written=[y], untouched=[x])


@pytest.mark.parametrize("side", ["before", "past"])
def test_one_element_overrun_is_caught(side):
    a, x, y = _arena()
    y.copy_(x * 2)
    first = (y.data_ptr() - a.raw.data_ptr()) // 4
    idx = first - 1 if side == "before" else first + y.numel()
    a.raw.view(torch.float32)[idx] = 1.0  # plain indexing on the raw buffer
    with pytest.raises(ArenaError) as ei:
        a.check(written=[y], untouched=[x])
    msg = str(ei.value)
    assert "byte %d of the arena" % (idx * 4) in msg
    assert ("guard before 'output'" in msg) if side == "before" else ("guard after 'output'" in msg)


def test_write_into_a_stride_gap_is_caught():
    a = Arena(1 << 16)
    t = a.carve_batch_strided((2, 3, 8), torch.float32, 3, name="target")
    assert t.stride() == (27, 8, 1) and t.shape == (2, 3, 8)
    a.fill(t, torch.ones(2, 3, 8))
    a.check(untouched=[t])
    first = (t.data_ptr() - a.raw.data_ptr()) // 4
    a.raw.view(torch.float32)[first + 24] = 0.0  # the first gap element
    with pytest.raises(ArenaError) as ei:
        a.check(untouched=[t])
    assert "stride gap of 'target'" in str(ei.value) and "byte %d of the arena" % ((first + 24) * 4) in str(ei.value)
    # a gap is a guard for a written view as well
    b = Arena(1 << 16)
    o = b.carve_batch_strided((2, 4), torch.float32, 1, name="out")
    o.fill_(0.0)
    b.check(written=[o])
    b.raw.view(torch.float32)[(o.data_ptr() - b.raw.data_ptr()) // 4 + 4] = 0.0
    with pytest.raises(ArenaError) as ei:
        b.check(written=[o])
    assert "stride gap of 'out'" in str(ei.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_an_unwritten_output_element_is_caught(dtype):
    a = Arena(1 << 16)
    y = a.carve((2, 3, 8), dtype, skew_bytes=8, name="output")
    for miss in (0, 17, 47):  # (16-bit: both halves of a pattern word)
        y.view(-1)[:] = torch.arange(48).to(dtype)
        if dtype == torch.float32:
            y.view(torch.int32).view(-1)[miss] = PATTERN
        else:
            y.view(torch.int16).view(-1)[miss] = PATTERN >> 16
        with pytest.raises(ArenaError) as ei:
            a.check(written=[y])
        assert "unwritten element in 'output'" in str(ei.value) and "byte offset %d " % (miss * y.element_size()) in str(ei.value)
    y.view(-1)[:] = torch.arange(48).to(dtype)
    a.check(written=[y])


def test_a_modified_input_is_caught():
    a, x, y = _arena()
    y.copy_(x * 2)
    x[1, 2, 7] = -0.0 + x[1, 2, 7]  # the same value: no change
    a.check(written=[y], untouched=[x])
    x[0, 0, 0] = -0.0  # 0.0 -> -0.0: equal as floats, not as bits
    with pytest.raises(ArenaError) as ei:
        a.check(written=[y], untouched=[x])
    assert "'input' (byte 3 of the view's span)" in str(ei.value)
    a, x, y = _arena()
    y.copy_(x * 2)
    x[1, 0, 5] += 1
    with pytest.raises(ArenaError) as ei:
        a.check(written=[y], untouched=[x])
    assert "'input'" in str(ei.value)


def test_u8_views_and_foreign_tensors():
    a = Arena(1 << 16)
    m = a.carve((2, 5), torch.uint8, skew_bytes=1, name="mask")
    a.fill(m, torch.ones(2, 5, dtype=torch.uint8))
    a.check(untouched=[m])
    with pytest.raises(ValueError):
        a.check(written=[m])
    with pytest.raises(ValueError):
        a.check(untouched=[torch.zeros(3)])
