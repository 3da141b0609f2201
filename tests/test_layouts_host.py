"""CPU: the layout decisions of the Python layer, without a device.

The C ABI reads item b of a target / weight map / mask at data_ptr + b * (bstride or K * S) elements as ONE dense [K, S] block
(include/pea.h: a *_bstride of 0 means "dense").  affinity_op._batch_layout (the device-free half of _batch_strided) and mask_arg
decide what tensor and what stride the library gets; here every layout of tests/layouts.py goes through them and what the ABI would
read -- torch.as_strided over the returned tensor's storage with exactly that rule -- must be the input's values, bit for bit:

  * a batch-broadcast tensor (stride(0) == 0, B > 1) never comes back with stride 0: the descriptor would read it as dense, K * S * b
    elements past a storage that holds one item (the sources sit in a guard-banded arena, so the misread lands in its NaN pattern);
  * a dense per-item block at a positive batch stride (channel slice of a packed tensor, t[::2], overlapping as_strided windows) comes
    back as it is: same data_ptr(), its own stride, no copy;
  * B == 1 gives stride 0 and a dense tensor.

The same for the device-free halves of the other hand-written normalisers: fgmask._logits_arg / _labels_arg(gpu=False) and
disc._args(gpu=False).
"""
import importlib

import pytest
import torch

import __graft_entry__ as ge
import layouts as ly
from arena import Arena

SHAPES = [(3, 4, 6, 10), (2, 3, 3, 4, 6), (2, 1, 5, 7)]
# kind -> (dtype of the input, dtype the library is handed, converted on the way?)
KINDS = {
    "f32": (torch.float32, torch.float32, False),
    "f64": (torch.float64, torch.float32, True),
    "u8": (torch.uint8, torch.uint8, False),
    "bool": (torch.bool, torch.uint8, False),
    "mask_f32": ("mask_f32", torch.float32, False),
}


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(ge.PKG_NAME + ".affinity_op")


def _normalise(op, kind, view, shape):
    """-> (tensor, batch stride) the way the training entries get them: target / weightmap through _batch_layout, masks through mask_arg"""
    if kind in ("f32", "f64"):
        return op._batch_layout(view, "target", torch.float32, shape)
    m, ms, flag = op.mask_arg(view, shape, gpu=False)
    assert flag == (op._lib.FLAG_MASK_F32 if kind == "mask_f32" else 0)
    return m, ms


def _as_handed(twin, out_dtype):
    return twin.view(torch.uint8) if twin.dtype == torch.bool else twin.to(out_dtype)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("layout", ly.VALUE_LAYOUTS)
def test_what_the_abi_reads_is_the_input(op, layout, kind, shape):
    in_dtype, out_dtype, converted = KINDS[kind]
    B, K, S = shape[0], shape[1], ly.numel(shape[2:])
    ar = Arena(8 * 3 * B * K * S + 8192)  # the source and a guard of B * K * S elements on either side, at 8 bytes per element
    view, rec = ly.make(layout, shape, in_dtype, 11, arena=ar, name="source")
    assert tuple(view.shape) == shape
    twin, before = ly.dense(view), view.clone()
    out, bs = _normalise(op, kind, view, shape)
    assert out.dtype == out_dtype and tuple(out.shape) == shape
    want = _as_handed(twin, out_dtype).reshape(B, K, S)
    got = ly.abi_view(out, bs, shape)
    assert torch.equal(got, want), "the library would not read the input's values (layout %s, batch stride %d)" % (layout, bs)
    assert bs > 0, "B > 1: a batch stride of 0 means dense to the library"
    if view.stride(0) == 0:
        assert bs == K * S and out.is_contiguous()
    if layout in ly.ZERO_COPY and not converted:
        assert out.data_ptr() == view.data_ptr() and bs == view.stride(0), "a dense per-item block was copied"
        assert bs == {"L4": 3 * K * S, "L5": 2 * K * S, "L8": S}[layout]
    elif layout not in ly.ZERO_COPY:
        assert bs == K * S and out.is_contiguous()
    assert torch.equal(view, before)
    if rec is not None:
        ar.check(untouched=[rec])


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("layout", ly.VALUE_LAYOUTS)
def test_a_batch_of_one_is_dense_with_stride_zero(op, layout, kind):
    in_dtype, out_dtype, _ = KINDS[kind]
    shape = (1, 3, 5, 8)
    view, _ = ly.make(layout, shape, in_dtype, 12)
    twin = ly.dense(view)
    out, bs = _normalise(op, kind, view, shape)
    assert bs == 0 and out.is_contiguous() and out.dtype == out_dtype
    assert torch.equal(out, _as_handed(twin, out_dtype))
    if view.is_contiguous() and in_dtype != torch.float64:
        assert out.data_ptr() == view.data_ptr()


def test_dense_input_is_taken_as_it_is(op):
    shape = (3, 4, 6, 10)
    for kind, (in_dtype, out_dtype, converted) in KINDS.items():
        view, _ = ly.make("dense", shape, in_dtype, 13)
        out, bs = _normalise(op, kind, view, shape)
        assert bs == 4 * 60 and out.is_contiguous()
        assert converted or out.data_ptr() == view.data_ptr()


def test_shape_and_type_are_checked_before_the_layout(op):
    t = torch.zeros(3, 4, 6, 10)
    with pytest.raises(ValueError, match="target has shape"):
        op._batch_layout(t, "target", torch.float32, (3, 4, 6, 11))
    with pytest.raises(TypeError):
        op._batch_layout(None, "target", torch.float32, (3, 4, 6, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the device check stays in front of the entry points
        op._batch_strided(t, "target", torch.float32, (3, 4, 6, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.mask_arg(t, (3, 4, 6, 10))
    assert op.mask_arg(None, (3, 4, 6, 10), gpu=False) == (None, 0, 0)


# ---- the foreground-mask and discriminative-loss normalisers ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fg(pkg):
    return importlib.import_module(ge.PKG_NAME + ".harness.fgmask")


@pytest.fixture(scope="module")
def disc(pkg):
    return importlib.import_module(ge.PKG_NAME + ".harness.disc")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("layout", ly.VALUE_LAYOUTS + ("dense",))
def test_fgmask_logits_come_out_dense(fg, layout, dtype):
    shape = (3, 2, 6, 10)
    view, _ = ly.make(layout, shape, dtype, 14)
    twin, before = ly.dense(view), view.clone()
    out = fg._logits_arg(view, gpu=False)
    assert out.is_contiguous() and out.dtype == dtype and tuple(out.shape) == shape
    assert torch.equal(out.view(torch.int16) if dtype != torch.float32 else out.view(torch.int32),
                       twin.view(torch.int16) if dtype != torch.float32 else twin.view(torch.int32))
    assert torch.equal(view, before)
    if layout == "dense":
        assert out.data_ptr() == view.data_ptr()


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32], ids=str)
@pytest.mark.parametrize("layout", ly.LABEL_LAYOUTS + ("dense",))
def test_fgmask_labels_come_out_dense(fg, pkg, layout, dtype):
    B, sp = 3, (6, 10)
    logits = torch.zeros((B, 2) + sp)
    view = ly.make_labels(layout, B, sp, dtype, 15)
    twin, before = ly.dense(view).reshape((B,) + sp), view.clone()
    out, code = fg._labels_arg(view, logits, "labels", gpu=False)
    assert code == (pkg._lib.FG_LABELS_I32 if dtype == torch.int32 else pkg._lib.FG_LABELS_U8)
    assert out.is_contiguous() and tuple(out.shape) == (B,) + sp
    assert out.dtype == (torch.int32 if dtype == torch.int32 else torch.uint8)
    assert torch.equal(out, twin.view(torch.uint8) if dtype == torch.bool else twin)
    assert torch.equal(view, before)
    if layout == "dense":
        assert out.data_ptr() == view.data_ptr()


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16, torch.uint8], ids=str)
@pytest.mark.parametrize("lab_layout", ly.LABEL_LAYOUTS + ("dense",))
@pytest.mark.parametrize("e_layout", ["L3", "L6", "L7", "dense"])
def test_disc_arguments_come_out_dense(disc, e_layout, lab_layout, dtype):
    B, D, sp = 2, 5, (6, 10)
    e, _ = ly.make(e_layout, (B, D) + sp, torch.float32, 16)
    lab = ly.make_labels(lab_layout, B, sp, dtype, 17)
    e_twin, lab_twin = ly.dense(e), ly.dense(lab).reshape(B, -1)
    e_before, lab_before = e.clone(), lab.clone()
    e_c, lab_c, num_ids = disc._args(e, lab, None, gpu=False)
    assert e_c.is_contiguous() and torch.equal(e_c, e_twin)
    assert lab_c.is_contiguous() and lab_c.dtype == torch.int32 and tuple(lab_c.shape) == (B, 60)
    assert torch.equal(lab_c, lab_twin.to(torch.int32))
    assert num_ids == int(lab_twin.max()) + 1
    assert disc._args(e, lab, 9, gpu=False)[2] == 9
    assert torch.equal(e, e_before) and torch.equal(lab, lab_before)
    if e_layout == "dense":
        assert e_c.data_ptr() == e.data_ptr()


def test_disc_and_fgmask_still_refuse_cpu_tensors(disc, fg):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        disc._args(torch.zeros(2, 5, 6, 10), torch.zeros(2, 6, 10, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fg._labels_arg(torch.zeros(2, 6, 10, dtype=torch.uint8), torch.zeros(2, 2, 6, 10), "labels")
