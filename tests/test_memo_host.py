"""Host-only: the Python layer's shared helpers (affinity_op.py) -- the identity-keyed memo behind cross_supported / multi_supported /
the labels table's query / the accumulating descriptors, the weight-table check, and the argument errors of the operand helpers that
need no device."""
import importlib
import threading

import pytest
import torch


@pytest.fixture(scope="module")
def op(pkg):
    return pkg.affinity_op


def _desc(pkg, H=32):
    d = pkg._lib.PeaDesc()
    d.ndim, d.B, d.D, d.K = 2, 1, 16, 2
    d.dims[:] = [1, H, 32]
    return d


def test_a_hit_needs_identity_not_equality(pkg, op):
    memo, calls = op._IdMemo(8), []
    a = _desc(pkg)
    b = type(a).from_buffer_copy(a)
    assert bytes(a) == bytes(b) and a is not b
    ask = lambda d: memo.get((d,), (1,), lambda: calls.append(d) or len(calls))
    assert ask(a) == 1 and ask(a) == 1 and calls == [a]  # remembered
    assert ask(b) == 2 and calls == [a, b]               # an equal copy is another question
    assert ask(a) == 1 and ask(b) == 2 and len(calls) == 2
    assert memo.get((a,), (2,), lambda: "other extra") == "other extra" and ask(a) == 1
    assert memo.get((a, b), (1,), lambda: "pair") == "pair" and memo.get((b, a), (1,), lambda: "riap") == "riap"
    assert memo.get((a, b), (1,), lambda: "again") == "pair"


def test_an_entry_keeps_its_objects_alive(pkg, op):
    """an id is reused once its object is gone: the memo must never answer for a new object that got an old one's id"""
    memo = op._IdMemo(1 << 20)
    seen = set()
    for i in range(200):
        d = _desc(pkg, 32 + i)
        assert id(d) not in seen  # (every earlier descriptor is pinned by its entry)
        seen.add(id(d))
        assert memo.get((d,), (), lambda: i) == i
        del d  # (reference counting frees an unpinned descriptor at once)
    assert len(memo) == 200
    memo.clear()
    # with the pins gone ids do come back; a stale entry planted under such an id does not answer for the new object
    old, new = _desc(pkg), _desc(pkg)
    memo._d[(id(new), ())] = ("stale", (old,))
    assert memo.get((new,), (), lambda: "fresh") == "fresh" and memo.get((new,), (), lambda: "x") == "fresh"


def test_the_cap_clears_the_memo(pkg, op):
    memo = op._IdMemo(4)
    ds = [_desc(pkg, 32 + i) for i in range(7)]
    for i, d in enumerate(ds[:5]):
        memo.get((d,), (), lambda: i)
    assert len(memo) == 5  # cleared when an insertion finds MORE than cap entries
    assert memo.get((ds[5],), (), lambda: 5) == 5 and len(memo) == 1
    assert memo.get((ds[0],), (), lambda: "recomputed") == "recomputed"
    assert op._CROSS_OK.cap == 2048 and op._MULTI_OK.cap == op._MULTI_LABELS_OK.cap == 256


def test_clear_from_another_thread_while_get_runs(pkg, op):
    memo = op._IdMemo(16)
    ds = [_desc(pkg, 32 + i) for i in range(64)]
    stop, errors = threading.Event(), []

    def clearer():
        try:
            while not stop.is_set():
                memo.clear()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    t = threading.Thread(target=clearer)
    t.start()
    try:
        for rep in range(50):
            for i, d in enumerate(ds):
                assert memo.get((d,), (rep & 1,), lambda: i) == i
    finally:
        stop.set()
        t.join()
    assert not errors


def test_the_modules_memos_are_instances(pkg, op):
    sec = importlib.import_module(pkg.__name__ + ".harness.loss_section")
    for memo in (op._CROSS_OK, op._MULTI_OK, op._MULTI_LABELS_OK, sec._ACC_DESC):
        assert isinstance(memo, op._IdMemo)
    assert op._CROSS_OK.clear in pkg._lib._RELOAD_HOOKS
    d = _desc(pkg)
    da = sec._accumulating(d)
    assert da is sec._accumulating(d) and da is not d and da.flags == d.flags | pkg._lib.FLAG_ACCUMULATE_DE
    assert sec._accumulating(type(d).from_buffer_copy(d)) is not da


def test_check_weight_table(op):
    B, K, cpu = 2, 3, torch.device("cpu")
    good = torch.zeros(B * K * 2)
    assert op.check_weight_table(good, 0, B, K, cpu) is good
    assert op.check_weight_table(good.view(B, K, 2), 0, B, K, cpu).shape == (B, K, 2)
    with pytest.raises(ValueError, match="weight table 1 does not fit this batch / stencil"):
        op.check_weight_table(torch.zeros(B * K * 2 + 2), 1, B, K, cpu)
    with pytest.raises(ValueError, match="weight table 2 does not fit"):
        op.check_weight_table(good.double(), 2, B, K, cpu)
    with pytest.raises(ValueError, match="weight table 3 does not fit"):
        op.check_weight_table(good, 3, B, K, torch.device("meta"))
    with pytest.raises(ValueError, match="weight table 4 must be contiguous"):
        op.check_weight_table(torch.zeros(B * K * 4)[::2], 4, B, K, cpu)
    with pytest.raises(ValueError, match="weight table 5 must be contiguous"):
        op.check_weight_table(torch.zeros(2, K, B).permute(2, 1, 0), 5, B, K, cpu)


def test_operand_helpers_refuse_bad_arguments_before_any_device_work(pkg, op):
    e = torch.zeros(2, 16, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op._pair_args(e, None)
    with pytest.raises(TypeError, match="embedding must be a torch.Tensor"):
        op._pair_args(None, e)
    spec = pkg.AffinitySpec(2, [[0, 1], [1, 0]], None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    with pytest.raises(RuntimeError, match="target is on cpu"):  # (the first operand's device check: nothing was copied or built)
        op._loss_operands(spec, e, torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), None)
    # what _loss_operands does to each operand, without the device check
    kshape = op._affs_shape(e, spec.K)
    assert kshape == (2, 2, 8, 8)
    with pytest.raises(ValueError, match=r"target has shape \(2, 3, 8, 8\), expected \(2, 2, 8, 8\)"):
        op._batch_layout(torch.zeros(2, 3, 8, 8), "target", torch.float32, kshape)
    with pytest.raises(TypeError, match="weightmap must be a torch.Tensor"):
        op._batch_layout(None, "weightmap", torch.float32, kshape)
    with pytest.raises(ValueError, match="mask has shape"):
        op.mask_arg(torch.zeros(2, 2, 8, 4), kshape, gpu=False)
    assert op.mask_arg(None, kshape, gpu=False) == (None, 0, 0)
    m, ms, flag = op.mask_arg(torch.ones(4, 2, 8, 8)[::2], kshape, gpu=False)
    assert (ms, flag) == (2 * 2 * 64, pkg._lib.FLAG_MASK_F32)
    m, ms, flag = op.mask_arg(torch.ones(2, 2, 8, 8, dtype=torch.bool), kshape, gpu=False)
    assert m.dtype == torch.uint8 and (ms, flag) == (2 * 64, 0)
    for D, border, ok in ((16, pkg._lib.BORDER_REPLICATE, True), (24, pkg._lib.BORDER_REPLICATE, False), (24, pkg._lib.BORDER_CIRCULAR, True)):
        spec = pkg.AffinitySpec(3, [[0, 0, 1]], None, border, pkg._lib.NORM_FULL)
        if ok:
            op._check_trainable(spec, D)
        else:
            with pytest.raises(NotImplementedError, match="replicate-border backward needs D in"):
                op._check_trainable(spec, D)
