"""GPU: the mutex watershed (include/pea_mws.h, csrc/pea_k_mws.hip) held to its ROUND RULE on the graphs that the rule is weakest on, and
to every integer that the header fixes -- not the final partition alone.  test_gpu_mws.py compares complete results on random maps of
about 37 x 41; here

  * stats[ROUNDS] is the simulation's count and stats[EXCLUSIONS] the sequential procedure's distinct exclusive pairs, on every case;
  * a call whose rounds ran out is compared EXACTLY with the simulation stopped at that round (mws_reference.rounds_trace): labels,
    counts, ROUNDS, UNDECIDED, MERGES and EXCLUSIONS -- a round that decides too little, or an edge that it should have left waiting,
    shows at that round even where the end result agrees;
  * the named graphs of mws_cases.py: one round that hooks a single chain through 4100 pixels (the path halving at depth S across
    workgroups), one decided edge a round for 299 rounds (the flags' parity, W_DONE, resume, the Python layer's doubling batches), an
    exclusion table at 0.4 of its capacity, opposite / repeated / zero offsets, positive steps in 3D, K = 32 with steps up to the ends of
    int32, more than 65536 pixels (the second trip of k_mws_scan's carry loop), more than 256 images (the second workgroup of
    k_mws_begin and k_mws_stats).
test_mws_host.py asserts on the reference alone that every named graph is what its name says.

House rules of test_gpu_mws.py: every C call in a guard-banded arena, the workspace lent unprepared, np.array_equal / torch.equal only."""
import functools
import importlib

import numpy as np
import pytest
import torch

import mws_cases as C
import mws_reference as R
from mws_cases import EXCLUSIONS, MERGES, NAMED, ROUNDS, UNDECIDED, Call, check, reference, tt

pytestmark = pytest.mark.gpu
INPUT_NAMES = {v: k for k, v in R.INPUTS.items()}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def trace(name, b=0):
    """-> (the simulation's (labels, used, undecided slots, merged, active) after every round, the same at the end) of image b"""
    case = (NAMED[name] if name in NAMED else C.CASES[name])()
    hist = []
    return hist, R.rounds_trace(C.graph(case, b), history=hist)


def after(name, n, b=0):
    """what the header fixes after n rounds of a call (n = 0: the set-up alone is not traced)"""
    hist, end = trace(name, b)
    return hist[n - 1] if n <= len(hist) else end


def check_partial(what, got, name, n):
    """a call whose n rounds may have run out, image by image against the simulation stopped there"""
    labels, counts, stats = (t.cpu().numpy() for t in got)
    for b in range(len(counts)):
        lab, used, slots, merged, active = after(name, n, b)
        assert stats[b, :4].tolist() == [used, slots, merged, active], (what, n, b, stats[b].tolist())
        assert counts[b] == lab.max() and np.array_equal(labels[b].ravel(), lab), (what, n, b)


def same(a, b):
    return all(torch.equal(s.reshape(-1), t.reshape(-1)) for s, t in zip(a, b))


def python_call(pkg, dev, case, rounds=None):
    """pkg.mutex_watershed on a case -> (labels, counts, stats)"""
    x, offsets, nA, strides, mask, input = case
    two_d = len(offsets[0]) == 2
    X = tt(x[:, :, 0] if two_d else x).to(dev)
    M = None if mask is None else tt(mask[:, 0] if two_d else mask).to(dev)
    out = pkg.mutex_watershed(X, offsets, list(strides), M, input=INPUT_NAMES[input], n_attractive=nA, rounds=rounds)
    assert out.labels.shape == X.shape[:1] + X.shape[2:] and out.labels.dtype == torch.int32
    return out.labels, out.counts, out.stats


def step_through(what, call, name, limit=400):
    """one round a call, resumed, each compared with the simulation stopped at that round, until nothing is undecided -> the last result
    and its round"""
    got = call.run(1)
    n = 1
    check_partial(what, got, name, n)
    while int(got[2][:, UNDECIDED].max()) > 0:
        assert n < limit, what
        got = call.run(1, resume=True)
        n += 1
        check_partial(what, got, name, n)
    return got, n


SMALL = sorted(set(NAMED) - {"more than 65536 pixels", "more than 256 images"})


@pytest.mark.parametrize("name", SMALL)
def test_named_graph_equals_the_reference(pkg, dev, name):
    x, offsets, nA, strides, mask, input = NAMED[name]()
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = c.complete(batch=8)
    c.check()
    check(name, got, reference(name), mask)
    stats = got[2].cpu().numpy()
    if name in ("rising line", "snake"):  # one round hooks one chain through every pixel, and the compress follows it to its end
        assert got[1].tolist() == [1] and stats[0, ROUNDS] == 1 and stats[0, MERGES] == x[0, 0].size - 1
        one = Call(pkg, dev, x, offsets, nA, strides, mask, input)
        first = one.run(1)
        one.check()
        check_partial(name, first, name, 1)
        assert int(first[2][0, UNDECIDED]) == 0 and torch.equal(first[0], got[0]) and bool((first[0] == 1).all())
    if name == "falling line":
        assert got[1].tolist() == [2] and stats[0, :4].tolist() == [299, 0, 298, 1]
    if name == "falling line, reach 2":
        assert got[1].tolist() == [150] and stats[0, :4].tolist() == [151, 0, 150, 149]
    if name == "three tempos":
        assert stats[:2, ROUNDS].tolist() == [1, 299] and stats[2, ROUNDS] == trace(name, 2)[1][1] and 1 < stats[2, ROUNDS] < 32
    if name in ("positive steps 3D", "twins quantised", "twins noise", "K32 far"):  # few rounds: every one of them against the trace
        step = Call(pkg, dev, x, offsets, nA, strides, mask, input)
        last, n = step_through(name, step, name)
        step.check()
        assert same(last, got)
    if name == "K32 far":  # the channels that reach an extent, alone: every slot is outside, whatever x holds; and the Python layer
        far = [k for k, o in enumerate(offsets) if o in C.FAR]
        alone = Call(pkg, dev, x[:, far], [offsets[k] for k in far], 1, strides, mask, input)
        out = alone.run(2)
        alone.check()
        assert out[2].tolist() == [[0, 0, 0, 0, 0, 0, 0, len(far) * 99]] and out[1].tolist() == [99]
        assert same(python_call(pkg, dev, NAMED[name]()), got)


def test_falling_line_three_ways(pkg, dev):
    """299 rounds of one decided edge each: in batches of 8, one round at a time, and in the Python layer's doubling batches"""
    name = "falling line"
    x, offsets, nA, strides, mask, input = NAMED[name]()
    batches = Call(pkg, dev, x, offsets, nA, strides, mask, input).complete(batch=8)
    check(name, batches, reference(name), mask)
    step = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = step.run(1)
    n = 1
    while int(got[2][0, UNDECIDED]) > 0:
        if n in (1, 2, 3, 50, 150, 298):
            check_partial(name, got, name, n)
        assert n < 310
        got = step.run(1, resume=True)
        n += 1
    step.check()
    assert 299 <= n <= 300 and same(got, batches)
    assert same(step.run(5, resume=True), batches)
    step.check()
    mws = importlib.import_module(pkg.__name__ + ".harness.mws")
    assert mws.FIRST_BATCH == 32 and 32 + 64 + 128 < 299 < 32 + 64 + 128 + 256  # the fourth batch ends it
    assert same(python_call(pkg, dev, NAMED[name]()), batches)


def test_three_tempos_leave_a_finished_image_alone(pkg, dev):
    name = "three tempos"
    x, offsets, nA, strides, mask, input = NAMED[name]()
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = c.run(8)
    first = got
    calls = 1
    assert np.array_equal(first[0][0].cpu().numpy().ravel(), reference(name)[0][0].ravel()) and first[2][0].tolist()[:4] == [1, 0, 299, 0]
    assert int(first[2][1, UNDECIDED]) > 0
    while int(got[2][:, UNDECIDED].max()) > 0:
        assert calls < 64
        got = c.run(8, resume=True)
        calls += 1
        assert torch.equal(got[0][0], first[0][0]) and torch.equal(got[1][0], first[1][0]) and torch.equal(got[2][0], first[2][0]), calls
    c.check()
    check(name, got, reference(name), mask)
    check_partial(name, first, name, 8)


def test_table_at_its_fullest_round_by_round(pkg, dev):
    name = "table at its fullest"
    x, offsets, nA, strides, mask, input = NAMED[name]()
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    # the workspace implies the capacity: the layout of test_workspace_bytes_is_monotone_in_each_extent with cap = 4096
    al8 = lambda v: (v + 7) // 8 * 8
    B, K, S, cap = 1, 8, 16 * 21, C.FULLEST_CAPACITY
    assert c.nb == 4 * al8(4 * B * S) + al8(4 * B * -(-S // 256)) + 8 * B * S + 8 * B * cap + 8 * (16 + 32 * 8) * B + al8(B * S) + al8(B * S * K)
    got, n = step_through(name, c, name)
    c.check()
    check(name, got, reference(name), mask)
    hist = trace(name)[0]
    assert max(h[4] for h in hist) >= 0.35 * cap and int(got[2][0, EXCLUSIONS]) >= 1200


def test_a_side_stream(pkg, dev):
    name = "table at its fullest"
    case = NAMED[name]()
    with torch.cuda.stream(torch.cuda.Stream()):
        side = python_call(pkg, dev, case)
        side = [t.clone() for t in side]
    torch.cuda.synchronize()
    main = python_call(pkg, dev, case)
    check(name + " side stream", side, reference(name), None)
    check(name + " default stream", main, reference(name), None)
    assert same(side, main)


def test_more_than_65536_pixels(pkg, dev):
    name = "more than 65536 pixels"
    x, offsets, nA, strides, mask, input = NAMED[name]()
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = c.run(16)
    c.check()
    ref = reference(name)
    assert int(ref[1][0]) > 100 and np.array_equal(got[1].cpu().numpy(), ref[1]) and np.array_equal(got[0].cpu().numpy(), ref[0])
    check(name, got, ref, mask)
    assert same(python_call(pkg, dev, NAMED[name]()), got)


def test_more_than_256_images(pkg, dev):
    name = "more than 256 images"
    x, offsets, nA, strides, mask, input = NAMED[name]()
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = c.run(16)
    c.check()
    check(name, got, reference(name), mask)
    assert len(set(got[1].tolist())) >= 3
    assert same(c.run(0, resume=True), got)
    assert same(c.run(3, resume=True), got)  # k_mws_begin clears the flags of every image; no image has anything left
    c.check()
    for b in (0, 255, 256):
        one = Call(pkg, dev, x[b:b + 1], offsets, nA, strides, mask, input)
        alone = one.run(16)
        one.check()
        assert same(alone, [t[b:b + 1] for t in got]), b
    # a call whose rounds run out, on every image at once: past the first workgroup of the per-image kernels too
    short = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    check_partial(name, short.run(1), name, 1)
    check_partial(name, short.run(1, resume=True), name, 2)
    short.check()


def test_rounds_far_past_the_end(pkg, dev):
    name = "1x7"
    x, offsets, nA, strides, mask, input = C.CASES[name]()
    done = Call(pkg, dev, x, offsets, nA, strides, mask, input).complete()
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = c.run(4096)
    c.check()
    check(name, got, reference(name), mask)
    assert same(got, done) and int(got[2][0, ROUNDS]) == trace(name)[1][1] < 4096


def test_order_preserving_maps_of_the_weights(pkg, dev):
    """2 * w + 1 is exact on multiples of 2^-20 and keeps the order: the same partition, rounds and exclusions.  Negating one attractive
    channel reverses the order: complete, both are the rows; after ONE round the two are different partitions, each the simulation's"""
    name = "positive steps 3D"
    x, offsets, nA, strides, mask, input = C.positive_steps(2, 1)
    assert np.array_equal(x, np.float32(2) * NAMED[name]()[0] + np.float32(1))
    c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = c.complete()
    c.check()
    check(name + " mapped", got, reference(name), mask)
    firsts = []
    for sign in (1, -1):
        x, offsets, nA, strides, mask, input = C.one_channel(sign)
        g = C.graph(C.one_channel(sign))
        c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
        first = c.run(1)
        lab, used, slots, merged, active = R.rounds_trace(g, 1)
        assert np.array_equal(first[0].cpu().numpy().ravel(), lab) and first[2][0, :4].tolist() == [used, slots, merged, active]
        firsts.append(first[0])
        got = c.complete()
        c.check()
        check("one channel %+d" % sign, got, R.segment(x, C.off3(offsets), nA, C.st3(strides), mask, input, with_rounds=True), mask)
        assert got[1].tolist() == [37]
    assert not torch.equal(firsts[0], firsts[1])
