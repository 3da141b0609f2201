"""GPU: the mutex watershed on the device (include/pea_mws.h, csrc/pea_k_mws.hip) through the C ABI, through pea.mutex_watershed and
through seg_mutex, against the sequential definition restated in tests/mws_reference.py (which test_mws_host.py holds to a naive
second form and to a simulation of the round rule).

labels, counts and every column of stats are integers that the definition fixes (the exclusions are the sequential procedure's
exclusive pairs, the rounds the simulation's): every comparison is torch.equal / np.array_equal, no tolerance anywhere.  Every C call
of this file runs in a guard-banded arena (arena.py): the inputs come back untouched, every element of every output is written,
nothing else changes; the workspace is lent as it is -- filled with the arena's pattern, never prepared.  The call, the cases, their
shared reference and check() live in mws_cases.py, which test_gpu_mws_rounds.py uses too.

Case sizing: 37 x 41 is six runs of 256 pixels with a ragged one; 3 x 300 has a row that crosses a run; 33 x 65 x 2 and 5 x 12 x 20 step
along z; three images of different content exercise image isolation; reaches 9 and 27 leave channels with few or no edges."""
import importlib

import numpy as np
import pytest
import torch

import mws_reference as R
from mws_cases import CASES, EXCLUSIONS, OFF2, ROUNDS, UNDECIDED, Call, check, off3, reference, tt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_sequential_definition(pkg, dev, name):
    x, offsets, nA, strides, mask, input = CASES[name]()
    c = Call(pkg, dev, x[:, :, :, :, :], offsets, nA, strides, mask, input)
    got = c.complete()
    c.check()
    check(name, got, reference(name), mask)
    if name == "1x1":
        assert got[0].tolist() == [[[[1]]]] and got[2][0, :4].tolist() == [0, 0, 0, 0]
    if name == "mask isolated and empty":
        assert got[1].tolist()[1] == 0 and not bool(got[0][1].any()) and got[1].tolist()[0] >= 60  # singletons, label 0, counts = 0
    if name == "all attractive":
        assert got[2][:, EXCLUSIONS].tolist() == [0, 0]  # one cluster per connected valid region
    if name == "all equal":
        assert got[2][0, ROUNDS].item() < 40  # ties by edge id alone: the prune keeps the rounds few


def test_input_modes_order_the_edges_as_their_weights(pkg, dev):
    """the kernel's weights are the header's, bit for bit: handing it the reference's float32 weights as they are gives the same
    partition as the affinities, on a map where fl(1 - fl(1 - a)) != a decides ties"""
    rng = np.random.default_rng(20)
    a = (rng.integers(0, 6, (1, 8, 1, 37, 41)) * np.float32(0.1) + rng.integers(0, 3, (1, 8, 1, 37, 41)) * np.float32(2.0 ** -25)).astype(np.float32)
    assert (R.weights(a[:, :2], True, R.IN_AFFS) != a[:, :2]).any()
    w = np.concatenate([R.weights(a[:, :2], True, R.IN_AFFS), R.weights(a[:, 2:], False, R.IN_AFFS)], 1)
    c = np.float32(1) - a
    ref = R.segment(a, off3(OFF2), 2, [1, 2, 2], None, R.IN_AFFS, with_rounds=True)
    for x, input in ((a, R.IN_AFFS), (w, R.IN_WEIGHTS), (c, R.IN_ELF)):
        call = Call(pkg, dev, x, OFF2, 2, (2, 2), None, input)
        got = call.complete()
        call.check()
        check("input %d" % input, got, ref, None)
    # and taken as plain weights the affinities give another partition: the modes are not the same map
    other = R.segment(a, off3(OFF2), 2, [1, 2, 2], None, R.IN_WEIGHTS)
    assert not np.array_equal(other[0], ref[0])


def test_one_round_at_a_time_resumed_equals_the_one_shot_call(pkg, dev):
    name = "37x41 K10 B3"
    x, offsets, nA, strides, mask, input = CASES[name]()
    one = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    shot = one.run(64)
    one.check()
    check(name + " one shot", shot, reference(name), mask)
    step = Call(pkg, dev, x, offsets, nA, strides, mask, input)
    got = step.run(1)
    n = 1
    final = reference(name)[0]
    while int(got[2][:, UNDECIDED].max()) > 0:
        assert n < 64
        if n in (1, 2, 5, 12):  # the rounds ran out: a refinement of the final partition, image by image
            assert all(R.is_refinement(got[0][b].cpu().numpy(), final[b]) for b in range(len(final))), n
            assert n > 1 or not np.array_equal(got[0].cpu().numpy(), final)
        got = step.run(1, resume=True)
        n += 1
    step.check()
    print("rounds one at a time:", n, "stats", got[2].tolist())
    assert all(torch.equal(a, b) for a, b in zip(got, shot))
    # the images end at different rounds; their stats say how many each one used, and a round more changes nothing
    assert int(shot[2][:, ROUNDS].max()) <= n <= int(shot[2][:, ROUNDS].max()) + 2
    again = step.run(3, resume=True)
    assert all(torch.equal(a, b) for a, b in zip(again, shot))
    zero = Call(pkg, dev, x, offsets, nA, strides, mask, input).run(0)  # no round: every pixel is its own cluster
    S = 37 * 41
    assert torch.equal(zero[0].cpu(), torch.arange(1, S + 1, dtype=torch.int32).reshape(1, 1, 37, 41).expand(3, 1, 37, 41)) and zero[1].tolist() == [S] * 3
    assert (zero[2][:, UNDECIDED] > 0).all() and zero[2][:, :1].tolist() == [[0]] * 3


def test_two_runs_give_the_same_bits(pkg, dev):
    for name in ("noise", "2x33x65 K10 B3"):
        x, offsets, nA, strides, mask, input = CASES[name]()
        c = Call(pkg, dev, x, offsets, nA, strides, mask, input)
        first = c.run(64)
        second = c.run(64)  # on the workspace as the first call left it
        c.check()
        other = Call(pkg, dev, x, offsets, nA, strides, mask, input).run(64)
        assert all(torch.equal(a, b) for a, b in zip(first, second)) and all(torch.equal(a, b) for a, b in zip(first, other)), name
        check(name, first, reference(name), mask)


def test_element_aligned_pointers_in_a_guard_band(pkg, dev):
    name = "mask random"
    x, offsets, nA, strides, mask, input = CASES[name]()
    aligned = Call(pkg, dev, x, offsets, nA, strides, mask, input).complete()
    for skew in ((4, 1, 12, 4, 8), (12, 3, 4, 12, 4)):
        c = Call(pkg, dev, x, offsets, nA, strides, mask, input, skew=skew)
        got = c.complete()
        c.check()
        assert all(torch.equal(a, b) for a, b in zip(got, aligned)), skew
    check(name, aligned, reference(name), mask)


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def test_python_call_runs_to_completion(pkg, dev):
    for name in ("37x41 K10 B3", "5x12x20 K12", "mask random", "strides 5 5"):
        x, offsets, nA, strides, mask, input = CASES[name]()
        two_d = len(offsets[0]) == 2
        X = tt(x[:, :, 0] if two_d else x).to(dev)
        M = None if mask is None else tt(mask[:, 0] if two_d else mask).to(dev)
        out = pkg.mutex_watershed(X, offsets, strides, M, n_attractive=nA)
        rl, rc, rm, rx, ru = reference(name)
        assert out.labels.dtype == torch.int32 and out.labels.shape == (X.shape[:1] + X.shape[2:])
        assert np.array_equal(out.labels.cpu().numpy().reshape(rl.shape), rl) and np.array_equal(out.counts.cpu().numpy(), rc), name
        assert int(out.stat("undecided").max()) == 0 and np.array_equal(out.stats[:, 4:].cpu().numpy(), rm)
        assert np.array_equal(out.stat("exclusions").cpu().numpy(), rx) and np.array_equal(out.stat("rounds").cpu().numpy(), ru), name
        if M is not None:  # a bool mask, and pea.foreground_mask's own output (uint8 [B, H, W])
            assert torch.equal(pkg.mutex_watershed(X, offsets, strides, M.bool(), n_attractive=nA).labels, out.labels)
            logits = torch.stack([torch.zeros_like(M, dtype=torch.float32), M.float() - 0.5], 1)
            fg = pkg.foreground_mask(logits)
            assert torch.equal(fg, M) and torch.equal(pkg.mutex_watershed(X, offsets, strides, fg, n_attractive=nA).labels, out.labels)
        one = pkg.mutex_watershed(X[1 % len(X)], offsets, strides, None if M is None else M[1 % len(X)], n_attractive=nA)  # one image in, one out
        assert torch.equal(one.labels, out.labels[1 % len(X)]) and one.counts.dim() == 0 and one.stats.shape == (8,)
    # a view that is not dense is copied
    x, offsets, nA, strides, mask, input = CASES["strides 2 2"]()
    wide = torch.zeros((1, 8, 37, 82), device=dev)
    wide[..., ::2] = tt(x[:, :, 0]).to(dev)
    assert np.array_equal(pkg.mutex_watershed(wide[..., ::2], offsets, strides).labels.cpu().numpy(), reference("strides 2 2")[0][:, 0])


def test_graphed_call_with_fixed_rounds_replays_the_eager_result(pkg, dev):
    x, offsets, nA, strides, mask, input = CASES["quantised"]()
    X = tt(x[:, :, 0]).to(dev)

    def step(X):
        out = pkg.mutex_watershed(X, offsets, strides, rounds=48)
        return out.labels, out.counts, out.stats

    eager = [t.clone() for t in step(X)]
    g = pkg.graphed(step, X)
    for got in ([t.clone() for t in g.replay()], [t.clone() for t in g.replay()]):
        assert all(torch.equal(a, c) for a, c in zip(got, eager))
    assert int(eager[2][:, UNDECIDED].max()) == 0 and np.array_equal(eager[0].cpu().numpy(), reference("quantised")[0][:, 0])
    X.copy_(tt(np.ascontiguousarray(x[::-1, :, 0])))  # the input buffer refilled: the replay segments what it holds now
    got = [t.clone() for t in g.replay()]
    assert torch.equal(got[0], eager[0].flip(0)) and torch.equal(got[1], eager[1].flip(0))
    few = pkg.mutex_watershed(X, offsets, strides, rounds=2)  # rounds too small: said in stats, and a refinement
    assert int(few.stat("undecided").min()) > 0
    assert all(R.is_refinement(few.labels[b].cpu().numpy(), got[0][b].cpu().numpy()) for b in range(2))


def test_seg_mutex_on_a_leaf_image(pkg, dev):
    """the reference's call chain: embedding -> embedding2affs(activation='relu') -> seg_mutex(affs, offsets, strides), tensor and
    numpy forms, against the sequential definition on the same floats"""
    import __graft_entry__ as ge
    synth = importlib.import_module(ge.PKG_NAME + ".utils.synth")
    leaves = synth.synth_nuclei(1, 64, 64, 9, 11, seed=31)[0]
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((int(leaves.max()) + 1, 16)).astype(np.float32)
    e = centres[leaves].transpose(2, 0, 1)[None] + 0.15 * rng.standard_normal((1, 16, 64, 64)).astype(np.float32)
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], neighbor=4)
    affs = pkg.embedding2affs(tt(e).to(dev), offsets, activation="relu")[0]
    a = affs.cpu().numpy()
    for strides, mask in (([5, 5], None), ([1, 1], leaves > 0)):
        ref = R.segment(a[None, :, None], off3(offsets), 2, [1] + strides, None if mask is None else mask[None, None], R.IN_AFFS)[0][0, 0]
        m = None if mask is None else tt(mask).to(dev)
        got = pkg.seg_mutex(affs, offsets, strides, mask=m)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref)
        gn = pkg.seg_mutex(a, offsets, strides, mask=mask)
        assert isinstance(gn, np.ndarray) and gn.dtype == np.uint64 and np.array_equal(gn, ref)
        ge_ = pkg.elf_mutex_watershed(1.0 - affs, offsets, strides, mask=m)  # the AC3/AC4 call site hands 1 - affs
        assert np.array_equal(ge_.cpu().numpy(), R.segment((np.float32(1) - a)[None, :, None], off3(offsets), 2, [1] + strides,
                                                          None if mask is None else mask[None, None], R.IN_ELF)[0][0, 0])
        print("leaf image, strides", strides, "clusters", int(got.max()), "leaves", int(leaves.max()))
        assert 2 <= int(got.max())
