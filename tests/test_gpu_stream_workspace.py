"""The one per-stream workspace of the Python layer (affinity_op.stream_workspace): a block per (family, device, raw stream), prepared
once, replaced by a larger one when a call needs more -- the smaller one retired, not freed -- and never shared between families.
The callers are the loss states (affinity_op.workspace) and the four streaming families (harness/metrics.py, fgmask.py, disc.py,
segscore.py); the shapes are the smallest that make each of them call (B = 1, D = 4, S = 64)."""
import ctypes
import importlib

import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
B, D, Y, X = 1, 4, 8, 8
FAMILIES = ("metrics", "fgmask", "disc", "seg")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(ge.PKG_NAME + ".affinity_op")


def inputs(dev):
    g = torch.Generator().manual_seed(5)
    e = torch.randn((B, D, Y, X), generator=g).to(dev)
    labels = (torch.arange(Y * X).reshape(B, Y, X) // 16).to(torch.int32).to(dev)  # ids 0 .. 3
    logits = torch.randn((B, 2, Y, X), generator=g).to(dev)
    pred = torch.rand((B, 2, Y, X), generator=g).to(dev)
    target = (torch.rand((B, 2, Y, X), generator=g) < 0.5).float().to(dev)
    return e, labels, logits, pred, target


def call(pkg, family, t, num_ids=8):
    e, labels, logits, pred, target = t
    if family == "metrics":
        return pkg.affinity_metrics(pred, target).table
    if family == "fgmask":
        return pkg.foreground_mask_loss(logits, labels)[1]
    if family == "disc":
        return pkg.discriminative_loss_stats(e, labels, num_ids=num_ids)[1]
    return pkg.segmentation_scores(labels, labels).table


def block(op, family, dev):
    """the family's block of the current stream (None: none yet)"""
    return op._WS.get((family, dev.index, torch.cuda.current_stream(dev).cuda_stream))


def forget(op, family):
    """the family's blocks leave the cache as a growth would retire them (earlier tests may have grown them on a pooled stream)"""
    for k in [k for k in op._WS if k[0] == family]:
        op._RETIRED.append(op._WS.pop(k))


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def disc_by_hand(pkg, dev, e, labels, num_ids):
    """pea_disc_loss_fwd on a workspace made here, on the null stream -> (loss, stats)"""
    lib, L = pkg._lib, pkg._lib.lib()
    d = lib.PeaDiscDesc()
    d.B, d.D, d.S, d.num_ids, d.dtype, d.flags = B, D, Y * X, num_ids, 0, 0
    d.delta_v, d.delta_d, d.alpha, d.beta, d.gamma = 0.5, 1.5, 1.0, 1.0, 0.001
    nb = int(L.pea_disc_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    lib.check(L.pea_disc_workspace_init(vp(ws), nb, None), "pea_disc_workspace_init")
    loss, stats = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(lib.DISC_STATS + 4 * B, dtype=torch.float64, device=dev)
    ctx = torch.empty(int(L.pea_disc_context_bytes(ctypes.byref(d))) // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    lib.check(L.pea_disc_loss_fwd(ctypes.byref(d), vp(e), vp(labels.reshape(B, -1)), vp(loss), vp(stats), vp(ctx), vp(ws), nb, None), "pea_disc_loss_fwd")
    torch.cuda.synchronize()
    return loss.reshape(()), stats


@pytest.mark.parametrize("family", FAMILIES)
def test_a_stream_reuses_its_block_and_a_second_stream_gets_its_own(pkg, op, dev, family):
    t = inputs(dev)
    first = call(pkg, family, t).clone()
    w = block(op, family, dev)
    assert w is not None
    again = call(pkg, family, t)
    assert block(op, family, dev) is w and same_bits(first, again)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = call(pkg, family, t).clone()
        w2 = block(op, family, dev)
    side.synchronize()
    assert w2 is not None and w2 is not w and w2.data_ptr() != w.data_ptr()
    assert block(op, family, dev) is w and same_bits(first, other)


def test_families_do_not_share_blocks(pkg, op, dev):
    t = inputs(dev)
    blocks = []
    for family in FAMILIES:
        call(pkg, family, t)
        blocks.append(block(op, family, dev))
    assert all(w is not None for w in blocks) and len({w.data_ptr() for w in blocks}) == len(FAMILIES)


def test_loss_states_are_one_block_per_count(pkg, op, dev):
    e = inputs(dev)[0]
    d = op.make_desc(pkg.AffinitySpec(2, [[-1, 0], [0, -1]], None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX), e)
    one = int(pkg._lib.lib().pea_workspace_bytes(ctypes.byref(d)))
    w1, n1 = op.workspace(dev, d, 1)
    w2, n2 = op.workspace(dev, d, 2)
    assert (n1, n2) == (one, 2 * one) and w1.numel() * w1.element_size() == one and w2.numel() * w2.element_size() == 2 * one
    assert w1.data_ptr() != w2.data_ptr()
    assert op.workspace(dev, d, 1)[0] is w1 and op.workspace(dev, d)[0] is w1 and op.workspace(dev, d, 2)[0] is w2


def test_a_larger_request_replaces_the_block_and_retires_the_old_one(pkg, op, dev):
    t = inputs(dev)
    e, labels = t[:2]
    forget(op, "disc")
    call(pkg, "disc", t, num_ids=8)
    small = block(op, "disc", dev)
    call(pkg, "disc", t, num_ids=4096)
    large = block(op, "disc", dev)
    assert large is not small and large.numel() > small.numel()
    assert any(r is small for r in op._RETIRED)
    loss, stats = pkg.discriminative_loss_stats(e, labels, num_ids=4096)
    assert block(op, "disc", dev) is large
    ref_loss, ref_stats = disc_by_hand(pkg, dev, e, labels, 4096)
    assert same_bits(loss.detach(), ref_loss) and same_bits(stats, ref_stats)
    call(pkg, "disc", t, num_ids=8)  # a smaller request stays on the larger block
    assert block(op, "disc", dev) is large


def test_a_graph_captured_before_a_growth_replays_its_bits_after_it(pkg, op, dev):
    e, labels = inputs(dev)[:2]
    E = e.clone()

    def step(E, labels):
        return pkg.discriminative_loss_stats(E, labels, num_ids=8)

    forget(op, "disc")
    g = pkg.graphed(step, E, labels)  # captures on a stream of its own: the one disc block there is now, sized for num_ids = 8
    first = [o.detach().clone() for o in g.replay()]
    torch.cuda.synchronize()
    (key, captured), = [(k, w) for k, w in op._WS.items() if k[0] == "disc"]
    with torch.cuda.stream(torch.cuda.ExternalStream(key[2], device=dev)):  # the capture stream again: its block grows
        pkg.discriminative_loss_stats(e, labels, num_ids=4096)
    torch.cuda.synchronize()
    assert op._WS[key] is not captured and op._WS[key].numel() > captured.numel() and any(r is captured for r in op._RETIRED)
    second = [o.detach().clone() for o in g.replay()]
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(first, second))
    ref_loss, ref_stats = disc_by_hand(pkg, dev, e, labels, 8)
    assert same_bits(second[0], ref_loss) and same_bits(second[1], ref_stats)
