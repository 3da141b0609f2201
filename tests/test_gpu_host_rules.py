"""GPU (-m gpu): the host-side rules that the autograd nodes and the section nodes share (affinity_op.py: _backward_operands,
multi_forward) hand the library the same operands from either caller.

  1. Which of the 1 / norm planes (inv), the affinity map (affs) and the raw map of the backward (raw) are NULL in pea_affinity_fwd_ex /
     pea_affinity_bwd_ex2: embedding_loss + backward against loss 0 of cvppp_loss_section / ac3ac4_loss_section on the same tensors, at
     the smallest shapes that take each branch of the rule.  The full-resolution stencil has K = 4 offsets of reach 1, not 2: the 2D
     section slices offsets[:nb_half * (4, 3, 2, 1)], so its full resolution cannot have fewer than four.
  2. A second backward over a retained graph gives the first one's bits: op.MultiAffinityMSE and a batched section on one four-scale
     table of 32^2 .. 4^2 pixels.
"""
import importlib

import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

OFFSETS = [[-1, 0], [0, -1], [1, 0], [0, 1]]     # K = 4, reach 1, both in-plane axes (the role-A cross kernels want both)
SMALL_2D = [(16, 16), (12, 12), (8, 8), (6, 6)]  # the deep-supervision scales: never the full resolution's size
E_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(ge.PKG_NAME + ".affinity_op")


def null(p):
    return p is None or p.value is None


class Spy(object):
    """(function, image dims, second operand is NULL, inv is NULL, affs / raw is NULL) of every forward / backward launch of a single
    loss that returned PEA_OK while it is installed.  The fused pair (pea_affinity_fwd_dual_ex / pea_affinity_bwd_dual_ex: 2D, D = 16)
    is logged as its self loss: it writes both planes and the map, and its backward reads no raw map."""
    # name -> (kind, index of the second operand or None, of inv, of affs / raw or None)
    CALLS = {"pea_affinity_fwd_ex": ("fwd", 2, 8, 6), "pea_affinity_bwd_ex2": ("bwd", 2, 4, 5),
             "pea_affinity_fwd_dual_ex": ("fwd", None, 10, 7), "pea_affinity_bwd_dual_ex": ("bwd", None, 5, None)}

    def __init__(self, pkg, monkeypatch):
        L = pkg._lib.lib()
        self.log = []
        for name, (kind, i_o, i_inv, i_map) in self.CALLS.items():
            real = getattr(L, name)

            def wrapped(*a, _real=real, _kind=kind, _o=i_o, _inv=i_inv, _map=i_map):
                rc = _real(*a)
                if rc == 0:
                    self.log.append((_kind, tuple(a[0]._obj.dims), _o is None or null(a[_o]), null(a[_inv]), _map is None or null(a[_map])))
                return rc
            monkeypatch.setattr(L, name, wrapped)

    def take(self, dims, self_loss=True):
        """-> ((inv, affs NULL) of the forward, (inv, raw NULL) of the backward) of the one loss on an image of `dims`, and forget"""
        hits = [r for r in self.log if r[1] == tuple(dims) and r[2] == self_loss]
        self.log = []
        fwd, bwd = [r[3:] for r in hits if r[0] == "fwd"], [r[3:] for r in hits if r[0] == "bwd"]
        assert len(fwd) == 1 and len(bwd) == 1, hits
        return fwd[0], bwd[0]


@pytest.fixture
def spy(pkg, monkeypatch):
    return Spy(pkg, monkeypatch)


def rnd(dev, seed, *shape):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def inputs_2d(dev, D, H, W, seed):
    """what cvppp_loss_section takes at nb_half = 1: full resolution with K = 4, scales with K = 4, 3, 2, 1 and packed float thirds"""
    K = len(OFFSETS)
    a = dict(e=rnd(dev, seed, 1, D, H, W), ema=rnd(dev, seed + 1, 1, D, H, W), t=(rnd(dev, seed + 2, 1, K, H, W) > 0).float(),
             w=rnd(dev, seed + 3, 1, K, H, W).abs() + 0.5, m=(rnd(dev, seed + 4, 1, K, H, W) > -1).to(torch.uint8), emds=[], downs=[])
    for j, (h, w) in enumerate(SMALL_2D):
        k = 4 - j
        a["emds"].append(rnd(dev, seed + 10 + j, 1, D, h, w))
        thirds = rnd(dev, seed + 20 + j, 1, 3 * k, h, w)
        a["downs"].append(torch.cat([(thirds[:, :k] > 0).float(), thirds[:, k:2 * k].abs() + 0.5, (thirds[:, 2 * k:] > -1).float()], dim=1))
    return a


def modes(pkg, op, e, ndim, offsets, border, norm):
    d = op.make_desc(pkg.AffinitySpec(ndim, offsets, None, border, norm), e)
    return [op.cross_supported(d, mode) for mode in range(6)]


def smallest_with_plane_and_raw(pkg, op, dev, D):
    """the smallest [1, D, Y, X] f32 image on which the self backward stages the 1 / norm plane (mode 1) AND reads the raw map (mode 3)"""
    L = pkg._lib
    for _, Y, X in sorted((Y * X, Y, X) for Y in range(16, 72, 2) for X in range(32, 132, 4)):
        ms = modes(pkg, op, torch.empty((1, D, Y, X), device="meta"), 2, OFFSETS, L.BORDER_CIRCULAR, L.NORM_BX)
        if ms[1] and ms[3]:
            return Y, X
    raise AssertionError("no image up to 70 x 128 takes modes 1 and 3 at D = %d" % D)


def check_2d(pkg, op, dev, spy, D, H, W, want_inv, want_raw):
    crit = pkg.WeightedMSE()
    a = inputs_2d(dev, D, H, W, 7 * D + H)
    ms = modes(pkg, op, a["e"], 2, OFFSETS, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)
    assert (bool(ms[1]), bool(ms[1] and ms[3])) == (want_inv, want_raw), ms   # the shape takes the branch it is here for
    e = a["e"].clone().requires_grad_(True)
    loss, _, _ = pkg.embedding_loss(e, a["t"], a["w"], a["m"], crit, OFFSETS)
    loss.backward()
    single = spy.take((1, H, W))
    assert single == ((not want_inv, False), (not want_inv, not want_raw)), single
    leaves = [x.clone().requires_grad_(True) for x in [a["e"]] + a["emds"]]
    loss, _, _ = pkg.cvppp_loss_section(leaves[0], leaves[1:], a["ema"], a["t"], a["w"], a["m"], a["downs"], crit, OFFSETS, 1)
    loss.backward()
    torch.cuda.synchronize()
    assert spy.take((1, H, W)) == single


def test_2d_d32_plane_and_raw_map(pkg, op, dev, spy):
    """D = 32 keeps the section off the fused pair: _TensorSection.run::forward_one makes the launch"""
    H, W = smallest_with_plane_and_raw(pkg, op, dev, 32)
    check_2d(pkg, op, dev, spy, 32, H, W, True, True)


def test_2d_d32_no_mode_holds_at_30x30(pkg, op, dev, spy):
    """X % 4 != 0: no cross kernel takes the image; inv and raw are NULL from both callers"""
    check_2d(pkg, op, dev, spy, 32, 30, 30, False, False)


def test_2d_d16_plane_without_raw_map(pkg, op, dev, spy):
    H, W = smallest_with_plane_and_raw(pkg, op, dev, 32)
    check_2d(pkg, op, dev, spy, 16, H, W, True, False)


def test_3d_norm1_self_and_detached_cross(pkg, op, dev, spy):
    """[1, 16, 4, 32, 32], norm1: the self loss (modes 1 / 3) and the cross loss with a detached second operand (modes 2 / 4).  The
    section asks for the cross loss' planes only if its self loss got one; the cross loss' map is the section's own business (it hands
    none out), so inv and raw are compared there"""
    crit = pkg.WeightedMSE()
    dims, small = (4, 32, 32), [(4, 16, 16), (4, 8, 8), (2, 8, 8), (2, 4, 4)]
    e, ema = rnd(dev, 1, 1, 16, *dims), rnd(dev, 2, 1, 16, *dims)
    t, w = (rnd(dev, 3, 1, 3, *dims) > 0).float(), rnd(dev, 4, 1, 3, *dims).abs() + 0.5
    emds = [rnd(dev, 10 + j, 1, 16, *s) for j, s in enumerate(small)]
    downs = [torch.cat([(rnd(dev, 20 + j, 1, 3, *s) > 0).float(), rnd(dev, 30 + j, 1, 3, *s).abs() + 0.5], dim=1) for j, s in enumerate(small)][::-1]
    x = e.clone().requires_grad_(True)
    pkg.embedding_loss_norm1(x, t, w, crit)[0].backward()
    own = spy.take(dims)
    x = e.clone().requires_grad_(True)
    pkg.ema_embedding_loss_norm1(x, ema, t, w, crit)[0].backward()
    cross = spy.take(dims, self_loss=False)
    leaves = [v.clone().requires_grad_(True) for v in [e] + emds]
    loss, _ = pkg.ac3ac4_loss_section(leaves[0], leaves[1:], ema, t, w, downs, crit, embedding_mode=1)
    loss.backward()
    torch.cuda.synchronize()
    log = list(spy.log)
    assert spy.take(dims) == own
    spy.log = log
    sec_cross = spy.take(dims, self_loss=False)
    flat = lambda r: (r[0][0], r[1][0], r[1][1])  # noqa: E731 -- inv of the forward, inv and raw of the backward
    assert flat(sec_cross) == (flat(cross) if not own[0][0] else (True, True, True)), (own, cross, sec_cross)


class MultiSpy(object):
    def __init__(self, pkg, monkeypatch):
        L = pkg._lib.lib()
        self.rc = []
        for name in ("pea_affinity_fwd_multi", "pea_affinity_bwd_multi"):
            real = getattr(L, name)
            monkeypatch.setattr(L, name, lambda *a, _real=real, _name=name: (self.rc.append((_name, _real(*a))), self.rc[-1][1])[1])


def four_scales(dev):
    """one table of 32^2 .. 4^2 pixels, B = 1, D = 16, K = 4, 3, 2, 1"""
    sizes = [32, 16, 8, 4]
    embs = [rnd(dev, 40 + j, 1, 16, s, s) for j, s in enumerate(sizes)]
    ts = [(rnd(dev, 50 + j, 1, 4 - j, s, s) > 0).float() for j, s in enumerate(sizes)]
    ws = [rnd(dev, 60 + j, 1, 4 - j, s, s).abs() + 0.5 for j, s in enumerate(sizes)]
    ms = [(rnd(dev, 70 + j, 1, 4 - j, s, s) > -1).float() for j, s in enumerate(sizes)]
    return embs, ts, ws, ms


def test_multi_node_second_backward_over_a_retained_graph(pkg, dev, monkeypatch):
    spy = MultiSpy(pkg, monkeypatch)
    embs, ts, ws, ms = four_scales(dev)
    leaves = [x.clone().requires_grad_(True) for x in embs]
    out = pkg.embedding_loss_multi(leaves, ts, ws, ms, pkg.WeightedMSE(), [OFFSETS[:4 - j] for j in range(4)])
    total = sum((j + 1) * 0.375 * l for j, (l, _, _) in enumerate(out))
    g1 = [g.clone() for g in torch.autograd.grad(total, leaves, retain_graph=True)]
    g2 = torch.autograd.grad(total, leaves, retain_graph=True)
    torch.cuda.synchronize()
    assert spy.rc == [("pea_affinity_fwd_multi", 0), ("pea_affinity_bwd_multi", 0), ("pea_affinity_bwd_multi", 0)]
    for a, b in zip(g1, g2):
        assert bool(a.abs().sum() > 0) and torch.equal(a, b)


def test_batched_section_second_backward_over_a_retained_graph(pkg, dev, monkeypatch):
    spy = MultiSpy(pkg, monkeypatch)
    embs, ts, ws, ms = four_scales(dev)
    K = len(OFFSETS)
    full = [rnd(dev, 80, 1, 16, 64, 64), rnd(dev, 81, 1, 16, 64, 64), (rnd(dev, 82, 1, K, 64, 64) > 0).float(),
            rnd(dev, 83, 1, K, 64, 64).abs() + 0.5, (rnd(dev, 84, 1, K, 64, 64) > -1).to(torch.uint8)]
    downs = [torch.cat([t, w, m], dim=1) for t, w, m in zip(ts, ws, ms)]
    leaves = [x.clone().requires_grad_(True) for x in [full[0]] + embs]
    loss, _, _ = pkg.cvppp_loss_section(leaves[0], leaves[1:], full[1], full[2], full[3], full[4], downs, pkg.WeightedMSE(), OFFSETS, 1,
                                        deep_weight=2, batched=True)
    g1 = [g.clone() for g in torch.autograd.grad(loss * 0.5, leaves, retain_graph=True)]
    g2 = torch.autograd.grad(loss * 0.5, leaves, retain_graph=True)
    torch.cuda.synchronize()
    # the section's forward makes both launches; the second backward computes the section again
    assert spy.rc == [("pea_affinity_fwd_multi", 0), ("pea_affinity_bwd_multi", 0)] * 2
    for a, b in zip(g1, g2):
        assert bool(a.abs().sum() > 0) and torch.equal(a, b)
