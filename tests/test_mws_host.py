"""CPU: the mutex watershed (include/pea_mws.h) -- the three restatements of tests/mws_reference.py, which the GPU tests compare the
kernels with, agree with each other as partitions: (a) the sequential definition, (b) a naive form that answers "exclusive?" by scanning
the earlier exclusion edges, (c) the round rule of the header as a simulation.  The key order is held to np.lexsort, the three input
modes' weights to a float64 computation rounded step by step.  The header and the library agree on the three new symbols, the ctypes
mirror has the header's layout, every refusal of pea_mws_validate and pea_mws_segment is reached before anything is launched and in the
header's order (dummy device pointers, no GPU), pea_mws_workspace_bytes is monotone, and the Python entry points say what is wrong with
a call before they look for a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mws_cases as C
import mws_reference as R
from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
RESUME = 1
NEW = ["pea_mws_segment", "pea_mws_validate", "pea_mws_workspace_bytes"]
SIZE_MAX = 2 ** 64 - 1
OFFSETS = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-3, -3], [-9, 0], [0, -9], [3, -3]]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def graphs():
    """a few dozen seeded graphs, 8 x 8 to 40 x 40: five weight kinds x four strides, a mask on every other one"""
    out = []
    seed = 0
    for kind in ("noise", "blobs", "quantised", "ties", "clean"):
        for strides in ((1, 1), (2, 2), (1, 3), (5, 5)):
            for Y, X in ((8, 8), (40, 40)) if strides in ((1, 1), (5, 5)) else ((13, 21),):
                seed += 1
                out.append((seed, Y, X, strides, kind, seed % 2 == 0))
    return out


@pytest.mark.parametrize("case", graphs(), ids=lambda c: "%s-%dx%d-s%d%d%s" % (c[4], c[1], c[2], c[3][0], c[3][1], "-mask" if c[5] else ""))
def test_three_restatements_agree(case):
    seed, Y, X, strides, kind, masked = case
    x, offsets, mask = R.graph_cases(*case)
    g = R.edges(x, offsets, 2, strides, mask, R.IN_AFFS)
    a = R.sequential(g)
    assert np.array_equal(a, R.naive(g)), "the sequential form and the naive scan differ"
    c, used, left = R.rounds(g)
    assert left == 0 and np.array_equal(a, c), "the round rule differs from the sequential form"
    assert (a[~g.valid] == 0).all() and (a[g.valid] > 0).all() and a.max() == len(np.unique(a[g.valid]))
    # rounds that run out leave a refinement of the final partition, and the prefix property of the definition itself
    few, used_few, left_few = R.rounds(g, max_rounds=2)
    assert R.is_refinement(few, a) and (left_few > 0 or np.array_equal(few, a))
    assert R.is_refinement(R.sequential(g, limit=len(g.p) // 3), a)
    # the trace is the same simulation; its counts at the end are those of the sequential form: the active exclusions are the distinct
    # exclusive pairs, every merge took one cluster away
    a2, pairs = R.sequential(g, with_exclusions=True)
    t, t_used, slots, merged, active = R.rounds_trace(g)
    assert np.array_equal(a2, a) and np.array_equal(t, c) and t_used == used and slots == 0
    assert active == pairs and merged == int(g.valid.sum()) - int(a.max())
    before = len(g.p)
    for n in (1, 2, 5):
        part, n_used, slots, merged, active = R.rounds_trace(g, n)
        short, short_used, short_left = R.rounds(g, max_rounds=n)
        assert np.array_equal(part, short) and n_used == short_used == min(n, used)
        assert (short_left > 0 and slots > 0) if n < used else (n == used or short_left == slots == 0)
        assert R.is_refinement(part, a) and slots <= before and slots + merged + active <= len(g.p)
        assert merged == int(g.valid.sum()) - int(part.max()) and (n < used or np.array_equal(part, a))
        before = slots


def test_the_table_prune_is_part_of_the_rule():
    """without the prune the result is the same and the rounds are many more (the header's remark on all-tie images)"""
    x, offsets, mask = R.graph_cases(5, 24, 24, (1, 1), "clean", False)
    g = R.edges(x, offsets, 2, (1, 1), mask)
    a, with_prune, _ = R.rounds(g)
    b, without, _ = R.rounds(g, prune_table=False)
    assert np.array_equal(a, b) and np.array_equal(a, R.sequential(g)) and without > with_prune


# ---- the named graphs of test_gpu_mws_rounds.py: what each name promises, held on the reference alone --------------------------------------
def traced(case, b=0):
    """-> (graph, sequential labels, exclusive pairs, the trace's final tuple with the states, history, hooks)"""
    g = C.graph(case, b)
    lab, pairs = R.sequential(g, with_exclusions=True)
    hist, hooks = [], []
    end = R.rounds_trace(g, history=hist, states=True, hooks=hooks)
    assert np.array_equal(end[0], lab) and end[2] == 0 and end[4] == pairs and end[3] == int(g.valid.sum()) - int(lab.max())
    assert len(hist) == len(hooks) == end[1] and all(h[1] == i + 1 for i, h in enumerate(hist))
    return g, lab, pairs, end, hist, hooks


def one_chain(hooked):
    """the hooks of a round are ONE chain through every node: one root (so one tree), which is the smaller end of the last, mutual
    edge, and no node with more than two neighbours -- a path, with the root next to its far end"""
    nodes = np.arange(len(hooked))
    children = np.bincount(hooked[hooked != nodes], minlength=len(hooked))
    degree = children + (hooked != nodes)
    return int((hooked == nodes).sum()) == 1 and int(degree.max()) == 2 and int((degree == 1).sum()) == 2


def test_named_rising_line_and_snake_hook_one_chain_in_one_round():
    for name, edges_, S in (("rising line", 4099, 4100), ("snake", 4354, 65 * 67)):
        g, lab, pairs, end, hist, hooks = traced(C.NAMED[name]())
        assert len(g.p) == edges_ == S - 1 and g.att.all() and g.S == S
        assert end[1] == 1 and hist[0][3] == edges_ and hist[0][2] == 0, name  # one round decides every edge
        assert int(lab.max()) == 1 and pairs == 0
        hooked, doublings = hooks[0]
        assert one_chain(hooked) and doublings == 13, (name, doublings)  # 2^12 < 4098 and 4353 <= 2^13
    g = C.graph(C.NAMED["snake"]())
    assert g.missing == dict(stride=0, mask=0, nan=64 * 67 - 64, outside=65 + 67)
    # the hooks of the snake run both ways along x and cross rows: ends one row apart, and x steps of both signs
    hooked = traced(C.NAMED["snake"]())[5][0][0]
    step = hooked - np.arange(g.S)
    assert (step == 1).any() and (step == -1).any() and (np.abs(step) == 67).any()
    assert C.NAMED["rising line"]()[0][0, 0, 0, 0, 4099] == 4099 and len(np.unique(g.w)) == len(g.w)


def test_named_falling_lines_decide_one_edge_a_round():
    g, lab, pairs, end, hist, hooks = traced(C.NAMED["falling line"]())
    assert end[1] == 299 and int(lab.max()) == 2 and pairs == 1
    # the first round makes the 150 repulsive edges exclusions; every later one decides exactly one edge, a merge
    assert hist[0][3:5] == (0, 150) and all(hist[i][3] == i for i in range(1, 299))
    assert [h[2] for h in hist] == sorted((h[2] for h in hist), reverse=True) and hist[-1][2] == 0
    for n in (1, 2, 3, 50, 150, 298):  # the snapshot rounds of the GPU test: all different, none final
        assert not np.array_equal(hist[n - 1][0], lab) and hist[n - 1][2] > 0
    g, lab, pairs, end, hist, hooks = traced(C.NAMED["falling line, reach 2"]())
    assert end[1] == 151 and int(lab.max()) == 150 and pairs == 149 and (np.bincount(lab)[1:] == 2).all()


def test_named_three_tempos_end_at_different_rounds():
    case = C.NAMED["three tempos"]()
    used = [traced(case, b)[3][1] for b in range(3)]
    assert used[0] == 1 and used[1] == 299 and 1 < used[2] < 32 and C.reference("three tempos")[4].tolist() == used
    assert np.isnan(case[0][0, 1]).all() and not np.isnan(case[0][1:]).any()
    assert np.array_equal(case[0][1], C.NAMED["falling line"]()[0][0])


def test_named_fullest_table_loads_the_table():
    case = C.NAMED["table at its fullest"]()
    g, lab, pairs, end, hist, hooks = traced(case)
    lattice = 16 * 21
    cap = 64
    while cap < 2 * 6 * lattice:
        cap *= 2
    assert cap == C.FULLEST_CAPACITY == 4096 and 2 * 6 * lattice == 4032
    top = max(h[4] for h in hist)
    print("active exclusions at most", top, "of", cap, "at the end", pairs)
    assert top >= 0.35 * cap and pairs >= 1200
    assert float(case[0][0, 2:].min()) >= 2 and float(case[0][0, :2].max()) < 1


def test_named_twins_name_one_pair_more_than_once():
    for kind in ("quantised", "noise"):
        case = C.NAMED["twins " + kind]()
        g, lab, pairs, end, hist, hooks = traced(case)
        S, state = g.S, end[5]
        zero = g.eid // S == 6
        assert int(zero.sum()) == S and np.array_equal(g.p[zero], g.q[zero])  # every slot of the zero offset is inside and exists
        assert (state[zero] == 1).all()
        rep = ~g.att & ~zero
        pair = np.minimum(g.p, g.q)[rep] * S + np.maximum(g.p, g.q)[rep]
        names, inv, count = np.unique(pair, return_inverse=True, return_counts=True)
        assert set(count.tolist()) == {3} and len(names) == 10 * 21  # (-3, 0) twice and (3, 0) name every pair of pixels 3 rows apart
        active = np.bincount(inv, weights=state[rep] == 3, minlength=len(names))
        assert active.max() == 1 and int(active.sum()) >= 1  # of the edges that name one pair at most one stays active, and some do
        if kind == "quantised":  # the twins tie, the lower edge id goes first: channel 3 wins over channels 4 and 5
            assert (np.asarray(case[0]) * 4 == np.round(np.asarray(case[0]) * 4)).all()
            assert len(np.unique(g.w)) <= 8


def test_named_positive_steps_and_its_order_preserving_map():
    case = C.NAMED["positive steps 3D"]()
    g, lab, pairs, end, hist, hooks = traced(case)
    assert all(min(o) >= 0 for o in case[1][:3]) and all(max(o) > 0 for o in case[1]) and g.missing["stride"] > 0 and g.missing["mask"] > 0
    assert int(lab.max()) > 2 and pairs > 0
    mapped = C.graph(C.positive_steps(2, 1))
    assert np.array_equal(mapped.w, np.float32(2) * g.w + np.float32(1)) and np.array_equal(mapped.w.astype(np.float64), 2 * g.w.astype(np.float64) + 1)
    assert np.array_equal(mapped.eid, g.eid)  # the sorted order of the keys is the same edge for edge
    # one channel and its negation: complete, both are the rows; after one round they are two different partitions
    up, down = C.graph(C.one_channel(1)), C.graph(C.one_channel(-1))
    assert np.array_equal(np.sort(up.eid), np.sort(down.eid)) and np.array_equal(up.eid, down.eid[::-1])
    assert np.array_equal(R.sequential(up), R.sequential(down)) and int(R.sequential(up).max()) == 37
    assert not np.array_equal(R.rounds_trace(up, 1)[0], R.rounds_trace(down, 1)[0])


def test_named_k32_far_channels_hold_no_edge():
    x, offsets, nA, strides, mask, input = C.NAMED["K32 far"]()
    S = 9 * 11
    far = [k for k, (dy, dx) in enumerate(offsets) if abs(dy) >= 9 or abs(dx) >= 11]
    # (OFF2's own (-9, 0) reaches the 9 rows as well: it is there twice)
    assert len(offsets) == 32 and len(C.FAR) == 10 and sorted(offsets[k] for k in far) == sorted(C.FAR + [[-9, 0]]) and min(far) >= nA
    for k in far:  # alone, attracting or repelling, whatever x holds: outside, and under nothing else
        assert np.isnan(x[0, k]).any() and not np.isnan(x[0, k]).all()
        for att in (0, 1):
            one = R.edges(x[0, k:k + 1], C.off3([offsets[k]]), att, C.st3(strides), None, input)
            assert one.missing == dict(stride=0, mask=0, nan=0, outside=S) and len(one.p) == 0, offsets[k]
    g = C.graph(C.NAMED["K32 far"]())
    assert not np.isin(g.eid // S, far).any()
    for k in (offsets.index([-8, -10]), offsets.index([8, 10])):  # one slot inside
        one = R.edges(np.zeros((1, 1, 9, 11), np.float32), C.off3([offsets[k]]), 1, [1, 1, 1], None, input)
        assert len(one.p) == 1 and one.missing["outside"] == S - 1
    traced(C.NAMED["K32 far"]())


def test_named_large_cases_cross_their_thresholds():
    g, lab, pairs, end, hist, hooks = traced(C.NAMED["more than 65536 pixels"]())
    assert g.S == 260 * 261 > 65536 and -(-g.S // 256) == 266
    firsts = np.unique(lab, return_index=True)[1]
    assert int(lab.max()) > 100 and (firsts < 65536).sum() > 1 and (firsts >= 65536).sum() > 1
    ref = C.reference("more than 256 images")
    assert len(ref[1]) == 257 and len(np.unique(ref[1])) >= 3 and len(np.unique(ref[4])) >= 2


def test_missing_edges_are_counted_once_by_their_first_cause():
    x = np.full((3, 1, 4, 6), 0.5, np.float32)
    x[2, 0, 0, 2] = np.nan            # repulsive, on the stride lattice, inside, valid: a NaN
    x[2, 0, 0, 0] = np.nan            # its far end (2, 2) is masked: counted as mask
    x[2, 0, 1, 1] = np.nan            # off the lattice: counted as stride
    x[2, 0, 3, 5] = np.nan            # its far end is outside: counted as outside
    x[0, 0, 3, 5] = np.nan            # attractive: a NaN
    mask = np.ones((1, 4, 6), np.uint8)
    mask[0, 2, 2] = 0
    g = R.edges(x, [[-1, 0], [0, -1], [2, 2]], 2, (2, 2), mask)
    # outside: the first row, the first column, and for (2, 2) all but the 2 x 4 pixels with y < 2, x < 4
    assert g.missing["outside"] == 6 + 4 + (24 - 8)
    # the masked pixel (2, 2) is an end of two slots of each attractive channel and the far end of (0, 0) + (2, 2)
    assert g.missing["mask"] == 2 + 2 + 1
    # of the 8 - 1 repulsive slots left, (0, 2) alone is on the lattice
    assert g.missing["stride"] == 6 and g.missing["nan"] == 2
    assert len(g.p) == 3 * 24 - 26 - 5 - 6 - 2 and int(g.att.sum()) == 2 * 24 - 10 - 4 - 1


def test_key_order_against_lexsort():
    rng = np.random.default_rng(1)
    w = np.concatenate([rng.standard_normal(500), rng.integers(-2, 3, 500) * 0.5, [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40]]).astype(np.float32)
    w[rng.random(w.size) < 0.1] = np.float32(-0.0)
    eid = rng.permutation(2 ** 32 - 1 - np.arange(w.size)).astype(np.uint64)
    key = R.keys(w, eid)
    assert len(np.unique(key)) == key.size
    got = np.argsort(key)[::-1]  # a larger key comes first
    # the higher weight first (-0.0 below +0.0), equal weights by the lower edge id
    sign = np.signbit(w) & (w == 0)
    want = np.lexsort((eid, sign, -w.astype(np.float64)))
    assert np.array_equal(got, want)
    v = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 2.0, np.inf], np.float32)
    assert (np.diff(R.ord32(v).astype(np.int64)) > 0).all() and R.ord32(np.float32(0.0)) == 0x80000000


def test_input_modes_weights_bit_for_bit():
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.random(4000), [0.0, 1.0, 0.1, 0.3, 2.0 ** -20, 1 - 2.0 ** -24, 0.7]]).astype(np.float32)
    fl = lambda v: np.asarray(v, np.float64).astype(np.float32)  # (1 - a of a float32 in [2^-20, 2] is exact in float64: one rounding)
    one = np.float64(1.0)
    bits = lambda v: np.asarray(v, np.float32).view(np.uint32)
    assert np.array_equal(bits(R.weights(a, True, R.IN_AFFS)), bits(fl(one - fl(one - a.astype(np.float64)).astype(np.float64))))
    assert np.array_equal(bits(R.weights(a, False, R.IN_AFFS)), bits(fl(one - a.astype(np.float64))))
    c = R.ONE - a
    assert np.array_equal(bits(R.weights(c, True, R.IN_ELF)), bits(R.weights(a, True, R.IN_AFFS)))
    assert np.array_equal(bits(R.weights(c, False, R.IN_ELF)), bits(c)) and np.array_equal(bits(R.weights(a, True, R.IN_WEIGHTS)), bits(a))
    # the round trip is not the identity: the attractive weight of "affs" is not a itself
    differs = R.weights(a, True, R.IN_AFFS) != a
    assert differs.any() and R.weights(np.float32(0.1), True, R.IN_AFFS) != np.float32(0.1)
    assert R.weights(np.float32(0.1), True, R.IN_AFFS) == np.float32(1) - (np.float32(1) - np.float32(0.1))


# ---- exports -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_mws.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_MWS) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src
    for name, val in (("MAX_K", "32"), ("RESUME", "1u"), ("IN_AFFS", "0"), ("IN_ELF", "1"), ("IN_WEIGHTS", "2"), ("STATS", "8"),
                      ("MAX_ROUNDS", "65536")):
        assert re.search(r"#define\s+PEA_MWS_%s\s+%s\b" % (name, val), src), name
    for i, col in enumerate(pkg._lib.MWS_STAT_COLUMNS):
        assert re.search(r"#define\s+PEA_MWS_%s\s+%d\b" % (col.upper(), i), src), col
    assert (pkg._lib.MWS_MAX_K, pkg._lib.MWS_RESUME, pkg._lib.MWS_STATS, pkg._lib.MWS_MAX_ROUNDS) == (32, 1, 8, 65536)
    assert pkg._lib.MWS_INPUTS == {"affs": 0, "elf": 1, "weights": 2} == R.INPUTS
    for cite in ("seg_mutex", "not elf's", "unspecified among equal", "strict total order", "Why it is exact"):
        assert cite in src, cite
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert not set(NEW) & set(pkg._lib.EXPORTS)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "pea_mws" in open(os.path.join(ROOT, doc)).read(), doc
    assert "unspecified" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaMwsDesc
    names = ["B", "Z", "Y", "X", "K", "n_attractive", "offsets", "strides", "input", "rounds", "flags"]
    assert [f[0] for f in D._fields_] == names and ctypes.sizeof(D) == 4 * (6 + 96 + 3 + 3)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_mws.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaMwsDesc \{(.*?)\} PeaMwsDesc;", src, flags=re.S).group(1)
    declared = [re.sub(r"\[.*", "", n) for decl in body.split(";") if decl.strip()
                for n in re.sub(r"^\s*(u?int32_t)", "", decl.strip()).replace(" ", "").split(",")]
    assert declared == names
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 24 + 384, 420, 424, 428]


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
PTR = {n: 0x10000000 * (i + 1) for i, n in enumerate(("x", "mask", "labels", "counts", "stats", "work"))}


def desc(pkg, B=2, Z=1, Y=37, X=41, K=8, n_attractive=2, offsets=OFFSETS, strides=(1, 2, 2), input=0, rounds=3, flags=0):
    d = pkg._lib.PeaMwsDesc()
    d.B, d.Z, d.Y, d.X, d.K, d.n_attractive, d.input, d.rounds, d.flags = B, Z, Y, X, K, n_attractive, input, rounds, flags
    for k, o in enumerate(offsets[:32]):
        d.offsets[k][:] = [0] * (3 - len(o)) + list(o)
    d.strides[:] = strides
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def call(pkg, lib, d="default", wbytes=None, **kw):
    """pea_mws_segment on dummy pointers: anything but an early return would fault"""
    p = dict(PTR)
    for k in list(kw):
        if k in p:
            p[k] = kw.pop(k)
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = lib.pea_mws_workspace_bytes(ctypes.byref(d)) if d is not None else 0
    return lib.pea_mws_segment(None if d is None else ctypes.byref(d), vp(p["x"]), vp(p["mask"]), vp(p["labels"]), vp(p["counts"]),
                               vp(p["stats"]), vp(p["work"]), wbytes, None)


BIG = dict(B=1, Z=1, Y=1 << 15, X=1 << 14, K=8)        # K * S = 2^32
WIDE = dict(B=1, Z=1, Y=1 << 16, X=1 << 15, K=1, n_attractive=1)  # S = 2^31
HUGE = dict(B=2 ** 31 - 1, Z=2 ** 31 - 1, Y=2 ** 31 - 1, X=2 ** 31 - 1)


def test_validate_and_its_order(pkg, lib):
    v = lambda **kw: lib.pea_mws_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_mws_validate(None) == E_NULL and call(pkg, lib, d=None) == E_NULL and lib.pea_mws_workspace_bytes(None) == 0
    assert v() == OK and v(B=1, Z=1, Y=1, X=1, K=1, n_attractive=1) == OK and v(n_attractive=8) == OK and v(flags=RESUME) == OK
    assert v(K=32, offsets=OFFSETS * 4) == OK and v(input=2, rounds=0) == OK and v(rounds=65536) == OK and v(**HUGE) == OK and v(**BIG) == OK
    bad = [dict(flags=2), dict(flags=1 << 31), dict(B=0), dict(Z=0), dict(Y=-3), dict(X=0), dict(K=0), dict(K=33), dict(n_attractive=0),
           dict(n_attractive=9), dict(strides=(0, 1, 1)), dict(strides=(1, 1, -2)), dict(input=3), dict(input=-1), dict(rounds=-1),
           dict(rounds=65537)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert call(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_mws_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0, kw
    # a descriptor is refused before a NULL pointer, a short workspace or a size is looked at
    assert call(pkg, lib, x=0, labels=0, work=0, K=33, **{k: v_ for k, v_ in BIG.items() if k != "K"}) == E_DESC


def test_refusals_before_a_launch_and_their_order(pkg, lib):
    for name in ("x", "labels", "counts", "stats"):
        assert call(pkg, lib, **{name: 0}) == E_NULL, name
    assert call(pkg, lib, mask=0, work=0) == E_WORKSPACE  # the mask is optional
    # K * S >= 2^32 or S >= 2^31; more than 2^31 - 1 workgroups
    assert call(pkg, lib, **BIG) == E_UNSUPPORTED and call(pkg, lib, **WIDE) == E_UNSUPPORTED and call(pkg, lib, wbytes=SIZE_MAX, **HUGE) == E_UNSUPPORTED
    assert call(pkg, lib, B=1, Z=1, Y=1 << 15, X=(1 << 14) - 1, K=8, work=0) == E_WORKSPACE  # one column fewer is served
    assert call(pkg, lib, B=1 << 12, Z=1, Y=1 << 12, X=1 << 12, K=32, offsets=OFFSETS * 4) == E_UNSUPPORTED  # 2^31 workgroups
    for skew in (1, 2, 3):
        for name in ("x", "labels", "counts", "stats", "work"):
            assert call(pkg, lib, **{name: PTR[name] + skew}) == E_ALIGN, (name, skew)
        assert call(pkg, lib, mask=PTR["mask"] + skew, work=0) == E_WORKSPACE  # bytes: any address
    assert call(pkg, lib, work=PTR["work"] + 4) == E_ALIGN
    need = lib.pea_mws_workspace_bytes(ctypes.byref(desc(pkg)))
    assert call(pkg, lib, work=0) == E_WORKSPACE and call(pkg, lib, wbytes=need - 1) == E_WORKSPACE and call(pkg, lib, wbytes=0) == E_WORKSPACE
    assert call(pkg, lib, work=0, flags=RESUME) == E_WORKSPACE
    # the stated order: descriptor, NULL, size, alignment, workspace
    assert call(pkg, lib, work=0, labels=PTR["labels"] + 2) == E_ALIGN
    assert call(pkg, lib, work=0, labels=PTR["labels"] + 2, **BIG) == E_UNSUPPORTED
    assert call(pkg, lib, x=0, work=0, labels=PTR["labels"] + 2, **BIG) == E_NULL
    assert call(pkg, lib, x=0, work=0, labels=PTR["labels"] + 2, rounds=-1, **BIG) == E_DESC


def al8(x):
    return (x + 7) // 8 * 8


def test_workspace_bytes_is_monotone_in_each_extent(pkg, lib):
    nb = lambda **kw: lib.pea_mws_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    base = dict(B=2, Z=3, Y=37, X=41, K=8)
    for name in ("B", "Z", "Y", "X"):
        sizes = [nb(**dict(base, **{name: v})) for v in range(1, 70)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], name
    sizes = [nb(**dict(base, K=k, offsets=OFFSETS * 4)) for k in range(2, 33)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    # the layout: four int32 images, the scan's totals, best, the table (a power of two >= twice the repulsive slots), 16 + 32 * 8 words, has_con, states
    for B, Z, Y, X, K, nA, st in ((1, 1, 1, 1, 1, 1, (1, 1, 1)), (2, 1, 37, 41, 8, 2, (1, 2, 2)), (3, 5, 12, 20, 12, 3, (1, 2, 2)), (1, 1, 64, 64, 8, 2, (1, 5, 5))):
        S = Z * Y * X
        lattice = -(-Z // st[0]) * -(-Y // st[1]) * -(-X // st[2])
        cap = 64
        while cap < 2 * (K - nA) * lattice:
            cap *= 2
        want = 4 * al8(4 * B * S) + al8(4 * B * -(-S // 256)) + 8 * B * S + 8 * B * cap + 8 * (16 + 32 * 8) * B + al8(B * S) + al8(B * S * K)
        assert nb(B=B, Z=Z, Y=Y, X=X, K=K, n_attractive=nA, strides=st, offsets=OFFSETS * 4) == want, (B, Z, Y, X, K)
    assert nb(rounds=0, input=2, flags=RESUME) == nb() and nb() % 8 == 0
    assert nb(strides=(1, 1, 1)) >= nb(strides=(1, 2, 2)) >= nb(strides=(1, 5, 5))
    assert nb(**HUGE) == SIZE_MAX


# ---- the Python entry points -------------------------------------------------------------------------------------------------------------
def test_python_entry_points(pkg):
    from importlib import import_module
    for name in pkg.MWS_EXPORTS:
        assert hasattr(pkg, name), name
    mod = import_module(pkg.__name__ + ".utils.seg_mutex")
    assert mod.seg_mutex is pkg.seg_mutex and mod.mutex_watershed is pkg.elf_mutex_watershed
    sig = inspect.signature(pkg.seg_mutex)  # the reference's signature
    assert list(sig.parameters) == ["affs", "offsets", "strides", "randomize_strides", "mask"]
    assert [p.default for p in sig.parameters.values()][1:] == [[[-1, 0], [0, -1]], [1, 1], False, None]
    sig = inspect.signature(mod.mutex_watershed)  # elf's
    assert list(sig.parameters) == ["affs", "offsets", "strides", "randomize_strides", "mask"]
    assert sig.parameters["randomize_strides"].default is False and sig.parameters["mask"].default is None
    sig = inspect.signature(pkg.mutex_watershed)
    assert list(sig.parameters) == ["x", "offsets", "strides", "mask", "input", "n_attractive", "rounds"]
    assert [p.default for p in sig.parameters.values()][2:] == [None, None, "affs", None, None]
    assert "sequential by construction.  So are seg_mutex" not in pkg.postprocessing.__doc__ and "seg_mutex" in pkg.postprocessing.__doc__

    a = torch.zeros(8, 20, 30)
    if not torch.cuda.is_available():
        for f in (lambda: pkg.mutex_watershed(a, OFFSETS), lambda: pkg.mutex_watershed(a[None], OFFSETS, rounds=4),
                  lambda: pkg.seg_mutex(a, OFFSETS), lambda: pkg.seg_mutex(a.numpy(), OFFSETS, [5, 5]),
                  lambda: pkg.elf_mutex_watershed(1 - a, OFFSETS, [1, 1], mask=np.ones((20, 30), bool))):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f()
    for kw in (dict(randomize_strides=True),):
        with pytest.raises(NotImplementedError, match="randomize_strides"):
            pkg.seg_mutex(a, OFFSETS, **kw)
        with pytest.raises(NotImplementedError, match="randomize_strides"):
            pkg.elf_mutex_watershed(a.numpy(), OFFSETS, [1, 1], **kw)
    with pytest.raises(ValueError, match="channels"):
        pkg.mutex_watershed(a, OFFSETS[:5])
    with pytest.raises(ValueError, match=r"\[K, Y, X\] or \[B, K, Y, X\]"):
        pkg.mutex_watershed(torch.zeros(20, 30), OFFSETS)
    with pytest.raises(ValueError, match="steps"):
        pkg.mutex_watershed(a, [[-1, 0], [0, -1, 0]] + OFFSETS[2:])
    with pytest.raises(ValueError, match="offsets are served"):
        pkg.mutex_watershed(torch.zeros(33, 4, 4), [[-1, 0]] * 33)
    with pytest.raises(TypeError, match="float32"):
        pkg.mutex_watershed(a.double(), OFFSETS)
    with pytest.raises(TypeError, match="torch.Tensor"):
        pkg.mutex_watershed(a.numpy(), OFFSETS)
    with pytest.raises(ValueError, match="empty"):
        pkg.mutex_watershed(torch.zeros(8, 0, 30), OFFSETS)
    for st in ([0, 1], [1], [1, 1, 1]):
        with pytest.raises(ValueError, match="strides"):
            pkg.mutex_watershed(a, OFFSETS, st)
    for na in (0, 9):
        with pytest.raises(ValueError, match="n_attractive"):
            pkg.mutex_watershed(a, OFFSETS, n_attractive=na)
    with pytest.raises(ValueError, match="input"):
        pkg.mutex_watershed(a, OFFSETS, input="costs")
    for r in (-1, 65537):
        with pytest.raises(ValueError, match="rounds"):
            pkg.mutex_watershed(a, OFFSETS, rounds=r)
    with pytest.raises(TypeError, match="uint8 or bool"):
        pkg.mutex_watershed(a, OFFSETS, mask=torch.ones(20, 30))
    with pytest.raises(ValueError, match="mask must have the shape"):
        pkg.mutex_watershed(a, OFFSETS, mask=torch.ones(1, 20, 30, dtype=torch.uint8))
    with pytest.raises(ValueError, match="32 bits"):
        pkg.mutex_watershed(torch.zeros(1).expand(8, 1 << 15, 1 << 14), OFFSETS)
    with pytest.raises(TypeError, match="floats"):
        pkg.seg_mutex(np.zeros((8, 20, 30), np.int32), OFFSETS)
