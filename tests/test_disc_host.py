"""CPU: the discriminative instance loss (include/pea_disc.h) -- the header and the library agree on the six new symbols, the ctypes
mirror has the header's layout, pea_disc_validate refuses what the header lists, the two size queries are monotone 8-byte multiples,
every refusal of the forward / backward calls is reached before anything is launched and in the header's order (dummy device pointers,
no GPU), the Python entry points say what is wrong with a call before they look at the device, discriminative_loss has the reference's
signature plus num_ids, and the float64 restatement tests/disc_reference.py -- what the GPU tests compare the kernels with --
reproduces the reference's own float64 numbers on every fixture (tests/golden/make_golden_disc.py) to 1e-12."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from disc_reference import disc_reference, load_disc_golden

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
BACKGROUND, NEED_GRAD = 1, 2
NEW = ["pea_disc_context_bytes", "pea_disc_loss_bwd", "pea_disc_loss_fwd", "pea_disc_validate", "pea_disc_workspace_bytes",
       "pea_disc_workspace_init"]
GOLDENS = ("gdisc_2d_b3_37x53", "gdisc_2d_b3_37x53_bg", "gdisc_3d_b2_5x20x24", "gdisc_d5")


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- exports and layout --------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_disc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_DISC) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src and lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    for name, text, value in (("MAX_IDS", "4096", 4096), ("MAX_D", "64", 64), ("BACKGROUND", "1u", 1), ("NEED_GRAD", "2u", 2), ("STATS", "5", 5)):
        assert re.search(r"#define\s+PEA_DISC_%s\s+%s\b" % (name, text), src), name
        assert getattr(pkg._lib, "DISC_" + name) == value
    for cite in ("scripts_ac3ac4/loss/loss_discriminative.py:6-60", "scripts_cvppp/loss/loss_discriminative.py",
                 "scripts_bbbc039v1/loss/loss_discriminative.py"):
        assert cite in src, cite


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaDiscDesc
    names = ["B", "D", "S", "num_ids", "dtype", "flags", "delta_v", "delta_d", "alpha", "beta", "gamma"]
    assert [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 16, 20, 24, 28, 32, 36, 40, 44] and ctypes.sizeof(D) == 48
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_disc.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaDiscDesc \{(.*?)\} PeaDiscDesc;", src, flags=re.S).group(1)
    decl = [n for d in body.split(";") if d.strip() for n in re.sub(r"^\s*(u?int(32|64)_t|float)", "", d.strip()).replace(" ", "").split(",")]
    assert decl == names


# ---- return codes --------------------------------------------------------------------------------------------------------------------
E, LABELS, LOSS, STATS, CTX, WORK, DLOSS, DE = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000, 0x80000000


def desc(pkg, B=2, D=16, S=37 * 53, num_ids=64, dtype=F32, flags=NEED_GRAD, delta_v=0.5, delta_d=1.5, alpha=1.0, beta=1.0, gamma=0.001):
    d = pkg._lib.PeaDiscDesc()
    d.B, d.D, d.S, d.num_ids, d.dtype, d.flags = B, D, S, num_ids, dtype, flags
    d.delta_v, d.delta_d, d.alpha, d.beta, d.gamma = delta_v, delta_d, alpha, beta, gamma
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def fwd(pkg, lib, d="default", e=E, labels=LABELS, loss=LOSS, stats=STATS, ctx=CTX, work=WORK, wbytes=None, **kw):
    """pea_disc_loss_fwd on dummy pointers: anything but an early return would fault"""
    if isinstance(d, str):
        d = desc(pkg, **kw)
    if wbytes is None:
        wbytes = 0 if d is None else lib.pea_disc_workspace_bytes(ctypes.byref(d))
    return lib.pea_disc_loss_fwd(None if d is None else ctypes.byref(d), vp(e), vp(labels), vp(loss), vp(stats), vp(ctx), vp(work), wbytes, None)


def bwd(pkg, lib, d="default", e=E, labels=LABELS, ctx=CTX, dloss=DLOSS, de=DE, **kw):
    if isinstance(d, str):
        d = desc(pkg, **kw)
    return lib.pea_disc_loss_bwd(None if d is None else ctypes.byref(d), vp(e), vp(labels), vp(ctx), vp(dloss), vp(de), None)


BIG = dict(B=8, S=2 ** 31)                      # S > 2^31 - 1
EDGE = dict(B=1 << 21, S=1 << 20, num_ids=1)    # exactly 2^31 workgroups of 1024 pixels: one too many
INF, NAN = float("inf"), float("nan")


def test_descriptor_refusals(pkg, lib):
    v = lambda **kw: lib.pea_disc_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_disc_validate(None) == E_NULL and fwd(pkg, lib, d=None) == E_NULL and bwd(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(dtype=F16, flags=0) == OK and v(dtype=BF16, flags=BACKGROUND | NEED_GRAD) == OK
    assert v(B=1, D=1, S=1, num_ids=1) == OK and v(D=64, num_ids=4096) == OK and v(delta_v=0.0, delta_d=0.0) == OK
    assert v(alpha=-1.0, beta=0.0, gamma=-0.5) == OK  # the weights are the caller's business
    bad = [dict(B=0), dict(B=-1), dict(D=0), dict(D=-4), dict(S=0), dict(S=-1),
           dict(num_ids=0), dict(num_ids=-1), dict(num_ids=4097),
           dict(dtype=3), dict(dtype=-1),
           dict(flags=4), dict(flags=1 | 8), dict(flags=1 << 31),
           dict(delta_v=-0.5), dict(delta_v=INF), dict(delta_v=NAN), dict(delta_d=-1.0), dict(delta_d=INF), dict(delta_d=NAN)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert fwd(pkg, lib, **kw) == E_DESC and bwd(pkg, lib, **kw) == E_DESC, kw
        assert lib.pea_disc_workspace_bytes(ctypes.byref(desc(pkg, **kw))) == 0 and lib.pea_disc_context_bytes(ctypes.byref(desc(pkg, **kw))) == 0
    for D in (65, 128, 2 ** 31 - 1):
        assert v(D=D) == E_UNSUPPORTED and fwd(pkg, lib, D=D) == E_UNSUPPORTED and bwd(pkg, lib, D=D) == E_UNSUPPORTED
    assert v(D=65, num_ids=0) == E_DESC  # PEA_E_UNSUPPORTED is checked last


def test_sizes_are_monotone_multiples_of_eight(pkg, lib):
    ws = lambda **kw: lib.pea_disc_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    cx = lambda **kw: lib.pea_disc_context_bytes(ctypes.byref(desc(pkg, **kw)))
    for f in (ws, cx):
        for axis, values in (("B", (1, 2, 3, 8, 33)), ("num_ids", (1, 2, 3, 64, 65, 4095, 4096)), ("D", (1, 2, 5, 16, 17, 64))):
            sizes = [f(**{axis: x}) for x in values]
            assert all(s > 0 and s % 8 == 0 for s in sizes), (axis, sizes)
            assert all(a < b for a, b in zip(sizes, sizes[1:])), (axis, sizes)
        assert f(S=1) == f(S=1 << 30) and f(dtype=F16) == f() and f(flags=0) == f(flags=3)  # pixels, dtype and flags play no part
    # a row of 2 + 3 D words per (image, id), an accumulator per image and a header
    assert ws(B=2, num_ids=64, D=16) == 8 * (8 + 4 * 2 + 2 * 64 * 50)
    # mu and G / n per (image, id, channel), four words per (image, id), C_b, dist_b and reg_b per image
    assert cx(B=2, num_ids=64, D=16) == 16 * 2 + 8 + 4 * 4 * 128 + 2 * 4 * 128 * 16
    assert lib.pea_disc_workspace_bytes(None) == 0 and lib.pea_disc_context_bytes(None) == 0


def test_exact_sizes(pkg, lib):
    ws = lambda **kw: lib.pea_disc_workspace_bytes(ctypes.byref(desc(pkg, **kw)))
    cx = lambda **kw: lib.pea_disc_context_bytes(ctypes.byref(desc(pkg, **kw)))
    al8 = lambda x: (x + 7) // 8 * 8
    # odd B, B * num_ids and B * num_ids * D among them: every int32 / f32 array of the context is padded to 8 bytes on its own
    cases = ((1, 1, 1), (1, 3, 5), (3, 1, 1), (3, 5, 7), (2, 64, 16), (5, 4095, 63), (33, 4096, 64), (7, 77, 1))
    for B, N, D in cases:
        # the tables: a header of 8 words, 4 words per image, a row of 2 + 3 D words per (image, id)
        assert ws(B=B, num_ids=N, D=D) == 8 * (8 + 4 * B + B * N * (2 + 3 * D)), (B, N, D)
        # the context: dist_b and reg_b (f64) per image, C_b; n_c, the id list, k_c and w_c per (image, id); mu_c and G_c / n_c per channel
        assert cx(B=B, num_ids=N, D=D) == 16 * B + al8(4 * B) + 4 * al8(4 * B * N) + 2 * al8(4 * B * N * D), (B, N, D)
    # The largest descriptor that pea_disc_validate admits is B = 2^31 - 1, num_ids = 4096, D = 64: 8 * B * num_ids * 194 < 2^54 and
    # 8 * B * num_ids * D = 2^52 bytes, so neither count can exceed 2^64 and neither query ever answers SIZE_MAX: the exact values
    B, N, D = 2 ** 31 - 1, 4096, 64
    assert ws(B=B, num_ids=N, D=D) == 8 * (8 + 4 * B + B * N * (2 + 3 * D)) < 2 ** 64 - 1
    assert cx(B=B, num_ids=N, D=D) == 16 * B + al8(4 * B) + 4 * al8(4 * B * N) + 2 * al8(4 * B * N * D) < 2 ** 64 - 1


def test_workspace_init_refusals(pkg, lib):
    f = lambda p, n: lib.pea_disc_workspace_init(vp(p), n, None)
    assert f(0, 4096) == E_NULL and f(WORK + 4, 4096) == E_ALIGN and f(WORK + 1, 4096) == E_ALIGN
    assert f(WORK, 0) == E_WORKSPACE and f(WORK, 56) == E_WORKSPACE and f(WORK, 4097) == E_WORKSPACE
    assert f(0, 0) == E_NULL and f(WORK + 4, 0) == E_ALIGN  # the order


def test_forward_refusals_before_a_launch(pkg, lib):
    for ptr in ("e", "labels", "loss", "stats", "ctx"):
        assert fwd(pkg, lib, **{ptr: 0}) == E_NULL, ptr
        assert fwd(pkg, lib, flags=0, **{ptr: 0}) == E_NULL, ptr  # ctx is needed without PEA_DISC_NEED_GRAD too
    for skew in (1, 2, 3):
        assert fwd(pkg, lib, e=E + skew) == E_ALIGN and fwd(pkg, lib, labels=LABELS + skew) == E_ALIGN and fwd(pkg, lib, loss=LOSS + skew) == E_ALIGN
    for dt in (F16, BF16):
        assert fwd(pkg, lib, e=E + 1, dtype=dt) == E_ALIGN and fwd(pkg, lib, e=E + 2, dtype=dt, work=0) == E_WORKSPACE
    for ptr, base in (("stats", STATS), ("ctx", CTX), ("work", WORK)):
        assert fwd(pkg, lib, **{ptr: base + 4}) == E_ALIGN and fwd(pkg, lib, **{ptr: base + 1}) == E_ALIGN, ptr
    need = lib.pea_disc_workspace_bytes(ctypes.byref(desc(pkg)))
    assert fwd(pkg, lib, work=0) == E_WORKSPACE and fwd(pkg, lib, wbytes=need - 8) == E_WORKSPACE and fwd(pkg, lib, wbytes=0) == E_WORKSPACE
    assert fwd(pkg, lib, **BIG) == E_UNSUPPORTED and fwd(pkg, lib, **EDGE) == E_UNSUPPORTED
    assert fwd(pkg, lib, B=1, S=2 ** 31 - 1, num_ids=1, work=0) == E_WORKSPACE  # the largest S passes the grid check's predecessors
    # the stated order: descriptor, NULL, alignment, workspace, grid
    assert fwd(pkg, lib, work=0, **BIG) == E_WORKSPACE
    assert fwd(pkg, lib, work=0, stats=STATS + 4, **BIG) == E_ALIGN and fwd(pkg, lib, wbytes=0, work=WORK + 4, **BIG) == E_ALIGN
    assert fwd(pkg, lib, e=E + 2, labels=0, work=0, **BIG) == E_NULL
    assert fwd(pkg, lib, e=0, labels=0, loss=0, stats=0, ctx=0, work=0, flags=4) == E_DESC
    assert fwd(pkg, lib, e=0, D=65) == E_UNSUPPORTED


def test_backward_refusals_before_a_launch(pkg, lib):
    for ptr in ("e", "labels", "ctx", "de"):
        assert bwd(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    for skew in (1, 2, 3):
        for ptr, base in (("e", E), ("labels", LABELS), ("dloss", DLOSS), ("de", DE)):
            assert bwd(pkg, lib, **{ptr: base + skew}) == E_ALIGN, (ptr, skew)
    for dt in (F16, BF16):
        assert bwd(pkg, lib, de=DE + 1, dtype=dt) == E_ALIGN and bwd(pkg, lib, e=E + 1, dtype=dt) == E_ALIGN
        assert bwd(pkg, lib, e=E + 2, de=DE + 6, dtype=dt, **BIG) == E_UNSUPPORTED  # element-aligned: accepted
    assert bwd(pkg, lib, ctx=CTX + 4) == E_ALIGN
    assert bwd(pkg, lib, **BIG) == E_UNSUPPORTED and bwd(pkg, lib, **EDGE) == E_UNSUPPORTED
    assert bwd(pkg, lib, dloss=0, **BIG) == E_UNSUPPORTED  # a missing dloss (= 1) is accepted
    assert bwd(pkg, lib, ctx=CTX + 4, **BIG) == E_ALIGN and bwd(pkg, lib, e=E + 2, de=0, **BIG) == E_NULL
    assert bwd(pkg, lib, e=0, de=0, dtype=7) == E_DESC


# ---- the Python entry points -----------------------------------------------------------------------------------------------------------
def test_python_entry_points_say_what_is_wrong_without_a_gpu(pkg):
    for name in ("discriminative_loss", "discriminative_loss_stats", "DiscriminativeLoss"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    from importlib import import_module
    assert import_module(pkg.__name__ + ".loss.loss_discriminative").discriminative_loss is pkg.discriminative_loss
    e, seg = torch.zeros(2, 16, 6, 6), torch.zeros(2, 6, 6, dtype=torch.int64)
    for call in (lambda: pkg.discriminative_loss(e, seg), lambda: pkg.discriminative_loss(e, seg[:, None], background=True, num_ids=8),
                 lambda: pkg.discriminative_loss_stats(e.half(), seg.to(torch.uint8)), lambda: pkg.discriminative_loss(e[:, :, 0], seg[:, 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="seg_gt has shape"):
        pkg.discriminative_loss(e, seg[:, :5])
    with pytest.raises(ValueError, match="seg_gt has shape"):
        pkg.discriminative_loss(e, seg[:1])
    with pytest.raises(ValueError, match=r"\[B, D, \*spatial\]"):
        pkg.discriminative_loss(e[:, :, 0, 0], seg[:, 0, 0])
    for dt in (torch.float32, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="integer ids"):
            pkg.discriminative_loss(e, seg.to(dt))
    with pytest.raises(ValueError, match="more than 64 channels"):
        pkg.discriminative_loss(torch.zeros(1, 65, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int32))
    for n in (0, -1, 4097):
        with pytest.raises(ValueError, match=r"num_ids must be in 1 \.\. 4096"):
            pkg.discriminative_loss(e, seg, num_ids=n)
    with pytest.raises(ValueError, match="empty"):
        pkg.discriminative_loss(torch.zeros(2, 16, 0, 6), torch.zeros(2, 0, 6, dtype=torch.int64))
    with pytest.raises(TypeError):
        pkg.discriminative_loss(e.double(), seg)
    with pytest.raises(TypeError):
        pkg.discriminative_loss(e.numpy(), seg)


def test_discriminative_loss_has_the_reference_signature_plus_num_ids(pkg):
    g = load_disc_golden("gdisc_d5")
    ref = [str(n) for n in g["params"]]
    assert ref == ["embedding", "seg_gt", "background", "delta_v", "delta_d", "alpha", "beta", "gama"]
    for f in (pkg.discriminative_loss, pkg.discriminative_loss_stats):
        sig = inspect.signature(f)
        assert list(sig.parameters) == ref + ["num_ids"]
        assert [float(sig.parameters[k].default) for k in ref[3:]] == [float(v) for v in g["defaults"]] == [0.5, 1.5, 1.0, 1.0, 0.001]
        assert sig.parameters["background"].default is False and sig.parameters["num_ids"].default is None


def test_train_step_takes_the_discriminative_term(pkg):
    sig = inspect.signature(pkg.CvpppTrainStep.__init__)
    assert sig.parameters["disc_weight"].default is None and sig.parameters["disc_num_ids"].default is None
    assert sig.parameters["disc_background"].default is False
    model = torch.nn.Conv2d(1, 1, 1)
    st = pkg.CvpppTrainStep(model)
    assert st.disc_weight is None and st.disc_num_ids is None and st.disc_background is False and st.mask_weight is None
    st = pkg.CvpppTrainStep(model, disc_weight=0.1, disc_num_ids=64, disc_background=True)
    assert st.disc_weight == 0.1 and st.disc_num_ids == 64 and st.disc_background is True


# ---- the restatement against the reference's numbers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_goldens(name):
    """loss to 1e-12 relative and the gradient to 1e-12 of its largest magnitude against the reference run in float64; the reference's
    own float32 numbers within float32's reach"""
    g = load_disc_golden(name)
    e, labels, bg = g["e"], g["labels"], g["background"]
    assert e.dtype == np.float32 and labels.dtype == np.int32 and g["de"].dtype == np.float32 and g["de64"].dtype == np.float64
    assert np.array_equal(e.astype(np.float16).astype(np.float32), e) and g["de"].shape == e.shape == g["de64"].shape
    loss, stats, de = disc_reference(e, labels, background=bg)
    ref = float(g["loss64"])
    top = np.abs(g["de64"]).max()
    print(name, "loss", loss, "float64 reference", ref, "float32 reference", float(g["loss"]), "C_b", stats[8::4])
    assert abs(loss - ref) <= 1e-12 * abs(ref) and stats[0] == loss and stats[4] == 0
    assert np.abs(de - g["de64"]).max() <= 1e-12 * top
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(ref) and np.abs(de - g["de"]).max() <= 1e-4 * top
    B = e.shape[0]
    for b in range(B):
        ids = set(np.unique(labels[b]).tolist()) - (set() if bg else {0})
        assert stats[5 + 4 * b + 3] == len(ids)
    assert math.isclose(stats[0], stats[1] + stats[2] + 0.001 * stats[3], rel_tol=1e-15)
    if not bg:
        assert not de[np.broadcast_to((labels == 0)[:, None], e.shape)].any()  # label 0 is not counted: exactly 0
    # what each fixture is there for
    if name.startswith("gdisc_2d"):
        assert e.shape == (3, 16, 37, 53) and (labels[2] == 0).all() and stats[5 + 8 + 3] == (1 if bg else 0)
        assert (labels[0] == 12).sum() == 1 and (labels[0] == 13).sum() == 1
        assert np.array_equal(e[0][:, labels[0] == 12], e[0][:, labels[0] == 13])
        if not bg:
            assert stats[5 + 8] == 0 and stats[5 + 9] == 0 and stats[5 + 10] == 0 and not de[2].any()
    if name == "gdisc_3d_b2_5x20x24":
        assert e.shape == (2, 16, 5, 20, 24) and bg and (labels == 0).any()
    if name == "gdisc_d5":
        assert e.shape[:2] == (1, 5) and stats[8] == 1 and stats[6] == 0.0 and stats[5] > 0
    # dloss scales the gradient and nothing else; num_ids that covers the ids changes nothing
    loss2, stats2, de2 = disc_reference(e, labels, background=bg, dloss=-2.5, num_ids=int(labels.max()) + 1)
    assert loss2 == loss and np.array_equal(stats2, stats) and np.abs(de2 + 2.5 * de).max() <= 1e-12 * 2.5 * top


def test_restatement_counts_labels_outside_the_table():
    g = load_disc_golden("gdisc_d5")
    labels = g["labels"].copy()
    labels[0, 0, :3] = (-1, 7, 9)
    labels[0, 20, 18] = 8
    loss, stats, de = disc_reference(g["e"], labels, num_ids=8)
    assert np.isnan(loss) and np.isnan(stats[:4]).all() and stats[4] == 3 and stats[8] == 1 and np.isfinite(stats[5:]).all()
    assert not de[0, :, 0, 0].any() and not de[0, :, 0, 2].any() and not de[0, :, 20, 18].any() and de[0, :, 0, 1].any()
