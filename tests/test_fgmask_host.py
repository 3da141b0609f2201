"""CPU: the foreground-mask loss and the validation mask (include/pea_fgmask.h) -- the header and the library agree on the five new
symbols and every older header keeps its own, the ctypes mirror has the header's layout, every refusal of the three calls is reached
before anything is launched and in the header's order (dummy device pointers, no GPU), the workspace is a whole number of loss
states, the Python entry points refuse CPU tensors, bad dtypes and C != 2, BCE_loss_func has the reference's signature, and the
float64 restatement tests/fgmask_reference.py -- what the GPU tests compare the kernels with -- reproduces the reference's own
numbers on every fixture (tests/golden/make_golden_fgmask.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from fgmask_reference import fgmask_reference, mask_reference

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
I32, U8 = 0, 1
NEW = ["pea_fgmask_argmax", "pea_fgmask_loss_bwd", "pea_fgmask_loss_fwd", "pea_fgmask_validate", "pea_fgmask_workspace_bytes"]
# the symbol counts of the older headers, as they were before pea_fgmask.h
OLDER = {"pea.h": ("EXPORTS", 33), "pea_infer.h": ("EXPORTS_INFER", 2), "pea_multi.h": ("EXPORTS_MULTI", 3), "pea_flip.h": ("EXPORTS_FLIP", 1),
         "pea_multi_labels.h": ("EXPORTS_MULTI_LABELS", 3), "pea_head16.h": ("EXPORTS_HEAD16", 3), "pea_metrics.h": ("EXPORTS_METRICS", 3)}
LOSS_GOLDENS = ("gfg_b2_37x53", "gfg_b3_64x80", "gfg_allbg")


def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_five_entry_points(pkg):
    assert declared_symbols("pea_fgmask.h") == sorted(pkg._lib.EXPORTS_FGMASK) == NEW
    src = open(os.path.join(ROOT, "include", "pea_fgmask.h")).read()
    assert '#include "pea.h"' in src
    for name, text, value in (("LABELS_I32", "0", 0), ("LABELS_U8", "1", 1), ("SKIP_EMPTY_CLASS", "1u", 1), ("STATS", "5", 5)):
        assert re.search(r"#define\s+PEA_FG_%s\s+%s\b" % (name, text), src), name
        assert getattr(pkg._lib, "FG_" + name) == value
    # the header cites the reference lines it replaces, and says where the mask differs from argmax(softmax)
    for cite in ("scripts_bbbc039v1/main.py:289", "scripts_bbbc039v1/loss/loss.py:187-194", "scripts_bbbc039v1/main.py:406-410", "equal probabilities"):
        assert cite in src, cite


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaFgDesc
    assert ctypes.sizeof(D) == 10 * 4  # ten 4-byte fields, no padding
    assert [f[0] for f in D._fields_] == ["B", "Y", "X", "logits_dtype", "labels_type", "flags", "origin", "out_dims"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_fgmask.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaFgDesc \{(.*?)\} PeaFgDesc;", src, flags=re.S).group(1)
    names = [n.split("[")[0] for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*u?int32_t", "", decl.strip()).replace(" ", "").split(",")]
    assert names == [f[0] for f in D._fields_]
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 32]


def test_library_exports_them_and_the_older_headers_are_unchanged(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    older = set()
    for header, (tup, count) in OLDER.items():
        names = getattr(pkg._lib, tup)
        assert declared_symbols(header) == sorted(names) and len(names) == count, header
        older |= set(names)
    assert not set(NEW) & older
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    src = open(os.path.join(ROOT, "include", "pea.h")).read()
    assert re.search(r"#define\s+PEA_ABI_VERSION\s+2\b", src)


# ---- return codes ------------------------------------------------------------------------------------------------------------------
LOGITS, LABELS, LOSS, STATS, WORK, DLOSS, DLOGITS, OUT = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000,
                                                          0x80000000)


def desc(pkg, B=2, Y=37, X=53, dtype=F32, ltype=I32, flags=0, origin=(0, 0), out_dims=(0, 0)):
    d = pkg._lib.PeaFgDesc()
    d.B, d.Y, d.X, d.logits_dtype, d.labels_type, d.flags = B, Y, X, dtype, ltype, flags
    d.origin[:], d.out_dims[:] = origin, out_dims
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def fwd(pkg, lib, d="default", logits=LOGITS, labels=LABELS, loss=LOSS, stats=STATS, work=WORK, wbytes=None, **kw):
    """pea_fgmask_loss_fwd on dummy pointers: anything but an early return would fault"""
    if isinstance(d, str):
        d = desc(pkg, **kw)
    wbytes = lib.pea_fgmask_workspace_bytes() if wbytes is None else wbytes
    return lib.pea_fgmask_loss_fwd(None if d is None else ctypes.byref(d), vp(logits), vp(labels), vp(loss), vp(stats), vp(work), wbytes, None)


def bwd(pkg, lib, d="default", logits=LOGITS, labels=LABELS, stats=STATS, dloss=DLOSS, dlogits=DLOGITS, **kw):
    if isinstance(d, str):
        d = desc(pkg, **kw)
    return lib.pea_fgmask_loss_bwd(None if d is None else ctypes.byref(d), vp(logits), vp(labels), vp(stats), vp(dloss), vp(dlogits), None)


def amax(pkg, lib, d="default", logits=LOGITS, out=OUT, **kw):
    if isinstance(d, str):
        kw.setdefault("out_dims", (16, 16))
        d = desc(pkg, **kw)
    return lib.pea_fgmask_argmax(None if d is None else ctypes.byref(d), vp(logits), vp(out), None)


BIG = dict(B=2 ** 31 - 1, Y=2 ** 31 - 1, X=2 ** 31 - 1)   # far more than 2^31 - 1 workgroups
EDGE = dict(B=1 << 19, Y=1 << 12, X=1 << 12)              # exactly 2^31 workgroups of 4096 pixels: one too many


def test_descriptor_refusals(pkg, lib):
    v = lambda **kw: lib.pea_fgmask_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_fgmask_validate(None) == E_NULL
    assert fwd(pkg, lib, d=None) == E_NULL and bwd(pkg, lib, d=None) == E_NULL and amax(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(dtype=F16, ltype=U8, flags=1) == OK and v(dtype=BF16) == OK and v(B=1, Y=1, X=1) == OK
    assert v(Y=200, X=24, origin=(92, 4), out_dims=(16, 16)) == OK and v(origin=(37, 53)) == OK and v(out_dims=(37, 53)) == OK
    bad = [dict(B=0), dict(B=-1), dict(Y=0), dict(X=0), dict(X=-3),
           dict(dtype=3), dict(dtype=-1), dict(ltype=2), dict(ltype=-1),
           dict(flags=2), dict(flags=1 | 4), dict(flags=1 << 31),                        # unknown flag bits
           dict(origin=(-1, 0)), dict(origin=(0, -1)), dict(out_dims=(-1, 4)), dict(out_dims=(4, -1)),
           dict(origin=(30, 0), out_dims=(8, 8)), dict(origin=(0, 50), out_dims=(8, 4)), dict(out_dims=(38, 1)),   # the crop leaves (Y, X)
           dict(origin=(2 ** 31 - 1, 0), out_dims=(1, 1))]                               # (no overflow in origin + out_dims)
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert fwd(pkg, lib, **kw) == E_DESC and bwd(pkg, lib, **kw) == E_DESC and amax(pkg, lib, **dict(dict(out_dims=(1, 1)), **kw)) == E_DESC, kw
    # the mask needs a crop of at least one pixel; the loss calls do not look at it
    assert amax(pkg, lib, out_dims=(0, 0)) == E_DESC and amax(pkg, lib, out_dims=(16, 0)) == E_DESC and amax(pkg, lib, out_dims=(0, 16)) == E_DESC


def test_forward_refusals_before_a_launch(pkg, lib):
    for ptr in ("logits", "labels", "loss", "stats"):
        assert fwd(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    # PEA_E_ALIGN: the logits' element (4 or 2 bytes), 4 for int32 labels and loss, 8 for stats and the workspace
    for skew in (1, 2, 3):
        assert fwd(pkg, lib, logits=LOGITS + skew) == E_ALIGN and fwd(pkg, lib, labels=LABELS + skew) == E_ALIGN, skew
        assert fwd(pkg, lib, loss=LOSS + skew) == E_ALIGN, skew
        assert fwd(pkg, lib, labels=LABELS + skew, ltype=U8, work=0) == E_WORKSPACE, skew   # (u8 labels: any address passes)
    for dt in (F16, BF16):
        assert fwd(pkg, lib, logits=LOGITS + 1, dtype=dt) == E_ALIGN and fwd(pkg, lib, logits=LOGITS + 2, dtype=dt, work=0) == E_WORKSPACE
    assert fwd(pkg, lib, stats=STATS + 4) == E_ALIGN and fwd(pkg, lib, work=WORK + 4) == E_ALIGN and fwd(pkg, lib, stats=STATS + 1) == E_ALIGN
    # PEA_E_WORKSPACE: missing or short
    need = lib.pea_fgmask_workspace_bytes()
    assert fwd(pkg, lib, work=0) == E_WORKSPACE and fwd(pkg, lib, wbytes=need - 1) == E_WORKSPACE and fwd(pkg, lib, wbytes=0) == E_WORKSPACE
    # PEA_E_UNSUPPORTED: more than 2^31 - 1 workgroups of 4096 pixels
    assert fwd(pkg, lib, **BIG) == E_UNSUPPORTED and fwd(pkg, lib, **EDGE) == E_UNSUPPORTED
    # the stated order: descriptor, NULL, alignment, workspace, grid
    assert fwd(pkg, lib, work=0, **BIG) == E_WORKSPACE
    assert fwd(pkg, lib, work=0, stats=STATS + 4, **BIG) == E_ALIGN and fwd(pkg, lib, wbytes=0, work=WORK + 4, **BIG) == E_ALIGN
    assert fwd(pkg, lib, logits=LOGITS + 2, labels=0, work=0, **BIG) == E_NULL
    assert fwd(pkg, lib, logits=0, labels=0, loss=0, stats=0, work=0, flags=2) == E_DESC


def test_backward_refusals_before_a_launch(pkg, lib):
    for ptr in ("logits", "labels", "stats", "dlogits"):
        assert bwd(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    for skew in (1, 2, 3):
        for ptr, base in (("logits", LOGITS), ("labels", LABELS), ("dloss", DLOSS), ("dlogits", DLOGITS)):
            assert bwd(pkg, lib, **{ptr: base + skew}) == E_ALIGN, (ptr, skew)
    for dt in (F16, BF16):
        assert bwd(pkg, lib, dlogits=DLOGITS + 1, dtype=dt) == E_ALIGN and bwd(pkg, lib, logits=LOGITS + 1, dtype=dt) == E_ALIGN
        assert bwd(pkg, lib, logits=LOGITS + 2, dlogits=DLOGITS + 6, dtype=dt, **BIG) == E_UNSUPPORTED  # element-aligned: accepted
    assert bwd(pkg, lib, stats=STATS + 4) == E_ALIGN
    assert bwd(pkg, lib, **BIG) == E_UNSUPPORTED and bwd(pkg, lib, **EDGE) == E_UNSUPPORTED
    # u8 labels at any address and a missing dloss (= 1) are accepted: the call gets as far as the grid
    assert bwd(pkg, lib, labels=LABELS + 3, ltype=U8, dloss=0, **BIG) == E_UNSUPPORTED
    # the order
    assert bwd(pkg, lib, stats=STATS + 4, **BIG) == E_ALIGN and bwd(pkg, lib, logits=LOGITS + 2, dlogits=0, **BIG) == E_NULL
    assert bwd(pkg, lib, logits=0, dlogits=0, dtype=7) == E_DESC


def test_argmax_refusals_before_a_launch(pkg, lib):
    assert amax(pkg, lib, logits=0) == E_NULL and amax(pkg, lib, out=0) == E_NULL
    assert amax(pkg, lib, logits=LOGITS + 2) == E_ALIGN and amax(pkg, lib, logits=LOGITS + 1, dtype=F16) == E_ALIGN
    big = dict(B=2 ** 31 - 1, Y=2 ** 31 - 1, X=2 ** 31 - 1, out_dims=(2 ** 31 - 1, 2 ** 31 - 1))
    assert amax(pkg, lib, **big) == E_UNSUPPORTED
    assert amax(pkg, lib, B=1 << 11, Y=1 << 15, X=1 << 15, out_dims=(1 << 15, 1 << 15)) == E_UNSUPPORTED   # 2^31 workgroups of 1024 pixels
    assert amax(pkg, lib, out=OUT + 1, logits=LOGITS + 2, dtype=BF16, **big) == E_UNSUPPORTED               # (any address for the u8 output)
    assert amax(pkg, lib, logits=LOGITS + 2, out=0, **big) == E_NULL and amax(pkg, lib, logits=0, out=0, out_dims=(0, 0)) == E_DESC


def test_workspace_is_a_whole_number_of_loss_states(pkg, lib):
    AffinitySpec, make_desc = pkg.AffinitySpec, pkg.affinity_op.make_desc
    spec = AffinitySpec(2, [(0, 1)], None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_FULL, 1e-12)
    one = lib.pea_workspace_bytes(ctypes.byref(make_desc(spec, torch.empty((1, 16, 8, 8), device="meta"))))
    nb = lib.pea_fgmask_workspace_bytes()
    assert one > 0 and nb >= one and nb % one == 0 and nb % 8 == 0


# ---- the Python entry points -------------------------------------------------------------------------------------------------------
def test_python_entry_points_are_device_calls(pkg):
    """no CPU fallback; a wrong shape or dtype is said before the device is looked at"""
    for name in ("BCE_loss_func", "foreground_mask_loss", "foreground_mask"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    from importlib import import_module
    assert import_module(pkg.__name__ + ".loss.loss").BCE_loss_func is pkg.BCE_loss_func
    logits, target = torch.zeros(2, 2, 6, 6), torch.zeros(2, 6, 6, dtype=torch.bool)
    for call in (lambda: pkg.BCE_loss_func(logits, target), lambda: pkg.BCE_loss_func(logits, target[:, None], weight_rate=[10, 1]),
                 lambda: pkg.foreground_mask_loss(logits, target.to(torch.int32), skip_empty=True), lambda: pkg.foreground_mask(logits),
                 lambda: pkg.foreground_mask(logits.half(), crop=((1, 1), (2, 2)))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # C != 2
    for bad in (torch.zeros(2, 3, 6, 6), torch.zeros(2, 1, 6, 6), torch.zeros(2, 6, 6)):
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            pkg.BCE_loss_func(bad, target)
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            pkg.foreground_mask(bad)
    # the target's dtype: bool, uint8 and int32 only, and the message names the fix
    for dt in (torch.int64, torch.float32, torch.int16):
        with pytest.raises(ValueError, match=r"torch\.gt\(.*, 0\).*torch\.int32"):
            pkg.BCE_loss_func(logits, target.to(dt))
        with pytest.raises(ValueError, match="bool, uint8 or int32"):
            pkg.foreground_mask_loss(logits, target.to(dt))
    with pytest.raises(ValueError):
        pkg.BCE_loss_func(logits, torch.zeros(2, 6, 5, dtype=torch.bool))
    with pytest.raises(TypeError):
        pkg.BCE_loss_func(logits.double(), target)
    with pytest.raises(TypeError):
        pkg.foreground_mask(logits.to(torch.int32))


def test_bce_loss_func_has_the_reference_signature(pkg):
    g = load_golden("gfg_b2_37x53")
    sig = inspect.signature(pkg.BCE_loss_func)
    assert list(sig.parameters) == [str(n) for n in g["params"]] == ["output", "target", "weight_rate"]
    assert sig.parameters["weight_rate"].default == [1, 1]


def test_train_step_constructs_as_before(pkg):
    sig = inspect.signature(pkg.CvpppTrainStep.__init__)
    assert sig.parameters["mask_weight"].default is None and sig.parameters["mask_skip_empty"].default is False
    assert list(sig.parameters)[-2:] == ["mask_weight", "mask_skip_empty"]  # (appended: positional callers are not disturbed)
    model = torch.nn.Conv2d(1, 1, 1)
    st = pkg.CvpppTrainStep(model)
    assert st.mask_weight is None and st.mask_skip_empty is False and st.model is model and st.ct_weight == 0.0
    st = pkg.CvpppTrainStep(model, mask_weight=1000, mask_skip_empty=True)
    assert st.mask_weight == 1000.0 and st.mask_skip_empty is True


# ---- the restatement against the reference's numbers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LOSS_GOLDENS)
def test_restatement_reproduces_the_loss_goldens(name):
    """loss to 1e-12 relative against nn.CrossEntropyLoss in float64 (NaN for NaN); the gradient to 1e-12 of its largest magnitude;
    the reference's own float32 numbers within float32's reach"""
    g = load_golden(name)
    assert g["logits"].dtype == np.float32 and g["labels"].dtype == np.int32 and g["logits"].shape[1] == 2
    loss, stats, dl = fgmask_reference(g["logits"], g["labels"])
    n1 = int((g["labels"] > 0).sum())
    assert stats[3] == g["labels"].size - n1 and stats[4] == n1
    if name == "gfg_allbg":
        assert n1 == 0 and np.isnan(g["loss64"]) and np.isnan(g["loss"]) and np.isnan(g["dlogits64"]).all() and np.isnan(g["dlogits"]).all()
        assert np.isnan(loss) and np.isnan(dl).all() and np.isnan(stats[0]) and np.isnan(stats[2]) and np.isfinite(stats[1])
        loss, stats, dl = fgmask_reference(g["logits"], g["labels"], skip_empty=True)
        assert np.isfinite(loss) and loss == 0.5 * stats[1] and stats[2] == 0.0 and np.isfinite(dl).all() and np.abs(dl).max() > 0
        return
    assert (g["labels"] < 0).any() and (g["labels"] > 2 ** 30).any() and 0 < n1 < g["labels"].size
    ref = float(g["loss64"])
    print(name, "loss", loss, "float64 CE", ref, "float32 reference", float(g["loss"]))
    assert abs(loss - ref) <= 1e-12 * abs(ref)
    top = np.abs(g["dlogits64"]).max()
    assert np.abs(dl - g["dlogits64"]).max() <= 1e-12 * top
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(ref) and np.abs(dl - g["dlogits"]).max() <= 1e-4 * top
    # dloss scales the gradient and nothing else
    loss2, _, dl2 = fgmask_reference(g["logits"], g["labels"], dloss=1000.0)
    assert loss2 == loss and np.abs(dl2 - 1000.0 * dl).max() <= 1e-12 * 1000.0 * top


def test_restatement_reproduces_the_mask_golden():
    g = load_golden("gfg_valid_200x24")
    crop = tuple(tuple(int(v) for v in r) for r in g["crop"])
    assert crop == ((92, 92), (4, 4)) and g["logits"].shape == (1, 2, 200, 24) and g["mask"].shape == (16, 16) and g["mask"].dtype == np.uint8
    l = g["logits"][0, :, 92:-92, 4:-4]
    assert int((l[0] == l[1]).sum()) >= 3 and int(np.isnan(l).any(axis=0).sum()) >= 3  # ties and NaNs inside the crop
    assert np.array_equal(mask_reference(g["logits"], crop)[0], g["mask"])
    assert np.array_equal(mask_reference(g["logits"])[0, 92:-92, 4:-4], g["mask"])
