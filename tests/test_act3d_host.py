"""CPU: the 3D losses on the activated affinity map (loss/embedding2affs_3d.py, loss/embedding2affs_3d_l2.py and the norm2 pair of
loss/loss_embedding_mse_3d.py) without a GPU.

  * the float64 restatement of tests/act3d_reference.py equals every tests/golden/ga3_*.npz fixture (the reference's own run);
  * the signatures of the new functions equal the parameter names recorded from the reference;
  * the descriptors the wrappers build carry the right flags, border, normaliser, lambda and eps, and the right border call follows;
  * the return codes of pea_affs_crop_zero that need no device (include/pea_crop.h).

Bounds.  The fixtures are float32 runs of the reference, the restatement is float64: a map value in [0, 1] agrees to a few f32 ulp
(1e-6 absolute); the loss is a mean of O(1) terms summed in f32 (1e-5 relative, the GPU suites' bound); the gradient goes through
the f32 normalisation and a sum over up to 24 terms (1e-4 of its max, the GPU suites' bound).
"""
import ctypes
import importlib
import inspect

import pytest
import torch

import __graft_entry__ as ge
import act3d_reference as ref
from conftest import golden_names, load_golden

GA3 = golden_names("ga3_")
LOSSES = [n for n in GA3 if not n.startswith("ga3_single")]
HALF, CLAMP, LOSS_ACT, LOSS_BCE = 4, 8, 64, 128
OK, E_NULL, E_DESC, E_ALIGN = 0, -1, -2, -5
BORDER_CROP_ZERO, NORM_CROPPED, NORM_FULL = 1, 1, 2


def test_the_fixture_set_is_complete():
    fns = {(str(load_golden(n)["module"]), str(load_golden(n)["fn"])) for n in LOSSES}
    assert fns == set(ref.FORMS)  # one fixture at least per function, norm4 and ema_norm2 included
    assert {"ga3_norm1_fill", "ga3_norm1_nofill", "ga3_norm1_s2", "ga3_norm5_wbce", "ga3_norm2_bce", "ga3_single", "ga3_single_cos"} <= set(GA3)
    assert str(load_golden("ga3_norm5_wbce")["criterion"]) == "WeightedBCE" and str(load_golden("ga3_norm2_bce")["criterion"]) == "BCELoss"


@pytest.mark.parametrize("name", LOSSES)
def test_restatement_equals_the_reference(name):
    g = load_golden(name)
    form = ref.form_of(g)
    assert int(g["edge_zeroed"]) <= ref.EDGE_MAX_FRACTION * int(g["terms"])
    loss, stored, grad, v = ref.restate(g["e"], g["ema"] if "ema" in g else None, g["target"], g["weight"], **form)
    # the fixture's weights already carry the edge rule: the restatement finds the same terms
    near = ref.near_edge(v, form["act"])
    assert int(near.sum()) == int(g["edge_zeroed"]) and near.numel() == int(g["terms"])
    if str(g["criterion"]) != "BCELoss":
        assert not torch.from_numpy(g["weight"])[near].any()
    print("%s: loss %.9g (ref %.9g)" % (name, loss.item(), float(g["loss"])))
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    assert float((stored - torch.from_numpy(g["affs"]).double()).abs().max()) < 1e-6
    gr = torch.from_numpy(g["grad"]).double()
    assert float((grad - gr).abs().max()) < 1e-4 * float(gr.abs().max())
    # the border of the stored map is an exact +0 wherever the pair does not exist and nothing was filled in
    if not form["fill_shift"]:
        gone = ~ref.exists(g["e"].shape[2:], form["shifts"])[None].expand(g["affs"].shape)
        assert not torch.from_numpy(g["affs"])[gone].view(torch.int32).any()


@pytest.mark.parametrize("name", ["ga3_single", "ga3_single_cos"])
def test_single_offset_restatement(name):
    g = load_golden(name)
    eps = 1e-6 if name.endswith("cos") else 1e-12
    for order in range(3):
        a = ref.single_offset64(g["e"], order, int(g["shift"]), eps)
        assert float((a - torch.from_numpy(g["affs"][:, order]).double()).abs().max()) < 1e-6


@pytest.mark.parametrize("name", GA3)
def test_signatures_are_the_reference(pkg, name):
    g = load_golden(name)
    mod = importlib.import_module(ge.PKG_NAME + ".loss." + str(g["module"]))
    sig = inspect.signature(getattr(mod, str(g["fn"]))).parameters
    assert list(sig) == [str(p) for p in g["params"]]
    if "defaults" in g:
        want = [str(d) for d in g["defaults"]]
        have = [repr(p.default) for p in sig.values() if p.default is not inspect.Parameter.empty]
        assert have == want


def test_modules_are_exported(pkg):
    assert pkg.embedding2affs_3d.embedding_loss_norm5 and pkg.embedding2affs_3d_l2.embedding_loss_l25
    assert pkg.embedding_loss_norm2 and pkg.ema_embedding_loss_norm2 and pkg.affs_crop_zero_


# ---- the descriptors the wrappers build ------------------------------------------------------------------------------------------

class _Recorder(object):
    """stands in for FusedAffinityMSE and the two border calls inside loss/_activated3d.py: records, computes nothing"""

    def __init__(self):
        self.specs, self.border = [], []

    def apply(self, e, ema, target, weight, mask, spec):
        self.specs.append((spec, ema is not None, weight, mask))
        return torch.zeros(()), torch.zeros(target.shape), None

    def crop(self, affs, offsets):
        self.border.append(("crop", [tuple(o) for o in offsets]))
        return affs

    def fill(self, affs, shift=1, relu=True):
        self.border.append(("fill", shift, relu))
        return affs


@pytest.fixture
def recorder(pkg, monkeypatch):
    a3 = importlib.import_module(ge.PKG_NAME + ".loss._activated3d")
    r = _Recorder()
    monkeypatch.setattr(a3, "FusedAffinityMSE", r)
    monkeypatch.setattr(a3, "affs_crop_zero_", r.crop)
    monkeypatch.setattr(a3, "fill_border_relu_", r.fill)
    return r


def _inputs(K, B=1, Z=6, Y=30, X=32):
    return torch.zeros(B, 16, Z, Y, X), torch.zeros(B, K, Z, Y, X), torch.full((B, K, Z, Y, X), 2.0)


def _offsets(shifts):
    return [tuple(-s if a == i % 3 else 0 for a in range(3)) for i, s in enumerate(shifts)]


CRITS = {"WeightedMSE": 0, "MSELoss": 0, "BCELoss": LOSS_BCE, "WeightedBCE": LOSS_BCE}


# every fused (form, criterion): norm4 runs composed, and binary cross-entropy needs the clamp (the L2 forms call it on the map)
FUSED = [(k, c) for k in sorted(ref.FORMS) for c in sorted(CRITS) if ref.FORMS[k][2] != "norm4" and (ref.FORMS[k][1] & CLAMP or not CRITS[c])]


@pytest.mark.parametrize("key,crit", FUSED, ids=["-".join(k + (c,)) for k, c in FUSED])
def test_descriptor_of_every_form(pkg, recorder, key, crit):
    table, act, mode, first, fills, eps = ref.FORMS[key]
    shifts = list(table) if table is not None else [2] * 3
    K = len(shifts)
    e, t, w = _inputs(K)
    fn = getattr(importlib.import_module(ge.PKG_NAME + ".loss." + key[0]), key[1])
    args = (e, e.clone(), t, w) if key[1].startswith("ema_") else (e, t, w)
    out = fn(*args, getattr(pkg, crit)(), affs0_weight=0.25, shift=2, fill=True)
    assert isinstance(out, tuple) and len(out) == 2
    (spec, has_other, weight, mask), = recorder.specs
    assert has_other == key[1].startswith("ema_") and mask is None
    assert spec.ndim == 3 and spec.border == BORDER_CROP_ZERO and spec.offsets == _offsets(shifts)
    assert spec.act == act | LOSS_ACT | CRITS[crit]
    assert spec.eps == eps
    if mode == "cropped":
        assert spec.norm == NORM_CROPPED and spec.lam == [0.25] * first + [1.0] * (K - first)
    else:  # one call over the whole map: WeightedMSE divides by B*Z*Y*X, torch's means by B*K*Z*Y*X
        assert spec.norm == NORM_FULL and spec.lam == [1.0 if crit == "WeightedMSE" else 1.0 / K] * K
    # the unweighted criteria read a ones weight, the weighted ones the caller's
    assert bool((weight == 2).all()) == (crit in ("WeightedMSE", "WeightedBCE")) and bool((weight == 1).all()) == (crit in ("MSELoss", "BCELoss"))
    if fills:
        assert recorder.border == [("fill", 2, False)]
    elif act & HALF:
        assert recorder.border == [("crop", _offsets(shifts))]
    else:
        assert recorder.border == []  # act(0) = 0 under the clamp alone: no launch


def test_norm1_without_fill_zeroes_the_border(pkg, recorder):
    e, t, w = _inputs(3)
    pkg.embedding2affs_3d.embedding_loss_norm1(e, t, w, pkg.WeightedMSE(), shift=1, fill=False)
    assert recorder.border == [("crop", _offsets([1, 1, 1]))]


def test_crop_desc(pkg):
    pp = importlib.import_module(ge.PKG_NAME + ".utils.postproc")
    d = pp.crop_desc((2, 3, 6, 30, 32), [(0, 0, -1), (2, -3, 0), (0, 0, 0)])
    assert (d.B, d.K, list(d.dims), d.border, d.ndim) == (2, 3, [6, 30, 32], BORDER_CROP_ZERO, 3)
    assert [list(d.offsets[i]) for i in range(3)] == [[0, 0, -1], [2, -3, 0], [0, 0, 0]]
    d2 = pp.crop_desc((2, 2, 30, 32), [(-1, 0), (0, 5)])
    assert (list(d2.dims), d2.ndim, [list(d2.offsets[i]) for i in range(2)]) == ([1, 30, 32], 2, [[0, -1, 0], [0, 0, 5]])
    with pytest.raises(ValueError):
        pp.crop_desc((2, 3, 6, 30, 32), [(0, 0, -1)])


# ---- pea_affs_crop_zero: the refusals, none of which launches anything -------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def test_crop_zero_return_codes(pkg, lib):
    pp = importlib.import_module(ge.PKG_NAME + ".utils.postproc")
    good = lambda: pp.crop_desc((1, 2, 4, 8, 8), [(0, 0, -1), (1, -1, 0)])
    p = ctypes.c_void_p
    assert lib.pea_affs_crop_zero(None, p(64), None) == E_NULL
    for border in (0, 2):  # CIRCULAR, REPLICATE: every pair exists
        d = good()
        d.border = border
        assert lib.pea_affs_crop_zero(ctypes.byref(d), p(64), None) == E_DESC
        assert lib.pea_affs_crop_zero(ctypes.byref(d), None, None) == E_DESC  # the border is judged before the pointer
    d = good()
    d.K = 0
    assert lib.pea_affs_crop_zero(ctypes.byref(d), p(64), None) == E_DESC  # pea_desc_validate's own code
    d = good()
    d.offsets[0][2] = -8  # |o| == dim
    assert lib.pea_affs_crop_zero(ctypes.byref(d), p(64), None) == E_DESC
    d = good()
    assert lib.pea_affs_crop_zero(ctypes.byref(d), None, None) == E_NULL
    for off in (1, 2, 3):
        assert lib.pea_affs_crop_zero(ctypes.byref(d), p(64 + off), None) == E_ALIGN
    # a stencil without a non-zero component has no border: PEA_OK and no launch (the pointer is never used)
    d = pp.crop_desc((1, 1, 4, 8, 8), [(0, 0, 0)])
    assert lib.pea_affs_crop_zero(ctypes.byref(d), p(4), None) == OK
    assert "pea_affs_crop_zero" in pkg._lib.EXPORTS_CROP
