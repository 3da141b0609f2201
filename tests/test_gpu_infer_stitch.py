"""GPU (-m gpu): the fused 3D window inference -- VolumeStitcher.add_embedding -> pea_affinity_infer_stitch (csrc/pea_k_infer_stitch.hip):
affinities, border fill, activation and blend into the stitched volume in one launch per window -- against the CPU oracle with the
reference's fill / relu / add_vol / get_results statements restated in numpy (scripts_ac3ac4/inference.py:160-164,
scripts_ac3ac4/data/provider_valid.py:320-349), and against the three-call composition it replaces.

Shapes: windows (5, 43, 70) -- beyond the 27-voxel reach of norm5 in y and x, ox no multiple of 4 (ragged last quad, rows of no window
and of no volume 16-byte aligned at an odd x0: the element-wise path) -- plus (5, 43, 72) at x0 = 12 / 13 for the aligned vector loads
and stores and the mixed case.  Tolerance: affs abs 1e-5 against the oracle as in test_gpu_parity.py / test_gpu_zmarch.py; the blended
value is a product with w <= 1 + 1e-6 and the stitched result a weighted mean of affinities, so the bound carries over.  The weight
map sums the same f32 numbers in the same order as numpy: bit-exact."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
AFFS_ATOL = 1e-5
NORM5 = [1, 1, 1, 2, 3, 3, 3, 9, 9, 4, 27, 27]
NORM1 = [1, 1, 1]
WIN = (5, 43, 70)
WALK_VOL, WALK_STRIDE = (13, 59, 110), (4, 8, 20)
WALK_POS = [(z, y, x) for z in range(0, 9, 4) for y in range(0, 17, 8) for x in range(0, 41, 20)]  # 3 x 3 x 3 overlapping windows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def synth():
    ge.load_package()
    return importlib.import_module(ge.PKG_NAME + ".utils.synth")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def np_fill_act(pred, fill, relu, one_minus=False):
    """inference.py:160-164 on pred [K, oz, oy, ox] (a copy), then the descriptor's 1 - a"""
    pred = pred.copy()
    s = fill
    if s:
        pred[1, :, :s, :] = pred[1, :, s:s * 2, :]
        pred[2, :, :, :s] = pred[2, :, :, s:s * 2]
        pred[0, :s, :, :] = pred[0, s:s * 2, :, :]
    if relu:
        pred = np.maximum(pred, np.float32(0))
    if one_minus:
        pred = np.float32(1) - pred
    return pred


def np_add_vol(out, wmap, pred, w, pos, win):
    """provider_valid.py:326-331"""
    z, y, x = pos
    out[:, z:z + win[0], y:y + win[1], x:x + win[2]] += pred * w
    wmap[:, z:z + win[0], y:y + win[1], x:x + win[2]] += w


def window_inputs(synth, orc, D, win, shifts, seed):
    """one window with zero-norm voxels at a corner, on the three fill source slices (z = 1, y = 1, x = 1) and in the interior"""
    e, _, _ = synth.synth_inputs_3d(1, D, win[0], win[1], win[2], orc.norm_offsets(shifts), seed)
    e[0, :, 0, 0, 0] = 0.0
    e[0, :, win[0] - 1, win[1] - 1, win[2] - 1] = 1e-14
    e[0, :, 1, 20, 30] = 0.0
    e[0, :, 3, 1, 40] = 0.0
    e[0, :, 2, 25, 1] = 0.0
    e[0, :, 2, 30, 35] = 0.0
    e[0, :, 1, 1, 1] = 0.0
    return e


_SINGLE = {}


def single_reference(synth, orc, D, win, shifts):
    """(e, raw oracle affs [K, oz, oy, ox]) of one window: computed once per shape and stencil, shared by the cases"""
    key = (D, win, tuple(shifts))
    if key not in _SINGLE:
        e = window_inputs(synth, orc, D, win, shifts, 17 + D + win[2])
        affs, _ = orc.c_fwd(orc.desc_3d(e, shifts), e, want_affs=True)
        affs.setflags(write=False)
        _SINGLE[key] = (e, affs[0])
    return _SINGLE[key]


# the issue's window, and three more shapes for the paths it does not reach: aligned loads and stores, aligned loads with unaligned
# stores, D = 32
SINGLE_SHAPES = [(16, WIN, (2, 9, 13), (9, 60, 100)), (16, (5, 43, 72), (2, 9, 12), (9, 60, 100)), (16, (5, 43, 72), (2, 9, 13), (9, 60, 100)),
                 (32, (5, 43, 72), (2, 9, 12), (9, 60, 100))]


@pytest.mark.parametrize("act", ["none", "relu", "relu_one_minus"])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("mode", [5, 1])
@pytest.mark.parametrize("D,win,pos,vol", SINGLE_SHAPES)
def test_single_window_vs_oracle(pkg, dev, orc, synth, D, win, pos, vol, mode, fill, act):
    shifts = NORM5 if mode == 5 else NORM1
    e, o_affs = single_reference(synth, orc, D, win, shifts)
    K = len(shifts)
    relu = act != "none"
    st = pkg.VolumeStitcher(K, vol, win, dev)
    spec = None
    if act == "relu_one_minus":
        spec = pkg.AffinitySpec(3, orc.norm_offsets(shifts), None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_CROPPED, 1e-12,
                                act=pkg._lib.FLAG_RELU_AFFS | pkg._lib.FLAG_ONE_MINUS)
    et = cu(e, dev)
    d = pkg.affinity_op.make_desc(spec or pkg.AffinitySpec(3, orc.norm_offsets(shifts), None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_CROPPED), et)
    assert pkg._lib.lib().pea_infer_stitch_supported(ctypes.byref(d), fill) == 1
    st.add_embedding(et, pos, embedding_mode=mode, shift=fill, relu=relu, spec=spec, fused=True)
    w = st.weight_vol.cpu().numpy()
    want = np.zeros((K,) + tuple(vol), np.float32)
    want_w = np.zeros((1,) + tuple(vol), np.float32)
    np_add_vol(want, want_w, np_fill_act(o_affs, fill, relu, act == "relu_one_minus"), w, pos, win)
    got, got_w = st.out_affs.cpu().numpy(), st.weight_map.cpu().numpy()
    err = float(np.abs(got - want).max())
    print("single window D=%d win=%s pos=%s mode=%d fill=%d act=%s: max |out_affs - oracle| = %.3g" % (D, win, pos, mode, fill, act, err))
    assert err < AFFS_ATOL
    assert np.array_equal(got_w, want_w)


@pytest.fixture(scope="module")
def walk(synth, orc):
    """27 overlapping windows with an embedding each (f32, D = 16): inputs, the oracle's raw maps, and the numpy restatement of the
    reference's add_vol / get_results over them"""
    n = len(WALK_POS)
    e = synth.synth_embedding((n, 16) + WIN, 73)
    e[0, :, 0, 0, 0] = 0.0
    e[5, :, 1, 7, 1] = 0.0
    e[13, :, 2, 30, 35] = 0.0
    affs, _ = orc.c_fwd(orc.desc_3d(e, NORM5), e, want_affs=True)
    w = ge.load_package().harness.stitch.get_weight(WIN)
    out = np.zeros((12,) + WALK_VOL, np.float32)
    wmap = np.zeros((1,) + WALK_VOL, np.float32)
    for b, pos in enumerate(WALK_POS):
        np_add_vol(out, wmap, np_fill_act(affs[b], 1, True), w, pos, WIN)
    res = (out / wmap)[:, 1:-1, 4:-4, 4:-4]
    for a in (e, res, wmap):
        a.setflags(write=False)
    return {"e": e, "res": res, "wmap": wmap}


def run_walk(pkg, dev, e, fused, D=16):
    st = pkg.VolumeStitcher(12, WALK_VOL, WIN, dev)
    for b, pos in enumerate(WALK_POS):
        st.add_embedding(e[b:b + 1], pos, embedding_mode=5, shift=1, relu=True, fused=fused)
    wmap = st.weight_map.clone()
    return st.get_results((1, 4, 4)).clone(), wmap


def test_overlapping_windows_vs_reference_statements(pkg, dev, walk):
    res, wmap = run_walk(pkg, dev, cu(walk["e"], dev), True)
    assert tuple(res.shape) == walk["res"].shape
    err = float(np.abs(res.cpu().numpy() - walk["res"]).max())
    print("27-window walk: max |get_results - reference statements over oracle affs| = %.3g" % err)
    assert err < AFFS_ATOL
    assert np.array_equal(wmap.cpu().numpy(), walk["wmap"])


class Recorder(object):
    """counts the calls of one entry point of the loaded library"""

    def __init__(self, monkeypatch, lib, name):
        self.n, real = 0, getattr(lib, name)

        def wrapped(*a):
            self.n += 1
            return real(*a)
        monkeypatch.setattr(lib, name, wrapped)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [16, 32])
def test_fused_vs_composed(pkg, dev, synth, walk, monkeypatch, D, dtype):
    e = cu(walk["e"] if D == 16 else synth.synth_embedding((len(WALK_POS), D) + WIN, 91), dev).to(dtype)
    L = pkg._lib.lib()
    new, add = Recorder(monkeypatch, L, "pea_affinity_infer_stitch"), Recorder(monkeypatch, L, "pea_stitch_add")
    res_f, wmap_f = run_walk(pkg, dev, e, True, D)
    assert (new.n, add.n) == (len(WALK_POS), 0)      # the fused leg took the new entry point, once per window
    res_c, wmap_c = run_walk(pkg, dev, e, False, D)
    assert (new.n, add.n) == (len(WALK_POS), len(WALK_POS))
    err = float((res_f - res_c).abs().max())
    print("fused vs composed D=%d %s: max |difference| = %.3g" % (D, dtype, err))
    assert err < AFFS_ATOL
    assert torch.equal(wmap_f, wmap_c)


@pytest.mark.parametrize("case", ["circular", "d5"])
def test_unsupported_descriptors_fall_back_to_the_composition(pkg, dev, orc, synth, monkeypatch, case):
    D = 5 if case == "d5" else 16
    border, norm = (pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_FULL) if case == "circular" else (pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_CROPPED)
    spec = pkg.AffinitySpec(3, orc.norm_offsets(NORM5), None, border, norm, 1e-12)
    e = cu(synth.synth_embedding((1, D) + WIN, 5), dev)
    pos, vol = (2, 9, 13), (9, 60, 100)
    new = Recorder(monkeypatch, pkg._lib.lib(), "pea_affinity_infer_stitch")
    st = pkg.VolumeStitcher(12, vol, WIN, dev)
    st.add_embedding(e, pos, spec=spec, shift=1, relu=True, fused=True)
    assert new.n == 0
    ref = pkg.VolumeStitcher(12, vol, WIN, dev)
    pred = pkg.fill_border_relu_(pkg.affinity_infer(e, None, spec), shift=1, relu=True)
    ref.add_vol(pred[0], pos)
    assert torch.equal(st.out_affs, ref.out_affs) and torch.equal(st.weight_map, ref.weight_map)
    assert float(st.out_affs.abs().max()) > 0


def test_batch_form_equals_single_calls(pkg, dev, walk):
    e = cu(walk["e"][3:5], dev)
    pos = [(0, 0, 0), (2, 8, 20)]
    a = pkg.VolumeStitcher(12, WALK_VOL, WIN, dev)
    a.add_embedding(e, pos, fused=True)
    b = pkg.VolumeStitcher(12, WALK_VOL, WIN, dev)
    for i in range(2):
        b.add_embedding(e[i:i + 1], pos[i], fused=True)
    assert torch.equal(a.out_affs, b.out_affs) and torch.equal(a.weight_map, b.weight_map)
    # one position for every item of the batch: the same voxels twice, in order
    c = pkg.VolumeStitcher(12, WALK_VOL, WIN, dev)
    c.add_embedding(e, (1, 3, 7), fused=True)
    d = pkg.VolumeStitcher(12, WALK_VOL, WIN, dev)
    for i in range(2):
        d.add_embedding(e[i:i + 1], (1, 3, 7), fused=True)
    assert torch.equal(c.out_affs, d.out_affs) and torch.equal(c.weight_map, d.weight_map)
    with pytest.raises(ValueError):
        a.add_embedding(e, [(0, 0, 0)] * 3, fused=True)
