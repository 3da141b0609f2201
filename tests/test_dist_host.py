"""CPU: the distance-form affinities (include/pea_dist.h) -- the header and the library agree on the three new symbols, the ctypes mirror
has the header's layout, pea_dist_validate accepts and refuses what the header lists, every refusal of the two calls is reached before
anything is launched and in the header's order (dummy device pointers, no GPU), the Python mirrors have the reference's signatures and
say what is wrong with a call before they look at the device, the package's earlier exports are untouched, and the float64 restatement
tests/dist_reference.py -- what the GPU tests compare the kernels with -- reproduces the reference's own numbers on every fixture
(tests/golden/make_golden_dist.py)."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import ROOT
from dist_reference import dist_reference, dist_vjp_reference, load_dist_golden

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -5
F32, F16, BF16 = 0, 1, 2
CIRCULAR, CROP_ZERO, REPLICATE, ZERO_VECTOR = 0, 1, 2, 3
INVERT = 1
NEW = ["pea_dist_affinity", "pea_dist_affinity_vjp", "pea_dist_validate"]
GOLDENS = ("gdist_2d_b2_d5_37x53", "gdist_2d_k1", "gdist_3d_b2_5x20x24", "gdist_3d_reach_3x7x9")
INF, NAN = float("inf"), float("nan")

# __all__ of the package before this family was added
EARLIER = """PeaLibraryError build backward graphed Graphed check_label_ranges AffinityMap AffinitySpec FusedAffinityMSE affinity_infer
WeightedMSE WeightedBCE BCELoss MSELoss embedding_loss ema_embedding_loss embedding2affs embedding_loss_norm1 embedding_loss_norm5
ema_embedding_loss_norm1 ema_embedding_loss_norm5 inf_embedding_loss_norm1 inf_embedding_loss_norm5 gen_offsets multi_offset
fill_border_relu_ relu_ cvppp_loss_section ac3ac4_loss_section deep_weight_factor finish_pred_2d_ finish_pred_3d_ gen_targets
gen_affs_ours seg_to_aff VolumeStitcher embedding_loss_from_labels ema_embedding_loss_from_labels LabelsAffinityMSE
cvppp_loss_section_from_labels cvppp_loss_section_composed ac3ac4_loss_section_composed ac3ac4_loss_section_from_labels
embedding_loss_norm1_from_labels embedding_loss_norm5_from_labels ema_embedding_loss_norm5_from_labels loss_embedding
loss_embedding_exp loss_embedding_norm embedding_loss_half_clamp ema_embedding_loss_half_clamp embedding2affs_half_clamp
embedding_loss_clamp embedding2affs_clamp embedding_loss_normalized ema_embedding_loss_normalized embedding2affs_normalized
embedding_loss_norm6 ema_embedding_loss_norm6 EmbeddingHead OutConv head_conv3d_block head16_supported cvppp_label_weight_tables
cvppp_validation_section MultiAffinityMSE embedding_loss_multi embedding_loss_norm1_multi unflip convert_consistency_flip
MultiLabelsAffinityMSE embedding_loss_from_labels_multi embedding_loss_norm1_from_labels_multi affinity_metrics AffinityMetrics
BCE_loss_func foreground_mask_loss foreground_mask ForegroundMaskCE discriminative_loss discriminative_loss_stats DiscriminativeLoss
embedding2affs_3d embedding2affs_3d_l2 embedding_loss_norm2 ema_embedding_loss_norm2 affs_crop_zero_""".split()
ADDED = ["distance_affinities", "DistanceAffinities", "emb2affs", "embeddings_ours"]


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


# ---- exports and layout --------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_new_entry_points(pkg, lib):
    src = open(os.path.join(ROOT, "include", "pea_dist.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", code))) == sorted(pkg._lib.EXPORTS_DIST) == NEW
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    assert '#include "pea.h"' in src and lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    for name, text, value in (("MAX_D", "64", 64), ("BORDER_ZERO_VECTOR", "3", 3), ("INVERT", "1u", 1)):
        assert re.search(r"#define\s+PEA_DIST_%s\s+%s\b" % (name, text), src), name
        assert getattr(pkg._lib, "DIST_" + name) == value
    assert pkg._lib.DIST_BORDER_ZERO_VECTOR not in (pkg._lib.BORDER_CIRCULAR, pkg._lib.BORDER_CROP_ZERO, pkg._lib.BORDER_REPLICATE)
    for cite in ("utils/emb2affs.py:63-75", "scripts_ac3ac4/utils/embeddings_ours.py:47-98", "scripts_ac3ac4/utils/embeddings.py:78-114"):
        assert cite in src, cite


def test_ctypes_mirror_has_the_headers_layout(pkg):
    D = pkg._lib.PeaDistDesc
    names = ["B", "D", "dims", "K", "offsets", "dtype", "border", "flags", "delta_v", "delta_d"]
    assert [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == [0, 4, 8, 20, 24, 408, 412, 416, 420, 424] and ctypes.sizeof(D) == 428
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pea_dist.h")).read(), flags=re.S)
    body = re.search(r"typedef struct PeaDistDesc \{(.*?)\} PeaDistDesc;", src, flags=re.S).group(1)
    decl = [re.sub(r"\[.*", "", n) for d in body.split(";") if d.strip()
            for n in re.sub(r"^\s*(u?int(32|64)_t|float)", "", d.strip()).replace(" ", "").split(",")]
    assert decl == names


def test_earlier_exports_are_untouched(pkg):
    assert pkg.__all__[:len(EARLIER)] == EARLIER and pkg.__all__[len(EARLIER):] == ADDED
    for name in EARLIER + ADDED:
        assert hasattr(pkg, name), name
    assert not set(ADDED) & set(EARLIER)
    assert pkg.emb2affs is import_module(pkg.__name__ + ".utils.emb2affs")
    assert pkg.embeddings_ours is import_module(pkg.__name__ + ".utils.embeddings_ours")
    assert pkg.distance_affinities is import_module(pkg.__name__ + ".harness.dist").distance_affinities
    assert pkg.embedding2affs is import_module(pkg.__name__ + ".loss.loss_embedding_mse").embedding2affs  # the cosine form keeps its name
    assert "add_distance_embedding" in vars(pkg.VolumeStitcher) and "add_embedding" in vars(pkg.VolumeStitcher)
    sig = inspect.signature(pkg.VolumeStitcher.add_distance_embedding)
    assert list(sig.parameters) == ["self", "embedding", "pos", "offsets", "delta_v", "delta_d", "border", "invert"]
    assert sig.parameters["invert"].default is False


# ---- return codes --------------------------------------------------------------------------------------------------------------------
E, AFFS, G, DSCALE, DE = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000


def desc(pkg, B=2, D=16, dims=(5, 20, 24), offsets=((-1, 0, 0), (0, -1, 0), (1, -2, 3)), dtype=F32, border=REPLICATE, flags=0, delta_v=0.5,
         delta_d=1.5, K=None):
    d = pkg._lib.PeaDistDesc()
    d.B, d.D, d.K, d.dtype, d.border, d.flags = B, D, len(offsets) if K is None else K, dtype, border, flags
    d.dims[:] = dims
    for i, o in enumerate(offsets[:32]):
        d.offsets[i][:] = o
    d.delta_v, d.delta_d = delta_v, delta_d
    return d


def vp(a):
    return ctypes.c_void_p(a) if a else None


def fwd(pkg, lib, d="default", e=E, affs=AFFS, **kw):
    """pea_dist_affinity on dummy pointers: anything but an early return would fault"""
    if isinstance(d, str):
        d = desc(pkg, **kw)
    return lib.pea_dist_affinity(None if d is None else ctypes.byref(d), vp(e), vp(affs), None)


def vjp(pkg, lib, d="default", e=E, g=G, dscale=DSCALE, de=DE, **kw):
    if isinstance(d, str):
        d = desc(pkg, **kw)
    return lib.pea_dist_affinity_vjp(None if d is None else ctypes.byref(d), vp(e), vp(g), vp(dscale), vp(de), None)


BIG = dict(B=1, dims=(2048, 1024, 1024))         # Z Y X = 2^31 > 2^31 - 1
EDGE = dict(B=1 << 12, dims=(1, 1 << 10, 1 << 17))  # S = 2^27: 2^19 workgroups per image, 2^31 in all: one too many


def test_descriptor_refusals(pkg, lib):
    v = lambda **kw: lib.pea_dist_validate(ctypes.byref(desc(pkg, **kw)))
    assert lib.pea_dist_validate(None) == E_NULL and fwd(pkg, lib, d=None) == E_NULL and vjp(pkg, lib, d=None) == E_NULL
    assert v() == OK and v(dtype=F16, border=ZERO_VECTOR) == OK and v(dtype=BF16, flags=INVERT) == OK
    assert v(B=1, D=1, dims=(1, 1, 1), offsets=((0, 0, 0),)) == OK and v(D=64, K=32) == OK and v(delta_v=0.0) == OK
    assert v(D=5, dims=(1, 37, 53)) == OK and v(delta_v=7.0, delta_d=1e-3) == OK
    # offsets of any size are valid under either border: every pair is defined
    far = ((2 ** 31 - 1, -2 ** 31, 0), (9, 0, 0), (0, 0, 27), (-(2 ** 31), -(2 ** 31), -(2 ** 31)))
    assert v(offsets=far) == OK and v(offsets=far, border=ZERO_VECTOR) == OK
    bad = [dict(B=0), dict(B=-1), dict(D=0), dict(D=-4), dict(D=65), dict(D=128), dict(D=2 ** 31 - 1),
           dict(dims=(0, 20, 24)), dict(dims=(5, 0, 24)), dict(dims=(5, 20, -1)),
           dict(K=0), dict(K=-1), dict(K=33),
           dict(dtype=3), dict(dtype=-1),
           dict(border=CIRCULAR), dict(border=CROP_ZERO), dict(border=4), dict(border=-1),
           dict(flags=2), dict(flags=1 | 4), dict(flags=1 << 31),
           dict(delta_d=0.0), dict(delta_d=-1.0), dict(delta_d=INF), dict(delta_d=NAN),
           dict(delta_v=-0.5), dict(delta_v=INF), dict(delta_v=NAN)]
    for kw in bad:
        assert v(**kw) == E_DESC, kw
        assert fwd(pkg, lib, **kw) == E_DESC and vjp(pkg, lib, **kw) == E_DESC, kw
        assert fwd(pkg, lib, e=0, affs=0, **kw) == E_DESC and vjp(pkg, lib, e=0, g=0, de=0, **kw) == E_DESC, kw  # the descriptor first


def test_forward_refusals_before_a_launch(pkg, lib):
    assert fwd(pkg, lib, e=0) == E_NULL and fwd(pkg, lib, affs=0) == E_NULL
    for skew in (1, 2, 3):
        assert fwd(pkg, lib, e=E + skew) == E_ALIGN and fwd(pkg, lib, affs=AFFS + skew) == E_ALIGN
    for dt in (F16, BF16):
        assert fwd(pkg, lib, e=E + 1, dtype=dt) == E_ALIGN and fwd(pkg, lib, e=E + 2, affs=AFFS + 2, dtype=dt) == E_ALIGN
        assert fwd(pkg, lib, e=E + 2, dtype=dt, **BIG) == E_UNSUPPORTED  # element-aligned: accepted
    assert fwd(pkg, lib, **BIG) == E_UNSUPPORTED and fwd(pkg, lib, **EDGE) == E_UNSUPPORTED
    assert fwd(pkg, lib, border=ZERO_VECTOR, flags=INVERT, D=5, **BIG) == E_UNSUPPORTED
    # the stated order: descriptor, NULL, alignment, range
    assert fwd(pkg, lib, e=E + 1, affs=0, **BIG) == E_NULL and fwd(pkg, lib, e=E + 1, **BIG) == E_ALIGN
    assert fwd(pkg, lib, e=0, affs=0, border=CIRCULAR) == E_DESC


def test_vjp_refusals_before_a_launch(pkg, lib):
    for ptr in ("e", "g", "de"):
        assert vjp(pkg, lib, **{ptr: 0}) == E_NULL, ptr
    for skew in (1, 2, 3):
        for ptr, base in (("e", E), ("g", G), ("dscale", DSCALE), ("de", DE)):
            assert vjp(pkg, lib, **{ptr: base + skew}) == E_ALIGN, (ptr, skew)
    for dt in (F16, BF16):
        assert vjp(pkg, lib, e=E + 1, dtype=dt) == E_ALIGN and vjp(pkg, lib, de=DE + 1, dtype=dt) == E_ALIGN
        assert vjp(pkg, lib, g=G + 2, dtype=dt) == E_ALIGN and vjp(pkg, lib, dscale=DSCALE + 2, dtype=dt) == E_ALIGN
        assert vjp(pkg, lib, e=E + 2, de=DE + 6, dtype=dt, **BIG) == E_UNSUPPORTED
    assert vjp(pkg, lib, **BIG) == E_UNSUPPORTED and vjp(pkg, lib, **EDGE) == E_UNSUPPORTED
    assert vjp(pkg, lib, dscale=0, **BIG) == E_UNSUPPORTED  # a missing dscale (= 1) is accepted
    assert vjp(pkg, lib, g=G + 1, de=0, **BIG) == E_NULL and vjp(pkg, lib, g=G + 1, **BIG) == E_ALIGN
    assert vjp(pkg, lib, e=0, g=0, de=0, dtype=7) == E_DESC


# ---- the Python entry points -----------------------------------------------------------------------------------------------------------
def test_signatures_are_the_references(pkg):
    g = load_dist_golden("gdist_2d_k1")
    t, n = pkg.emb2affs, pkg.embeddings_ours
    assert list(inspect.signature(t.embeddings_to_affinities).parameters) == [str(s) for s in g["params_emb2affs"]] == ["embeddings", "offsets", "delta"]
    assert inspect.signature(t.embeddings_to_affinities).parameters["delta"].default == float(g["default_delta"]) == 1.5
    assert list(inspect.signature(t.segmentation_to_affinities).parameters) == [str(s) for s in g["params_seg2affs"]] == ["segmentation", "offsets"]
    assert list(inspect.signature(t.invert_offsets).parameters) == [str(s) for s in g["params_invert"]] == ["offsets"]
    sig = inspect.signature(n.embeddings_to_affinities)
    assert list(sig.parameters) == [str(s) for s in g["params_ours"]] == ["embeddings", "offsets", "delta_v", "delta_d", "invert"]
    assert [float(sig.parameters[k].default) for k in ("delta_v", "delta_d", "invert")] == [float(v) for v in g["defaults_ours"]] == [0.5, 1.5, 0.0]
    assert sig.parameters["invert"].default is False
    assert sig.parameters["offsets"].default == g["offsets_ours"].tolist() == [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    sig = inspect.signature(pkg.distance_affinities)
    assert list(sig.parameters) == ["e", "offsets", "delta_v", "delta_d", "border", "invert"]
    assert [sig.parameters[k].default for k in ("delta_v", "delta_d", "border", "invert")] == [0.0, 1.5, "replicate", False]
    assert t.invert_offsets([[1, -2, 3], [0, 0, 0]]) == [[-1, 2, -3], [0, 0, 0]]


def test_python_entry_points_say_what_is_wrong_without_a_gpu(pkg):
    t, n = pkg.emb2affs, pkg.embeddings_ours
    e2, e3 = torch.zeros(2, 5, 6, 7), torch.zeros(1, 16, 3, 6, 7)
    o2, o3 = [[-1, 0], [0, 9]], [[-1, 0, 0], [1, -2, 3]]
    for call in (lambda: pkg.distance_affinities(e2, o2), lambda: pkg.distance_affinities(e3.half(), o3, 0.5, 1.5, "zero", True),
                 lambda: t.embeddings_to_affinities(e3, o3), lambda: t.embeddings_to_affinities(e2.bfloat16(), o2, delta=2.0),
                 lambda: n.embeddings_to_affinities(e3[0]), lambda: n.embeddings_to_affinities(e2[0], o2, invert=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            n.embeddings_to_affinities(np.zeros((16, 3, 6, 7), np.float32))
    with pytest.raises(ValueError, match=r"\[B, D, H, W\] or \[B, D, Z, Y, X\]"):
        pkg.distance_affinities(e2[0], o2)
    for offs in (o3, [[1]], [[0, 1], [1, 2, 3]]):
        with pytest.raises(ValueError, match="Incosistent dimension"):
            pkg.distance_affinities(e2, offs)
        with pytest.raises(ValueError, match="Incosistent dimension"):
            n.embeddings_to_affinities(e2[0], offs)
    with pytest.raises(ValueError, match="between 1 and 32 offsets"):
        pkg.distance_affinities(e2, [])
    with pytest.raises(ValueError, match="between 1 and 32 offsets"):
        pkg.distance_affinities(e2, [[0, 1]] * 33)
    with pytest.raises(ValueError, match="more than 64 channels"):
        pkg.distance_affinities(torch.zeros(1, 65, 4, 4), o2)
    with pytest.raises(ValueError, match="border must be"):
        pkg.distance_affinities(e2, o2, border="circular")
    for kw in (dict(delta_d=0.0), dict(delta_d=-1.0), dict(delta_d=INF), dict(delta_d=NAN), dict(delta_v=-0.1), dict(delta_v=INF), dict(delta_v=NAN)):
        with pytest.raises(ValueError, match="delta_d must be finite"):
            pkg.distance_affinities(e2, o2, **kw)
    with pytest.raises(ValueError, match="empty"):
        pkg.distance_affinities(torch.zeros(2, 5, 0, 7), o2)
    with pytest.raises(TypeError):
        pkg.distance_affinities(e2.double(), o2)
    with pytest.raises(TypeError):
        pkg.distance_affinities(e2.numpy(), o2)
    with pytest.raises(TypeError):
        n.embeddings_to_affinities([[1.0]])


# ---- the restatement and the torch-composed mirror against the reference's numbers -------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_goldens(pkg, name):
    """the float64 map and gradient of the torch form to 1e-12; the reference's float32 maps (torch form and numpy form, dead zone and
    inversion) within float32's reach away from the dead zone's edge"""
    g = load_dist_golden(name)
    e, offs, delta = g["e"], g["offsets"], g["delta"]
    B, D = e.shape[:2]
    K, sp = len(offs), e.shape[2:]
    assert e.dtype == np.float32 and np.array_equal(e.astype(np.float16).astype(np.float32), e)
    assert g["affs64"].dtype == np.float64 and g["affs"].dtype == np.float32 and g["de64"].dtype == np.float64
    assert g["affs64"].shape == g["affs"].shape == g["g"].shape == (B, K) + sp and g["de64"].shape == e.shape
    a, d = dist_reference(e, offs, 0.0, delta, "replicate")
    assert np.abs(a - g["affs64"]).max() <= 1e-12
    assert np.abs(a - g["affs"]).max() <= 1e-6
    de = dist_vjp_reference(e, offs, g["g"], 0.0, delta, "replicate")
    top = np.abs(g["de64"]).max()
    assert top > 0.1 and np.abs(de - g["de64"]).max() <= 1e-12 * top
    de2 = dist_vjp_reference(e, offs, g["g"], 0.0, delta, "replicate", invert=True, dscale=-2.5)
    assert np.abs(de2 - 2.5 * de).max() <= 1e-12 * 2.5 * top
    # d == 0: a == 1 exactly and no contribution; the planted pair lies away from every border
    assert (a[d == 0] == 1.0).all() and (d == 0).mean() > 0.01
    zero_inside = (d == 0).copy()
    for i, o in enumerate(offs):
        if not any(o):
            zero_inside[:, i] = False
    inner = tuple(slice(1, -1) for _ in sp)
    assert zero_inside[(slice(None), slice(None)) + inner].any() or name == "gdist_3d_reach_3x7x9"
    # the numpy form: one volume, the zero vector outside, the dead zone
    for key, dv in (("np_dv05", 0.5), ("np_dv0", 0.0)):
        an, dn = dist_reference(e[:1], offs, dv, delta, "zero")
        keep = np.abs(dn[0] - dv) >= 1e-4 if dv > 0 else np.ones(dn[0].shape, bool)
        assert keep.mean() > 0.999
        assert g[key].shape == (K,) + sp and np.abs(an[0] - g[key])[keep].max() <= 1e-6
        ai, _ = dist_reference(e[:1], offs, dv, delta, "zero", invert=True)
        assert np.abs(ai[0] - g[key + "_inv"])[keep].max() <= 1e-6
        assert np.array_equal(g[key + "_inv"], np.float32(1) - g[key])
    if name != "gdist_3d_reach_3x7x9":  # (there every pair leaves the volume: d = |e(p)|, far outside the dead zone)
        assert (np.abs(g["np_dv05"] - g["np_dv0"]) > 1e-3).mean() > 0.02  # the dead zone matters on these inputs
    # what each fixture is there for
    flat = [tuple(o) for o in offs]
    if name == "gdist_2d_b2_d5_37x53":
        assert e.shape == (2, 5, 37, 53) and K == 8
    if name == "gdist_2d_k1":
        assert K == 1
    if name == "gdist_3d_b2_5x20x24":
        assert e.shape == (2, 16, 5, 20, 24) and (1, -2, 3) in flat and (0, 0, 0) in flat and len(set(flat)) < K
        assert any(abs(o[0]) == 9 for o in flat) and any(abs(o[2]) == 27 for o in flat)
        assert any(v < 0 for o in flat for v in o) and any(v > 0 for o in flat for v in o)
    if name == "gdist_3d_reach_3x7x9":
        assert e.shape == (1, 16, 3, 7, 9) and K == 32 and all(abs(o[0]) >= 3 or abs(o[1]) >= 7 or abs(o[2]) >= 9 for o in flat)


@pytest.mark.parametrize("border", ["replicate", "zero"])
@pytest.mark.parametrize("invert", [False, True])
def test_restatement_vjp_is_autograds_under_both_borders(border, invert):
    """the fixtures hold a gradient for the replicate border without a dead zone only: the restatement's vjp with the zero-vector border,
    the dead zone and the invert flag against torch's autograd on the transform composed in float64"""
    g = load_dist_golden("gdist_3d_reach_3x7x9")
    e = np.concatenate([g["e"], g["e"][:, :, ::-1].copy()])  # B = 2
    offs = [[-1, 0, 0], [0, -1, 0], [1, -2, 3], [0, 0, 0], [0, 0, -1], [0, 9, 0], [-3, 2, 0]]
    dv, dd = 0.5, 1.5
    up = np.random.default_rng(3).standard_normal((2, len(offs), 3, 7, 9))
    x = torch.from_numpy(e).double().requires_grad_(True)
    maps = []
    for o in offs:
        pad = [v for a in (2, 1, 0) for v in (max(0, -o[a]), max(0, o[a]))]
        big = torch.nn.functional.pad(x, pad, mode="replicate" if border == "replicate" else "constant")
        nb = big[(slice(None), slice(None)) + tuple(slice(max(0, o[a]) + 0, max(0, o[a]) + n) if o[a] >= 0 else slice(0, n)
                                                   for a, n in enumerate((3, 7, 9)))]
        d = torch.norm(x - nb, dim=1)
        h = torch.where(d <= dv, torch.zeros_like(d), d)
        a = torch.clamp((2 * dd - h) / (2 * dd), min=0) ** 2
        maps.append(1 - a if invert else a)
    a_t = torch.stack(maps, 1)
    (a_t * torch.from_numpy(up)).sum().backward()
    a, d64 = dist_reference(e, offs, dv, dd, border, invert)
    assert np.abs(a - a_t.detach().numpy()).max() <= 1e-12
    de = dist_vjp_reference(e, offs, up, dv, dd, border, invert)
    top = np.abs(x.grad.numpy()).max()
    assert top > 0.1 and np.abs(de - x.grad.numpy()).max() <= 1e-12 * top
    assert (d64 <= dv).mean() > 0.05 and (d64 == 0).mean() > 0.05 and (d64 >= 2 * dd).mean() > 0.005


@pytest.mark.parametrize("name", GOLDENS)
def test_segmentation_to_affinities_reproduces_the_goldens(pkg, name):
    g = load_dist_golden(name)
    seg = torch.from_numpy(g["labels"][:, None].astype(np.int64))
    out = pkg.emb2affs.segmentation_to_affinities(seg, g["offsets"])
    assert out.dtype == torch.float32 and np.array_equal(out.numpy(), g["seg_affs"].astype(np.float32))
    assert 0.05 < g["seg_affs"].mean() < 0.95
    out32 = pkg.emb2affs.segmentation_to_affinities(seg.int(), g["offsets"])
    assert torch.equal(out32, out)
