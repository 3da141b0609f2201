"""CPU: the batched labels-in self losses (include/pea_multi_labels.h: pea_multi_labels_supported, pea_multi_labels_scratch_bytes,
pea_affinity_fwd_bwd_labels_multi) -- the header and the library agree on the three new symbols while pea.h and pea_multi.h keep
theirs, the struct matches its ctypes mirror, the support query answers as the header documents, every return code of the call is
reached before anything is launched (dummy device pointers, no GPU), and the labels-in sections take label_downs=None / batched=False."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

OK, E_NULL, E_DESC, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -4, -5
CIRCULAR, CROP_ZERO, REPLICATE = 0, 1, 2
F32, F16, BF16 = 0, 1, 2
FLAG_HALF_SHIFT, FLAG_CLAMP01, FLAG_MASK_F32, FLAG_LOSS_ACT = 4, 8, 32, 64
TGT_PADDING, TGT_BOTH_FOREGROUND, TGT_MASK_INSIDE, TGT_ACCUMULATE = 1, 2, 4, 8
FLAGS_2D, FLAGS_3D = TGT_PADDING | TGT_MASK_INSIDE, TGT_BOTH_FOREGROUND
CROSS = [[-1, 0], [0, -1], [-3, 0], [0, -3], [-5, 0], [0, -5], [-9, 0], [0, -9], [-27, 0], [0, -27]]  # multi_offset([1, 3, 5, 9, 27], 4)
PEA_H = ["pea_affinity_bwd", "pea_affinity_bwd_dual", "pea_affinity_bwd_dual_ex", "pea_affinity_bwd_ex", "pea_affinity_bwd_ex2",
         "pea_affinity_fwd", "pea_affinity_fwd_bwd_labels", "pea_affinity_fwd_bwd_labels_dual", "pea_affinity_fwd_bwd_labels_ex",
         "pea_affinity_fwd_dual_ex", "pea_affinity_fwd_ex", "pea_affinity_infer", "pea_cross_supported", "pea_desc_validate",
         "pea_fill_border_relu", "pea_gen_targets", "pea_head_bwd", "pea_head_fwd", "pea_head_workspace_bytes", "pea_inv_norm",
         "pea_label_weights", "pea_labels_scratch_bytes", "pea_reload_env", "pea_scale_inplace", "pea_scale_inplace_multi",
         "pea_stitch_add", "pea_stitch_finalize", "pea_strerror", "pea_targets_workspace_bytes", "pea_version", "pea_weighted_sum",
         "pea_workspace_bytes", "pea_workspace_init"]
PEA_MULTI_H = ["pea_affinity_bwd_multi", "pea_affinity_fwd_multi", "pea_multi_supported"]
NEW = ["pea_affinity_fwd_bwd_labels_multi", "pea_multi_labels_scratch_bytes", "pea_multi_labels_supported"]


def header_text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def declared_symbols(header):
    return sorted(set(re.findall(r"\b(pea_[a-z_0-9]+)\s*\(", header_text(header))))


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def desc2d(pkg, H=136, W=136, offsets=CROSS[:8], B=2, D=16, **kw):
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 2, B, D, len(offsets)
    d.dims[:] = [1, H, W]
    d.border, d.dtype, d.norm, d.eps = CIRCULAR, F32, 0, 1e-12
    for i, o in enumerate(offsets):
        d.offsets[i][:] = [0] + list(o)
        d.lam[i] = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def desc3d(pkg, dims=(18, 80, 80), shift=1, B=2, D=16, **kw):
    d = pkg._lib.PeaDesc()
    d.abi, d.ndim, d.B, d.D, d.K = pkg._lib.PEA_ABI_VERSION, 3, B, D, 3
    d.dims[:] = list(dims)
    d.border, d.dtype, d.norm, d.eps = CROP_ZERO, F32, 1, 1e-12
    for i in range(3):
        o = [0, 0, 0]
        o[i] = -shift
        d.offsets[i][:] = o
        d.lam[i] = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


DUMMY = dict(e=0x10000, labels=0x20000, wtab=None, affs=None, loss_out=0x50000, dloss=None, de=0x60000)


def entry(d, label_dims=None, step=(1, 1, 1), **over):
    """(descriptor, label_dims, label_step, pointer overrides); label_dims=None: exactly what the step needs"""
    if label_dims is None:
        label_dims = [(d.dims[a] - 1) * step[a] + 1 for a in range(3)] if d is not None else [1, 1, 1]
    return (d, list(label_dims), list(step), over)


def table_of(pkg, ents):
    tab = (pkg._lib.PeaMultiLabels * max(len(ents), 1))()
    for j, (d, ldims, step, over) in enumerate(ents):
        args = dict(DUMMY, desc=ctypes.pointer(d) if d is not None else None)
        args.update(over)
        for k, v in args.items():
            setattr(tab[j], k, v)
        tab[j].label_dims[:] = ldims
        tab[j].label_step[:] = step
    return tab


def cvppp_steps(pkg, full=544, **kw):
    """the four CVPPP deep scales sampling ONE full x full label image: 272^2 .. 34^2 with steps 2 .. 16"""
    return [entry(desc2d(pkg, full >> (j + 1), full >> (j + 1), CROSS[:2 * (4 - j)], **kw), (1, full, full), (1, 2 << j, 2 << j)) for j in range(4)]


def cvppp_own(pkg):
    return [entry(desc2d(pkg, 272 >> j, 272 >> j, CROSS[:2 * (4 - j)])) for j in range(4)]


def norm1_steps(pkg):
    return [entry(desc3d(pkg, (18, 160 >> (j + 1), 160 >> (j + 1))), (18, 160, 160), (1, 2 << j, 2 << j)) for j in range(4)]


def norm1_own(pkg):
    return [entry(desc3d(pkg, (18, 80 >> j, 80 >> j))) for j in range(4)]


def supported(pkg, lib, ents, flags=FLAGS_2D, n=None):
    return lib.pea_multi_labels_supported(table_of(pkg, ents), len(ents) if n is None else n, flags)


def call(pkg, lib, ents, flags=FLAGS_2D, n=None, ws=0x100000, ws_bytes=None, scratch=0x200000, scratch_bytes=None):
    """pea_affinity_fwd_bwd_labels_multi on dummy pointers"""
    tab = table_of(pkg, ents)
    n = len(ents) if n is None else n
    state = lib.pea_workspace_bytes(ctypes.byref(desc2d(pkg)))
    need = sum(d.B * d.K for d, _, _, _ in ents if d is not None)
    return lib.pea_affinity_fwd_bwd_labels_multi(tab, n, flags, ctypes.c_void_p(ws) if ws else None, n * state if ws_bytes is None else ws_bytes,
                                                 ctypes.c_void_p(scratch) if scratch else None, 4 * need if scratch_bytes is None else scratch_bytes,
                                                 None)


def test_header_declares_exactly_the_three_entry_points(pkg):
    assert declared_symbols("pea_multi_labels.h") == sorted(pkg._lib.EXPORTS_MULTI_LABELS) == NEW
    assert '#include "pea_multi.h"' in open(os.path.join(ROOT, "include", "pea_multi_labels.h")).read()


def test_library_exports_them_and_the_older_headers_are_unchanged(pkg, lib):
    raw = ctypes.CDLL(pkg._lib.SO_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    older = set(pkg._lib.EXPORTS) | set(pkg._lib.EXPORTS_INFER) | set(pkg._lib.EXPORTS_MULTI) | set(pkg._lib.EXPORTS_FLIP)
    assert not set(NEW) & older
    assert declared_symbols("pea.h") == sorted(pkg._lib.EXPORTS) == PEA_H
    assert declared_symbols("pea_multi.h") == sorted(pkg._lib.EXPORTS_MULTI) == PEA_MULTI_H
    assert lib.pea_version() == pkg._lib.PEA_ABI_VERSION == 2
    assert re.search(r"#define\s+PEA_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "include", "pea.h")).read())


def test_entry_struct_matches_the_header(pkg):
    body = re.search(r"typedef struct PeaMultiLabels \{(.*?)\} PeaMultiLabels;", header_text("pea_multi_labels.h"), flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*(?:\[\s*3\s*\])?\s*;", body)
    assert fields == [f[0] for f in pkg._lib.PeaMultiLabels._fields_]
    assert fields == ["desc", "e", "labels", "label_dims", "label_step", "wtab", "affs", "loss_out", "dloss", "de"]
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(pkg._lib.PeaMultiLabels) == 8 * P + 6 * 4
    assert pkg._lib.PeaMultiLabels.label_dims.offset == 3 * P and pkg._lib.PeaMultiLabels.label_step.offset == 3 * P + 12
    assert pkg._lib.PeaMultiLabels.wtab.offset == 3 * P + 24


def test_supported_query(pkg, lib):
    q = lambda ents, flags=FLAGS_2D, n=None: supported(pkg, lib, ents, flags, n)
    # the two pyramids, sampling one image with steps and with label images of their own
    assert q(cvppp_steps(pkg)) == 1 and q(cvppp_steps(pkg, B=8)) == 1 and q(cvppp_own(pkg)) == 1
    assert q(cvppp_steps(pkg, full=160)) == 1                                               # 160^2 -> 80^2 .. 10^2
    assert q(norm1_steps(pkg), FLAGS_3D) == 1 and q(norm1_own(pkg), FLAGS_3D) == 1
    assert q(cvppp_steps(pkg)[:1]) == 1 and q(cvppp_steps(pkg)[:2]) == 1
    assert q([cvppp_steps(pkg)[0], norm1_own(pkg)[0], entry(desc2d(pkg, D=32))], 0) == 1    # entries may differ in every field
    for flags in range(8):
        assert q(cvppp_own(pkg), flags) == 1
    # n = 0 / 5
    assert q([], n=0) == 0
    assert q(cvppp_own(pkg) + [entry(desc2d(pkg))]) == 0
    assert lib.pea_multi_labels_supported(None, 1, FLAGS_2D) == 0
    base = cvppp_steps(pkg)[:3]
    assert q(base + [entry(None)]) == 0
    assert q(base + [entry(desc2d(pkg, abi=7))]) == 0
    assert q(base + [entry(desc2d(pkg, dtype=BF16))]) == 0
    assert q(base + [entry(desc2d(pkg, dtype=F16))]) == 0
    assert q(base + [entry(desc2d(pkg, D=64))]) == 0 and q(base + [entry(desc2d(pkg, D=8))]) == 0
    k13 = CROSS + [[-2, 0], [0, -2], [-4, 0]]
    assert q([entry(desc2d(pkg, offsets=k13[:12]))]) == 1 and q([entry(desc2d(pkg, offsets=k13))]) == 0   # K = 13
    assert q(base + [entry(desc2d(pkg, border=REPLICATE))]) == 0
    assert q(base + [entry(desc2d(pkg, flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT | FLAG_CLAMP01))]) == 0
    assert q(base + [entry(desc2d(pkg, flags=FLAG_HALF_SHIFT | FLAG_CLAMP01))]) == 1        # (an activation of the map alone is fine)
    assert q(base + [entry(desc2d(pkg, flags=FLAG_MASK_F32))]) == 0                         # the labels-in calls derive their own masks
    assert q(base, FLAGS_2D | TGT_ACCUMULATE) == 0 and q(base, 16) == 0                      # flags beyond the three target bits
    # steps
    d = desc2d(pkg, 34, 34, CROSS[:2])
    assert q(base + [entry(d, (1, 544, 544), (1, 16, 16))]) == 1
    assert q(base + [entry(d, (1, 544, 544), (1, 0, 16))]) == 0 and q(base + [entry(d, (1, 544, 544), (0, 16, 16))]) == 0
    assert q(base + [entry(d, (1, 544, 544), (1, -1, 16))]) == 0
    assert q(base + [entry(d, (1, 529, 529), (1, 16, 16))]) == 1                            # (34 - 1) * 16 + 1: the last sample is the last pixel
    assert q(base + [entry(d, (1, 528, 529), (1, 16, 16))]) == 0                            # one row past label_dims
    assert q(base + [entry(d, (1, 529, 528), (1, 16, 16))]) == 0                            # one column past
    d3 = desc3d(pkg, (18, 10, 10))
    assert q([entry(d3, (18, 160, 160), (1, 16, 16))], FLAGS_3D) == 1 and q([entry(d3, (17, 160, 160), (1, 16, 16))], FLAGS_3D) == 0
    # sizes: B * LZ * LY * LX and S * max(D, K) fit int32
    small = desc2d(pkg, 8, 8, CROSS[:2], B=8)
    assert q([entry(small, (1, 16384, 16383), (1, 2, 2))]) == 1 and q([entry(small, (1, 16384, 16384), (1, 2, 2))]) == 0
    assert q([entry(desc3d(pkg, (511, 512, 512), B=1))], FLAGS_3D) == 1 and q([entry(desc3d(pkg, (512, 512, 512), B=1))], FLAGS_3D) == 0
    # an offset beyond int16
    far, near = desc2d(pkg, 8, 40000, [[0, -32769]], B=1), desc2d(pkg, 8, 40000, [[0, -32768]], B=1)
    assert lib.pea_desc_validate(ctypes.byref(far)) == OK
    assert q([entry(near)]) == 1 and q([entry(far)]) == 0
    assert q([entry(desc2d(pkg, 8, 40000, [[0, 32767]], B=1))]) == 1 and q([entry(desc2d(pkg, 8, 40000, [[0, 32768]], B=1))]) == 0


def test_scratch_bytes_hold_one_count_per_image_and_channel(pkg, lib):
    sb = lambda ents, n=None: lib.pea_multi_labels_scratch_bytes(table_of(pkg, ents), len(ents) if n is None else n)
    assert sb(cvppp_steps(pkg)) == 4 * 2 * (8 + 6 + 4 + 2)
    assert sb(cvppp_steps(pkg, B=8)) == 4 * 8 * (8 + 6 + 4 + 2)
    assert sb(cvppp_steps(pkg)[:2]) == 4 * 2 * (8 + 6)
    assert sb(norm1_steps(pkg)) == 4 * 2 * 3 * 4
    assert sb([], 0) == 0 and lib.pea_multi_labels_scratch_bytes(None, 2) == 0


def test_error_codes_are_returned_before_a_launch(pkg, lib):
    """host-only: the pointers are dummies, so anything but an early return would fault"""
    four = cvppp_steps(pkg)
    state = lib.pea_workspace_bytes(ctypes.byref(four[0][0]))
    over = lambda j, **kw: [e if i != j else (e[0], e[1], e[2], kw) for i, e in enumerate(four)]
    # PEA_E_DESC: n out of range, an entry whose descriptor does not validate
    assert call(pkg, lib, four, n=0) == E_DESC
    assert call(pkg, lib, four + [entry(desc2d(pkg))], n=5) == E_DESC
    assert call(pkg, lib, four[:3] + [entry(desc2d(pkg, abi=7))]) == E_DESC
    assert call(pkg, lib, four[:3] + [entry(desc2d(pkg, flags=FLAG_MASK_F32))]) == E_DESC
    # PEA_E_NULL: the table, a descriptor, each required pointer of any entry
    assert lib.pea_affinity_fwd_bwd_labels_multi(None, 4, FLAGS_2D, ctypes.c_void_p(0x100000), 4 * state, ctypes.c_void_p(0x200000), 4096,
                                                 None) == E_NULL
    assert call(pkg, lib, four[:2] + [entry(None)]) == E_NULL
    for field in ("e", "labels", "loss_out", "de"):
        for j in (0, 3):
            assert call(pkg, lib, over(j, **{field: None})) == E_NULL, (field, j)
    # PEA_E_ALIGN: element alignment of every pointer, 8 bytes for the workspace, 4 for the scratch
    for field in ("e", "labels", "wtab", "affs", "loss_out", "dloss", "de"):
        assert call(pkg, lib, over(2, **{field: 0x70002})) == E_ALIGN, field
    assert call(pkg, lib, four, ws=0x100004) == E_ALIGN
    assert call(pkg, lib, four, scratch=0x200002) == E_ALIGN
    # PEA_E_WORKSPACE: missing, or shorter than n states / than the counts
    assert call(pkg, lib, four, ws=None) == E_WORKSPACE
    assert call(pkg, lib, four, ws_bytes=4 * state - 1) == E_WORKSPACE
    assert call(pkg, lib, four, scratch=None) == E_WORKSPACE
    assert call(pkg, lib, four, scratch_bytes=4 * 2 * 20 - 4) == E_WORKSPACE
    # PEA_E_UNSUPPORTED: wherever pea_multi_labels_supported is 0 for a table of valid descriptors
    for bad in (dict(dtype=BF16), dict(D=64), dict(border=REPLICATE), dict(flags=FLAG_LOSS_ACT | FLAG_HALF_SHIFT)):
        assert call(pkg, lib, four[:3] + [entry(desc2d(pkg, **bad))]) == E_UNSUPPORTED, bad
    assert call(pkg, lib, four, flags=FLAGS_2D | TGT_ACCUMULATE) == E_UNSUPPORTED
    d = desc2d(pkg, 34, 34, CROSS[:2])
    assert call(pkg, lib, four[:3] + [entry(d, (1, 544, 544), (1, 0, 16))]) == E_UNSUPPORTED
    assert call(pkg, lib, four[:3] + [entry(d, (1, 528, 529), (1, 16, 16))]) == E_UNSUPPORTED
    # the order: n, descriptor errors, pointer errors, alignment, the workspace, "unsupported"
    bad64 = lambda **kw: [entry(desc2d(pkg, D=64), **kw)]
    assert call(pkg, lib, [entry(desc2d(pkg, abi=7), e=None)]) == E_DESC
    assert call(pkg, lib, bad64(e=None, de=0x60002)) == E_NULL
    assert call(pkg, lib, bad64(de=0x60002), ws=None) == E_ALIGN
    assert call(pkg, lib, bad64(), ws=0x100004, ws_bytes=0) == E_ALIGN
    assert call(pkg, lib, bad64(), ws=None) == E_WORKSPACE
    assert call(pkg, lib, bad64(), scratch=None) == E_WORKSPACE
    assert call(pkg, lib, bad64()) == E_UNSUPPORTED
    # entry 0 is looked at before entry 1
    assert call(pkg, lib, [entry(desc2d(pkg), e=0x10002), entry(desc2d(pkg), e=None)]) == E_ALIGN


def test_sections_keep_their_defaults_and_accept_label_downs_none(pkg):
    for name in ("cvppp_loss_section_from_labels", "ac3ac4_loss_section_from_labels"):
        p = inspect.signature(getattr(pkg, name)).parameters
        assert list(p)[:6] == ["embedding", "emds", "ema_embedding", "labels", "label_downs", "criterion"], name
        assert p["label_downs"].default is None and p["batched"].default is False, name
    p = inspect.signature(pkg.cvppp_loss_section_from_labels).parameters
    assert list(p)[6:8] == ["offsets", "nb_half"] and p["weight_tables"].default is None
    p = inspect.signature(pkg.cvppp_label_weight_tables).parameters
    assert list(p)[:4] == ["labels", "label_downs", "offsets", "nb_half"] and p["label_downs"].default is None
    for name in ("MultiLabelsAffinityMSE", "embedding_loss_from_labels_multi", "embedding_loss_norm1_from_labels_multi"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    p = inspect.signature(pkg.embedding_loss_from_labels_multi).parameters
    assert list(p)[:7] == ["embeddings", "labels", "criterion", "offsets_list", "label_steps", "need_affs", "weight_tables"]
    assert p["label_steps"].default is None and p["need_affs"].default is False and p["weight_tables"].default is None
    p = inspect.signature(pkg.embedding_loss_norm1_from_labels_multi).parameters
    assert list(p)[:5] == ["embeddings", "labels", "criterion", "label_steps", "affs0_weight"] and p["label_steps"].default is None


def test_label_downs_none_needs_sizes_that_divide(pkg):
    """host-only: the check comes before any tensor is looked at on a device (meta tensors carry the shapes)"""
    crit = pkg.WeightedMSE()
    offsets = pkg.multi_offset([1, 3, 5, 9, 27], 4)
    meta = lambda *shape, **kw: torch.empty(shape, device="meta", **kw)
    emb, ema = meta(2, 16, 100, 96), meta(2, 16, 100, 96)
    emds = [meta(2, 16, 50, 48), meta(2, 16, 25, 24), meta(2, 16, 13, 12), meta(2, 16, 7, 6)]  # 100 / 13 does not divide
    labels = meta(2, 100, 96, dtype=torch.int32)
    for batched in (False, True):
        with pytest.raises(ValueError, match="label_downs"):
            pkg.cvppp_loss_section_from_labels(emb, emds, ema, labels, None, crit, offsets, 2, batched=batched)
    with pytest.raises(ValueError, match="label_downs"):
        pkg.cvppp_label_weight_tables(labels, None, offsets, 2)
    emb3, lab3 = meta(2, 16, 4, 30, 48), meta(2, 4, 30, 48, dtype=torch.int32)
    emds3 = [meta(2, 16, 4, 15, 24), meta(2, 16, 4, 8, 12), meta(2, 16, 4, 4, 6), meta(2, 16, 4, 2, 3)]  # 30 / 8
    for batched in (False, True):
        with pytest.raises(ValueError, match="label_downs"):
            pkg.ac3ac4_loss_section_from_labels(emb3, emds3, emb3, lab3, None, crit, embedding_mode=1, batched=batched)
    emds3z = [meta(2, 16, 2, 15, 24)] * 4  # the z extent halves: the provider never does that
    with pytest.raises(ValueError, match="label_downs"):
        pkg.ac3ac4_loss_section_from_labels(emb3, emds3z, emb3, lab3, None, crit, embedding_mode=1)
    with pytest.raises(ValueError):
        pkg.embedding_loss_from_labels_multi(emds, labels, crit, [offsets[:2]] * 4)
    with pytest.raises(ValueError):  # a step that reads past the label image
        pkg.embedding_loss_from_labels_multi(emds[:1], labels, crit, [offsets[:2]], label_steps=[3])
