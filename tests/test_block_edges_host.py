"""CPU: what the host-only planner queries answer on either side of the 2 GiB block limit (csrc/pea_plan.h:33-43, pea_xdma.h:997-998,
pea_k_box.hip:82, pea_box.h:350): the shapes of tests/test_gpu_block_edges.py, four columns apart, without a device.  A guard that is
off by one plane, multiplies by the storage type's size instead of 4, or is skipped by a family shows here first; the GPU file then
holds the kernels to their results on both sides.

  pea_cross_supported       1 under the limit in the modes the shape is meant for, 0 at it, in every mode
  pea_labels_scratch_bytes  (K + 1) * S * 4 bytes (rounded up to 16) under it: the two-launch labels-in step runs; 0 at it
  pea_infer_stitch_supported, pea_multi_supported   1 on both sides: gathers through 64-bit pointers, limited by 2^31 ELEMENTS of a
                            tensor (pea_multi_common.h), not by the block's bytes"""
import ctypes

import pytest
import torch

BBBC = [1, 3, 5, 9, 11]


def query(pkg, spec, shape, dtype=torch.float32):
    """-> (cross answers in modes 0 .. 5, labels scratch bytes, infer-stitch answer, one-entry multi answer)"""
    op, L = pkg.affinity_op, pkg._lib.lib()
    L.pea_labels_scratch_bytes.restype = ctypes.c_size_t
    d = op._build_desc(spec, torch.empty(shape, device="meta", dtype=dtype), 0, 0, 0)
    arr = (ctypes.POINTER(pkg._lib.PeaDesc) * 1)(ctypes.pointer(d))
    return ([int(L.pea_cross_supported(ctypes.byref(d), m)) for m in range(6)], int(L.pea_labels_scratch_bytes(ctypes.byref(d))),
            int(L.pea_infer_stitch_supported(ctypes.byref(d), 1)), int(L.pea_multi_supported(arr, 1)))


def spec_2d(pkg, offsets):
    return pkg.AffinitySpec(2, offsets, None, pkg._lib.BORDER_CIRCULAR, pkg._lib.NORM_BX)


# (D, under shape, at shape, the cross modes that answer 1 under the limit)
F32_2D = [(16, (4096, 8188), (4096, 8192), (0, 1, 2, 5)), (32, (4096, 4092), (4096, 4096), (0, 1, 2, 3, 4))]


@pytest.mark.parametrize("D,under,at,modes", F32_2D, ids=["d16", "d32"])
def test_2d_f32_d_block(pkg, D, under, at, modes):
    pkg.build()
    spec = spec_2d(pkg, pkg.multi_offset(BBBC, 4))
    S = under[0] * under[1]
    assert D * S * 4 < 2 ** 31 and D * at[0] * at[1] * 4 == 2 ** 31
    cross, scratch, _, multi = query(pkg, spec, (1, D) + under)
    assert cross == [1 if m in modes else 0 for m in range(6)] and multi == 1
    assert scratch == (((10 + 1) * S * 4 + 15) & ~15)
    cross, scratch, _, multi = query(pkg, spec, (1, D) + at)
    assert cross == [0] * 6 and scratch == 0 and multi == 1
    # the guard counts one batch item: a batch of the largest accepted item is served
    assert query(pkg, spec, (3, D) + under)[0] == [1 if m in modes else 0 for m in range(6)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_2d_16bit_d64_block_counts_four_bytes(pkg, dtype):
    pkg.build()
    spec = spec_2d(pkg, pkg.multi_offset([1, 3, 5, 9, 27], 4)[:8])
    served = [1, 1, 1, 1, 1, 0]
    assert query(pkg, spec, (1, 64, 2048, 4088), dtype)[0] == served      # 64 * S * 4 = 2^31 - 2^22: the largest block with X % 8 == 0
    assert query(pkg, spec, (1, 64, 2048, 4092), dtype)[0] == [0] * 6     # rows of whole 8-element quads only
    assert query(pkg, spec, (1, 64, 2048, 4096), dtype)[0] == [0] * 6     # 64 * S * 4 = 2^31 although the tensor is 1 GiB
    assert query(pkg, spec, (1, 64, 2048, 4092), torch.float32)[0] == served and query(pkg, spec, (1, 64, 2048, 4096), torch.float32)[0] == [0] * 6


def test_3d_d16_block(pkg):
    pkg.build()
    ao = pkg.utils.affinity_ours
    offs = [list(o) for o in ao.axis_offsets_3d(ao.NORM5_SHIFTS)]
    spec = pkg.AffinitySpec(3, offs, None, pkg._lib.BORDER_CROP_ZERO, pkg._lib.NORM_CROPPED)
    cross, _, stitch, multi = query(pkg, spec, (1, 16, 32, 1024, 1020))
    assert cross == [1, 1, 1, 1, 0, 0] and stitch == 1 and multi == 1
    cross, _, stitch, multi = query(pkg, spec, (1, 16, 32, 1024, 1024))
    assert cross == [0] * 6 and stitch == 1 and multi == 1
