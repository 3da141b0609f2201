"""CPU: what pea_cross_supported answers, in modes 0 .. 5, for the axis-aligned stencils of tests/cross_stencils.py at the D, storage
type and border combinations tests/test_gpu_cross_stencils.py runs them at.  The GPU file asserts the same table before each case, so
"the cross family served this call" is a checked fact there and every refusal a deliberate one.

The table (cross_stencils.EXPECT) was derived from plan_xdma, fwd_self, bwd_self, bwd_hq and xdma_cross_supported before it was run;
the arithmetic is in that module's docstring.  Where the library answered differently on the first run:

    (none: all 73 entries, both borders, agreed)

Two entries are worth a second look, and the library is right in both: x_only / y_only say 1 in mode 5 (pea_affinity_fwd_dual_ex fuses
the pair's FORWARD; the one-launch backward, whose role-A plan refuses an axis without offsets, then returns PEA_E_UNSUPPORTED and the
caller makes two pea_affinity_bwd_ex calls, as include/pea.h prescribes), and two_sw64 under 16-bit storage says 0 in mode 0 but 1 in
mode 1 (the 16-bit forward has 30-unit planes, its backward 52-unit ones): two families in one step, both held to float64 on the GPU.
"""
import ctypes

import pytest

from cross_stencils import ENV, EXPECT, FAMILIES, LABELS_TWO_LAUNCH, PLANE, STENCILS, fill_desc, supported


@pytest.fixture(scope="module")
def lib(pkg):
    pkg.build()
    return pkg._lib.lib()


def _params():
    return [pytest.param(f, s, id="%s-%s" % (f, s)) for f in EXPECT for s in EXPECT[f]]


@pytest.mark.parametrize("family,stencil", _params())
def test_cross_supported_table(pkg, lib, monkeypatch, family, stencil):
    if family in ENV:
        monkeypatch.setenv(*ENV[family])
    borders = (1,) if FAMILIES[family][2][0] > 1 else (0, 1)  # (the 3D cross kernels and the march are CROP_ZERO forms)
    for border in borders:
        got = supported(pkg, fill_desc(pkg, family, stencil, border))
        assert got == EXPECT[family][stencil], "%s %s border %d: pea_cross_supported modes 0..5 = %s, expected %s" % (
            family, stencil, border, got, EXPECT[family][stencil])


def test_the_table_covers_the_issue(pkg):
    """every stencil of the issue's table is pinned at D = 16 / 32 / 64 and in both 16-bit families; every stencil is axis-aligned"""
    for fam in ("f32_16", "f32_32", "f32_64", "f16_32", "bf16_64"):
        assert set(PLANE) <= set(EXPECT[fam]), fam
    for name, offs in STENCILS.items():
        assert all(sum(1 for v in o if v) == 1 for o in offs), name
    assert STENCILS["unsorted"][0] == [0, -27] and STENCILS["unsorted"][-1] == [-1, 0]
    assert STENCILS["dup"][0] == STENCILS["dup"][2]


def test_reach_limit_in_every_mode(pkg, lib):
    """a reach of 32 (= TW) is accepted, 33 refused, whichever axis-aligned offsets come with it; along y the limit is the plane"""
    for fam in ("f32_16", "f32_32", "f16_32"):
        for border in (0, 1):
            assert supported(pkg, fill_desc(pkg, fam, "reach32", border))[:2] == "11"
            assert supported(pkg, fill_desc(pkg, fam, "reach33", border)) == "000000"


def test_two_sided_64_pixel_strips_need_96_columns(pkg, lib):
    """17 .. 32 both ways along x: 64-pixel strip rows, X >= TW + SW = 96; 16 or less: 32-pixel rows, X >= 64"""
    def at(X, stencil):
        d = fill_desc(pkg, "f32_16", stencil, 0)
        d.dims[2] = X
        return supported(pkg, d)[:2]
    assert at(96, "two_sw64") == "11" and at(92, "two_sw64") == "00"
    assert at(64, "two_sw32") == "11" and at(60, "two_sw32") == "00"
    # one-sided forward: one 32-pixel strip whatever the reach; the self backward adds role B, which makes +27 two-sided
    assert at(64, "pos") == "10" and at(96, "pos") == "11"


def test_labels_two_launch_set(pkg, lib):
    """pea_labels_scratch_bytes > 0 exactly where the 30-unit labels-in forward AND the self backward take the stencil"""
    for stencil in EXPECT["f32_16"]:
        sb = lib.pea_labels_scratch_bytes(ctypes.byref(fill_desc(pkg, "f32_16", stencil, 0)))
        assert (sb > 0) == (stencil in LABELS_TWO_LAUNCH), (stencil, sb)


def test_switches_turn_the_family_off(pkg, lib, monkeypatch):
    """PEA_FWD_XDMA=0 / PEA_BWD_XDMA=0 are what makes a refusal observable: every accepted entry turns 0"""
    monkeypatch.setenv("PEA_FWD_XDMA", "0")
    monkeypatch.setenv("PEA_BWD_XDMA", "0")
    for stencil in ("pos", "two_sw64", "dup"):
        assert supported(pkg, fill_desc(pkg, "f32_16", stencil, 0)) == "000000"
