"""Ion-mobility candidates whose tile does not fit the LDS of a CU: the inputs of tests/test_im_oversize_gpu.py meet
their conditions with the ORACLE alone (no GPU), and the rules of the dynamic route (own layout, launch group, spill
layout and spill block, the bound that is left) are restated in tests/box_sweep_im_oversize.py and pinned here.  These
are conditions on inputs and on declarations, not measurements of the kernels."""

import os

import numpy as np
import pytest

import box_sweep_im as bi
import box_sweep_im_oversize as bo
from alphadia_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_restated():
    assert bo.LDS_LIMIT == 161280 and bo.SMALL_LDS == 38784
    # the existing restatement (launch maxima) is the same function wherever K * O >= I
    for shape in ((12, 1, 40, 32, 3), (200, 2, 40, 32, 3), (40, 6, 32, 24, 3), (16, 2, 48, 36, 4), (3, 1, 2, 2, 3)):
        assert bo.layout_bytes(*shape) == bi._layout_bytes(*shape, shape[2] * shape[3]), shape
    # ... and the work region holds the isotope scan sums of a materialised tile where it does not
    assert bo.layout_bytes(1, 1, 40, 32, 3) == bi._layout_bytes(1, 1, 40, 32, 3, 1280) + 2 * 40 * 4
    # the first K refused before
    for O, S, F, k in ((1, 40, 32, 180), (2, 40, 32, 94), (2, 24, 20, 143), (3, 32, 24, 79), (6, 32, 24, 39), (6, 48, 36, 27)):
        assert bo.layout_bytes(k - 1, O, S, F, 3) <= bo.LDS_LIMIT < bo.layout_bytes(k, O, S, F, 3), (O, S, F, k)
    # the spill layout: 221 bytes per kept fragment at two observations, nothing in K * (S + F)
    assert bo.layout_bytes(300, 2, 40, 32, 3, spill=True) == 78872
    assert bo.layout_bytes(200, 6, 48, 36, 3, spill=True) == 146544
    assert bo.layout_bytes(1300, 2, 40, 32, 3, True) - bo.layout_bytes(300, 2, 40, 32, 3, True) == pytest.approx(221 * 1000, abs=16)
    assert bo.layout_bytes(300, 2, 48, 36, 3, True) - bo.layout_bytes(300, 2, 2, 2, 3, True) < 16 * 1024
    # what the spill layout leaves out is the spill block, but for the template that stays in R1
    for K, O, S, F in ((200, 2, 40, 32), (200, 6, 48, 36), (300, 2, 40, 32), (17, 1, 5, 7), (40, 6, 32, 24)):
        floats = K * O * max(S, F) + 2 * K * O * (S + F)
        assert 0 <= bo.spill_block_bytes(K, O, S, F, 3) - floats * 4 < 32
        diff = bo.layout_bytes(K, O, S, F, 3) - bo.layout_bytes(K, O, S, F, 3, spill=True)
        assert abs(diff - (floats - min(O * S * F, K * O * (S + F))) * 4) <= 8


def test_grouping_rule_restated():
    assert bo.launch_group(12, 1, 40, 32, 3) == (bo.GROUP_SMALL, bo.layout_bytes(12, 1, 40, 32, 3))
    assert bo.launch_group(93, 2, 40, 32, 3) == (bo.GROUP_LARGE, bo.layout_bytes(93, 2, 40, 32, 3))
    assert bo.launch_group(94, 2, 40, 32, 3) == (bo.GROUP_SPILL, bo.layout_bytes(94, 2, 40, 32, 3, spill=True))
    assert bo.launch_group(12, 1, 40, 32, 3, spill_all=True) == (bo.GROUP_SPILL, bo.layout_bytes(12, 1, 40, 32, 3, spill=True))
    # no observation (a candidate that keeps nothing): sized as one
    assert bo.launch_group(12, 0, 40, 32, 3) == bo.launch_group(12, 1, 40, 32, 3)
    # the edge between the LDS groups
    k = max(k for k in range(1, 200) if bo.layout_bytes(k, 2, 24, 20, 3) <= bo.SMALL_LDS)
    assert bo.launch_group(k, 2, 24, 20, 3)[0] == bo.GROUP_SMALL and bo.launch_group(k + 1, 2, 24, 20, 3)[0] == bo.GROUP_LARGE
    # every candidate a fixed layout can take is in the small group: a class on a fixed layout is one run of the plan's order
    assert bo.layout_bytes(bi.COMMON_K, 2, bi.COMMON_S, bi.COMMON_F, 3) <= bo.SMALL_LDS


def test_the_bound_that_is_left():
    for O, S, F in ((1, 40, 32), (2, 40, 32), (2, 2, 2), (6, 48, 36), (6, 32, 24), (8, 64, 36)):
        k = bo.spill_k_max(O, S, F, 3)
        assert bo.launch_group(k, O, S, F, 3)[1] is not None and bo.launch_group(k + 1, O, S, F, 3) == (bo.GROUP_SPILL, None)
    assert bo.spill_k_max(2, 40, 32, 3) >= 300 and bo.spill_k_max(6, 48, 36, 3) >= 200
    assert bo.spill_k_max(6, 48, 36, 3) < bo.spill_k_max(2, 40, 32, 3) < bo.spill_k_max(1, 40, 32, 3)


@pytest.mark.parametrize("name", bo.CONFIG_NAMES)
def test_input_b_holds_the_shapes_it_is_for(oracle_lib, name):
    case, soa, spec = bo.oversize_by_fragments()
    cfg = bo.config_of(name, "B")
    t = bi.shape_table(case, soa, cfg)
    planted = spec["density"].values == ""
    assert (t["nl"].values[planted] == 200).all() and (t["k_cap"].values == t["nl"].values).all()
    valid = bo.oracle_tables(oracle_lib, "B", name)["valid"].astype(bool)
    own = bo.own_layouts(t, 3)
    over = own > bo.LDS_LIMIT
    O = t["O"].values
    assert (valid & over).sum() >= 60 and (valid & over & (O == 1)).sum() >= 10 and (valid & over & (O == 2)).sum() >= 40
    assert (valid & ~over & (t["k_cap"].values == 200)).sum() >= 60
    for rung in bi.DENSE_BY_DESIGN:
        assert (valid & ~over & (spec["density"].values == rung)).any(), rung
    assert bo.own_layouts(t, 3, spill=True).max() <= bo.LDS_LIMIT
    stats, group = bo.expected_stats(case, soa, cfg)
    # (a class whose maxima a fixed layout holds keeps it: the density rows of 12 fragments in small boxes)
    assert np.array_equal(group == bo.GROUP_SPILL, over) and len(spec) - 8 <= stats["candidates"].sum() == (group >= 0).sum()
    assert stats["lds_bytes"][bo.GROUP_SPILL] < 64 * 1024 < stats["lds_bytes"][bo.GROUP_LARGE] <= bo.LDS_LIMIT


def test_input_a_is_refused_for_its_maxima_only():
    case, soa, spec = bo.ragged()
    for name in bo.CONFIG_NAMES:
        cfg = bo.config_of(name, "A")
        t = bi.shape_table(case, soa, cfg)
        assert bo.own_layouts(t, 3).max() <= bo.LDS_LIMIT
        caps = bi.batch_caps(t, np.arange(len(t)), cfg)
        assert bo.layout_bytes(caps["k"], caps["o"], caps["s"], caps["f"], 3) > bo.LDS_LIMIT
        assert bi.feature_lds_bytes(caps) > bo.LDS_LIMIT   # (what the host compared before)
        stats, group = bo.expected_stats(case, soa, cfg)
        assert stats["candidates"][bo.GROUP_SPILL] == 0 and len(spec) - 8 <= stats["candidates"].sum() == (group >= 0).sum()
        assert stats["candidates"][bo.GROUP_SMALL] >= 4 and stats["candidates"][bo.GROUP_LARGE] >= 60


@pytest.mark.parametrize("name", bo.CONFIG_NAMES)
def test_input_c_holds_the_shapes_it_is_for(oracle_lib, name):
    case, soa, spec = bo.oversize_by_observations()
    cfg = bo.config_of(name, "C")
    t = bi.shape_table(case, soa, cfg)
    assert (t["k_cap"].values == 40).all() and {3, 6} <= set(t["O"].values) and t["O"].values.max() == 6
    valid = bo.oracle_tables(oracle_lib, "C", name)["valid"].astype(bool)
    over = bo.own_layouts(t, 3) > bo.LDS_LIMIT
    assert (valid & over & (t["O"].values == 6)).sum() >= 5 and not (over & (t["O"].values != 6)).any()
    assert (valid & ~over).sum() >= 60
    stats, group = bo.expected_stats(case, soa, cfg)
    assert np.array_equal(group == bo.GROUP_SPILL, over)


def test_im_launch_stats_is_declared():
    """In the prototype table (tests/test_abi.py holds it against the header) with its three parameters, its group
    count that of the header, and wrapped by the context (checked without loading the library)."""
    header = open(os.path.join(ROOT, "include", "alphadia_hip.h")).read()
    assert len(_abi.PROTOTYPES["adh_im_launch_stats"][1]) == 3
    src = open(os.path.join(ROOT, "alphadia_amd", "runtime.py")).read()
    assert "#define ADH_IM_LAUNCH_STATS 6" in header and 2 * _abi.N_IM_GROUPS == 6
    assert "def im_launch_stats(self, reset: bool = False)" in src
