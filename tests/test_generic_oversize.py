"""Candidates whose tile does not fit the LDS of a CU: the inputs of tests/test_generic_oversize_gpu.py meet their
conditions with the ORACLE alone (no GPU), and the rules the device plan applies to the generic class (36) are
restated here in Python: the LDS layout of ONE candidate, the launch group it sorts into, the spill layout and the
bound that is left.  These are conditions on inputs and on declarations, not measurements of the kernels.

Input A is the ragged sweep of tests/box_sweep.py scored as ONE batch (no candidate is too large, only the product of
the maxima over the batch); input B is the same generator with 200-fragment slices at every cycle count (``oversize_sweep``).

The figures of B, by cycle count F of its 200-fragment, two-observation rows (9 rows per F: 3 centres x 3 positions),
with three isotopes: F = 22: 153 192 bytes, F = 23: 158 888, F = 24: 164 592 ... F = 36: 232 992.  The rows of F = 22
and 23 (18) sit just under the limit and the 117 rows of F = 24 ... 36 above it.  The issue behind these tests also asks
for "at least 10 rows within 6 KiB below the limit"; the layout grows by 5 700 bytes per cycle, so exactly the 9 rows of
F = 23 can lie within 6 KiB of any limit between 158 888 and 164 591 bytes.  The test below pins the 9 and the 18."""

import functools
import os

import numpy as np
import pytest

import box_sweep as bs
import helpers as H
from alphadia_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- adh_feature_layout.h, restated ---------------------------------------------------------------------------
CU_LDS = 160 * 1024
STATIC_LDS = 2 * 16 * 17 * 4            # gram / redm of the generic kernel's MFMA contraction
LDS_LIMIT = CU_LDS - STATIC_LDS         # dynamic LDS a block of the generic kernel may ask for
SMALL_LDS = 40 * 1024 - STATIC_LDS      # edge between the two LDS groups
GROUP_SMALL, GROUP_LARGE, GROUP_SPILL = 0, 1, 2

CONFIG_NAMES = ("all_fragments", "no_xic_all_fragments", "all_fragments_best")


def layout_bytes(K, O, F, I, spill=False):
    """feat::Layout(feat::own_caps(K, O, F, I), spill).bytes(): the [K][O][F] planes fi, fm, ffp and bp[K][F] are
    left out of the spill layout."""
    K, O, F, I = int(K), int(O), int(F), int(I)
    n_double = O * 2 * F + 2 * F + I * O + 2 * K * O + 4 * K + 2 * O + 2 * I
    n_float = (0 if spill else 3 * K * O * F + K * F) + 2 * I * F + 2 * O * F + 6 * K + 3 * K * O + 4 * O + 3 * I + 3 * F + 46
    n_int = 3 * K + K * O + O
    return n_double * 8 + (n_float * 4 + 7) // 8 * 8 + (n_int * 4 + 7) // 8 * 8 + (5 * K + 7) // 8 * 8


def spill_block_bytes(K, O, F):
    K, O, F = int(K), int(O), int(F)
    return ((3 * K * O * F + K * F) * 4 + 31) // 32 * 32


def launch_group(K, O, F, I, spill_all=False):
    """(group, dynamic LDS) of one generic candidate, or (GROUP_SPILL, None) beyond the bound that is left."""
    own = layout_bytes(K, O, F, I)
    if own <= LDS_LIMIT and not spill_all:
        return (GROUP_SMALL if own <= SMALL_LDS else GROUP_LARGE), own
    sp = layout_bytes(K, O, F, I, spill=True)
    return GROUP_SPILL, (sp if sp <= LDS_LIMIT else None)


def own_layouts(table, I):
    return np.array([layout_bytes(k, o, f, I) for k, o, f in zip(table["k_cap"], table["O"], table["F"])], dtype=np.int64)


def expected_stats(case, soa, cfg, spill_all=False, **switches):
    """What Context.generic_launch_stats() must report after ONE plan over ``soa``, and the group of every row
    (-1: not in the generic class).  Rows flagged to be skipped sit in the first group and ask for no LDS."""
    t = bs.shape_table(case, soa, cfg)
    I = min(int(cfg.top_k_isotopes), 4)
    classes = bs.classes_of(case, soa, cfg, **switches)
    flags = np.asarray(soa.get("flags", np.zeros(len(classes), np.uint8)))
    group = np.full(len(classes), -1, dtype=np.int64)
    cand, lds = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for r in np.flatnonzero(classes == bs.CLASS_GENERIC):
        g, need = (GROUP_SMALL, 0) if flags[r] & 1 else launch_group(t["k_cap"][r], t["O"][r], t["F"][r], I, spill_all)
        assert need is not None, r
        group[r] = g
        cand[g] += 1
        lds[g] = max(lds[g], need)
    return {"candidates": cand, "lds_bytes": lds}, group


def spill_k_max(O, F, I):
    """The bound that is left: the most fragments a candidate of O observations and F cycles may keep."""
    k = 1
    while layout_bytes(k + 1, O, F, I, spill=True) <= LDS_LIMIT:
        k += 1
    return k


# ---- the inputs ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ragged_sweep():
    """Input A: (case, assembled table, specification)."""
    case = bs.sweep_case(True)
    return case, H.soa_for(case, bs.config_of("defaults")), bs.spec_rows(True)


@functools.lru_cache(maxsize=None)
def oversize_sweep():
    """Input B: the ragged sweep with 200-fragment slices at every cycle count.  The two module attributes are put
    back before this returns: other modules build their sweeps from them."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(bs, "NL_ALL", (200,) * 18)
        mp.setattr(bs, "NL_LONG_FMAX", 36)
        case = bs.sweep_case(True)
        spec = bs.spec_rows(True)
    assert bs.NL_ALL[0] == 1 and bs.NL_LONG_FMAX == 16
    return case, H.soa_for(case, bs.config_of("defaults")), spec


_oracle_cache = {}


def oracle_tables(oracle_lib, which, name):
    """The oracle's tables of input ``which`` ("A" / "B") under a configuration: computed once, never written to."""
    if (which, name) not in _oracle_cache:
        case, soa, _ = ragged_sweep() if which == "A" else oversize_sweep()
        _oracle_cache[which, name] = H.oracle_score(oracle_lib, case, bs.config_of(name), soa=soa, n_threads=4, with_stats=True)[0]
    return _oracle_cache[which, name]


# ---- tests --------------------------------------------------------------------------------------------------

def test_layout_restated():
    assert STATIC_LDS == 2176 and LDS_LIMIT == 161664 and SMALL_LDS == 38784
    # the maxima of a chunk with one 200-fragment candidate in 16 cycles and one 20-fragment one in 36
    assert layout_bytes(200, 2, 36, 3) == 232992 and layout_bytes(200, 2, 16, 3) < CU_LDS and layout_bytes(20, 2, 36, 3) < CU_LDS
    assert layout_bytes(200, 2, 24, 3) == 164592 and layout_bytes(200, 2, 23, 3) == 158888
    # the existing restatement (maxima) is the same function
    from test_kernel_classes import _feature_lds_bytes
    for shape in ((12, 1, 8, 3), (200, 2, 36, 4), (65, 2, 33, 1), (1, 1, 2, 3)):
        assert layout_bytes(*shape) == _feature_lds_bytes(*shape)
    # what the spill layout leaves out is the spill block, to its 32-byte rounding and the layout's 8-byte ones
    for K, O, F in ((200, 2, 24), (200, 2, 36), (17, 1, 5), (1170, 2, 8)):
        diff = layout_bytes(K, O, F, 3) - layout_bytes(K, O, F, 3, spill=True)
        assert abs(diff - (3 * K * O * F + K * F) * 4) <= 8 and 0 <= spill_block_bytes(K, O, F) - (3 * K * O * F + K * F) * 4 < 32
    # the spill layout: 32 bytes per (fragment, observation) pair and 73 per fragment, nothing in K * F
    assert layout_bytes(1001, 2, 8, 3, True) - layout_bytes(1, 2, 8, 3, True) == pytest.approx(1000 * (2 * 32 + 73), abs=16)
    assert layout_bytes(1000, 2, 36, 3, True) - layout_bytes(1000, 2, 8, 3, True) < 4096


def test_grouping_rule_restated():
    assert launch_group(12, 1, 8, 3) == (GROUP_SMALL, layout_bytes(12, 1, 8, 3))
    assert launch_group(200, 2, 23, 3) == (GROUP_LARGE, 158888)
    assert launch_group(200, 2, 24, 3) == (GROUP_SPILL, layout_bytes(200, 2, 24, 3, spill=True))
    assert launch_group(12, 1, 8, 3, spill_all=True) == (GROUP_SPILL, layout_bytes(12, 1, 8, 3, spill=True))
    # the edge between the LDS groups
    k = max(k for k in range(1, 200) if layout_bytes(k, 2, 16, 3) <= SMALL_LDS)
    assert launch_group(k, 2, 16, 3)[0] == GROUP_SMALL and launch_group(k + 1, 2, 16, 3)[0] == GROUP_LARGE
    # the bound that is left
    for O, F in ((2, 8), (2, 36), (1, 8)):
        k = spill_k_max(O, F, 3)
        assert launch_group(k, O, F, 3)[1] is not None and launch_group(k + 1, O, F, 3) == (GROUP_SPILL, None)
    assert spill_k_max(2, 8, 3) == 1171 and 1100 < spill_k_max(2, 36, 3) < 1171 < spill_k_max(1, 8, 3)


def test_input_a_is_refused_for_its_maxima_only():
    case, soa, spec = ragged_sweep()
    assert len(spec) == 1386
    for name in CONFIG_NAMES:
        cfg = bs.config_of(name)
        t = bs.shape_table(case, soa, cfg)
        own = own_layouts(t, 3)
        assert own.max() == 141392 <= LDS_LIMIT
        assert layout_bytes(t["k_cap"].max(), t["O"].max(), t["F"].max(), 3) == 232992 > CU_LDS
        stats, group = expected_stats(case, soa, cfg, no_fast=True)
        assert stats["candidates"][GROUP_SPILL] == 0 and stats["candidates"].sum() == 1386
        assert stats["candidates"][GROUP_SMALL] >= 100 and stats["candidates"][GROUP_LARGE] >= 100
        assert stats["lds_bytes"][GROUP_LARGE] == 141392 and stats["lds_bytes"][GROUP_SMALL] <= SMALL_LDS


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_input_b_holds_the_shapes_it_is_for(oracle_lib, name):
    case, soa, spec = oversize_sweep()
    cfg = bs.config_of(name)
    assert len(spec) == 1386 and (spec["nl"].values[:630] == 200).all()
    t = bs.shape_table(case, soa, cfg)
    assert np.array_equal(t["F"], spec["F"]) and np.array_equal(t["O"], spec["O"]) and np.array_equal(t["nl"], spec["nl"])
    exp = oracle_tables(oracle_lib, "B", name)
    assert exp["valid"].astype(bool).all()
    own = own_layouts(t, 3)
    over = own > LDS_LIMIT
    assert np.array_equal(over, own > CU_LDS)  # (no row of the input between the two readings of "the LDS of a CU")
    assert over.sum() == 117 >= 100 and own[over].min() == 164592
    assert set(t["F"][over]) == set(range(24, 37)) and set(t["O"][over]) == {2} and set(t["k_cap"][over]) == {200}
    assert {0, 1, 2} == set(spec["centre"][over]) == set(spec["position"][over])
    L = case.dia.cycle_len
    assert (soa["frame_stop"][over] % L != 0).any()  # clipped boxes among them
    # just under: the 18 rows of F = 22 and 23 (module docstring), the 9 of F = 23 within 6 KiB
    under = ~over & (own > LDS_LIMIT - 2 * 5700)
    assert under.sum() == 18 and set(t["F"][under]) == {22, 23} and own[~over].max() == 158888
    assert (~over & (own > LDS_LIMIT - 6 * 1024)).sum() == 9
    stats, group = expected_stats(case, soa, cfg, no_fast=True)
    assert stats["candidates"][GROUP_SPILL] == 117 and (group[under] == GROUP_LARGE).all()
    assert stats["lds_bytes"][GROUP_SPILL] == layout_bytes(200, 2, 36, 3, spill=True) < 32 * 1024


def test_generic_launch_stats_is_declared():
    """In the prototype table (tests/test_abi.py holds it against the header) with its three parameters, its group
    count that of the header, and wrapped by the context (checked without loading the library)."""
    header = open(os.path.join(ROOT, "include", "alphadia_hip.h")).read()
    assert len(_abi.PROTOTYPES["adh_generic_launch_stats"][1]) == 3
    src = open(os.path.join(ROOT, "alphadia_amd", "runtime.py")).read()
    assert "#define ADH_GENERIC_LAUNCH_STATS 6" in header and 2 * _abi.N_GENERIC_GROUPS == 6
    assert "def generic_launch_stats(self, reset: bool = False)" in src
