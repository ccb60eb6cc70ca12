"""The comparator of the resident FDR stage (tests/fdr_resident_cases.py) without a GPU: it reproduces what the
reference returned - perform_fdr with fixed probabilities (tests/golden/fdr.npz, ``pf_*``) and FragmentCompetition
(tests/golden/fragcomp.npz) - bit for bit, and on a seeded stand-in table every case of
tests/test_fdr_resident_edges_gpu.py meets its conditions and answers differently once a rule it rests on is
switched to its wrong restatement.  The rules can so be told apart before a GPU is involved."""

from __future__ import annotations

import os

import numpy as np
import pytest

import fdr_resident_cases as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("competitive", [False, True])
def test_no_cycle_path_reproduces_the_reference(competitive):
    """q-values -> best row per group -> q-values on the reference's own table: its precursor_idx / qval / proba."""
    g = np.load(os.path.join(GOLDEN, "fdr.npz"), allow_pickle=False)
    decoy = g["pf_decoy"]
    n = len(decoy)
    rows = np.concatenate([np.flatnonzero(decoy == 0), np.flatnonzero(decoy == 1)])  # staging order
    pidx = np.arange(n)
    ga, gb = (g["pf_elution_group_idx"], np.zeros(n, np.int64)) if competitive else (pidx, None)
    nothing = [np.zeros(0, np.float32)] * n
    exp = F.expected_resident(g["pf_fixed_proba"][rows], decoy[rows], pidx[rows], ga[rows], None if gb is None else gb[rows],
                              np.zeros(n, np.float32), np.zeros(n, np.float32), nothing, rows, None, None)
    tag = "pf_comp" if competitive else "pf_plain"
    np.testing.assert_array_equal(pidx[exp.rows], g[tag + "_precursor_idx"])
    np.testing.assert_array_equal(exp.qval, g[tag + "_qval"])
    np.testing.assert_array_equal(exp.proba, g[tag + "_proba"])
    assert exp.info["n_out"] == len(exp.rows) == (n // 2 if competitive else n) and exp.info["cut"] is None


def test_competition_reproduces_the_reference(oracle_lib):
    """Window of every PSM, processing order and the competition on the reference's FragmentCompetition run: the
    surviving (precursor_idx, rank), in its order.  The golden has ties in proba, PSMs outside every window and PSMs
    without fragment rows (its caveat says how it was drawn)."""
    z = np.load(os.path.join(GOLDEN, "fragcomp.npz"), allow_pickle=False)
    pidx, rank = z["psm_precursor_idx"], z["psm_rank"]
    lists = F.fragment_lists(F.candidate_key(pidx, rank), F.candidate_key(z["frag_precursor_idx"], z["frag_rank"]),
                             z["frag_mz_observed"])
    info = {}
    left = F.compete(np.arange(len(pidx)), z["psm_proba"], pidx, z["psm_mz_observed"], z["psm_rt_observed"], lists,
                     z["cycle"], oracle_lib.fragcomp, 3, 15, info=info)
    np.testing.assert_array_equal(pidx[left], z["surviving_precursor_idx"])
    np.testing.assert_array_equal(rank[left], z["surviving_rank"])
    assert info["removed"] > 0 and info["competing"] + info["no_fragments"] == len(pidx)
    print("[fdr_resident_oracle] fragcomp golden:", info)


def test_window_limits_and_edges():
    """[lower, upper) on float32 m/z promoted to float64; first match; row 0 without a match; extremes over scans."""
    cyc = F.two_scan_cycle()
    lower, upper = F.window_limits(cyc)
    assert np.array_equal(lower[1:], np.arange(400.0, 480.0, 10.0)) and np.array_equal(upper[1:], lower[1:] + 10.0)
    assert np.array_equal(F.window_limits(cyc, scan0_only=True)[1][1:], lower[1:] + 6.0)
    below = np.nextafter(np.float32(410.0), np.float32(0.0))
    mz = np.array([400.0, below, 410.0, 479.99, 480.0, 399.99, 407.0], dtype=np.float32)
    assert F.window_of(mz, cyc).tolist() == [1, 1, 2, 8, 0, 0, 1]
    assert F.window_of(mz, cyc, scan0_only=True).tolist() == [1, 0, 2, 0, 0, 0, 0]
    # 430.1 as float32 is 430.100006...: above a float64 limit of 430.1, which a comparison in float32 would miss
    edge = F.cycle_of([(-1.0, -1.0), (400.0, 430.1), (430.1, 480.0)])
    assert F.window_of(np.array([430.1], np.float32), edge).tolist() == [2]
    over = F.overlapping_cycle()
    mz = np.array([405.0, 415.0, 425.0, 445.0, 472.0, 485.0], np.float32)
    assert F.window_of(mz, over).tolist() == [1, 1, 1, 2, 4, 0]
    assert F.window_of(mz, over, last=True).tolist() == [1, 5, 2, 3, 6, 6]
    assert F.window_hits(np.array([435.0, 445.0, 455.0], np.float32), F.uncovered_cycle()).any(axis=1).tolist() == [False, False, True]


def test_planted_levels_on_the_host():
    """The levels give distinct increasing float32 probabilities with exact ends, as the GPU test asserts of the
    device's read-back."""
    levels = np.repeat(np.asarray(F.LEVELS, np.float32), 3)
    proba = F.stand_in_proba(levels)
    assert proba[0] == 0.0 and proba[-1] == 1.0 and proba.dtype == np.float32
    F.check_planted(levels, proba)
    with pytest.raises(AssertionError):
        F.check_planted(levels, proba[::-1].copy())
    params, rm, rv = F.planted_state()
    assert params.shape == (6,) and rm.shape == rv.shape == (1,)


@pytest.fixture(scope="module")
def stand_in(oracle_lib):
    table = F.stand_in_table(seed=3)
    return table, F.make_cases(table, seed=5)


def test_stand_in_cases_cover_the_list(stand_in):
    """The case list holds what the stage is to be tested on, every switch is some case's, names are unique."""
    table, cases = stand_in
    names = [c.name for c in cases]
    assert tuple(names) == F.CASE_NAMES and len(set(names)) == len(names)
    assert {s for c in cases for s in c.switches} == set(F.SWITCHES)
    assert all(c.switches for c in cases)
    for c in cases:
        assert 200 < len(c.planted) < 2500 and len(c.planted) == len(table.valid)


def test_every_case_meets_its_conditions_and_every_switch_changes_its_answer(stand_in, oracle_lib):
    """On the stand-in table: the conditions that make a case count hold, and the comparator with a case's switch on
    gives another answer than without it."""
    table, cases = stand_in
    for case in cases:
        rows, _ = F.staged(table, case)
        proba = F.stand_in_proba(case.planted[rows])
        exp = F.evaluate(table, case, proba, oracle_lib.fragcomp, with_chains="chain_able" in case.needs)
        info = F.figures(table, case, proba, exp)
        assert not F.unmet(case, info), (case.name, F.unmet(case, info), info)
        assert F.same(exp, F.evaluate(table, case, proba, oracle_lib.fragcomp)), case.name  # deterministic
        for switch in case.switches:
            other = F.evaluate(table, case, proba, oracle_lib.fragcomp, switches=[switch])
            assert not F.same(exp, other), (case.name, switch)


def test_order_decides_the_stand_in_competition(stand_in, oracle_lib):
    """The stand-in competition has real chains: survivors that a removed row would have removed."""
    table, cases = stand_in
    case = next(c for c in cases if c.name == "ties")
    rows, _ = F.staged(table, case)
    exp = F.evaluate(table, case, F.stand_in_proba(case.planted[rows]), oracle_lib.fragcomp, with_chains=True)
    assert exp.info["chain_spared"] > 0 and exp.info["no_fragments"] > 0
