"""The resident FDR stage (``adh_fdr_resident``, alphadia_amd/csrc/adh_fdr_device.hip) with planted probabilities
at its edges, against a comparator that runs no kernel of this project (tests/fdr_resident_cases.py: NumPy,
oracle/fdr_oracle.py and the CPU fragment competition; pinned to the reference's goldens in
tests/test_fdr_resident_oracle.py).

One scoring call per module leaves its tables in HBM: a few hundred precursors, two candidates each, a third of
the candidate rows once or twice more under the next ranks with the same frame limits, so that the competition has
rows that share every fragment.  Nothing here scores again.  The probabilities do not come from a trained network:
the classifier's one column is an extra column of the host (a level per table row, NaN keeps a row out of the
stage, as dropna does) and the network - BatchNorm1d(1) and Linear(1, 2), its state set by hand - turns it into a
strictly increasing probability, exactly 0.0 and 1.0 at the extreme levels.  The staged rows' probabilities are
read back (``predict``) and are the comparator's: what is compared is order and selection, bit for bit - rows in
order, float32 probabilities, float64 q-values (ratios of the same integer counts), count.  No tolerances.

Every case (``fdr_resident_cases.make_cases``) names the rules it rests on; it counts only if the comparator with
such a rule switched to its wrong restatement answers differently on the case's own inputs, and if the figures it
needs (rows in levels with both labels, share of competing rows removed, rows without a window, rows in two
windows, groups whose best rows tie) are there.  Both are asserted, from the comparator's answer alone.  The figures
of every case are printed, one JSON line each, before anything is asserted.
"""

from __future__ import annotations

import json

import numpy as np
import pytest

import fdr_resident_cases as F
import synthetic as syn

pytestmark = pytest.mark.gpu


def _log(record: dict) -> None:
    """One line per case, printed before anything is asserted (pytest -rA shows it for passing tests too)."""
    print("[fdr_resident_edges]", json.dumps(record))


@pytest.fixture(scope="module")
def scored():
    """The one scoring call: ``(ctx, table, cases)``; ``table`` holds per row of the device tables what the
    comparator needs, taken from the frames the call returned."""
    from alphadia_amd import runtime
    from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring, assemble_candidates

    case = syn.make_case(400, 80, config_id=79, per_precursor=2, n_ms2=8, ms1_peaks=400, ms2_peaks=150, mz_lo=400, mz_hi=480,
                         frag_mz_lo=200, frag_mz_hi=350, ms1_mz_range=(395, 500), ms2_mz_range=(195, 355),
                         planted_fraction=1.0, threads=1)
    cands = F.add_copies(case.candidates_df, seed=7)
    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                    experimental_xic=True))
    scorer = HipCandidateScoring(dia_data=case.dia, precursors_flat=case.library.precursor_df,
                                 fragments_flat=case.library.fragment_df, config=cfg, device=0, rt_column="rt_library",
                                 mobility_column="mobility_library", precursor_mz_column="mz_library",
                                 fragment_mz_column="mz_library")
    features_df, fragments_df = scorer(cands, thread_count=1)
    ctx = runtime.get_context(0)
    soa = assemble_candidates(cands, scorer.precursors_flat_df, "mz_library")  # the rows of the device tables, in order
    n = len(soa["precursor_idx"])
    assert n == len(cands) == int(ctx.device_tables().n)
    key = F.candidate_key(soa["precursor_idx"], soa["rank"])
    assert len(np.unique(key)) == n
    by = np.argsort(key)
    at = by[np.searchsorted(key[by], F.candidate_key(features_df["precursor_idx"].to_numpy(), features_df["rank"].to_numpy()))]
    valid = np.zeros(n, dtype=bool)
    valid[at] = True
    assert valid.sum() == len(features_df) and np.array_equal(valid, ctx.table_rows_to_host("valid", 0, n).astype(bool))
    assert features_df["mz_observed"].dtype == features_df["rt_observed"].dtype == np.float32
    mz, rt = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    mz[at], rt[at] = features_df["mz_observed"].to_numpy(), features_df["rt_observed"].to_numpy()
    lists = F.fragment_lists(key, F.candidate_key(fragments_df["precursor_idx"].to_numpy(), fragments_df["rank"].to_numpy()),
                             fragments_df["mz_observed"].to_numpy())
    table = F.Table(valid, soa["precursor_idx"].astype(np.int64), soa["rank"].astype(np.int64),
                    soa["elution_group_idx"].astype(np.int64), soa["decoy"].astype(np.uint8), mz, rt, lists,
                    np.asarray(case.dia.cycle, dtype=np.float64))
    cases = F.make_cases(table, seed=5)
    assert tuple(c.name for c in cases) == F.CASE_NAMES
    _log(dict(table_rows=n, valid=int(valid.sum()), valid_targets=int((valid & (table.decoy == 0)).sum()),
              rows_without_fragments=int(sum(len(lists[r]) == 0 for r in np.flatnonzero(valid))),
              copies=int((table.rank >= 2).sum())))
    return ctx, table, {c.name: c for c in cases}


def _device(ctx, table, case, mlp, **stage_kw):
    """Stage, read the probabilities back, run the stage: ``(proba of the staged rows, (rows, proba, qval))``."""
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    n_t, n_d = mlp.stage_rows_device([len(DEFAULT_FEATURE_COLUMNS)], case.decoy, [case.planted], channel=case.channel,
                                     part=case.part)
    rows, label = F.staged(table, case)
    assert (n_t, n_d) == (int((label == 0).sum()), int((label != 0).sum()))
    assert np.array_equal(mlp.staged_rows(), rows)
    proba = mlp.predict()[:, 1]
    F.check_planted(case.planted[rows], proba)
    mlp.predict_resident()
    kw = {} if case.heuristic == 0.1 else dict(
        fdr_heuristic=case.heuristic(proba, label, case.tiebreak[rows]) if callable(case.heuristic) else case.heuristic)
    kw.update(stage_kw)
    kw.setdefault("tiebreak", case.tiebreak)
    return proba, ctx.fdr_resident(mlp, case.group_a, case.group_b, cycle=case.cycle, **kw)


def _planted_mlp(ctx):
    from alphadia_amd import runtime

    mlp = runtime.DeviceMlp(ctx, 1, [], 2)
    mlp.set_state(*F.planted_state())
    return mlp


def _compare(table, case, proba, got, fragcomp, tag=None):
    """Log the case's figures, then assert its conditions, its switches and the device's answer."""
    exp = F.evaluate(table, case, proba, fragcomp, with_chains="chain_able" in case.needs)
    info = F.figures(table, case, proba, exp)
    changed = {s: not F.same(exp, F.evaluate(table, case, proba, fragcomp, switches=[s])) for s in case.switches}
    rows, p, q = got
    _log(dict(case=case.name if tag is None else f"{case.name} ({tag})", switches=changed, device_n_out=int(len(rows)),
              **{k: v for k, v in info.items() if k != "targets"}))
    assert not F.unmet(case, info), (F.unmet(case, info), info)
    assert case.switches and all(changed.values()), changed
    assert len(rows) == exp.info["n_out"]
    assert np.array_equal(rows, exp.rows)
    assert np.array_equal(q.view(np.uint64), exp.qval.view(np.uint64))
    assert p.dtype == np.float32 and np.array_equal(p.view(np.uint32), exp.proba.view(np.uint32))
    return exp


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_resident_stage_equals_the_comparator(scored, oracle_lib, name):
    ctx, table, cases = scored
    case = cases[name]
    mlp = _planted_mlp(ctx)
    try:
        proba, got = _device(ctx, table, case, mlp)
    finally:
        mlp.close()
    _compare(table, case, proba, got, oracle_lib.fragcomp)


def test_second_call_leaves_nothing_of_the_first(scored, oracle_lib):
    """The same network object and the same tables: all rows, then 257, then one row, then all rows again - every
    answer is the comparator's, and the last is the first's."""
    ctx, table, cases = scored
    mlp = _planted_mlp(ctx)
    try:
        answers = []
        for i, name in enumerate(("ties", "staged-257", "staged-1", "ties")):
            proba, got = _device(ctx, table, cases[name], mlp)
            answers.append(got)
            _compare(table, cases[name], proba, got, oracle_lib.fragcomp, tag=f"call {i + 1} on one object")
    finally:
        mlp.close()
    for a, b in zip(answers[0], answers[3]):
        assert np.array_equal(a, b)
    assert len(answers[1][0]) < 257 and len(answers[2][0]) == 1
    # the tables in HBM are still the ones of the module's scoring call
    assert np.array_equal(ctx.table_rows_to_host("valid", 0, len(table.valid)).astype(bool), table.valid)


def _equal(got, exp) -> bool:
    rows, p, q = got
    return (np.array_equal(rows, exp.rows) and np.array_equal(q.view(np.uint64), exp.qval.view(np.uint64)) and
            np.array_equal(p.view(np.uint32), exp.proba.view(np.uint32)))


def test_stage_without_a_tiebreak_key(scored, oracle_lib):
    """The entry takes no tie-break key as well: ties then fall in (proba, decoy, staging order) in both q-value sorts
    and in (window, proba, q-value order) in the competition - the comparator with both tie-break switches on, which
    answers differently from the keyed stage on this table."""
    ctx, table, cases = scored
    case = cases["ties"]
    mlp = _planted_mlp(ctx)
    try:
        proba, got = _device(ctx, table, case, mlp, tiebreak=None)
    finally:
        mlp.close()
    exp = F.evaluate(table, case, proba, oracle_lib.fragcomp, switches=["no_qvalue_tiebreak", "no_order_tiebreak"])
    assert not F.same(exp, F.evaluate(table, case, proba, oracle_lib.fragcomp))
    assert _equal(got, exp)


@pytest.mark.parametrize("rt_tol, ppm_tol", [(0.0, 15.0), (3.0, 0.0), (0.25, 2.0)])
def test_tolerances_reach_the_competition(scored, oracle_lib, rt_tol, ppm_tol):
    """The two tolerances are arguments of the entry, not constants of the stage: a copy is 0 s and 0 ppm from its
    original, so a tolerance of 0 (the tests are ``<``) removes no row where the defaults remove a quarter, and a
    narrow pair still removes the copies."""
    ctx, table, cases = scored
    case = cases["window-run-cycle"]
    mlp = _planted_mlp(ctx)
    try:
        proba, got = _device(ctx, table, case, mlp, rt_tol_seconds=rt_tol, mass_tol_ppm=ppm_tol)
    finally:
        mlp.close()
    exp = F.evaluate(table, case, proba, oracle_lib.fragcomp, rt_tol_seconds=rt_tol, mass_tol_ppm=ppm_tol)
    usual = F.evaluate(table, case, proba, oracle_lib.fragcomp)
    _log(dict(case=f"{case.name} (rt_tol {rt_tol}, ppm_tol {ppm_tol})", competing=exp.info["competing"],
              removed=exp.info["removed"], removed_with_defaults=usual.info["removed"], device_n_out=int(len(got[0]))))
    assert usual.info["removed"] >= 0.1 * usual.info["competing"]
    if 0.0 in (rt_tol, ppm_tol):
        assert exp.info["removed"] == 0
    else:
        assert 0 < exp.info["removed"] <= usual.info["removed"]
    assert _equal(got, exp)
