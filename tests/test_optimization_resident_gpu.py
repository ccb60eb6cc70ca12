"""Resident optimisation steps on the GPU: batches scored behind each other into the device tables, the FDR stage over
all of them in HBM, and the calibration frames copied back for the survivors only.  Each step must return what the
python branch of OptimizationHandler._process_batch (optimization_handler.py:381-456) returns from the chained calls
and the host frames of the reference's lock, while moving less."""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import synthetic as syn

pytestmark = pytest.mark.gpu

NAMES = SimpleNamespace(get_rt_column=lambda: "rt_calibrated", get_mobility_column=lambda: "mobility_library",
                        get_precursor_mz_column=lambda: "mz_calibrated", get_fragment_mz_column=lambda: "mz_calibrated")
CLASSIFIER = dict(test_size=0.2, batch_size=500, learning_rate=0.001, epochs=4, random_state=11)
CONFIG = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                     "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
          "general": {"thread_count": 4},
          "fdr": {"fdr": 0.01, "competitive_scoring": True, "channel_wise_fdr": False},
          "calibration": {"optimization_lock_target": 10**9, "batch_size": 400, "min_correlation": 0.5,
                          "max_fragments": 5000}}


@pytest.fixture(scope="module")
def case():
    c = syn.make_case(5000, 260, config_id=78, per_precursor=2, planted_fraction=0.5, threads=4)
    pre, frag = c.library.precursor_df, c.library.fragment_df
    pre["mz_calibrated"] = pre["mz_library"]
    pre["rt_calibrated"] = pre["rt_library"]
    frag["mz_calibrated"] = frag["mz_library"]
    return c


class _Calibration:
    """Stands in for the calibration manager: every call shifts the calibrated columns a little more."""

    def __init__(self):
        self.calls = 0

    def predict(self, df, group):
        self.calls += 1
        k = self.calls
        if group == "precursor":
            df["mz_calibrated"] = df["mz_library"] * (1 + 1e-6 * k)
            df["rt_calibrated"] = df["rt_library"] + 0.5 * k
        else:
            df["mz_calibrated"] = (df["mz_library"] * (1 + 2e-6 * k)).astype(df["mz_library"].dtype)


def _features():
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    return [c for c in DEFAULT_FEATURE_COLUMNS if c not in ("mobility_observed", "base_width_mobility")] + [
        "delta_rt", "mz_library", "charge", "n_K", "n_R", "n_P"]


def _manager(dia, seed=7):
    from alphadia_amd import fdr

    return fdr.HipFDRManager(_features(), fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=dia.cycle,
                             random_state=seed, device=0)


def _handler(candidates_df, manager):
    from alphadia_amd.extraction_handler import HipExtractionHandler

    opt = SimpleNamespace(ms1_error=10, ms2_error=15, rt_error=30.0, mobility_error=0.1, num_candidates=2, fwhm_rt=5.0,
                          fwhm_mobility=0.01, score_cutoff=0.0, classifier_version=-1)
    reporter = SimpleNamespace(log_string=lambda msg, **k: None)
    # the case's candidates of the batch library's precursors stand in for the selection step
    selection = SimpleNamespace(select_candidates=lambda dia, lib, apply_cutoff=False: candidates_df[
        candidates_df["precursor_idx"].isin(lib.precursor_df["precursor_idx"])])
    return HipExtractionHandler(CONFIG, opt, manager, reporter, NAMES, selection_handler=selection, device=0)


def _assert_same(got: pd.DataFrame, exp: pd.DataFrame, what: str, dtypes: bool = True):
    got, exp = got.reset_index(drop=True), exp.reset_index(drop=True)
    assert list(got.columns) == list(exp.columns), what
    assert len(got) == len(exp), (what, len(got), len(exp))
    for c in exp.columns:
        a, b = got[c], exp[c]
        assert a.dtype == b.dtype or not dtypes, (what, c, a.dtype, b.dtype)
        if c == "proba":  # (the bounds of tests/test_fdr_resident.py)
            assert np.allclose(a.to_numpy(), b.to_numpy(), rtol=0, atol=1e-6), (what, c)
        elif c == "qval":
            assert np.allclose(a.to_numpy(), b.to_numpy(), rtol=1e-12, atol=0), (what, c)
        elif a.dtype == object:
            assert (a.to_numpy() == b.to_numpy()).all(), (what, c)
        else:
            assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True), (what, c)


def _scorer(case, top_k=12, precursors=None):
    from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring

    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                    experimental_xic=True, top_k_fragments=top_k))
    return HipCandidateScoring(dia_data=case.dia,
                               precursors_flat=case.library.precursor_df if precursors is None else precursors,
                               fragments_flat=case.library.fragment_df, config=cfg, device=0, rt_column="rt_library",
                               mobility_column="mobility_library", precursor_mz_column="mz_library",
                               fragment_mz_column="mz_library")


def _rows_by_key(tables):
    key = tables["precursor_idx"].astype(np.int64) * 256 + tables["rank"].astype(np.int64)
    assert len(np.unique(key)) == len(key)
    return np.argsort(key, kind="stable")


def test_append_equals_one_resident_call(case):
    """A then B appended (B with longer library slices: the tables widen and the rows of A move) hold, row for row
    and byte for byte, what one resident call over A and B leaves; a reset empties the tables."""
    from alphadia_amd import runtime
    from alphadia_amd.scoring import AccumulatedScores

    ctx = runtime.get_context(0)
    # every other precursor with a library slice of 5 fragments instead of 12: A holds those, B the others
    pre = case.library.precursor_df.copy()
    short = (pre["precursor_idx"] % 2 == 0).to_numpy()
    pre.loc[short, "flat_frag_stop_idx"] = pre.loc[short, "flat_frag_start_idx"] + 5
    scorer = _scorer(case, top_k=12, precursors=pre)
    in_a = (case.candidates_df["precursor_idx"] % 2 == 0).to_numpy()
    a, b = case.candidates_df[in_a], case.candidates_df[~in_a]
    assert len(a) > 1000 and len(b) > 1000
    acc = AccumulatedScores(0)
    assert acc.append(scorer, a) == 0
    width_a = int(ctx.device_tables().top_k)
    assert acc.append(scorer, b) == acc.batches[0].n_table
    width = int(ctx.device_tables().top_k)
    assert (width_a, width) == (5, 12)
    got = ctx.device_tables_to_host()
    assert int(ctx.device_tables().n) == len(a) + len(b)
    n_valid, n_slots = acc.counts()
    scorer.score_resident(pd.concat([a, b]))
    exp = ctx.device_tables_to_host()
    assert int(ctx.device_tables().top_k) == width
    ga, ea = _rows_by_key(got), _rows_by_key(exp)
    assert set(got) == set(exp)
    for name in exp:
        assert got[name].shape == exp[name].shape, name
        assert got[name][ga].tobytes() == exp[name][ea].tobytes(), name
    assert n_valid == int(exp["valid"].sum()) and n_valid > 500
    assert n_slots == int((exp["fragment_lib_slot"][exp["valid"].astype(bool)] > 0).sum())
    # a reset empties the accumulated tables; the next append starts at row 0 again
    acc = AccumulatedScores(0)
    assert int(ctx.device_tables().n) == 0
    assert acc.append(scorer, b) == 0 and int(ctx.device_tables().n) == len(b)
    # wide, narrow, wide: the narrow batch lands behind 12-slot rows (zeroed slots from row first_a on, through the
    # relayout kernel), and both later batches outgrow the capacity with the width unchanged (one copy per column)
    b1, b2 = b.iloc[: len(b) // 2], b.iloc[len(b) // 2:]
    acc = AccumulatedScores(0)
    assert acc.append(scorer, b1) == 0
    first_a = acc.append(scorer, a)
    assert first_a == len(b1) and acc.append(scorer, b2) == len(b1) + len(a)
    assert int(ctx.device_tables().top_k) == 12
    got = ctx.device_tables_to_host()
    ga = _rows_by_key(got)
    for name in exp:
        assert got[name].shape == exp[name].shape, name
        assert got[name][ga].tobytes() == exp[name][ea].tobytes(), name
    assert (got["fragment_lib_slot"][first_a: first_a + len(a), 5:] == 0).all()
    assert np.array_equal(acc.valid(first_a, first_a + len(a)), got["valid"][first_a: first_a + len(a)].astype(bool))


def _sequence(case, resident: bool):
    """Grow (target not reached), recalibrate, accumulate a second batch and reach the target, then shrink after
    the reset with another recalibration: per step the psm frame, the calibration frames, the lock's frames and
    the batch index, and the bytes copied device -> host."""
    from alphadia_amd import runtime
    from alphadia_amd.optimization import HipOptimizationLock

    ctx = runtime.get_context(0)
    manager = _manager(case.dia)
    handler = _handler(case.candidates_df, manager)
    lib = SimpleNamespace(_precursor_df=case.library.precursor_df.copy(), _fragment_df=case.library.fragment_df.copy())
    lock = HipOptimizationLock(lib, CONFIG, device=0)
    calibration = _Calibration()
    if not resident:  # the chained calls, as for channel-wise FDR
        handler.resident_refusal = lambda: "chained reference"
    steps = []
    ctx.d2h_bytes(reset=True)
    for i in range(3):
        if i == 1:
            lock._precursor_target_count = 1  # (reached at the second step)
        psm = handler.process_optimization_batch(case.dia, lock)
        step = {"batch_idx": lock.batch_idx, "psm": psm, "n": (lock.n_features, lock.n_fragments),
                "groups": lock.total_elution_groups,
                "target": lock.has_target_num_precursors}
        if i == 1:  # (built on demand, not part of a step: kept out of the byte count)
            before = ctx.d2h_bytes()
            step["lock_frames"] = (lock.features_df, lock.fragments_df)
            lock_bytes = ctx.d2h_bytes() - before
        if lock.has_target_num_precursors:
            step["filtered"] = handler.filter_for_calibration(psm, CONFIG)
        steps.append(step)
        lock.update()
        lock.update_with_calibration(calibration)
    return steps, ctx.d2h_bytes() - lock_bytes


def test_lock_sequence_equals_the_chained_lock(case):
    chained, moved_chained = _sequence(case, resident=False)
    resident, moved = _sequence(case, resident=True)
    assert [s["batch_idx"] for s in resident] == [s["batch_idx"] for s in chained] == [0, 1, 0]
    assert [s["target"] for s in resident] == [s["target"] for s in chained] == [False, True, True]
    for i, (r, c) in enumerate(zip(resident, chained, strict=True)):
        assert r["n"] == c["n"] and r["n"][0] > 0
        assert r["groups"] == c["groups"] > 0
        exp = c["psm"]
        got = r["psm"]
        assert "table_row" in got.columns
        cols = ["precursor_idx", "rank", "elution_group_idx", "channel", "decoy", "proba", "qval"]
        # (the id columns of the resident frame have the candidate table's dtypes: values are compared)
        _assert_same(got[cols], exp[cols], f"psm of step {i}", dtypes=False)
        if "filtered" in c:
            _assert_same(r["filtered"][0], c["filtered"][0], f"calibration precursors of step {i}")
            _assert_same(r["filtered"][1], c["filtered"][1], f"calibration fragments of step {i}")
            assert len(r["filtered"][0]) > 20 and len(r["filtered"][1]) > 50
    # the lock's frames after two accumulated batches, the second scored after a recalibration: each row with the
    # library values of the time it was scored, and the reference's index (each batch's own RangeIndex)
    for got, exp, what in zip(resident[1]["lock_frames"], chained[1]["lock_frames"], ("features", "fragments")):
        assert got.index.equals(exp.index), what
        _assert_same(got, exp, f"lock {what}")
    feats = chained[1]["lock_frames"][0]
    assert feats["rt_calibrated"].ne(feats["rt_library"]).any() and feats["rt_calibrated"].eq(feats["rt_library"]).any()
    assert resident[1]["n"] == (len(feats), len(chained[1]["lock_frames"][1]))
    assert moved < moved_chained, (moved, moved_chained)
    print(f"D2H over the three steps: resident {moved} B, chained {moved_chained} B")
