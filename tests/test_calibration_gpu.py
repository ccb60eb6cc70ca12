"""Library calibration on the GPU: ``adh_calibration_predict`` against the reference's LOESS predictions
(tests/golden/calibration.npz) and against the NumPy evaluator of tests/test_calibration.py, chunk edges, 12 M rows,
and a calibrated library going through candidate selection and scoring."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import synthetic as syn
from alphadia_amd import _abi, runtime
from alphadia_amd import calibration as cal
from test_calibration import CASES, FITTED, golden_model, np_predict

pytestmark = pytest.mark.gpu

CHUNK = _abi.CALIBRATION_CHUNK_ROWS


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


def f32_knife_edge(y64: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """Rows whose float64 value lies within ``bound`` of a float32 rounding midpoint: their float32 rounding may
    flip under a change of the last bits."""
    f = y64.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    down = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    mid_up, mid_down = (f.astype(np.float64) + up) / 2, (f.astype(np.float64) + down) / 2
    return (np.abs(y64 - mid_up) <= bound) | (np.abs(y64 - mid_down) <= bound)


def check_against(got, want, scale, max_edge_fraction=1e-4):
    finite = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~finite)
    err = np.abs(got[finite] - want[finite])
    bound = 1e-13 * scale[finite]
    assert (err <= bound).all(), float((err / np.maximum(scale[finite], 1e-300)).max())
    edge = f32_knife_edge(want[finite], bound)
    same = got[finite].astype(np.float32) == want[finite].astype(np.float32)
    assert (same | edge).all()
    assert edge.sum() <= max(2, max_edge_fraction * finite.sum()), int(edge.sum())


@pytest.mark.parametrize("name", FITTED)
def test_device_matches_reference_predictions(ctx, name):
    c = CASES[name]
    model = golden_model(c)
    for q, want in ((c["query"], c["pred"]), (c["query_nan"], c["pred_nan"])):
        got = ctx.calibration_predict(model, q)
        assert got.dtype == np.float64 and got.shape == q.shape
        _, scale = np_predict(model.scale_mean, model.scale_max, model.beta, q)
        check_against(got, want, np.where(np.isnan(scale), 0, scale))
    # the input dtype matters: the float32 design row has x^2 rounded to float32
    if c["query"].dtype == np.float32:
        as64 = ctx.calibration_predict(model, c["query"].astype(np.float64))
        want64, scale64 = np_predict(model.scale_mean, model.scale_max, model.beta, c["query"].astype(np.float64))
        check_against(as64, want64, scale64)


@pytest.mark.parametrize("n", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunk_edges(ctx, n, dtype):
    model = golden_model(CASES["rt_f64"])
    rng = np.random.default_rng(n)
    x = rng.uniform(-500.0, 7800.0, n).astype(dtype)
    got = ctx.calibration_predict(model, x)
    assert got.shape == (n,)
    want, scale = np_predict(model.scale_mean, model.scale_max, model.beta, x)
    check_against(got, want, scale)
    assert ctx.calibration_time_ms() >= 0.0


def test_twelve_million_fragment_rows(ctx):
    model = golden_model(CASES["mz_f32"])
    rng = np.random.default_rng(12)
    x = rng.uniform(150.0, 2000.0, 12_000_000).astype(np.float32)
    got = ctx.calibration_predict(model, x)
    assert ctx.calibration_time_ms() > 0.0
    sample = rng.choice(x.size, 200_000, replace=False)
    want, scale = np_predict(model.scale_mean, model.scale_max, model.beta, x[sample])
    check_against(got[sample], want, scale)
    mismatched = 0
    for a in range(0, x.size, 2_000_000):  # float32 rounding of every row
        want, scale = np_predict(model.scale_mean, model.scale_max, model.beta, x[a:a + 2_000_000])
        same = got[a:a + 2_000_000].astype(np.float32) == want.astype(np.float32)
        edge = f32_knife_edge(want, 1e-13 * scale)
        assert (same | edge).all()
        mismatched += int((~same).sum())
    assert mismatched <= 100


def test_model_limits(ctx):
    m = cal.HipLOESSRegression(n_kernels=33)
    m.scale_mean, m.scale_max, m.beta = np.zeros(33), np.ones(33), np.zeros((3, 33))
    with pytest.raises(ValueError, match="at most 32"):
        ctx.calibration_predict(m, np.zeros(4))
    m = cal.HipLOESSRegression()
    with pytest.raises(ValueError, match="not fitted"):
        m.predict(np.zeros(4))


def _psms(case, rng, shift_ppm=8.0):
    """PSMs of the planted precursors of ``case`` against a library whose m/z is off by ``shift_ppm`` and whose
    retention times are warped; the run is the truth."""
    pdf = case.library.precursor_df
    fdf = case.library.fragment_df
    true_rt = pdf["rt_library"].to_numpy(np.float64)
    lo, hi = true_rt.min(), true_rt.max()
    warped = lo + (true_rt - lo) * 0.85 + 0.04 * (true_rt - lo) ** 2 / max(hi - lo, 1.0) - 20.0
    lib_p = pdf.copy()
    lib_p["mz_library"] = (pdf["mz_library"].to_numpy(np.float64) * (1 - shift_ppm * 1e-6)).astype(np.float32)
    lib_p["rt_library"] = warped.astype(np.float32)
    lib_f = fdf.copy()
    lib_f["mz_library"] = (fdf["mz_library"].to_numpy(np.float64) * (1 - shift_ppm * 1e-6)).astype(np.float32)
    planted = np.unique(case.candidates_df["precursor_idx"].to_numpy())
    rows = np.flatnonzero(np.isin(pdf["precursor_idx"].to_numpy(), planted))
    psm_p = pd.DataFrame({
        "mz_library": lib_p["mz_library"].to_numpy()[rows],
        "mz_observed": pdf["mz_library"].to_numpy(np.float64)[rows] * (1 + rng.normal(0, 0.5e-6, rows.size)),
        "rt_library": lib_p["rt_library"].to_numpy()[rows],
        "rt_observed": true_rt[rows] + rng.normal(0, 0.5, rows.size),
    })
    frag_rows = np.concatenate([np.arange(a, b) for a, b in zip(pdf["flat_frag_start_idx"].to_numpy()[rows],
                                                                 pdf["flat_frag_stop_idx"].to_numpy()[rows])])
    true_f = fdf["mz_library"].to_numpy(np.float64)[frag_rows]
    psm_f = pd.DataFrame({
        "mz_library": lib_f["mz_library"].to_numpy()[frag_rows],
        "mz_observed": true_f * (1 + rng.normal(0, 1e-6, frag_rows.size)),
    })
    return lib_p, lib_f, psm_p, psm_f


def test_manager_round_trip_and_calibrated_search(tmp_path):
    from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring
    from alphadia_amd.selection import CandidateSelectionConfig, HipCandidateSelection

    case = syn.make_case(n_precursors=600, n_cycles=120, config_id=77, per_precursor=2, n_ms2=8, ms1_peaks=400,
                         ms2_peaks=150, mz_lo=400, mz_hi=480, frag_mz_lo=200, frag_mz_hi=350,
                         ms1_mz_range=(395, 500), ms2_mz_range=(195, 355), planted_fraction=0.5, threads=4)
    rng = np.random.default_rng(5)
    lib_p, lib_f, psm_p, psm_f = _psms(case, rng)
    path = str(tmp_path / "calibration_manager.pkl")
    m = cal.HipCalibrationManager(path=path, load_from_file=False, has_ms1=True, has_mobility=False)
    m.fit(psm_f, "fragment", plot=False)
    m.fit(psm_p, "precursor", plot=False)
    assert m.all_fitted
    m.save()
    m = cal.HipCalibrationManager(path=path, load_from_file=True, has_ms1=True, has_mobility=False)
    assert m.is_loaded_from_file and m.all_fitted

    before = np.median((psm_f.mz_observed - psm_f.mz_library) / psm_f.mz_library * 1e6)
    assert before > 7.0
    m.predict(psm_f, "fragment")
    m.predict(psm_p, "precursor")
    after = np.median((psm_f.mz_observed - psm_f.mz_calibrated) / psm_f.mz_calibrated * 1e6)
    assert abs(after) < 1.0, after
    assert np.median(np.abs(psm_p.rt_observed - psm_p.rt_calibrated)) < 1.0
    assert m.get_estimator("fragment", "mz").ci(psm_f, 0.95) < 3.0

    m.predict(lib_f, "fragment")
    m.predict(lib_p, "precursor")
    assert lib_f["mz_calibrated"].dtype == np.float64 and lib_p["rt_calibrated"].dtype == np.float64
    true_mz = case.library.fragment_df["mz_library"].to_numpy(np.float64)
    assert np.median(np.abs(lib_f["mz_calibrated"] - true_mz) / true_mz * 1e6) < 1.0

    # the calibrated columns drive candidate selection and scoring as the true ones do
    scfg = CandidateSelectionConfig()
    scfg.update(dict(rt_tolerance=60.0, precursor_mz_tolerance=10.0, fragment_mz_tolerance=15.0))

    def search(pdf, fdf, mz_col, rt_col):
        sel = HipCandidateSelection(case.dia, pdf, fdf, scfg, rt_column=rt_col, mobility_column="mobility_library",
                                    precursor_mz_column=mz_col, fragment_mz_column=mz_col, device=0)()
        cfg = CandidateScoringConfig()
        cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15))
        scorer = HipCandidateScoring(dia_data=case.dia, precursors_flat=pdf, fragments_flat=fdf, rt_column=rt_col,
                                     mobility_column="mobility_library", precursor_mz_column=mz_col,
                                     fragment_mz_column=mz_col, config=cfg, device=0)
        features, fragments = scorer(sel)
        return sel, features, fragments

    sel_true, feat_true, _ = search(case.library.precursor_df, case.library.fragment_df, "mz_library", "rt_library")
    sel_cal, feat_cal, frag_cal = search(lib_p, lib_f, "mz_calibrated", "rt_calibrated")
    assert len(sel_cal) > 0 and len(feat_cal) > 0 and len(frag_cal) > 0
    assert len(feat_cal) >= 0.9 * len(feat_true), (len(feat_cal), len(feat_true))
