"""CPU: the synthetic generators on general cycles (tests/synthetic.py) - the default arguments still draw the runs the
committed fixtures hold, peaks are planted where a cycle says they belong, and the fixtures of the general cycles
regenerate from their generator."""

import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import ref_shim  # noqa: E402  (only for the place the reference is expected at)

# tests/golden/make_golden.py, small_case(101): the run of scoring_handler_default.npz
SMALL_CASE = dict(n_precursors=300, n_cycles=60, config_id=101, per_precursor=2, n_ms2=8, ms1_peaks=400, ms2_peaks=150,
                  mz_lo=400, mz_hi=480, frag_mz_lo=200, frag_mz_hi=350, ms1_mz_range=(395, 500), ms2_mz_range=(195, 355),
                  few_fragment_fraction=0.05, even_fraction=0.3, planted_fraction=0.5, threads=1)


def test_default_arguments_draw_the_committed_alpharaw_run():
    """``cycle=None`` is the touching-window cycle with the random numbers drawn in the order they always were: the
    run, library and candidates of a committed fixture come out array for array."""
    z = np.load(H.golden_path("scoring_handler_default.npz"))
    case = syn.make_case(**SMALL_CASE)
    explicit = syn.make_case(**SMALL_CASE, cycle=syn.make_cycle(n_ms2=8, mz_lo=400, mz_hi=480))
    for c in (case, explicit):
        for key, got in (("dia_cycle", c.dia.cycle), ("dia_rt_values", c.dia.rt_values), ("dia_peak_start", c.dia.peak_start_idx_list),
                         ("dia_peak_stop", c.dia.peak_stop_idx_list), ("dia_mz", c.dia.mz_values), ("dia_intensity", c.dia.intensity_values)):
            assert got.dtype == z[key].dtype and np.array_equal(got, z[key]), key
        for col in H.CAND_COLS:
            assert np.array_equal(c.candidates_df[col].values, z["cand_" + col]), col
        for col in H.PREC_COLS:
            assert np.array_equal(c.library.precursor_df[col].values, z["prec_" + col]), col


def test_default_arguments_draw_the_committed_timstof_run():
    z = np.load(H.golden_path("scoring_timstof.npz"))
    case = syn.make_timstof_case(n_precursors=160, n_cycles=36)
    for name in ("cycle", "dia_precursor_cycle", "rt_values", "mobility_values", "mz_values", "tof_indptr", "push_indices",
                 "intensity_values"):
        got = getattr(case.dia, name)
        assert got.dtype == z["tims_" + name].dtype and np.array_equal(got, z["tims_" + name]), name
    for col in H.CAND_COLS:
        assert np.array_equal(case.candidates_df[col].values, z["cand_" + col]), col


def _peaks_near(dia, spec, mz, ppm=8.0):
    a, b = dia.peak_start_idx_list[spec], dia.peak_stop_idx_list[spec]
    m = dia.mz_values[a:b].astype(np.float64)
    return dia.intensity_values[a:b][np.abs(m - mz) <= ppm * 1e-6 * mz]


@pytest.mark.parametrize("geometry", ["staggered", "multi_ms1", "multi_ms1_twin", "dense_overlap"])
def test_peaks_are_planted_where_the_cycle_says(geometry):
    """Isotope peaks in every MS1 row, fragment peaks in every window row that holds the precursor m/z and in no other
    row, noise density by row type - on cycles whose MS1 rows are not (only) row 0 and whose windows overlap."""
    cycle = {"staggered": syn.make_staggered_cycle, "dense_overlap": syn.make_dense_overlap_cycle,
             "multi_ms1": lambda: syn.make_multi_ms1_cycle(ms1_first=True),
             "multi_ms1_twin": lambda: syn.make_multi_ms1_cycle(ms1_first=False)}[geometry]()
    args = dict(SMALL_CASE, n_precursors=80, config_id=120, ms1_peaks=60, ms2_peaks=20, few_fragment_fraction=0.0)
    case = syn.make_case(**args, cycle=cycle)
    dia, L = case.dia, cycle.shape[1]
    ms1 = syn.ms1_rows_of(cycle)
    assert len(ms1) == {"staggered": 1, "multi_ms1": 2, "multi_ms1_twin": 2, "dense_overlap": 3}[geometry]
    assert (0 in ms1) == (geometry != "multi_ms1_twin")
    counts = (dia.peak_stop_idx_list - dia.peak_start_idx_list).reshape(-1, L)
    is_ms1 = np.isin(np.arange(L), ms1)
    assert (counts[:, is_ms1] >= 60).all() and (counts[:, ~is_ms1] >= 20).all() and counts[:, ~is_ms1].min() < 60
    assert np.all(np.diff(dia.rt_values) > 0)
    pdf, fdf = case.library.precursor_df, case.library.fragment_df
    planted = np.flatnonzero(case.apex_cycle >= 0)
    assert len(planted) >= 10
    n_windows = set()
    for p in planted:
        mz, apex = float(pdf["mz_library"].values[p]), int(case.apex_cycle[p])
        k = int(np.argmax(fdf["intensity"].values[pdf["flat_frag_start_idx"].values[p]:pdf["flat_frag_stop_idx"].values[p]]))
        fmz = float(fdf["mz_library"].values[pdf["flat_frag_start_idx"].values[p] + k])
        holds = 0
        for row in range(L):
            lo, hi = cycle[0, row, 0]
            if row in ms1:
                assert _peaks_near(dia, apex * L + row, mz).max(initial=0) > 1000, (p, row)
            elif lo <= mz < hi:
                holds += 1
                assert _peaks_near(dia, apex * L + row, fmz).max(initial=0) > 200, (p, row)
            else:
                assert _peaks_near(dia, apex * L + row, fmz).max(initial=0) < 200, (p, row)
        n_windows.add(holds)
    if geometry == "dense_overlap":  # three windows hold an m/z, fewer next to the uncovered stretch, none inside it
        assert 3 in n_windows and n_windows <= {0, 1, 2, 3}
    else:
        assert n_windows == ({2} if geometry == "staggered" else {1})


def test_timstof_cycle_with_two_ms1_frames_and_repeated_ms2_frames():
    base = syn.make_timstof_cycle(3, 2, 64, 400.0, 480.0)
    cycle = syn.make_timstof_cycle(3, 2, 64, 400.0, 480.0, n_ms1_frames=2, repeats=3)
    assert cycle.shape == (1, 2 + 9, 64, 2)
    ms1 = np.flatnonzero((cycle[0, :, :, 0] == -1.0).all(axis=1))
    assert ms1.tolist() == [0, 5]
    ms2 = [fr for fr in range(cycle.shape[1]) if fr not in ms1]
    for j, fr in enumerate(ms2):  # the MS2 frames of the plain cycle, three times over
        assert np.array_equal(cycle[0, fr], base[0, 1 + j % 3])
    case = syn.make_timstof_case(n_precursors=40, n_cycles=20, config_id=49, scan_max_index=64, n_tof=6000,
                                 events_per_push=2.0, cycle=cycle)
    assert case.dia.cycle_len == 11 and case.dia.rt_values.shape[0] == 20 * 11 + 1
    assert case.candidates_df["frame_start"].mod(11).eq(1).all()


@pytest.mark.skipif(not os.path.isdir(ref_shim.REFERENCE_ROOT), reason="the reference checkout is not on this machine")
def test_regenerating_the_cycle_goldens_reproduces_the_committed_files(tmp_path):
    """Three of the fixtures of the general cycles (one scoring table, the get_dense queries, the ion-mobility table)
    through the reference again: every array as committed."""
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden.py"), "--out", str(tmp_path), "--cycles-only",
                        "multi_ms1_twin", "get_dense", "timstof"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for name in ("scoring_multi_ms1_twin.npz", "get_dense_cycles.npz", "scoring_timstof_cycles.npz"):
        fresh, golden = np.load(tmp_path / name), np.load(H.golden_path(name))
        assert sorted(fresh.files) == sorted(golden.files), name
        for key in golden.files:
            assert fresh[key].dtype == golden[key].dtype, (name, key)
            assert np.array_equal(fresh[key], golden[key], equal_nan=golden[key].dtype.kind == "f"), (name, key)


@pytest.mark.skipif(not os.path.isdir(ref_shim.REFERENCE_ROOT), reason="the reference checkout is not on this machine")
def test_regenerating_the_mz_edge_golden_reproduces_the_committed_file(tmp_path):
    """get_dense_mz_edges.npz (tests/mz_edges.py through the reference's get_dense) takes seconds: every array as
    committed, and the file itself byte for byte."""
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden.py"), "--out", str(tmp_path), "--mz-edges-only"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    name = "get_dense_mz_edges.npz"
    fresh, golden = np.load(tmp_path / name), np.load(H.golden_path(name))
    assert sorted(fresh.files) == sorted(golden.files)
    for key in golden.files:
        assert fresh[key].dtype == golden[key].dtype, key
        assert np.array_equal(fresh[key], golden[key], equal_nan=golden[key].dtype.kind == "f"), key
    with open(tmp_path / name, "rb") as f, open(H.golden_path(name), "rb") as g:
        assert f.read() == g.read()
