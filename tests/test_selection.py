"""Candidate selection: oracle vs goldens produced by running the reference,
HIP vs oracle.

The reference smooths with a float32 FFT (selection/fft.py:119-212); the golden was produced with
``np.fft`` as a stand-in for rocket_fft (tests/golden/ref_shim.py), results cast to complex64 / float32.
The oracle and the HIP kernels evaluate the same circular convolution exactly (float64, rounded once).
Round 6 pins what that difference is and nothing more:

* with the golden's own smoothing plugged in (``oracle.set_selection_hooks``: rfft2 / irfft2 of the tile's shape in
  complex64 / float32, then ``log(smooth + 1)``) the restatement reproduces EVERY row of all three goldens - boxes,
  ranks and the bits of the score: everything behind the smoothing is pinned exactly;
* with the exact convolution a few rows differ (9 of 649, 4 of 1 134, 8 of 167): each belongs to a precursor whose
  score matrix the two smoothings move apart by at most ``NEAR_TIE_SCORE`` (5e-3 in units of the standardised score,
  whose range is +-130: 4e-5 of it; 3.7e-3 / 2.7e-3 / 1.8e-4 measured) - a perturbation of that size flips the
  outcome, i.e. a near-tie - and no precursor's best candidate is among them.

HIP vs oracle is exact, so the same holds for the product.

The fixtures at the kernels' limits (selection_limits.npz "many" / "k16", selection_timstof_limits.npz "many" / "wide":
4 ... 60 fragments per precursor, up to 16 candidates, a kernel of 16 cycles, 8 ... 64 m/z windows on the ion-mobility
run) are held to the same two statements: bit for bit with the golden's smoothing, and 2 of 1 888, 9 of 770, 0 of 808
and 0 of 488 near-tie rows with the exact convolution (N_DIFF; under 5 % of a fixture's rows).  They are drawn dense
enough that no tile has a stretch of cycles without any signal: there only the noise of the float32 FFT makes peaks,
with equal scores that the reference orders by an unstable sort, and 16 candidates reach down to them."""
import os
import types

import numpy as np
import pandas as pd
import pytest

import helpers as H
from alphadia_amd import _abi
from alphadia_amd.scoring import fragment_columns
from alphadia_amd.selection import CANDIDATE_COLUMNS, CandidateSelectionConfig, HipCandidateSelection, gaussian_kernel

BOX = ["scan_center", "scan_start", "scan_stop", "frame_center", "frame_start", "frame_stop"]


RAW_FIXTURE = {"cycles": "selection_cycles.npz", "many": "selection_limits.npz", "k16": "selection_limits.npz"}


def _load(name=None):
    # "cycles": staggered windows with two MS1 rows per cycle (two or three rows in each group of cycle rows that
    # selection sums); "many", "k16": 4 ... 60 fragments per precursor, 16 candidates, a kernel of 16 cycles
    # (selection_limits.npz); every other name lives in selection.npz
    z = np.load(H.golden_path(RAW_FIXTURE.get(name, "selection.npz")))
    dia = H.dia_from_npz(z)
    fdf = pd.DataFrame({c: z["frag_" + c] for c in H.FRAG_COLS})
    pdf = pd.DataFrame({c: z["prec_" + c] for c in H.PREC_COLS})
    for c, v in (("proteins", "P"), ("genes", "G"), ("sequence", "PEPTIDEK"), ("mods", ""), ("mod_sites", "")):
        pdf[c] = np.full(len(pdf), v, dtype=object)
    return z, dia, fdf, pdf


def _cfg(z, name):
    pre = name + "_cfg_"
    return types.SimpleNamespace(**{k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})


def _pack(pdf):
    pdf = pdf.sort_values("precursor_idx").reset_index(drop=True)
    iso = pdf[[c for c in pdf.columns if c.startswith("i_")]].values
    return _abi.pack_precursors(pdf.precursor_idx.values, pdf.flat_frag_start_idx.values,
                                pdf.flat_frag_stop_idx.values, pdf.charge.values, pdf.rt_library.values,
                                pdf.mobility_library.values, pdf.mz_library.values, iso)


def _frame(arrays):
    keep = arrays["score"] > 0
    return pd.DataFrame({c: arrays[c][keep] for c in CANDIDATE_COLUMNS})


NEAR_TIE_SCORE = 5e-3  # largest move of a score matrix between the two smoothings that explains a differing row


def golden_fft_smooth_log(kernel):
    """The smoothing + log the goldens were made with (ref_shim.py convolve_fourier, selection.py:206-226), for one
    (S, F) float32 tile: circular convolution through rfft2 / irfft2 of the tile's own shape in complex64 / float32,
    the kernel centred by the four-quadrant copy of selection/fft.py:163-212."""
    k0, k1 = kernel.shape
    d0, d1 = -k0 // 2, -k1 // 2

    def smooth_log(tile):
        shape = tile.shape
        ff = np.fft.rfft2(kernel.astype(np.float32), shape).astype(np.complex64)
        spec = np.fft.rfft2(tile).astype(np.complex64)
        layer = np.fft.irfft2(spec * ff, shape).astype(np.float32)
        o = np.zeros_like(tile)
        o[d0:, d1:] = layer[:-d0, :-d1]
        o[:d0, d1:] = layer[-d0:, :-d1]
        o[d0:, :d1] = layer[:-d0, -d1:]
        o[:d0, :d1] = layer[-d0:, -d1:]
        return np.log(o + 1)

    return smooth_log


def _golden_case(kind, name):
    if kind == "raw":
        z, dia, fdf, pdf = _load(name)
        return z, dia, fdf, pdf, _cfg(z, name), z[name + "_kernel"], name + "_out_"
    z, dia, fdf, pdf, cfg = _load_tims(name)
    pre = name + "_" if name else ""
    return z, dia, fdf, pdf, cfg, z[pre + "kernel"], pre + "out_"


def _differing_rows(got: pd.DataFrame, exp: pd.DataFrame) -> pd.DataFrame:
    """Rows (precursor_idx, rank) that are not in both tables with the same box."""
    m = got.merge(exp, on=["precursor_idx", "rank"], how="outer", suffixes=("_g", "_e"), indicator=True)
    diff = (m["_merge"] != "both").values
    for c in BOX:
        diff |= (m[c + "_g"] != m[c + "_e"]).values
    return m[diff]


_EXPLAINED = {}


def near_tie_precursors(oracle, kind, name):
    """precursor_idx -> largest absolute difference between the score matrix under the exact convolution and under the
    golden's FFT smoothing (both through the restatement, single-threaded; the score hook collects the matrices)."""
    key = (kind, name)
    if key not in _EXPLAINED:
        z, dia, fdf, pdf, cfg, kernel, _ = _golden_case(kind, name)
        sel = oracle.select if kind == "raw" else oracle.select_timstof
        cols, pm = fragment_columns(fdf, "mz_library"), _pack(pdf)
        exact, fft = {}, {}
        try:
            oracle.set_selection_hooks(None, lambda i, m: exact.__setitem__(i, m))
            sel(dia, cols, pm, cfg, kernel, n_threads=1)
            oracle.set_selection_hooks(golden_fft_smooth_log(kernel), lambda i, m: fft.__setitem__(i, m))
            sel(dia, cols, pm, cfg, kernel, n_threads=1)
        finally:
            oracle.set_selection_hooks(None, None)
        pidx = np.sort(pdf.precursor_idx.values)
        _EXPLAINED[key] = {int(pidx[i]): float(np.abs(fft[i] - exact[i]).max()) for i in exact if i in fft}
    return _EXPLAINED[key]


def _compare_with_golden(got: pd.DataFrame, z, name, oracle=None, kind="raw", prefix=None):
    """`got` (exact smoothing: the oracle's or the HIP kernels' table) against the reference golden: no row the
    reference does not have; every row that is missing or has another box belongs to a precursor whose score matrix
    the golden's FFT smoothing moves by at most NEAR_TIE_SCORE (and by more than 0), and is never a precursor's best
    candidate; scores of the rows with the same box within that move (relative to the score: 5e-3)."""
    from oracle import oracle as oracle_mod

    oracle = oracle or oracle_mod
    prefix = prefix if prefix is not None else name + "_out_"
    exp = pd.DataFrame({c: z[prefix + c] for c in CANDIDATE_COLUMNS})
    m = got.merge(exp, on=["precursor_idx", "rank"], how="outer", suffixes=("_g", "_e"), indicator=True)
    assert (m["_merge"] == "left_only").sum() == 0, "rows the reference does not have"
    diff = _differing_rows(got, exp)
    moved = near_tie_precursors(oracle, kind, name)
    for p in sorted(set(diff["precursor_idx"])):
        assert 0.0 < moved[int(p)] <= NEAR_TIE_SCORE, (p, moved[int(p)])
    assert (diff["rank"] > 0).all(), "a precursor's best candidate differs"
    both = m[m["_merge"] == "both"]
    same_box = np.ones(len(both), dtype=bool)
    for c in BOX:
        same_box &= (both[c + "_g"] == both[c + "_e"]).values
    rel = np.abs(both["score_g"] - both["score_e"]) / np.abs(both["score_e"])
    assert rel[same_box].max() <= 5e-3
    return len(both), len(diff)


@pytest.mark.parametrize("kind,name", [("raw", "default"), ("raw", "wide"), ("tims", None), ("raw", "cycles"),
                                       ("raw", "many"), ("raw", "k16"), ("tims", "many"), ("tims", "wide")])
def test_oracle_with_the_goldens_smoothing_reproduces_the_golden_exactly(oracle_lib, kind, name):
    """Everything behind the smoothing is pinned bit for bit: with the float32 FFT smoothing the golden was made with
    plugged into the restatement, every row of the golden comes out - boxes, ranks and the bits of the score."""
    z, dia, fdf, pdf, cfg, kernel, prefix = _golden_case(kind, name)
    sel = oracle_lib.select if kind == "raw" else oracle_lib.select_timstof
    try:
        oracle_lib.set_selection_hooks(golden_fft_smooth_log(kernel), None)
        got = _frame(sel(dia, fragment_columns(fdf, "mz_library"), _pack(pdf), cfg, kernel, n_threads=1))
    finally:
        oracle_lib.set_selection_hooks(None, None)
    exp = pd.DataFrame({c: z[prefix + c] for c in CANDIDATE_COLUMNS})
    assert len(got) == len(exp) > 150
    got = got.sort_values(["precursor_idx", "rank"]).reset_index(drop=True)
    exp = exp.sort_values(["precursor_idx", "rank"]).reset_index(drop=True)
    for c in CANDIDATE_COLUMNS:
        assert np.array_equal(got[c].to_numpy(), exp[c].to_numpy()), c


# rows of the oracle's table (exact convolution) that differ from the fixture, as measured on the CPU; the HIP tables are
# held to the same numbers (tests/test_selection_limits_gpu.py, tests/test_general_cycles_gpu.py)
N_DIFF = {("raw", "default"): 9, ("raw", "wide"): 4, ("tims", None): 8, ("raw", "cycles"): 34,
          ("raw", "many"): 2, ("raw", "k16"): 9, ("tims", "many"): 0, ("tims", "wide"): 0}


@pytest.mark.parametrize("kind,name,n_diff", [(kind, name, n) for (kind, name), n in N_DIFF.items()])
def test_every_box_that_differs_from_the_reference_is_a_near_tie(oracle_lib, kind, name, n_diff):
    """The exact convolution against the golden: the rows that differ are counted, each sits in a precursor whose score
    matrix the two smoothings move apart by <= NEAR_TIE_SCORE, none is a best candidate; every other precursor's rows
    are identical."""
    z, dia, fdf, pdf, cfg, kernel, prefix = _golden_case(kind, name)
    sel = oracle_lib.select if kind == "raw" else oracle_lib.select_timstof
    got = _frame(sel(dia, fragment_columns(fdf, "mz_library"), _pack(pdf), cfg, kernel, n_threads=4))
    exp = pd.DataFrame({c: z[prefix + c] for c in CANDIDATE_COLUMNS})
    diff = _differing_rows(got, exp)
    assert len(diff) == n_diff
    if name in ("many", "k16") or (kind == "tims" and name):  # (the fixtures at the kernels' limits were drawn to stay under 5 %)
        assert n_diff < 0.05 * len(exp)
    moved = near_tie_precursors(oracle_lib, kind, name)
    assert max(moved.values()) <= NEAR_TIE_SCORE  # (the move is small everywhere; it only matters where it flips a decision)
    worst = max((moved[int(p)] for p in set(diff["precursor_idx"])), default=0.0)
    print(f"[selection {kind} {name}] {len(diff)} rows of {len(exp)} differ, in {diff['precursor_idx'].nunique()} precursors; "
          f"largest score move among them {worst:.2e}, anywhere {max(moved.values()):.2e}")
    _compare_with_golden(got, z, name, oracle_lib, kind, prefix)


def test_kernel_matches_reference_kernel():
    z, dia, _, _ = _load()
    k = gaussian_kernel(dia, 10.0, 0.1, 30)
    assert k.dtype == np.float32 and np.array_equal(k, z["default_kernel"])


@pytest.mark.parametrize("name", ["default", "wide", "cycles", "many", "k16"])
def test_oracle_selection_vs_reference_golden(oracle_lib, name):
    z, dia, fdf, pdf = _load(name)
    got = oracle_lib.select(dia, fragment_columns(fdf, "mz_library"), _pack(pdf), _cfg(z, name),
                            z[name + "_kernel"], n_threads=4)
    n_both, n_missing = _compare_with_golden(_frame(got), z, name)
    assert n_both > (400 if name == "cycles" else 600)  # (the "cycles" golden holds 503 rows)


def test_selection_config_defaults_match_reference_golden():
    z, _, _, _ = _load()
    c = CandidateSelectionConfig()
    c.update(dict(rt_tolerance=30.0, candidate_count=3, min_size_rt=3))
    ref = _cfg(z, "default")
    for k in ("precursor_mz_tolerance fragment_mz_tolerance top_k_precursors exclude_shared_ions kernel_size "
              "f_mobility f_rt center_fraction min_size_mobility max_size_mobility max_size_rt "
              "use_weighted_score join_close_candidates join_close_candidates_scan_threshold "
              "join_close_candidates_cycle_threshold rt_tolerance candidate_count min_size_rt").split():
        assert getattr(c, k) == getattr(ref, k).item(), k


def test_symetric_limits_1d_matches_reference_function(oracle_lib):
    """400 random inputs through the reference's `_symetric_limits_1d` (selection/utils.py:218-280;
    its own test, tests/unit_tests/search/selection/test_search_utils.py:9-33, checks the same
    properties): the restatement returns the same limits."""
    z = np.load(H.golden_path("selection_kats.npz"))
    for row, exp in zip(z["limits_in"], z["limits_out"]):
        n, center, f, cf, mn, mx = int(row[40]), int(row[41]), row[42], row[43], int(row[44]), int(row[45])
        got = oracle_lib.symetric_limits_1d(row[:n], center, f, cf, mn, mx)
        assert np.array_equal(got, exp), (n, center, f, cf, mn, mx)
        if n > 0 and 0 <= center < n:
            assert got[0] <= center <= got[1] and got[0] >= 0 and got[1] <= n


def test_find_peaks_1d_matches_reference_function(oracle_lib):
    """200 random score rows (with ties) through the reference's `find_peaks_1d`
    (selection/utils.py:49-77).  Ties between equal scores are broken by an unstable sort there:
    compared as sets in that case."""
    z = np.load(H.golden_path("selection_kats.npz"))
    for row, cyc, val, n_exp in zip(z["peaks_in"], z["peaks_cycle"], z["peaks_score"], z["peaks_n"]):
        n, top_n = int(row[60]), int(row[61])
        got_c, got_v = oracle_lib.find_peaks_1d(row[:n], top_n)
        assert len(got_c) == n_exp
        assert np.array_equal(got_v, val[:n_exp])
        if len(np.unique(val[:n_exp])) == n_exp:
            assert np.array_equal(got_c, cyc[:n_exp])
        else:
            assert sorted(got_v) == sorted(val[:n_exp])


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "wide"])
def test_hip_selection_matches_oracle_and_golden(ctx, oracle_lib, name):
    z, dia, fdf, pdf = _load()
    cols = fragment_columns(fdf, "mz_library")
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    cfg = _cfg(z, name)
    got = ctx.select_candidates(_pack(pdf), cfg, z[name + "_kernel"])
    exp = oracle_lib.select(dia, cols, _pack(pdf), cfg, z[name + "_kernel"], n_threads=4)
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c
    _compare_with_golden(_frame(got), z, name)


@pytest.mark.gpu
def test_hip_selection_operator_dataframe(ctx):
    z, dia, fdf, pdf = _load()
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=30.0, candidate_count=3, min_size_rt=3))
    sel = HipCandidateSelection(dia, pdf, fdf, cfg, rt_column="rt_library", mobility_column="mobility_library",
                                precursor_mz_column="mz_library", fragment_mz_column="mz_library",
                                fwhm_rt=cfg.peak_len_rt, fwhm_mobility=cfg.peak_len_mobility)
    df = sel()
    assert list(df.columns) == CANDIDATE_COLUMNS + ["elution_group_idx", "decoy"]
    _compare_with_golden(df[CANDIDATE_COLUMNS], z, "default")
    # the boxes feed the scoring operator: frames are cycle aligned, scan range is [0, 1)
    L = dia.cycle.shape[1]
    last = dia.rt_values.shape[0] - 1  # wrap1 clips to frame_max_index (selection.py:488-491)
    assert (df["frame_start"] % L == 0).all()
    assert ((df["frame_stop"] % L == 0) | (df["frame_stop"] == last)).all()
    assert (df["scan_start"] == 0).all() and (df["scan_stop"] == 1).all()


@pytest.mark.gpu
def test_hip_selection_at_bench_density(ctx, oracle_lib):
    """A larger run (config-2 density): HIP equals the oracle on every row."""
    import synthetic as syn

    case = syn.make_case(3000, 400, config_id=2, per_precursor=1, threads=4)
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=45.0, candidate_count=3))
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    pm = _pack(case.library.precursor_df)
    got = ctx.select_candidates(pm, cfg, kern)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=16)
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c
    assert (got["score"] > 0).sum() > 3000


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("ADH_FUZZ_SEEDS_SELECT", "6")))))
def test_hip_selection_randomized(ctx, oracle_lib, monkeypatch, seed):
    """Differential test: random run geometry and selection settings, HIP == oracle."""
    import synthetic as syn

    rng = np.random.default_rng(3000 + seed)
    n_ms2 = int(rng.integers(3, 12))
    case = syn.make_case(
        int(rng.integers(100, 400)), int(rng.integers(50, 200)), config_id=700 + seed, per_precursor=1,
        n_ms2=n_ms2, ms1_peaks=int(rng.integers(100, 900)), ms2_peaks=int(rng.integers(40, 400)),
        mz_lo=400.0, mz_hi=400.0 + 10.0 * n_ms2, frag_mz_lo=200, frag_mz_hi=450,
        ms1_mz_range=(395, 430 + 10.0 * n_ms2), ms2_mz_range=(195, 470),
        few_fragment_fraction=float(rng.choice([0.0, 0.2])), planted_fraction=float(rng.uniform(0.2, 0.9)), threads=1,
    )
    if rng.random() < 0.5:
        card = case.library.fragment_df["cardinality"].values.copy()
        card[rng.random(card.size) < 0.2] = 2
        case.library.fragment_df["cardinality"] = card
    cfg = CandidateSelectionConfig()
    cfg.update(dict(
        rt_tolerance=float(rng.choice([5.0, 20.0, 45.0, 400.0])), candidate_count=int(rng.integers(1, 8)),
        top_k_precursors=int(rng.integers(1, 5)), exclude_shared_ions=bool(rng.integers(0, 2)),
        precursor_mz_tolerance=float(rng.choice([5, 15, 60])), fragment_mz_tolerance=float(rng.choice([7, 15, 80])),
        min_size_rt=int(rng.integers(1, 5)), max_size_rt=int(rng.integers(6, 20)),
        f_rt=float(rng.choice([0.9, 0.99])), center_fraction=float(rng.choice([0.2, 0.5])),
        join_close_candidates=bool(rng.integers(0, 2)), use_weighted_score=bool(rng.integers(0, 2)),
        sigma_scale_rt=float(rng.choice([0.1, 0.5])),
    ))
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    pm = _pack(case.library.precursor_df)
    got = ctx.select_candidates(pm, cfg, kern)
    got = {c: np.array(got[c], copy=True) for c in CANDIDATE_COLUMNS}
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=4)
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c
    # the smoothing with the kernel's non-zero columns as scalar operands (default where they fit) against the
    # generic loop with the taps in LDS: the same bits
    monkeypatch.setenv("ADH_DEBUG_SELECT_LDS_TAPS", "1")
    again = ctx.select_candidates(pm, cfg, kern)
    for c in CANDIDATE_COLUMNS:
        assert np.array_equal(again[c], got[c]), c


# ---------------------------------------------------------------- ion-mobility runs
def _load_tims(name=None):
    # name "many" / "wide": a setting of selection_timstof_limits.npz (4 ... 60 fragments per precursor, 16 candidates;
    # "wide": fragment windows in which the gather falls back to dense tiles for about half the precursors)
    import synthetic as syn

    z = np.load(H.golden_path("selection_timstof_limits.npz" if name else "selection_timstof.npz"))
    dia = syn.TimsTOFArrays(
        cycle=z["tims_cycle"], dia_precursor_cycle=z["tims_dia_precursor_cycle"], rt_values=z["tims_rt_values"],
        mobility_values=z["tims_mobility_values"], mz_values=z["tims_mz_values"], tof_indptr=z["tims_tof_indptr"],
        push_indices=z["tims_push_indices"], intensity_values=z["tims_intensity_values"],
        scan_max_index=int(z["tims_scan_max_index"]), zeroth_frame=bool(z["tims_zeroth_frame"]))
    fdf = pd.DataFrame({c: z["frag_" + c] for c in H.FRAG_COLS})
    pdf = pd.DataFrame({c: z["prec_" + c] for c in H.PREC_COLS})
    pre = (name + "_" if name else "") + "cfg_"
    cfg = types.SimpleNamespace(**{k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
    return z, dia, fdf, pdf, cfg


def _compare_tims_with_golden(got: pd.DataFrame, z):
    return _compare_with_golden(got, z, None, None, "tims", "out_")


def test_timstof_kernel_matches_reference_kernel():
    z, dia, _, _, cfg = _load_tims()
    k = gaussian_kernel(dia, float(cfg.peak_len_rt), float(cfg.sigma_scale_rt), int(cfg.kernel_size),
                        float(cfg.peak_len_mobility), float(cfg.sigma_scale_mobility))
    assert k.shape == z["kernel"].shape and np.array_equal(k, z["kernel"])


def test_oracle_timstof_selection_vs_reference_golden(oracle_lib):
    z, dia, fdf, pdf, cfg = _load_tims()
    got = oracle_lib.select_timstof(dia, fragment_columns(fdf, "mz_library"), _pack(pdf), cfg, z["kernel"], n_threads=4)
    _compare_tims_with_golden(_frame(got), z)
    assert (got["score"] > 0).sum() > 150


@pytest.mark.gpu
def test_hip_timstof_selection_matches_oracle_and_golden(ctx, oracle_lib):
    z, dia, fdf, pdf, cfg = _load_tims()
    cols = fragment_columns(fdf, "mz_library")
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    got = ctx.select_candidates(_pack(pdf), cfg, z["kernel"])
    exp = oracle_lib.select_timstof(dia, cols, _pack(pdf), cfg, z["kernel"], n_threads=4)
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c
    _compare_tims_with_golden(_frame(got), z)


@pytest.mark.gpu
def test_hip_timstof_selection_tile_forms_and_indices_agree(ctx, monkeypatch):
    """Sparse tiles / dense tiles, search indices on / off / one column per block of cycles: the same
    candidate table, bit for bit (scores included)."""
    import synthetic as syn
    from alphadia_amd.selection import CandidateSelectionConfig, gaussian_kernel

    case = syn.make_timstof_case(n_precursors=250, n_cycles=90, config_id=46, per_precursor=1, n_ms2_frames=5,
                                 windows_per_frame=2, scan_max_index=96, planted_fraction=0.6)
    case.dia.has_mobility = True
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=40.0, mobility_tolerance=0.08, candidate_count=3, peak_len_rt=3.0, sigma_scale_rt=0.5,
                    peak_len_mobility=0.02))
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size, cfg.peak_len_mobility,
                           cfg.sigma_scale_mobility)
    pdf = case.library.precursor_df.sort_values("precursor_idx").reset_index(drop=True)
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    pm = _pack(pdf)

    def run():
        ctx.stage_run(case.dia, force=True)
        ctx.stage_fragments(*cols, force=True)
        got = ctx.select_candidates(pm, cfg, kern)
        return {c: np.array(got[c], copy=True) for c in CANDIDATE_COLUMNS}

    base = run()
    assert len(base["precursor_idx"]) > 100
    # (ADH_DEBUG_SELECT_IM_ABL=5: pass 2 of the smoothing walks the rows per cell instead of reading its tap lists;
    #  8: pass 1 runs over zero-filled rows instead of the rows' events)
    # (ADH_SELECT_SCRATCH_MB=1: the precursors go through the kernels in many batches, cut from the device's prefix sums)
    for env in (dict(ADH_DEBUG_SELECT_IM_DENSE="1"), dict(ADH_IM_INDEX="0"), dict(ADH_IM_INDEX_MB="1"),
                dict(ADH_DEBUG_SELECT_IM_ABL="5"), dict(ADH_DEBUG_SELECT_IM_ABL="8"), dict(ADH_SELECT_SCRATCH_MB="1"),
                dict(ADH_SELECT_SCRATCH_MB="1", ADH_DEBUG_SELECT_IM_DENSE="1")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            got = run()
        for c in CANDIDATE_COLUMNS:
            assert np.array_equal(got[c], base[c]), (env, c)
    ctx.stage_run(case.dia, force=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("ADH_FUZZ_SEEDS_SELECT_IM", "5")))))
def test_hip_timstof_selection_randomized(ctx, oracle_lib, seed):
    """Differential test on ion-mobility runs: random geometry and settings, HIP == oracle."""
    import synthetic as syn

    rng = np.random.default_rng(4000 + seed)
    sm = int(rng.choice([64, 96, 128]))
    case = syn.make_timstof_case(
        n_precursors=int(rng.integers(40, 120)), n_cycles=int(rng.integers(50, 90)), config_id=800 + seed,
        per_precursor=1, n_ms2_frames=int(rng.integers(2, 6)), windows_per_frame=int(rng.integers(1, 4)),
        scan_max_index=sm, events_per_push=float(rng.choice([15.0, 40.0])), planted_fraction=float(rng.uniform(0.3, 0.8)),
    )
    cfg = CandidateSelectionConfig()
    cfg.update(dict(
        rt_tolerance=float(rng.choice([1.0, 2.5])), mobility_tolerance=float(rng.choice([0.2, 0.3, 0.45])),
        candidate_count=int(rng.integers(1, 6)), top_k_precursors=int(rng.integers(1, 5)),
        exclude_shared_ions=bool(rng.integers(0, 2)), min_size_rt=int(rng.integers(1, 4)),
        min_size_mobility=int(rng.integers(2, 9)), max_size_mobility=int(rng.integers(10, 25)),
        join_close_candidates=bool(rng.integers(0, 2)), use_weighted_score=bool(rng.integers(0, 2)),
        peak_len_rt=1.5, sigma_scale_rt=0.5, peak_len_mobility=0.06,
        kernel_size=int(rng.choice([20, 30])),
    ))
    case.dia.has_mobility = True
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size, cfg.peak_len_mobility,
                           cfg.sigma_scale_mobility)
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    pm = _pack(case.library.precursor_df)
    got = ctx.select_candidates(pm, cfg, kern)
    exp = oracle_lib.select_timstof(case.dia, cols, pm, cfg, kern, n_threads=4)
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c
