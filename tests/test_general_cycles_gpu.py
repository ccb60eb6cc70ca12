"""GPU: scoring and candidate selection on cycles the touching windows of ``syn.make_cycle`` cannot express - staggered
and overlapping isolation windows (two to five observations per candidate), several MS1 rows per cycle (also none at
row 0), a stretch of m/z outside every window - against the CPU oracle and against the reference's own tables
(tests/golden/make_golden.py, "general cycles").  Run with ``-m gpu`` on an MI355X."""

import numpy as np
import pytest

import helpers as H
import synthetic as syn
import test_oracle_golden as TG
import test_selection as TS
from alphadia_amd.scoring import CandidateScoringConfig, assemble_candidates, fragment_columns, pack_assembled
from test_gpu_parity import (PPM_ABS_TOL_GOLDEN, PPM_ABS_TOL_ORACLE, REL_TOL, _hip_score_tims, compare, hip_score)

pytestmark = pytest.mark.gpu

MAX_RESCUED = 2  # rows per feature that a knife-edge mask of `compare` may take out of a comparison


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def compare_bounded(got, exp, ppm_tol, **kw):
    """``compare`` with its knife-edge masks (features 16, 18, 19) bounded: they may rescue MAX_RESCUED rows each."""
    worst = compare(got, exp, ppm_tol, **kw)
    rescued = compare.last_masked["rescued"]
    assert all(rescued[f] <= MAX_RESCUED for f in (16, 18, 19)), rescued
    return worst


def copied(tables):
    return {k: np.array(v, copy=True) for k, v in tables.items()}


def equal_tables(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), k


def small_case(cycle, seed, n_precursors=160, n_cycles=60, per_precursor=2, **kw):
    """The shape of the scoring goldens (library m/z 400-480, fragments 200-350) on ``cycle``."""
    args = dict(n_precursors=n_precursors, n_cycles=n_cycles, per_precursor=per_precursor, ms1_peaks=300, ms2_peaks=100,
                mz_lo=400, mz_hi=480, frag_mz_lo=200, frag_mz_hi=350, ms1_mz_range=(395, 500), ms2_mz_range=(195, 355),
                few_fragment_fraction=0.05, even_fraction=0.3, planted_fraction=0.5, threads=1, seed=seed, cycle=cycle)
    args.update(kw)
    return syn.make_case(**args)


# ---------------------------------------------------------------- scoring against the oracle and the fixtures
@pytest.mark.parametrize("name", TG.CYCLE_GOLDENS)
def test_hip_matches_oracle_and_reference_on_general_cycles(ctx, oracle_lib, name):
    """Every fixture of the general cycles: HIP against the oracle (same typing, same order), the matched-peak
    counts exact, and HIP against the tables of the reference with the bounds of test_hip_matches_reference_goldens."""
    g = H.load_scoring_golden(name)
    got, soa = hip_score(ctx, g, g.config, with_stats=True)
    got = copied(got)
    exp, _ = H.oracle_score(oracle_lib, g, g.config, soa=soa, n_threads=4, with_stats=True)
    compare_bounded(got, exp, PPM_ABS_TOL_ORACLE)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    compare_bounded(got, g.expected, PPM_ABS_TOL_GOLDEN, rel_tol=REL_TOL, corr_abs=1e-3)
    assert got["valid"].sum() >= 140
    if name.startswith("dense_overlap"):  # candidates outside every window: the reference raises, here valid = 0
        key_out = soa["precursor_idx"].astype(np.int64) * 256 + soa["rank"]
        key_in = g.z["cand_precursor_idx"].astype(np.int64) * 256 + g.z["cand_rank"]
        outside = np.isin(key_out, key_in[g.z["cand_n_windows"] == 0])
        assert outside.sum() >= 1 and not got["valid"][outside].any()


# ---------------------------------------------------------------- every kernel family with several MS1 rows
@pytest.mark.parametrize("name", ["multi_ms1", "multi_ms1_twin", "multi_ms1_manyfrag"])
def test_every_kernel_family_with_several_ms1_rows(ctx, oracle_lib, monkeypatch, name):
    """With more than one MS1 row per cycle the fused kernel is off: the gather kernel collects the MS1 observations
    (raw1[(i * M1 + j) * F + f]) and collapses them for the register kernels, the wide register kernels (17-40
    fragments) and the generic kernel alike.  The default run records gather time, equals the oracle, and equals bit
    for bit the run that the generic kernel alone scores (ADH_DEBUG_NO_FAST) and, for the wide library, the run
    without the wide register kernels (ADH_DEBUG_NO_WIDE)."""
    g = H.load_scoring_golden(name)
    assert len(syn.ms1_rows_of(g.dia.cycle)) == 2
    ctx.kernel_time_ms(reset=True)
    got, soa = hip_score(ctx, g, g.config, with_stats=True)
    got = copied(got)
    gather_ms, feature_ms, _ = ctx.kernel_time_ms(reset=True)
    assert gather_ms > 0 and feature_ms > 0, (gather_ms, feature_ms)
    exp, _ = H.oracle_score(oracle_lib, g, g.config, soa=soa, n_threads=4, with_stats=True)
    compare_bounded(got, exp, PPM_ABS_TOL_ORACLE)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_NO_FAST", "1")
        generic, _ = hip_score(ctx, g, g.config, soa=soa, with_stats=True)
        equal_tables(got, generic)
    if name == "multi_ms1_manyfrag":
        kept = (got["fragment_mz_library"] > 0).sum(axis=1)
        assert kept.max() > 16  # (rows of the wide register kernels)
        with monkeypatch.context() as mp:
            mp.setenv("ADH_DEBUG_NO_WIDE", "1")
            no_wide, _ = hip_score(ctx, g, g.config, soa=soa, with_stats=True)
            equal_tables(got, no_wide)


# ---------------------------------------------------------------- two and three-plus observations, quant_all on / off
@pytest.mark.parametrize("quant_all", [True, False])
@pytest.mark.parametrize("name", ["staggered", "dense_overlap"])
def test_two_and_more_observations_with_quant_all_on_and_off(ctx, oracle_lib, name, quant_all):
    """The plan sends two observations to the register classes only with quant_all and three or more to the generic
    kernel: both geometries in both settings against the oracle."""
    g = H.load_scoring_golden(name)
    cfg = CandidateScoringConfig()
    cfg.update({k: getattr(g.config, k) for k in H.CFG_KEYS})
    cfg.update(dict(quant_all=quant_all))
    got, soa = hip_score(ctx, g, cfg, with_stats=True)
    exp, _ = H.oracle_score(oracle_lib, g, cfg, soa=soa, n_threads=4, with_stats=True)
    compare_bounded(got, exp, PPM_ABS_TOL_ORACLE)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    nobs = exp["features"][exp["valid"].astype(bool)][:, 17]
    assert (nobs >= 3).sum() >= 20 and (name != "staggered" or (nobs == 2).sum() >= 20)


# ---------------------------------------------------------------- tiles
@pytest.mark.parametrize("geometry", TG.GET_DENSE_GEOMETRIES)
def test_hip_dense_tile_matches_reference_on_general_cycles(ctx, geometry):
    """The gather kernel's tile (adh_debug_get_dense) against AlphaRawJIT.get_dense on the general cycles, fragment
    queries and MS1 queries (quadrupole (-1, -1): two or three MS1 rows): the observation list equal, both planes bit
    for bit."""
    z = np.load(H.golden_path("get_dense_cycles.npz"))
    ctx.stage_run(H.dia_from_npz({k[len(geometry) + 1:]: z[k] for k in z.files if k.startswith(geometry + "_dia_")}), force=True)
    hits, ms1_queries = 0, 0
    for i in range(int(z["n_cases"])):
        q = f"{geometry}_q{i}_"
        fl, quad, e = z[q + "frame_limits"], z[q + "quad"], z[q + "dense"]
        dense, obs = ctx.debug_get_dense(fl[0, 0], fl[0, 1], z[q + "mz"], z[q + "tol"], quad[0, 0], quad[0, 1])
        assert np.array_equal(obs, z[q + "pidx"]), i
        assert dense.shape == e.shape[:3] + (1,) + e.shape[4:], (dense.shape, e.shape)
        for slot in (0, 1):  # the reference writes the same value to both scan slots
            assert np.array_equal(dense[0, :, :, 0, :], e[0, :, :, slot, :]), f"intensity, case {i}"
            assert np.array_equal(dense[1, :, :, 0, :], e[1, :, :, slot, :]), f"m/z, case {i}"
        hits += int((e[0] > 0).sum())
        ms1_queries += int(quad[0, 0] == -1.0 and len(obs) == len(syn.ms1_rows_of(z[geometry + "_dia_cycle"])))
    assert hits > 30 and ms1_queries == int(z["n_cases"]) // 2


# ---------------------------------------------------------------- selection
N_DIFF_CYCLES = 34  # boxes of the exact convolution that differ from the fixture's FFT smoothing: from the oracle, on the CPU


def test_hip_selection_on_staggered_windows_with_two_ms1_rows(ctx, oracle_lib):
    """HipCandidateSelection where every precursor sums two or three fragment rows and two MS1 rows per cycle (in
    ascending row order: the reference's running float32 sum): the kernel's table equals the oracle's, and against
    the fixture every differing box is a near tie (NEAR_TIE_SCORE) and never a precursor's best - N_DIFF_CYCLES of
    them, the number the oracle gives against the fixture on the CPU
    (test_every_box_that_differs_from_the_reference_is_a_near_tie[raw-cycles])."""
    from alphadia_amd.selection import CANDIDATE_COLUMNS

    z, dia, fdf, pdf = TS._load("cycles")
    cols = fragment_columns(fdf, "mz_library")
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    cfg = TS._cfg(z, "cycles")
    got = ctx.select_candidates(TS._pack(pdf), cfg, z["cycles_kernel"])
    exp = oracle_lib.select(dia, cols, TS._pack(pdf), cfg, z["cycles_kernel"], n_threads=4)
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c
    n_both, n_diff = TS._compare_with_golden(TS._frame(got), z, "cycles", oracle_lib)
    assert n_both > 400 and n_diff == N_DIFF_CYCLES


# ---------------------------------------------------------------- ion mobility
def test_timstof_fixture_with_two_ms1_frames_and_repeated_ms2_frames(ctx, oracle_lib):
    z, dia, fragment_df, precursor_df, cand, cfg = TG._tims_golden("scoring_timstof_cycles.npz")
    soa = assemble_candidates(cand, precursor_df, "mz_library")
    got = _hip_score_tims(ctx, dia, fragment_df, soa, cfg, with_stats=True)
    exp = oracle_lib.score_timstof(dia, fragment_columns(fragment_df, "mz_library"), pack_assembled(soa),
                                   cfg.to_jitclass(), with_stats=True)
    assert np.array_equal(got["valid"].astype(bool), exp["valid"].astype(bool))
    compare_bounded(got, exp, PPM_ABS_TOL_ORACLE)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    golden = {n: z["out_" + n] for n in H.OUT_NAMES}
    compare_bounded(got, golden, PPM_ABS_TOL_GOLDEN, rel_tol=REL_TOL, corr_abs=1e-3)
    v = got["valid"].astype(bool)
    assert (got["features"][v][:, 17] >= 3).sum() >= 20


@pytest.mark.parametrize("repeats,quant_all", [(2, True), (2, False), (3, True), (3, False)])
def test_timstof_repeated_windows_and_two_ms1_frames(ctx, oracle_lib, repeats, quant_all):
    """Two MS1 frames per cycle (n_ms1 = 2) and the same m/z window at the same scans in two (class of two
    observations) or three MS2 frames (the generic ion-mobility class) against the oracle."""
    S = 64
    cycle = syn.make_timstof_cycle(3, 2, S, 400.0, 480.0, n_ms1_frames=2, repeats=repeats)
    case = syn.make_timstof_case(n_precursors=120, n_cycles=36, config_id=600 + repeats, scan_max_index=S, n_tof=24000,
                                 events_per_push=15.0, candidates_on_window=True, cycle=cycle)
    soa = assemble_candidates(case.candidates_df, case.library.precursor_df, "mz_library")
    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, quant_all=quant_all, experimental_xic=True))
    got = _hip_score_tims(ctx, case.dia, case.library.fragment_df, soa, cfg, with_stats=True)
    exp = oracle_lib.score_timstof(case.dia, fragment_columns(case.library.fragment_df, "mz_library"),
                                   pack_assembled(soa), cfg.to_jitclass(), n_threads=8, with_stats=True)
    assert np.array_equal(got["valid"].astype(bool), exp["valid"].astype(bool))
    compare_bounded(got, exp, PPM_ABS_TOL_ORACLE)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    nobs = exp["features"][exp["valid"].astype(bool)][:, 17]
    assert (nobs == repeats).sum() >= 20 and nobs.min() >= repeats
    if repeats == 3:
        assert (nobs >= 3).sum() >= 20


# ---------------------------------------------------------------- one randomised test
RANDOM_CYCLE_SEEDS = [0, 1, 2, 3]


def random_cycle_case(seed):
    """Drawn geometry (window overlap 0-0.7, 1-3 MS1 rows at random rows, an uncovered stretch half of the time) and
    the settings test_randomized_shapes_and_settings draws."""
    rng = np.random.default_rng(7000 + seed)
    cycle = syn.make_random_cycle(rng)
    case = small_case(cycle, seed=syn.BASE_SEED + 700 + seed, n_precursors=int(rng.integers(80, 260)),
                      n_cycles=int(rng.integers(40, 110)), per_precursor=int(rng.integers(1, 4)),
                      ms1_peaks=int(rng.integers(100, 900)), ms2_peaks=int(rng.integers(40, 400)),
                      frag_mz_hi=float(rng.choice([320.0, 500.0])), ms2_mz_range=(195, 520),
                      few_fragment_fraction=float(rng.choice([0.0, 0.15])), even_fraction=float(rng.choice([0.0, 0.5])),
                      planted_fraction=float(rng.uniform(0.2, 0.9)),
                      k_fragments=12 if rng.random() < 0.5 else (int(rng.integers(4, 14)), int(rng.integers(14, 61))))
    if rng.random() < 0.5:  # shared fragments
        card = case.library.fragment_df["cardinality"].values.copy()
        card[rng.random(card.size) < 0.2] = 2
        case.library.fragment_df["cardinality"] = card
    upd = dict(
        top_k_fragments=int(rng.choice([4, 6, 12, 16, 20, 33, 9999])), top_k_isotopes=int(rng.integers(1, 5)),
        precursor_mz_tolerance=float(rng.choice([5, 10, 40, 150])),
        fragment_mz_tolerance=float(rng.choice([7, 15, 60, 200])),
        exclude_shared_ions=bool(rng.integers(0, 2)), quant_window=int(rng.integers(1, 6)),
        quant_all=bool(rng.integers(0, 2)), experimental_xic=bool(rng.integers(0, 2)),
    )
    cfg = CandidateScoringConfig()
    cfg.update(upd)
    return case, cfg, upd


@pytest.mark.parametrize("seed", RANDOM_CYCLE_SEEDS)
def test_randomized_cycles_and_settings(ctx, oracle_lib, seed):
    case, cfg, upd = random_cycle_case(seed)
    got, soa = hip_score(ctx, case, cfg, with_stats=True)
    exp, _ = H.oracle_score(oracle_lib, case, cfg, soa=soa, n_threads=4, with_stats=True)
    # experimental_xic = False: the K x K contraction runs on MFMA, its summation order is not the oracle's: correlations
    # near zero get the absolute floor of test_randomized_shapes_and_settings
    compare_bounded(got, exp, PPM_ABS_TOL_ORACLE, corr_abs=0.0 if upd["experimental_xic"] else 2e-6)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"]), upd
    assert exp["valid"].sum() >= 20


# ---------------------------------------------------------------- refusals (host-side validation: no scoring kernel runs)
def _stage(ctx, case):
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)


def test_more_than_8_overlapping_windows_are_refused(ctx):
    from alphadia_amd.runtime import HipBackendError

    cycle = syn.cycle_from_rows([(-1.0, -1.0)] + [(400.0 - k, 480.0 + k) for k in range(9)])
    case = small_case(cycle, seed=syn.BASE_SEED + 801, n_precursors=24, n_cycles=40, ms1_peaks=50, ms2_peaks=20)
    cfg = CandidateScoringConfig()
    _stage(ctx, case)
    with pytest.raises(HipBackendError, match="more than 8 isolation windows"):
        ctx.score_host(pack_assembled(H.soa_for(case, cfg)), cfg.to_jitclass())
    # eight are scored
    cycle = syn.cycle_from_rows([(-1.0, -1.0)] + [(400.0 - k, 480.0 + k) for k in range(8)])
    case = small_case(cycle, seed=syn.BASE_SEED + 801, n_precursors=24, n_cycles=40, ms1_peaks=50, ms2_peaks=20)
    _stage(ctx, case)
    got = ctx.score_host(pack_assembled(H.soa_for(case, cfg)), cfg.to_jitclass())
    v = got["valid"].astype(bool)
    assert v.sum() >= 5 and (got["features"][v][:, 17] == 8).all()


def test_timstof_more_than_16_ms1_rows_in_the_scan_range_are_refused(ctx):
    from alphadia_amd.runtime import HipBackendError

    S = 48
    cycle = syn.make_timstof_cycle(2, 2, S, 400.0, 480.0, n_ms1_frames=17)
    case = syn.make_timstof_case(n_precursors=20, n_cycles=20, config_id=610, scan_max_index=S, n_tof=6000,
                                 events_per_push=2.0, cycle=cycle)
    soa = assemble_candidates(case.candidates_df, case.library.precursor_df, "mz_library")
    cfg = CandidateScoringConfig()
    _stage(ctx, case)
    with pytest.raises(HipBackendError, match="more than 16 unfragmented cycle rows"):
        ctx.score_host(pack_assembled(soa), cfg.to_jitclass())


@pytest.mark.parametrize("group", ["windows", "ms1"])
def test_selection_refuses_more_than_16_rows_of_a_group(ctx, group):
    """Candidate selection sums at most 16 cycle rows per group (rows overlapping the isotope range, MS1 rows): a
    cycle with more is refused on the host, as scoring refuses more than 8 observations - it used to sum the first 16
    silently, where the reference sums them all."""
    from alphadia_amd.runtime import HipBackendError
    from alphadia_amd.selection import CandidateSelectionConfig, gaussian_kernel

    many = [(400.0 - 0.1 * k, 480.0 + 0.1 * k) for k in range(17)]
    rows = ([(-1.0, -1.0)] + many) if group == "windows" else ([(-1.0, -1.0)] * 17 + [(400.0, 440.0), (440.0, 480.0)])
    case = small_case(syn.cycle_from_rows(rows), seed=syn.BASE_SEED + 802, n_precursors=24, n_cycles=40, ms1_peaks=20, ms2_peaks=20)
    _stage(ctx, case)
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=30.0, candidate_count=2))
    kernel = gaussian_kernel(case.dia, 10.0, 0.1, 30)
    with pytest.raises(HipBackendError, match="more than 16 cycle rows"):
        ctx.select_candidates(TS._pack(case.library.precursor_df), cfg, kernel)
    # sixteen are selected from
    rows = ([(-1.0, -1.0)] + many[:16]) if group == "windows" else ([(-1.0, -1.0)] * 16 + [(400.0, 440.0), (440.0, 480.0)])
    case = small_case(syn.cycle_from_rows(rows), seed=syn.BASE_SEED + 802, n_precursors=24, n_cycles=40, ms1_peaks=20, ms2_peaks=20)
    _stage(ctx, case)
    got = ctx.select_candidates(TS._pack(case.library.precursor_df), cfg, gaussian_kernel(case.dia, 10.0, 0.1, 30))
    assert (got["score"] > 0).sum() >= 10


def test_ms1_tile_beyond_the_lds_is_refused_before_any_launch(ctx):
    """The gather kernel keeps isotopes x MS1 rows x cycles raw cells in LDS (adh_gather_lds_bytes): 3 x 300 x 29
    cells of 8 bytes are 204 KiB, more than the 160 KiB of a CU.  The host refuses the batch; nothing is launched."""
    from alphadia_amd.runtime import HipBackendError

    rows = [(-1.0, -1.0)] * 300 + [(400.0 + 10.0 * k, 410.0 + 10.0 * k) for k in range(8)]
    case = small_case(syn.cycle_from_rows(rows), seed=syn.BASE_SEED + 803, n_precursors=12, n_cycles=40, ms1_peaks=2,
                      ms2_peaks=20, planted_fraction=0.2)
    cand = case.candidates_df
    L = case.dia.cycle_len
    cand.loc[0, ["frame_start", "frame_center", "frame_stop"]] = [5 * L, 19 * L, 34 * L]  # 29 cycles
    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, quant_all=True, experimental_xic=True))
    _stage(ctx, case)
    with pytest.raises(HipBackendError, match="MS1 tile too large"):
        ctx.score_host(pack_assembled(H.soa_for(case, cfg)), cfg.to_jitclass())
