"""Candidate selection past one batch of m/z windows and at its caps: the HIP kernels against the CPU oracle, which
tests/test_selection.py pins to the reference at these shapes (selection_limits.npz, selection_timstof_limits.npz).

Every comparison is the suite's own for selection (selection_limits.assert_tables_equal: integer columns equal, score
to 1e-6 relative, every row).  Every test first asserts, from its inputs or from the oracle's table alone, that it
reaches the path it is named for; those assertions hold without a GPU."""
import numpy as np
import pytest

import selection_limits as SL
import synthetic as syn
import test_selection as TS
from alphadia_amd.runtime import HipBackendError
from alphadia_amd.selection import gaussian_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def _sorted(pdf):
    return pdf.sort_values("precursor_idx").reset_index(drop=True)


# ---------------------------------------------------------------- AlphaRaw: batches of 16 windows
@pytest.fixture(scope="module")
def batch_case():
    return SL.window_batch_case()


@pytest.mark.parametrize("top_k_precursors,exclude_shared_ions", [(4, False), (1, False), (4, True)])
def test_window_batches(ctx, oracle_lib, batch_case, top_k_precursors, exclude_shared_ions):
    """K fragment windows and 1 or 4 isotope windows in batches of 16: one batch exactly (12 + 4), isotopes that open a
    batch (16 + 1, 16 + 4, 32 + 4), a batch that mixes the last fragments with the isotopes (13 + 4, 15 + 4, 17, 28,
    31, 33, 48, 60), the running sums carried over up to five batches (nine for the slices of 65 and 130 without the
    filter, whose slice and sort loops also go round more than once)."""
    case, special = batch_case
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    K = SL.kept_fragments(pdf, fdf, exclude_shared_ions)
    hist = {k: int((K == k).sum()) for k in SL.BATCH_K}
    assert all(c >= 8 for c in hist.values()), hist
    n_lib = (pdf.flat_frag_stop_idx.values.astype(np.int64) - pdf.flat_frag_start_idx.values)[special]
    assert sorted(set(n_lib)) == [10, 40, 65, 130]
    if exclude_shared_ions:  # long slices with few and many kept fragments; slices of more than three with K <= 3
        assert sorted(zip(n_lib, K[special])) == sorted(
            (n, n - s) for n, s in SL.BATCH_SPECIAL for _ in range(2))
        assert ((K[special] <= 3) & (n_lib > 3)).sum() == 4
    else:
        assert np.array_equal(K[special], n_lib)
    n_batches = -(-(K[K > 3] + top_k_precursors) // SL.WB)
    assert n_batches.min() == 1 and n_batches.max() >= 4
    mixed = (K > 3) & (K % SL.WB != 0) & (K // SL.WB > 0)  # fragments and isotopes share a batch behind the first
    assert mixed.sum() >= 40

    cfg = SL.config(rt_tolerance=30.0, candidate_count=3, min_size_rt=3, top_k_precursors=top_k_precursors,
                    exclude_shared_ions=exclude_shared_ions)
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=4)
    rows = SL.rows_per_precursor(exp, len(pdf), 3)
    assert (rows[K <= 3] == 0).all()
    assert (rows[K > 3] > 0).mean() >= 0.8
    for k in SL.BATCH_K:
        assert rows[K == k].sum() > 0, k
    got = ctx.select_candidates(pm, cfg, kern)
    SL.assert_tables_equal(got, exp)


# ---------------------------------------------------------------- AlphaRaw: sixteen candidates
@pytest.mark.parametrize("join", [False, True])
def test_sixteen_candidates(ctx, oracle_lib, join):
    """candidate_count = 16 on the run of the "many" fixture (every tile is the whole run of 260 cycles): the insertion
    list is full and goes on evicting, the joins run over 16 entries."""
    z, dia, fdf, pdf = TS._load("many")
    cfg = TS._cfg(z, "many")
    assert int(cfg.candidate_count) == SL.MAX_CAND and not bool(cfg.join_close_candidates)
    cfg.join_close_candidates = np.asarray(join)
    pdf, pm = _sorted(pdf), TS._pack(pdf)
    cols = SL.staged(ctx, dia, fdf)
    exp = oracle_lib.select(dia, cols, pm, cfg, z["many_kernel"], n_threads=4)
    rows = SL.rows_per_precursor(exp, len(pdf), 16)
    if not join:
        assert (rows == 16).sum() >= len(pdf) // 2  # (more peaks than ranks: 118 of 120)
    else:  # (the join of overlapping candidates took entries of full lists away)
        cfg.join_close_candidates = np.asarray(False)
        full = SL.rows_per_precursor(oracle_lib.select(dia, cols, pm, cfg, z["many_kernel"], n_threads=4), len(pdf), 16)
        cfg.join_close_candidates = np.asarray(True)
        assert ((full == 16) & (rows < 16)).sum() >= 10
    got = ctx.select_candidates(pm, cfg, z["many_kernel"])
    SL.assert_tables_equal(got, exp)
    if not join:
        n_both, n_diff = TS._compare_with_golden(TS._frame(got), z, "many", oracle_lib)
        assert n_both > 1800 and n_diff == TS.N_DIFF["raw", "many"]


def test_kernel_of_sixteen_cycles_on_the_fixture(ctx, oracle_lib):
    z, dia, fdf, pdf = TS._load("k16")
    cfg, pm = TS._cfg(z, "k16"), TS._pack(pdf)
    assert z["k16_kernel"].shape == (2, 16) and int(cfg.kernel_size) == 16
    cols = SL.staged(ctx, dia, fdf)
    exp = oracle_lib.select(dia, cols, pm, cfg, z["k16_kernel"], n_threads=4)
    got = ctx.select_candidates(pm, cfg, z["k16_kernel"])
    SL.assert_tables_equal(got, exp)
    n_both, n_diff = TS._compare_with_golden(TS._frame(got), z, "k16", oracle_lib)
    assert n_both > 700 and n_diff == TS.N_DIFF["raw", "k16"]


def test_seventeen_candidates_are_refused(ctx):
    z, dia, fdf, pdf = TS._load("many")
    cfg, pm = TS._cfg(z, "many"), TS._pack(pdf)
    SL.staged(ctx, dia, fdf)
    cfg.candidate_count = np.asarray(17)
    with pytest.raises(HipBackendError, match=r"candidate_count must be in 1\.\.16"):
        ctx.select_candidates(pm, cfg, z["many_kernel"])
    cfg.candidate_count = np.asarray(16)
    got = ctx.select_candidates(pm, cfg, z["many_kernel"])
    assert (got["score"] > 0).sum() > 1800


# ---------------------------------------------------------------- AlphaRaw: smoothing kernel shapes
@pytest.fixture(scope="module")
def smooth_case():
    return syn.make_case(100, 61, config_id=143, **SL.RAW_RUN)


def _hand_kernel(k1: int, first: int, count: int) -> np.ndarray:
    """(2, k1) float32 with `count` unequal, asymmetric positive taps from column `first` on, the rest zero."""
    rng = np.random.default_rng([k1, first, count])
    k = np.zeros((2, k1), dtype=np.float32)
    k[:, first:first + count] = (rng.uniform(0.05, 1.0, (2, count)) * np.linspace(0.3, 1.0, count)[None, :]).astype(np.float32)
    return k


def _smoothing_kernels(dia):
    cfg = SL.config()
    for ks in (16, 20, 31, 48):  # (an odd kernel_size gives the next even width, kernel.py)
        yield f"gaussian {ks}", ks, gaussian_kernel(dia, cfg.peak_len_rt, cfg.sigma_scale_rt, ks)
    yield "16 columns from 0", 30, _hand_kernel(30, 0, 16)       # col0 = 0
    yield "16 columns to 29", 30, _hand_kernel(30, 14, 16)       # col0 = k1 - 16
    yield "17 columns", 30, _hand_kernel(30, 6, 17)              # one too many for the fixed taps: taps from LDS
    yield "31 columns, odd", 31, _hand_kernel(31, 9, 13)         # odd k1: the centre column is k1 // 2
    yield "four columns at the end", 16, _hand_kernel(16, 12, 4) # the register window starts 19 cycles before the row


@pytest.mark.parametrize("which", range(9))
def test_smoothing_kernel_shapes(ctx, oracle_lib, smooth_case, monkeypatch, which):
    """The two-row smoothing kernel as scalar operands (up to 16 non-zero columns) and from LDS (more): against the
    oracle, and the two forms against each other bit for bit."""
    case = smooth_case
    label, ks, kern = list(_smoothing_kernels(case.dia))[which]
    nz = np.flatnonzero((kern != 0).any(axis=0))
    fixed = nz[-1] - nz[0] + 1 <= 16
    assert kern.shape[0] == 2 and kern.shape[1] == ks + ks % 2 * (label.startswith("gaussian"))
    assert fixed == (label != "17 columns" and not (label.startswith("gaussian") and nz.size > 16)), (label, nz)
    cfg = SL.config(rt_tolerance=20.0, candidate_count=5, min_size_rt=2, kernel_size=ks)
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=4)
    assert (exp["score"] > 0).sum() > 60
    got = SL.copy_table(ctx.select_candidates(pm, cfg, kern))
    SL.assert_tables_equal(got, exp, label)
    monkeypatch.setenv("ADH_DEBUG_SELECT_LDS_TAPS", "1")
    SL.assert_tables_identical(ctx.select_candidates(pm, cfg, kern), got, label)


@pytest.mark.parametrize("n_cycles,ks,rows", [(16, 16, True), (30, 30, True), (31, 30, True), (17, 16, True),
                                              (20, 30, False), (15, 16, False)])
def test_tile_as_long_as_the_kernel_and_shorter(ctx, oracle_lib, monkeypatch, n_cycles, ks, rows):
    """F == k1 (the tile is the whole run; with an odd number of cycles it starts at cycle 1): the register window of
    25 cycles is longer than a row of 16 or 17 and wraps more than once.  F < k1: no rows, as in the reference."""
    case = syn.make_case(60, n_cycles, config_id=144, **SL.RAW_RUN)
    cfg = SL.config(rt_tolerance=5.0, candidate_count=3, min_size_rt=1, kernel_size=ks)
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, ks)
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    cs, F, _ = SL.raw_tile_limits(case.dia, pdf.rt_library.values, 5.0, ks)
    if rows:
        assert (F == ks).all() and kern.shape[1] == ks and (cs + F <= n_cycles).all()
        assert n_cycles - ks == 1 or (cs == n_cycles % 2).all()  # (a run of one cycle more: tiles at cycle 0 and 1)
    else:
        assert (F < ks).all()
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=4)
    assert ((exp["score"] > 0).sum() > 20) == rows and (rows or (exp["score"] == 0).all())
    got = SL.copy_table(ctx.select_candidates(pm, cfg, kern))
    SL.assert_tables_equal(got, exp)
    monkeypatch.setenv("ADH_DEBUG_SELECT_LDS_TAPS", "1")
    SL.assert_tables_identical(ctx.select_candidates(pm, cfg, kern), got)


# ---------------------------------------------------------------- AlphaRaw: tile edges and length
@pytest.mark.parametrize("n_cycles", [60, 61])
@pytest.mark.parametrize("rt_tolerance", [20.0, 80.0, 400.0])
def test_tile_edges(ctx, oracle_lib, n_cycles, rt_tolerance):
    """Precursors at rt 0, at the last spectrum and in between, tolerances well under, a little under and well over the
    run (90 s): tiles that fit, tiles moved back from the end of the run (cs = cmax - len) and tiles longer than the
    run, which start at cycle 0 or 1 by the parity of the cycle count and are no multiple of 16 long."""
    case = syn.make_case(90, n_cycles, config_id=145, **SL.RAW_RUN)
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    rt = pdf.rt_library.values.copy()
    rt[0::3] = 0.0
    rt[1::3] = case.dia.rt_values[-1]
    pdf["rt_library"] = rt
    cs, F, branch = SL.raw_tile_limits(case.dia, rt, rt_tolerance, 30)
    if rt_tolerance == 20.0:
        assert (branch == 0).sum() >= 30 and (branch[1::3] == 1).all() and (F % 16 == 0).all() and (cs + F <= n_cycles).all()
        assert (cs[1::3] == n_cycles - F[1::3]).all() and (cs[0::3] == 0).all()
    else:
        assert (branch == 2).sum() >= 60 and (cs[branch == 2] == n_cycles % 2).all()
        assert (F[branch == 2] == n_cycles - n_cycles % 2).all() and (F[branch == 2] % 16 != 0).all()
    cfg = SL.config(rt_tolerance=rt_tolerance, candidate_count=4, min_size_rt=2)
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=4)
    assert (exp["score"] > 0).sum() > 150
    first = exp["frame_start"][exp["score"] > 0].min()
    assert first <= (cs.min() + 3) * case.dia.cycle.shape[1]  # (boxes at the first cycles of the tiles)
    got = ctx.select_candidates(pm, cfg, kern)
    SL.assert_tables_equal(got, exp)


@pytest.fixture(scope="module")
def long_case():
    return syn.make_case(40, 1100, config_id=146, per_precursor=1, n_ms2=4, ms1_peaks=60, ms2_peaks=30, mz_lo=400,
                         mz_hi=480, frag_mz_lo=200, frag_mz_hi=260, ms1_mz_range=(395, 500), ms2_mz_range=(195, 265),
                         planted_fraction=0.7, threads=4)


def test_longest_tile_and_its_refusal(ctx, oracle_lib, long_case):
    """The longest tile the LDS layout admits, and 16 cycles more: refused before the selection kernel is launched."""
    case = long_case
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    # sel::lds_bytes with 12 fragments, 4 isotopes and the (2, 30) kernel: 144 F + 16 windows x 20 + 12 x 4 + 480,
    # rounded up to 16 bytes, <= 153 600: F <= 1 060, so 1 056 as a multiple of 16
    f_max = SL.largest_raw_tile(12, 4, 2, 30)
    assert f_max == 1056 and SL.raw_lds_bytes(f_max + 16, 12, 4, 2, 30) > SL.LDS_LIMIT
    assert (pdf.flat_frag_stop_idx.values - pdf.flat_frag_start_idx.values == 12).all()
    cycle_time = 1.5
    fits, too_long = (f_max - 6) / 2 * cycle_time, (f_max + 10) / 2 * cycle_time
    _, F, _ = SL.raw_tile_limits(case.dia, pdf.rt_library.values, fits, 30)
    assert F.max() == f_max and (F == f_max).sum() >= 3
    _, F2, _ = SL.raw_tile_limits(case.dia, pdf.rt_library.values, too_long, 30)
    assert F2.max() == f_max + 16
    cfg = SL.config(rt_tolerance=fits, candidate_count=5, min_size_rt=2, top_k_precursors=4,
                    precursor_mz_tolerance=50.0, fragment_mz_tolerance=50.0)
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    assert kern.shape == (2, 30)
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=4)
    assert (SL.rows_per_precursor(exp, len(pdf), 5)[F == f_max] > 0).all()
    got = SL.copy_table(ctx.select_candidates(pm, cfg, kern))
    SL.assert_tables_equal(got, exp)
    cfg.update(dict(rt_tolerance=too_long))
    with pytest.raises(HipBackendError, match="exceeds 150 KiB"):
        ctx.select_candidates(pm, cfg, kern)
    cfg.update(dict(rt_tolerance=fits))
    SL.assert_tables_identical(ctx.select_candidates(pm, cfg, kern), got)


# ---------------------------------------------------------------- ion mobility: window counts
@pytest.fixture(scope="module")
def im_case():
    return SL.window_count_case()


@pytest.mark.parametrize("exclude_shared_ions", [False, True])
def test_im_window_counts(ctx, oracle_lib, im_case, exclude_shared_ions):
    """W = K + 4 m/z windows at 8, 16, 31, 32 (two lanes per window), 33, 63 and 64 (one lane per window, the cap)."""
    case = im_case
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    K = SL.kept_fragments(pdf, fdf, exclude_shared_ions)
    hist = {w: int((K + 4 == w).sum()) for w in SL.IM_W}
    assert all(c >= 6 for c in hist.values()), hist
    assert (K + 4).max() == SL.MAX_W
    if exclude_shared_ions:
        assert ((K[-6:] < 60) & (K[-6:] > 32)).all()  # (whole slices thinned by the filter)
    cfg = SL.config(candidate_count=16, top_k_precursors=4, exclude_shared_ions=exclude_shared_ions, **SL.IM_CFG)
    kern = SL.im_kernel(case.dia, cfg)
    _, _, _, _, ok = SL.tims_tiles(case.dia, pdf, cfg, kern.shape)
    assert ok.all()
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select_timstof(case.dia, cols, pm, cfg, kern, n_threads=4)
    rows = SL.rows_per_precursor(exp, len(pdf), 16)
    for w in SL.IM_W:
        assert (rows[K + 4 == w] > 0).sum() >= 3, w
    got = ctx.select_candidates(pm, cfg, kern)
    SL.assert_tables_equal(got, exp)


@pytest.mark.parametrize("name", ["many", "wide"])
def test_im_fixture_at_the_limits(ctx, oracle_lib, name):
    """selection_timstof_limits.npz: 8 ... 64 windows per precursor and 16 candidates against the oracle and the
    reference; "wide": about half the precursors queue more than 512 events in one window and fall back to dense tiles."""
    z, dia, fdf, pdf, cfg = TS._load_tims(name)
    pdf, pm = _sorted(pdf), TS._pack(pdf)
    kern = z[name + "_kernel"]
    K, worst, pairs, _ = SL.tims_gather_load(dia, pdf, fdf, cfg, kern.shape, 4)
    assert (K + 4).min() == 8 and (K + 4).max() == SL.MAX_W and (worst >= 0).all()
    over = (worst > SL.IM_SORT_CAP) | (pairs > SL.IM_PAIR_CAP)
    assert (over.sum() >= 10 and (~over).sum() >= 10) if name == "wide" else not over.any()
    cols = SL.staged(ctx, dia, fdf)
    exp = oracle_lib.select_timstof(dia, cols, pm, cfg, kern, n_threads=4)
    got = ctx.select_candidates(pm, cfg, kern)
    SL.assert_tables_equal(got, exp)
    n_both, n_diff = TS._compare_with_golden(TS._frame(got), z, name, oracle_lib, "tims", name + "_out_")
    assert n_both > 400 and n_diff == TS.N_DIFF["tims", name]


def test_im_more_than_64_windows_is_refused(ctx, im_case):
    """The refusal counts the slice, not K: 61 fragments and 4 isotopes are refused, and so are 70 fragments of which
    10 pass the cardinality filter, which the reference would process."""
    case = im_case
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df.copy()
    cfg = SL.config(candidate_count=3, top_k_precursors=4, exclude_shared_ions=True, **SL.IM_CFG)
    kern = SL.im_kernel(case.dia, cfg)
    SL.staged(ctx, case.dia, fdf)
    good = ctx.select_candidates(TS._pack(pdf), cfg, kern)
    good = SL.copy_table(good)
    assert (good["score"] > 0).sum() > 30
    start = pdf.flat_frag_start_idx.values.astype(np.int64)
    i = 6  # (a precursor with fragments of others behind its own)
    for n_lib in (61, 70):
        bad = pdf.copy()
        stop = bad.flat_frag_stop_idx.values.copy()
        stop[i] = start[i] + n_lib
        bad["flat_frag_stop_idx"] = stop
        if n_lib == 70:
            card = fdf["cardinality"].values.copy()
            card[start[i] + 10:start[i] + 70] = 2
            shared = fdf.copy()
            shared["cardinality"] = card
            assert SL.kept_fragments(bad, shared, True)[i] == 10
            SL.staged(ctx, case.dia, shared)
        with pytest.raises(HipBackendError, match="more than 64 m/z windows per precursor"):
            ctx.select_candidates(TS._pack(bad), cfg, kern)
    SL.staged(ctx, case.dia, fdf)
    SL.assert_tables_identical(ctx.select_candidates(TS._pack(pdf), cfg, kern), good)


# ---------------------------------------------------------------- ion mobility: dense tiles where the lists overflow
@pytest.mark.parametrize("setting", ["events", "pairs"])
def test_im_natural_dense_fallback(ctx, oracle_lib, monkeypatch, setting):
    """Sparse and dense precursors in one launch, decided by the gather itself: "events" - fragment windows of
    +-400 ppm in which some precursors queue more than 512 events for one window (after flushing the windows before
    it); "pairs" - up to 60 fragments at +-60 ppm on a fine TOF axis: more than 256 (window, TOF bin) pairs."""
    if setting == "events":
        case = syn.make_timstof_case(n_precursors=60, config_id=147, k_fragments=(4, 60),
                                     **dict(SL.IM_RUN, events_per_push=40.0, n_cycles=36))
        cfg = SL.config(candidate_count=5, top_k_precursors=4, **dict(SL.IM_CFG, fragment_mz_tolerance=400.0))
    else:
        case = syn.make_timstof_case(n_precursors=60, config_id=148, k_fragments=(4, 60),
                                     **dict(SL.IM_RUN, events_per_push=40.0, n_cycles=36, n_tof=60000))
        cfg = SL.config(candidate_count=5, top_k_precursors=4, **SL.IM_CFG)
    case.dia.has_mobility = True
    pdf, fdf = _sorted(case.library.precursor_df), case.library.fragment_df
    kern = SL.im_kernel(case.dia, cfg)
    K, worst, pairs, first_over = SL.tims_gather_load(case.dia, pdf, fdf, cfg, kern.shape, 4)
    live = worst >= 0
    over = live & ((worst > SL.IM_SORT_CAP) | (pairs > SL.IM_PAIR_CAP))
    under = live & ~over
    assert over.sum() >= 10 and under.sum() >= 10, (over.sum(), under.sum())
    if setting == "events":
        assert (live & (worst > SL.IM_SORT_CAP) & (pairs <= SL.IM_PAIR_CAP)).sum() >= 10
        # the overflowing window comes behind windows whose events were already flushed to where the tiles go
        assert ((pairs <= SL.IM_PAIR_CAP) & (first_over >= 3)).sum() >= 5
    else:
        assert (live & (pairs > SL.IM_PAIR_CAP) & (worst <= SL.IM_SORT_CAP)).sum() >= 10
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    exp = oracle_lib.select_timstof(case.dia, cols, pm, cfg, kern, n_threads=4)
    rows = SL.rows_per_precursor(exp, len(pdf), 5)
    assert (rows[over] > 0).sum() >= 8 and (rows[under] > 0).sum() >= 8
    got = SL.copy_table(ctx.select_candidates(pm, cfg, kern))
    SL.assert_tables_equal(got, exp)
    for env in (dict(ADH_DEBUG_SELECT_IM_DENSE="1"), dict(ADH_SELECT_SCRATCH_MB="1")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            SL.staged(ctx, case.dia, fdf)
            SL.assert_tables_identical(ctx.select_candidates(pm, cfg, kern), got, env)
    ctx.stage_run(case.dia, force=True)


# ---------------------------------------------------------------- ion mobility: sixteen candidates
@pytest.mark.parametrize("join", [False, True])
def test_im_sixteen_candidates(ctx, oracle_lib, join):
    """candidate_count = 16 on the run of the ion-mobility fixture: peak counts in every residue class mod 4 (the
    limits are worked out four peaks side by side) and full lists."""
    z, dia, fdf, pdf, cfg = TS._load_tims("many")
    assert int(cfg.candidate_count) == SL.MAX_CAND and not bool(cfg.join_close_candidates)
    cfg.join_close_candidates = np.asarray(join)
    pdf, pm = _sorted(pdf), TS._pack(pdf)
    cols = SL.staged(ctx, dia, fdf)
    exp = oracle_lib.select_timstof(dia, cols, pm, cfg, z["many_kernel"], n_threads=4)
    rows = SL.rows_per_precursor(exp, len(pdf), 16)
    assert {int(r) % 4 for r in rows[rows > 0]} == {0, 1, 2, 3}
    if not join:
        assert (rows == 16).sum() >= 1
    got = ctx.select_candidates(pm, cfg, z["many_kernel"])
    SL.assert_tables_equal(got, exp)
    print(f"[ion-mobility sixteen candidates join={join}] rows per precursor {np.bincount(rows, minlength=17)}")
