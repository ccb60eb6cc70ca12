"""Cases of candidate selection at the limits of the selection kernels (tests/test_selection_limits_gpu.py), and what
decides on the CPU that a case reaches the path it is meant for: the tile limits of both run layouts and the load of
the ion-mobility gather (events per m/z window, (window, TOF bin) pairs), recomputed in NumPy from the inputs.

Limits of the kernels (alphadia_amd/csrc/adh_select.hip, adh_select_im.hip):
  WB = 16 m/z windows per batch of the AlphaRaw kernel, MAX_CAND = 16 candidates, MAX_W = 64 windows per precursor on
  ion-mobility runs (one lane per window above 32), 512 events per window's sort list, 256 (window, TOF bin) pairs,
  150 KiB of LDS per tile."""
import numpy as np
import pandas as pd

import synthetic as syn
from alphadia_amd.scoring import fragment_columns
from alphadia_amd.selection import CANDIDATE_COLUMNS, CandidateSelectionConfig, gaussian_kernel

ISOTOPE_DELTA = 1.0033548350700006
WB, MAX_CAND, MAX_W = 16, 16, 64
IM_SORT_CAP, IM_PAIR_CAP = 512, 256
LDS_LIMIT = 150 * 1024
WINDOW_BYTES = 20  # gather::Window: three float32 bounds and two bin indices

RAW_RUN = dict(per_precursor=1, n_ms2=8, ms1_peaks=400, ms2_peaks=150, mz_lo=400, mz_hi=480, frag_mz_lo=200,
               frag_mz_hi=350, ms1_mz_range=(395, 500), ms2_mz_range=(195, 355), planted_fraction=0.7, threads=1)


def config(**updates) -> CandidateSelectionConfig:
    cfg = CandidateSelectionConfig()
    cfg.update(updates)
    return cfg


def assert_tables_equal(got: dict, exp: dict, what=""):
    """The suite's comparison for selection: every integer column equal, the score to 1e-6 relative; no row left out."""
    for c in CANDIDATE_COLUMNS:
        assert len(got[c]) == len(exp[c]), (what, c)
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), (what, c)
        else:
            assert np.array_equal(got[c], exp[c]), (what, c)
    print(f"[selection limits] {what} {int((np.asarray(exp['score']) > 0).sum())} rows equal to the oracle's")


def assert_tables_identical(got: dict, exp: dict, what=""):
    for c in CANDIDATE_COLUMNS:
        assert np.array_equal(got[c], exp[c]), (what, c)


def rows_per_precursor(table: dict, n_precursors: int, candidate_count: int) -> np.ndarray:
    """Filled ranks of every precursor (row i * candidate_count + r holds rank r of the i-th precursor)."""
    return (np.asarray(table["score"]).reshape(n_precursors, candidate_count) > 0).sum(axis=1)


def kept_fragments(pdf: pd.DataFrame, fdf: pd.DataFrame, exclude_shared_ions: bool) -> np.ndarray:
    """K of every precursor: fragments of the slice that pass the cardinality filter (selection.py:124-139)."""
    shared = np.concatenate([[0], np.cumsum(fdf["cardinality"].values > 1)])
    a, b = pdf.flat_frag_start_idx.values.astype(np.int64), pdf.flat_frag_stop_idx.values.astype(np.int64)
    return (b - a) - (shared[b] - shared[a] if exclude_shared_ions else 0)


# ---------------------------------------------------------------- AlphaRaw
def raw_tile_limits(dia, rt, rt_tolerance: float, kernel_size: int):
    """(first cycle, cycle count, branch) of every precursor's tile as adh_select_limits_kernel works them out
    (get_frame_indices_tolerance, alpharaw_jit.py:172-203).  branch: 0 the tile fits behind its first cycle, 1 moved
    back from the end of the run (cs = cmax - len >= 0), 2 longer than the run (cs = 0 or 1 by the parity of cmax)."""
    L = dia.cycle.shape[1]
    rts = np.asarray(dia.rt_values, dtype=np.float32)
    cmax = rts.shape[0] // L
    rt = np.asarray(rt, dtype=np.float32).astype(np.float64)
    lo, hi = (rt - rt_tolerance).astype(np.float32), (rt + rt_tolerance).astype(np.float32)
    c_lo, c_hi = np.searchsorted(rts, lo, "left") // L, np.searchsorted(rts, hi, "left") // L
    length = (np.maximum(c_hi - c_lo, kernel_size) + 15) // 16 * 16
    cs, ce, branch = c_lo.copy(), c_lo + length, np.zeros(len(rt), dtype=np.int64)
    over = ce > cmax
    branch[over] = np.where(cmax - length[over] >= 0, 1, 2)
    cs[over] = np.where(cmax - length[over] >= 0, cmax - length[over], cmax % 2)
    ce[over] = cmax
    return cs, ce - cs, branch


def raw_lds_bytes(f: int, n_lib: int, n_iso: int, k_rows: int, k_cols: int) -> int:
    """sel::lds_bytes: 144 bytes per cycle (score 8, two batches of 16 windows x 4, the two running sums 2 x 4) plus
    the window tables, the raw fragment m/z and the float64 smoothing kernel."""
    b = f * 8 + (n_lib + n_iso) * WINDOW_BYTES
    b = (b + 7) // 8 * 8
    b += ((n_lib + 1) & ~1) * 4 + WB * f * 4 + f * 4 * 2 + WB * f * 4
    b = (b + 7) // 8 * 8
    b += k_rows * k_cols * 8
    return (b + 15) // 16 * 16


def largest_raw_tile(n_lib: int, n_iso: int, k_rows: int, k_cols: int) -> int:
    f = 16
    while raw_lds_bytes(f + 16, n_lib, n_iso, k_rows, k_cols) <= LDS_LIMIT:
        f += 16
    return f


# K of the window-batch case: below, at and above one and two batches of 16 with four isotopes or one
BATCH_K = (4, 12, 13, 15, 16, 17, 28, 31, 32, 33, 48, 60)
# (slice length, shared fragments in it): with exclude_shared_ions K = 4 / 60 of 65, 6 / 60 of 130 (slice and sort
# loops longer than a wavefront), 2 of 10 and 3 of 40 (more than three in the library, no rows after the filter)
BATCH_SPECIAL = ((65, 61), (65, 5), (130, 124), (130, 70), (10, 8), (40, 37))


def window_batch_case():
    """A run of 100 cycles and a library of 60 fragments per precursor whose slices are cut by hand: eight precursors
    for every K of BATCH_K (no shared fragment among them: K is the same with and without the filter), then two for
    every entry of BATCH_SPECIAL, each followed by two precursors of two fragments (over whose fragments the long
    slices run)."""
    n_group, n_rep = 8, 2
    n = n_group * len(BATCH_K) + 3 * n_rep * len(BATCH_SPECIAL)
    case = syn.make_case(n, 100, config_id=141, k_fragments=60, **RAW_RUN)
    pdf, fdf = case.library.precursor_df, case.library.fragment_df
    start = pdf.flat_frag_start_idx.values.astype(np.int64)
    stop = start + 2
    k_group = np.repeat(BATCH_K, n_group)
    stop[: k_group.size] = start[: k_group.size] + k_group
    card = np.ones(len(fdf), dtype=np.uint8)
    rng = np.random.default_rng(141)
    special = []
    for j in range(n_rep * len(BATCH_SPECIAL)):
        i = k_group.size + 3 * j
        n_lib, n_shared = BATCH_SPECIAL[j // n_rep]
        stop[i] = start[i] + n_lib
        card[start[i] + rng.choice(n_lib, n_shared, replace=False)] = 2
        special.append(i)
    assert stop.max() <= len(fdf)
    pdf["flat_frag_stop_idx"] = stop.astype(np.uint32)
    fdf["cardinality"] = card
    return case, np.asarray(special)


# ---------------------------------------------------------------- ion mobility
def tims_tiles(dia, pdf: pd.DataFrame, cfg, kernel_shape):
    """(cycle_start, F, scan_start, S, ok) of every precursor as adh_select_plan_im_kernel works them out (frame limits
    as above with the zeroth frame, _get_scan_indices of bruker_jit.py:204-245 with its ceil of a negative quotient,
    the size rules of _is_valid)."""
    L, SM, z = dia.cycle.shape[1], int(dia.scan_max_index), int(dia.zeroth_frame)
    rts = np.asarray(dia.rt_values, dtype=np.float64)
    cmax = (rts.shape[0] - 1) // L
    rt = pdf.rt_library.values.astype(np.float32).astype(np.float64)
    lo = (rt - float(cfg.rt_tolerance)).astype(np.float32).astype(np.float64)
    hi = (rt + float(cfg.rt_tolerance)).astype(np.float32).astype(np.float64)
    c_lo, c_hi = (np.searchsorted(rts, lo, "left") + z) // L, (np.searchsorted(rts, hi, "left") + z) // L
    length = 16 * np.ceil(np.maximum(c_hi - c_lo, int(cfg.kernel_size)) / 16.0).astype(np.int64)
    cs, ce = c_lo.copy(), c_lo + length
    over = ce > cmax
    cs[over] = np.where(cmax - length[over] >= 0, cmax - length[over], cmax % 2)
    ce[over] = cmax
    mob = pdf.mobility_library.values.astype(np.float32).astype(np.float64)
    m_hi = (mob + float(cfg.mobility_tolerance)).astype(np.float32).astype(np.float64)
    m_lo = (mob - float(cfg.mobility_tolerance)).astype(np.float32).astype(np.float64)
    rev = np.asarray(dia.mobility_values, dtype=np.float64)[::-1]
    s_first, s_second = SM - np.searchsorted(rev, m_hi, "right"), SM - np.searchsorted(rev, m_lo, "right")
    opt = 16 * np.ceil((s_first - s_second) / 16.0).astype(np.int64)
    ss, se = s_first.copy(), s_first - opt
    neg = se < 0
    ss[neg] = np.minimum(opt[neg], SM)
    se[neg] = 0
    S, F = np.maximum(se - ss, 0), ce - cs
    ok = (F > 0) & (S > 0) & (S % 2 == 0) & (S >= kernel_shape[0]) & (F >= kernel_shape[1]) & (ss >= 0) & (ss + S <= SM)
    return cs, F, ss, S, ok


def tims_gather_load(dia, pdf: pd.DataFrame, fdf: pd.DataFrame, cfg, kernel_shape, n_iso: int):
    """Per precursor: K, the largest number of events that one m/z window queues (TOF index in the window's
    [tlo, thi), push inside the tile's frames, scan inside its scan range - before the quadrupole test, as the gather
    counts them), the number of (window, TOF bin) pairs and the first window (in the kernel's order: fragments by
    m/z, then isotopes) that queues more than IM_SORT_CAP events.  -1 where the precursor has no tile or K <= 3, and
    where no window is that full."""
    L, SM, z = dia.cycle.shape[1], int(dia.scan_max_index), int(dia.zeroth_frame)
    cs, F, ss, S, ok = tims_tiles(dia, pdf, cfg, kernel_shape)
    mzv = np.asarray(dia.mz_values, dtype=np.float64)
    push, indptr = np.asarray(dia.push_indices).astype(np.int64), np.asarray(dia.tof_indptr, dtype=np.int64)
    f_mz, f_card = fdf.mz_library.values.astype(np.float32), fdf.cardinality.values
    n = len(pdf)
    K, worst, pairs = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    first_over = np.full(n, -1, np.int64)
    for i, (a, b, mz, ch) in enumerate(zip(pdf.flat_frag_start_idx.values, pdf.flat_frag_stop_idx.values,
                                           pdf.mz_library.values, pdf.charge.values)):
        m = f_mz[a:b]
        if cfg.exclude_shared_ions:
            m = m[f_card[a:b] <= 1]
        K[i] = m.size
        if not ok[i] or K[i] <= 3:
            continue
        iso = (np.float64(np.float32(mz)) + np.arange(n_iso) * ISOTOPE_DELTA / float(ch)).astype(np.float32)
        centre = np.concatenate([np.sort(m), iso])
        tol = np.concatenate([np.full(m.size, np.float32(cfg.fragment_mz_tolerance)),
                              np.full(n_iso, np.float32(cfg.precursor_mz_tolerance))]).astype(np.float32)
        q = (tol * centre) / np.float32(1000000.0)  # mass_range (jitclasses/utils.py:15-20) in float32
        tlo = np.searchsorted(mzv, (centre - q).astype(np.float64), "left")
        thi = np.maximum(np.searchsorted(mzv, (centre + q).astype(np.float64), "left"), tlo)
        pairs[i] = int((thi - tlo).sum())
        p_lo, p_hi = (cs[i] * L + z) * SM, ((cs[i] + F[i]) * L + z) * SM
        worst[i] = 0
        for w, (t0, t1) in enumerate(zip(tlo, thi)):
            p = push[indptr[t0]:indptr[t1]]
            scan = p % SM
            queued = int(((p >= p_lo) & (p < p_hi) & (scan >= ss[i]) & (scan < ss[i] + S[i])).sum())
            worst[i] = max(worst[i], queued)
            if queued > IM_SORT_CAP and first_over[i] < 0:
                first_over[i] = w
    return K, worst, pairs, first_over


# W = K + 4 isotopes of the window-count case: 32 / 33 is where the gather goes from two lanes per window to one
IM_W = (8, 16, 31, 32, 33, 63, 64)
IM_RUN = dict(n_cycles=40, per_precursor=1, n_ms2_frames=3, windows_per_frame=2, scan_max_index=96,
              planted_fraction=0.5, n_tof=6000, events_per_push=10.0)
IM_CFG = dict(rt_tolerance=3.0, mobility_tolerance=0.3, min_size_rt=2, peak_len_rt=0.8, sigma_scale_rt=0.5,
              peak_len_mobility=0.03, sigma_scale_mobility=1.0, max_size_mobility=20, precursor_mz_tolerance=60.0,
              fragment_mz_tolerance=60.0)


def im_kernel(dia, cfg):
    return gaussian_kernel(dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size, cfg.peak_len_mobility,
                           cfg.sigma_scale_mobility)


def window_count_case():
    """An ion-mobility run and a library of 60 fragments per precursor whose slices are cut to K = W - 4 for every W
    of IM_W, six precursors each, followed by six whole slices of which a fifth of the fragments are shared."""
    n_group = 6
    n = n_group * (len(IM_W) + 1)
    case = syn.make_timstof_case(n_precursors=n, config_id=142, k_fragments=60, **IM_RUN)
    case.dia.has_mobility = True
    pdf, fdf = case.library.precursor_df, case.library.fragment_df
    start = pdf.flat_frag_start_idx.values.astype(np.int64)
    stop = pdf.flat_frag_stop_idx.values.astype(np.int64)
    k_group = np.repeat(IM_W, n_group) - 4
    stop[: k_group.size] = start[: k_group.size] + k_group
    card = np.ones(len(fdf), dtype=np.uint8)
    tail = np.arange(start[k_group.size], len(fdf))
    card[tail[np.random.default_rng(142).random(tail.size) < 0.2]] = 2
    pdf["flat_frag_stop_idx"] = stop.astype(np.uint32)
    fdf["cardinality"] = card
    return case


def staged(ctx, dia, fdf):
    cols = fragment_columns(fdf, "mz_library")
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    return cols


def copy_table(table: dict) -> dict:
    return {c: np.array(table[c], copy=True) for c in CANDIDATE_COLUMNS}
