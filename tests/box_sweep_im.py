"""A deterministic sweep of candidate SHAPES on an ion-mobility (timsTOF) run, and the routing rules of that path
restated in Python: what tests/box_sweep.py is for the AlphaRaw layout.

Candidate scoring on an ion-mobility run is routed twice.  The device plan (``adh_plan_rec_im_kernel``, adh_plan.hip)
puts a candidate into a class by its observation count and, with one observation, by its tile: ``plan_class_im``.
The host (``launch_scoring_im``, adh_score_host.hip) then picks one instantiation of the feature kernel per class from
the MAXIMA of a launch: ``instantiation_of``.  ``make_timstof_case`` draws boxes of 5 ... 21 cycles x 6 ... 24 scans away
from every edge of the run; this module crosses, on a small run that ends inside a cycle,

* the cycle count F = 2 ... 36 and the scan count S = 2 ... 48, paired so that planes of exactly 640, 641 ... 672, 1152
  and 1153 ... cells occur (both sides of every capacity of the three fixed layouts),
* boxes that touch scan 0, that touch ``scan_max_index`` and interior ones; boxes on the first frame after the zeroth,
  on the last complete cycle (``frame_stop`` on the cycle boundary, or clipped to the last frame) and interior ones,
* ``scan_center`` / ``frame_center`` on the first, the middle and the last scan / cycle of the box,
* one and two observations (precursor mid-window / isotope range across a window boundary), three and six on the
  cycle with every MS2 frame three times, and two MS1 rows on the cycle with two MS1 frames,
* library slices of 1 ... 40 fragments,
* scoring BATCHES (column ``batch``) whose maxima sit below, at and one step past the limits of the fixed layouts,
* and candidates whose events are written cell by cell (column ``density``), one per rung of the overflow ladder of
  the gather kernel (adh_gather_im.hip): nothing is drawn at random inside those boxes.  The pair capacity has a run
  of its own with a four times finer TOF axis ("fine"), on which planted peptides are over it or under it by the
  width of their windows alone.

Every other precursor is planted as a Gaussian in cycle and scan around the middle of its box.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

import synthetic as syn

# ---- the constants of the kernels, restated (adh_plan.hip, adh_device.h, adh_features_im.hip) --------------------
CLASS_ONE, CLASS_TWO, CLASS_SMALL, CLASS_GENERIC, N_CLASSES = 0, 1, 2, 36, 37
SMALL_K, SMALL_S, SMALL_F, SMALL_SF = 12, 32, 24, 640
COMMON_K, COMMON_S, COMMON_F, COMMON_I, COMMON_SF = 12, 40, 32, 3, 1152
SORT_CAP, PAIR_CAP = 512, 256
IM_STATIC_LDS = 128 * 20
LDS_LIMIT = 160 * 1024
NUM_FEATURES = 46
N_ISOTOPE_COLUMNS = 4
MARGIN = 1.5          # every designed event count is this factor away from the capacity on its side

# ---- the run ---------------------------------------------------------------------------------------------------
S_MAX = 64
N_MS2, WINDOWS_PER_FRAME = 5, 2
N_CYCLES = 48
TRUNCATE = 2          # frames cut off the end: the run ends inside its last cycle
N_TOF = 24000
N_TOF_FINE = 96000    # the run of the pair capacity: a 200 ppm fragment window holds 33 ... 44 TOF bins there
NOISE_PER_PUSH = 1.0
SEED = 20261019
MZ_LO, MZ_HI = 400.0, 480.0
RUNS = {"base": dict(), "obs3": dict(repeats=3), "ms1x2": dict(n_ms1_frames=2), "fine": dict(n_tof=N_TOF_FINE)}
# The draw of the fixture: one on which no row sits on the diff_b_y_ion_intensity cancellation (box_sweep.GOLDEN_SEED).
GOLDEN_SEED = 7

S_ALL = (2, 3, 4, 12, 20, 24, 27, 31, 32, 33, 36, 39, 40, 41, 48)
F_ALL = tuple(range(2, 37))
NL_ALL = (1, 2, 3, 11, 12, 13, 16, 40)
S_EDGES = ((32, 33), (40, 41))
F_EDGES = ((2, 3), (24, 25), (32, 33))
# planes on both sides of the two plane limits, as (S, F)
PLANES_AT = {640: ((32, 20),), 648: ((27, 24),), 672: ((32, 21),), 1152: ((36, 32),), 1120: ((40, 28),), 1160: ((40, 29),)}
DENSITIES = ("window_over_one", "window_over_two", "isotopes_over", "many_batches", "full_tile")
# the rungs whose candidates leave the sparse path by design
DENSE_BY_DESIGN = ("window_over_two", "full_tile")
# The pair capacity, on the run "fine" under the configuration "wide_tolerance": planted peptides whose twelve fragment
# windows hold 1.5 x ADH_IM_PAIR_CAP TOF bins and more ("pairs_over"), and ones with four fragments at the low end of the
# m/z range whose windows hold ADH_IM_PAIR_CAP / 1.5 bins at most ("pairs_fit").  (With a tile layout staged whose
# (window, tile) pairs fit, the gather counts those instead: the rung is met with ADH_IM_TILED=0.)
PAIR_DENSITIES = ("pairs_over", "pairs_fit")
PAIR_SHAPES = ((12, 12), (20, 20), (33, 12), (36, 20))


def _is_small(S, F):
    return S <= SMALL_S and F <= SMALL_F and S * F <= SMALL_SF


def _batch_shapes() -> dict:
    """(S, F) pairs of every scoring batch of the base run.  A batch is what one launch sees: its maxima choose the
    instantiation."""
    b = {}
    # (a) every row within the small limits
    b["a"] = [(S, F) for F in range(2, SMALL_F + 1) for S in S_ALL if _is_small(S, F)] + [(32, 20)] * 4
    # (b) maxima exactly at the common limits: 36 x 32 = 1152 cells, and 40 x 28 with S at its limit
    b["b1"] = [(S, F) for F in range(3, 33) for S in (20, 27, 31, 32, 33, 36) if not _is_small(S, F) or (S + F) % 5 == 0]
    b["b1"] += [(27, 24), (32, 21), (36, 32)] * 4
    b["b2"] = [(S, F) for F in range(3, 29) for S in (33, 39, 40)] + [(40, 28)] * 4
    b["b2"] += [(33, 2), (36, 2), (39, 2), (40, 2)] * 2   # two-cycle boxes in a split launch of the common layout
    # (c) one step past them: S = 41 and more, F = 33 and more, a plane of 1153 and more cells with both axes inside
    b["c_s"] = [(S, F) for F in range(2, 29, 2) for S in (41, 48) if S * F <= COMMON_SF] + [(12, 12), (20, 20), (33, 12)] * 4
    b["c_f"] = [(S, F) for F in (33, 34, 35, 36) for S in (2, 4, 12, 24, 31, 32)] + [(12, 12), (20, 20), (33, 12)] * 4
    b["c_sf"] = [(S, F) for F in (29, 30, 31, 32) for S in (36, 39, 40)] * 2 + [(12, 12), (20, 20), (33, 12), (40, 28), (40, 29)] * 4
    # a launch whose longest box has two cycles (the split path asks for three)
    b["f2"] = [(S, 2) for S in S_ALL if S <= COMMON_S] * 3
    return b


# density rows: (density, S, F, O, batch, scan position).  The boxes lie inside the scans of one group of windows
# (0 ... 30), so every cell of every plane can hold an event.
_DENSITY_ROWS = (
    [("full_tile", S, 3, O, "a", pos) for S in (2, 3, 4) for O in (1, 2) for pos in (0, 1)] +
    [("full_tile", 31, 25, O, "b1", 0) for O in (1, 1, 1, 1, 2, 2, 2, 2)] +
    [("window_over_two", 20, 20, 2, bt, pos) for bt in ("a", "b1") for pos in (0, 1) for _ in range(2)] +
    [("window_over_one", 30, 32, 1, "b1", pos) for pos in (0, 1) for _ in range(2)] +
    [("isotopes_over", 30, 32, 1, "b1", pos) for pos in (0, 1) for _ in range(2)] +
    [("many_batches", 24, 20, O, bt, pos) for bt in ("a", "b1") for O in (1, 2) for pos in (0, 1)]
)


def spec_rows(run: str = "base") -> pd.DataFrame:
    """One row per candidate.  Columns: S, F, the position of the box on the cycle axis (``pos_f``: 0 first frame after
    the zeroth / 1 interior / 2 last complete cycle / 3 the same with ``frame_stop`` clipped to the last frame) and on
    the scan axis (``pos_s``: 0 scan 0 / 1 interior / 2 ``scan_max_index``), the centres (0 first / 1 middle / 2 last),
    the designed observations ``O`` (1 mid-window, 2 across a window boundary), the slice length ``nl``, the scoring
    batch and the density design ('' = planted peptide).  Pure arithmetic: no random numbers."""
    rows = []
    i = 0

    def add(S, F, O, batch, density="", pos_s=None, nl=None):
        nonlocal i
        nl = nl if nl is not None else (12 if density else NL_ALL[(i + i // 8) % len(NL_ALL)])
        rows.append((S, F, i % 4, (i // 4) % 3 if pos_s is None else pos_s, (i // 12 + i) % 3, (i // 36 + i // 3) % 3, O,
                     nl, batch, density))
        i += 1

    if run == "base":
        for batch, shapes in _batch_shapes().items():
            for S, F in shapes:
                for O in (1, 2):
                    add(S, F, O, batch)
        for density, S, F, O, batch, pos_s in _DENSITY_ROWS:
            add(S, F, O, batch, density, pos_s)
    elif run == "obs3":   # (d) three and six observations: the generic class, the layout of the launch
        for S, F in [(S, F) for F in (2, 3, 8, 16, 24) for S in (2, 12, 24, 32)] * 2 + [(33, 25), (36, 12), (40, 20), (20, 32)] * 2:
            for O in (1, 2):
                add(S, F, O, "d")
    elif run == "ms1x2":  # two MS1 rows per cycle
        for S, F in [(S, F) for F in (2, 3, 12, 20, 24, 25) for S in (3, 12, 24, 32, 33)] * 2:
            for O in (1, 2):
                add(S, F, O, "m")
    elif run == "fine":   # the pair capacity: small, common and two-observation launches, dense next to sparse rows
        for _ in range(4):
            for S, F in PAIR_SHAPES:
                for O in (1, 2):
                    add(S, F, O, "p", "pairs_over", nl=12)
                    add(S, F, O, "p", "pairs_fit", nl=4)
    else:
        raise KeyError(run)
    return pd.DataFrame(rows, columns=["S", "F", "pos_f", "pos_s", "ce_f", "ce_s", "O", "nl", "batch", "density"])


def golden_spec() -> pd.DataFrame:
    """The thinned sweep of the reference fixture (tests/golden/make_golden.py, ``golden_boxes_timstof``): every 11th row
    of the base sweep (coprime to the periods 2, 3, 4 and 8 of the axes) and a row of every plane edge for one and for
    two observations.  No density rows, and no box with ``frame_stop`` clipped to the last frame: the reference indexes
    past its dense array there (bruker_jit.py:436-451).  The fixture is scored as one batch on the cycle "mixed"."""
    df = spec_rows("base")
    plain = (df["density"].values == "") & (df["pos_f"].values != 3)
    keep = (np.arange(len(df)) % 11 == 5) & plain
    full = plain & (df["nl"].values >= 11)   # every F and every S twice on rows that can be valid (candidate.py:190)
    for col, values in (("F", F_ALL), ("S", S_ALL)):
        for v in values:
            keep[np.flatnonzero(full & (df[col].values == v))[1:6:3]] = True
    for planes in PLANES_AT.values():
        for S, F in planes:
            for O in (1, 2):
                m = np.flatnonzero((df["S"].values == S) & (df["F"].values == F) & (df["O"].values == O) & full)
                keep[m[:1]] = True
    df = df[keep].reset_index(drop=True)
    df["batch"] = "g"
    return df


def make_cycle(run: str = "base") -> np.ndarray:
    """The cycle of a run of ``RUNS``; "mixed" (the fixture's): the base cycle with its first MS2 frame three times, so
    that one, two, three and four observations occur on one run."""
    if run == "mixed":
        base = make_cycle("base")
        return np.ascontiguousarray(np.concatenate([base, base[:, 1:2], base[:, 1:2]], axis=1))
    kw = {k: v for k, v in RUNS[run].items() if k != "n_tof"}
    return syn.make_timstof_cycle(N_MS2, WINDOWS_PER_FRAME, S_MAX, MZ_LO, MZ_HI, **kw)


def _windows_of_scan(cycle: np.ndarray, scan: int):
    """(frame of the cycle, lower, upper) of the distinct isolation windows at ``scan``, upper descending."""
    seen, out = set(), []
    for fr in range(cycle.shape[1]):
        lo, hi = cycle[0, fr, scan]
        if lo >= 0 and (lo, hi) not in seen:
            seen.add((lo, hi))
            out.append((fr, float(lo), float(hi)))
    return sorted(out, key=lambda w: -w[2])


def mz_table_of(n_tof: int) -> np.ndarray:
    """The m/z of the TOF bins: quadratic in the bin, 195 ... 490 Th."""
    t = np.arange(n_tof, dtype=np.float64)
    return (np.sqrt(195.0) + t * (np.sqrt(490.0) - np.sqrt(195.0)) / (n_tof - 1)) ** 2


# ClassicExtractionHandler's settings, but for the precursor tolerance: 20 ppm is wider than a TOF bin of this run at
# 400 ... 480 Th, so every isotope window holds a bin (at 10 ppm four in ten are empty, whatever the precursor)
HANDLER = dict(score_grouped=False, top_k_isotopes=3, reference_channel=-1, precursor_mz_tolerance=20,
               fragment_mz_tolerance=15, exclude_shared_ions=True, quant_window=3, quant_all=True, experimental_xic=True,
               top_k_fragments=12)

def _tof_range(mz_table, mzq: np.float32, tol: float):
    t = np.float32(tol) * mzq
    q = t / np.float32(1000000.0)
    a = int(np.searchsorted(mz_table, np.float64(mzq - q), side="left"))
    b = int(np.searchsorted(mz_table, np.float64(mzq + q), side="left"))
    return a, max(a, b)



def _isotope_mz(mono: np.float32, charge, k: int) -> np.float32:
    """The float32 m/z of isotope ``k`` as the kernels and the reference assemble it (candidate.py:151-163)."""
    return np.float32(np.float64(k) * syn.ISOTOPE_DELTA / np.float64(charge)) + np.float32(mono)


def _place_boxes(spec: pd.DataFrame, L: int, n_frames: int, written: np.ndarray) -> dict:
    """The boxes, centres and apexes of ``spec`` on a run of ``n_frames`` frames with cycles of ``L`` frames.  ``written``:
    the rows whose events are written cell by cell; their boxes lie inside the scans 0 ... 30 of one group of windows."""
    n = len(spec)
    idx = np.arange(n)
    complete = (n_frames - 1) // L
    S, F = spec["S"].values.astype(np.int64), spec["F"].values.astype(np.int64)
    pos_f, pos_s = spec["pos_f"].values, spec["pos_s"].values
    c_int = 1 + (idx * 13) % np.maximum(complete - F - 1, 1)
    c0 = np.where(pos_f == 0, 0, np.where(pos_f >= 2, complete - F, c_int)).astype(np.int64)
    s_int = 1 + (idx * 7) % np.maximum(S_MAX - S - 1, 1)
    s0 = np.where(pos_s == 0, 0, np.where(pos_s == 2, S_MAX - S, s_int)).astype(np.int64)
    s0 = np.where(written & (pos_s == 1), 1 + idx % np.maximum(30 - S, 1), s0)
    ce_f, ce_s = spec["ce_f"].values, spec["ce_s"].values
    return dict(
        S=S, F=F, c0=c0, s0=s0, frame_start=c0 * L + 1, frame_stop=np.where(pos_f == 3, n_frames, (c0 + F) * L + 1),
        frame_center=(c0 + np.where(ce_f == 0, 0, np.where(ce_f == 1, F // 2, F - 1))) * L + 1,
        scan_center=s0 + np.where(ce_s == 0, 0, np.where(ce_s == 1, S // 2, S - 1)),
        apex_c=c0 + F // 2, apex_s=np.clip(s0 + S // 2, 0, S_MAX - 3))


def _precursor_mz(spec: pd.DataFrame, cycle: np.ndarray, apex_s: np.ndarray, charge: np.ndarray, written: np.ndarray,
                  mz_table: np.ndarray) -> np.ndarray:
    """Precursor m/z: mid-window (one observation) or below a window boundary (two).  A written row sits on a TOF bin,
    the first in steps of 0.01 Th whose isotope windows meet those of no earlier written row."""
    n = len(spec)
    mz = np.zeros(n, dtype=np.float64)
    owned = np.zeros(len(mz_table) + 2, dtype=bool)   # TOF bins of the isotope windows of the written rows placed so far
    o_rank = {1: 0, 2: 0}                             # written rows take the windows in turn
    for i in range(n):
        wins = _windows_of_scan(cycle, int(apex_s[i]))
        O = int(spec["O"].values[i])
        w = i
        if written[i]:
            w = o_rank[O]
            o_rank[O] += 1
        if O == 1:
            _, lo, _ = wins[w % len(wins)]
            mz[i] = lo + 3.0 + 0.01 * (i % 50)
            room = 1.5
        else:
            _, lo, _ = wins[w % (len(wins) - 1)]   # the boundary below this window: the next one ends there
            # (0.48 ... 0.06 Th below: two observations with one isotope as well; planted rows 0.012 Th apart in turn)
            mz[i] = lo - (0.48 if written[i] else 0.4 - 0.012 * (i % 25))
            room = 0.42
        if written[i]:
            for n_steps in range(int(room / 0.01) + 1):
                b = int(np.searchsorted(mz_table, mz[i] + n_steps * 0.01))
                bins = [_tof_range(mz_table, _isotope_mz(mz_table[b], charge[i], k), HANDLER["precursor_mz_tolerance"]) for k in range(3)]
                if not any(owned[a:e].any() for a, e in bins):
                    break
            else:
                raise AssertionError(f"no free isotope windows for density row {i}")
            for a, e in bins:
                owned[a:e] = True
            mz[i] = mz_table[b]
    return mz


class _Events:
    """(push, TOF bin, intensity) events of a run under construction."""

    def __init__(self, mz_table, n_frames):
        self.mz_table, self.n_frames, self.parts = mz_table, n_frames, []

    def emit(self, frame, scan, amp, mz_true=None, tof=None):
        keep = (amp >= 1) & (frame < self.n_frames)
        if keep.any():
            tof = np.searchsorted(self.mz_table, mz_true[keep]) if tof is None else np.full(int(keep.sum()), tof)
            self.parts.append(((frame[keep] * S_MAX + scan[keep]).astype(np.int64),
                               np.clip(tof, 0, len(self.mz_table) - 1).astype(np.int64), np.clip(amp[keep], 1, 60000).astype(np.int64)))

    def drop_bins(self, reserved):
        self.parts = [tuple(a[~reserved[p[1]]] for a in p) for p in self.parts]


def _planted_events(ev: _Events, rows, box, cycle, lib, nl, narrow_rows):
    """Planted peptides: a Gaussian in cycle and scan around the middle of the box (7 x 5 cells for ``narrow_rows``, so
    that neither a window's events nor the entries come near their capacities), in every MS1 frame for three isotopes
    and in the MS2 frames whose window isolates the precursor for every fragment of the slice."""
    pdf, fdf = lib.precursor_df, lib.fragment_df
    L = cycle.shape[1]
    p_mz, charge = pdf["mz_library"].values.astype(np.float64), pdf["charge"].values.astype(np.float64)
    f_mz, f_int = fdf["mz_library"].values, fdf["intensity"].values.astype(np.float64)
    start = pdf["flat_frag_start_idx"].values.astype(np.int64)
    apex_c, apex_s = box["apex_c"], box["apex_s"]
    dc, ds = np.arange(-6, 7), np.arange(-5, 6)
    g_cell = (np.exp(-0.5 * (dc / 2.0) ** 2)[:, None] * np.exp(-0.5 * (ds / 1.8) ** 2)[None, :]).reshape(-1)
    cell_p = np.repeat(rows, g_cell.size)
    cell_c = apex_c[cell_p] + np.tile(np.repeat(dc, ds.size), rows.size)
    cell_s = apex_s[cell_p] + np.tile(np.tile(ds, dc.size), rows.size)
    cell_g = np.tile(g_cell, rows.size)
    inside = (cell_c >= 0) & (cell_c < N_CYCLES) & (cell_s >= 0) & (cell_s < S_MAX)
    narrow = (np.abs(cell_c - apex_c[cell_p]) <= 3) & (np.abs(cell_s - apex_s[cell_p]) <= 2)
    inside &= narrow | ~narrow_rows[cell_p]
    cell_p, cell_c, cell_s, cell_g = cell_p[inside], cell_c[inside], cell_s[inside], cell_g[inside]
    ms1_frames = np.flatnonzero((cycle[0, :, :, 0] == -1.0).all(axis=1))
    for k in range(3):
        for fr in ms1_frames:
            ev.emit(cell_c * L + 1 + int(fr), cell_s, 3000.0 * pdf[f"i_{k}"].values.astype(np.float64)[cell_p] * cell_g,
                    mz_true=p_mz[cell_p] + k * syn.ISOTOPE_DELTA / charge[cell_p])
    for fr in range(L):
        sel = (cycle[0, fr, cell_s, 0] <= p_mz[cell_p]) & (p_mz[cell_p] < cycle[0, fr, cell_s, 1])
        if not sel.any():
            continue
        sp, sg, sc, ss = cell_p[sel], cell_g[sel], cell_c[sel], cell_s[sel]
        for k in range(int(nl.max())):
            has = k < nl[sp]
            at = (start[sp] + k)[has]
            ev.emit(sc[has] * L + 1 + fr, ss[has], 1500.0 * f_int[at] * sg[has], mz_true=f_mz[at].astype(np.float64))


def _density_windows(i, lib, mz_table):
    """TOF bin ranges of the twelve fragment windows and the three isotope windows of written row ``i``."""
    pdf, fdf = lib.precursor_df, lib.fragment_df
    a = int(pdf["flat_frag_start_idx"].values[i])
    f32 = fdf["mz_library"].values.astype(np.float32)
    frag = [_tof_range(mz_table, f32[a + k], HANDLER["fragment_mz_tolerance"]) for k in range(12)]
    iso = [_tof_range(mz_table, _isotope_mz(np.float32(pdf["mz_library"].values[i]), pdf["charge"].values[i], k),
                      HANDLER["precursor_mz_tolerance"]) for k in range(3)]
    return frag, iso


def _density_events(ev: _Events, rows, design, spec, box, cycle, lib):
    """The written rows: events cell by cell, one in each TOF bin of the designated windows."""
    pdf, fdf = lib.precursor_df, lib.fragment_df
    L = cycle.shape[1]
    p_mz, charge = pdf["mz_library"].values.astype(np.float64), pdf["charge"].values.astype(np.float64)
    f_int = fdf["intensity"].values.astype(np.float64)
    start = pdf["flat_frag_start_idx"].values.astype(np.int64)
    apex_c, apex_s = box["apex_c"], box["apex_s"]
    ms1_frames = np.flatnonzero((cycle[0, :, :, 0] == -1.0).all(axis=1))

    def cells_of(i, every):
        cc, sc = np.meshgrid(np.arange(box["c0"][i], box["c0"][i] + box["F"][i]), np.arange(box["s0"][i], box["s0"][i] + box["S"][i]),
                             indexing="ij")
        cc, sc = cc.reshape(-1), sc.reshape(-1)
        keep = ((cc + sc) % 12 < every)
        g = np.exp(-0.5 * ((cc - apex_c[i]) / 4.0) ** 2 - 0.5 * ((sc - apex_s[i]) / 5.0) ** 2)
        return cc[keep], sc[keep], g[keep]

    for i in rows:
        d = design[i]
        O = int(spec["O"].values[i])
        frag_bins, iso_bins = _density_windows(i, lib, ev.mz_table)
        iso_amp = [3000.0 * float(pdf[f"i_{k}"].values[i]) for k in range(3)]
        q_lo = p_mz[i] - 0.5
        q_hi = p_mz[i] + 2 * syn.ISOTOPE_DELTA / charge[i] + 0.5
        # "many batches": about 200 events per window, on a fraction of the cells
        cc, sc, g = cells_of(i, (5 if O == 1 else 3) if d == "many_batches" else 12)
        frag_windows = {"full_tile": range(12), "many_batches": range(12), "window_over_one": (5,), "window_over_two": (5,),
                        "isotopes_over": ()}[d]
        iso_windows = {"full_tile": range(3), "many_batches": (0,), "isotopes_over": range(3)}.get(d, ())
        for fr in range(L):
            seen = (cycle[0, fr, sc, 0] <= q_hi) & (cycle[0, fr, sc, 1] >= q_lo)
            for k in frag_windows:
                for tof in range(*frag_bins[k]):
                    ev.emit((cc * L + 1 + fr)[seen], sc[seen], 20.0 + 1500.0 * f_int[start[i] + k] * g[seen], tof=tof)
        if d in ("window_over_one", "window_over_two", "isotopes_over"):
            # the other windows: the peptide's peak, a Gaussian around the middle of the box as for the planted rows
            ca, sa, _ = cells_of(i, 12)
            near = (np.abs(ca - apex_c[i]) <= 4) & (np.abs(sa - apex_s[i]) <= 3)   # (63 cells a window)
            ca, sa = ca[near], sa[near]
            ga = np.exp(-0.5 * ((ca - apex_c[i]) / 2.0) ** 2 - 0.5 * ((sa - apex_s[i]) / 1.8) ** 2)
            for fr in range(L):
                seen = (cycle[0, fr, sa, 0] <= p_mz[i]) & (p_mz[i] < cycle[0, fr, sa, 1])
                for k in set(range(12)) - set(frag_windows):
                    ev.emit((ca * L + 1 + fr)[seen], sa[seen], 1500.0 * f_int[start[i] + k] * ga[seen], tof=frag_bins[k][0])
            for fr in ms1_frames:
                for k in set(range(3)) - set(iso_windows):
                    ev.emit(ca * L + 1 + int(fr), sa, iso_amp[k] * ga, tof=iso_bins[k][0])
        for fr in ms1_frames:
            for k in iso_windows:
                bins = range(*iso_bins[k])
                for tof in (bins[:1] if d == "many_batches" else bins):
                    ev.emit(cc * L + 1 + int(fr), sc, 20.0 + iso_amp[k] * g, tof=tof)


def _assemble_run(ev: _Events, cycle, rt, mobility) -> syn.TimsTOFArrays:
    """The TOF-major arrays of the run; one event per (TOF bin, push): events of the same cell are added up."""
    L, n_tof = cycle.shape[1], len(ev.mz_table)
    n_push = len(rt) * S_MAX
    ev_push = np.concatenate([p[0] for p in ev.parts])
    ev_tof = np.concatenate([p[1] for p in ev.parts])
    ev_int = np.concatenate([p[2] for p in ev.parts])
    uniq, inv = np.unique(ev_tof * n_push + ev_push, return_inverse=True)
    ev_int = np.minimum(np.bincount(inv, weights=ev_int.astype(np.float64)), 60000).astype(np.int64)
    ev_tof, ev_push = uniq // n_push, uniq % n_push
    tof_indptr = np.concatenate([[0], np.cumsum(np.bincount(ev_tof, minlength=n_tof))]).astype(np.int64)
    return syn.TimsTOFArrays(
        cycle=cycle, dia_precursor_cycle=np.repeat(np.arange(L, dtype=np.int64), S_MAX), rt_values=rt,
        mobility_values=mobility, mz_values=ev.mz_table, tof_indptr=tof_indptr, push_indices=ev_push.astype(np.uint32),
        intensity_values=ev_int.astype(np.uint16), scan_max_index=S_MAX,
    )


def sweep_case(run: str = "base", golden: bool = False) -> syn.TimsTOFCase:
    """The run, the library (one precursor per candidate) and the candidate table of ``spec_rows(run)``, or of
    ``golden_spec()`` on the cycle "mixed"."""
    spec = golden_spec() if golden else spec_rows(run)
    n = len(spec)
    cycle = make_cycle("mixed" if golden else run)
    L = cycle.shape[1]
    n_frames = N_CYCLES * L + 1 - TRUNCATE
    assert (n_frames - 1) % L != 0
    seed = SEED + (GOLDEN_SEED if golden else list(RUNS).index(run))
    rt = np.arange(n_frames, dtype=np.float64) * 0.1
    mobility = np.linspace(1.6, 0.6, S_MAX).astype(np.float64)
    n_tof = N_TOF if golden else RUNS[run].get("n_tof", N_TOF)
    mz_table = mz_table_of(n_tof)
    design = spec["density"].values
    written = (design != "") & ~np.isin(design, PAIR_DENSITIES)   # (events written cell by cell; the others are planted)
    box = _place_boxes(spec, L, n_frames, written)

    # ---- the library: one precursor per candidate
    lib = syn.make_library(n, seed, k_fragments=40, mz_lo=MZ_LO, mz_hi=MZ_HI, rt_max=float(rt[-1]), frag_mz_lo=200.0, frag_mz_hi=350.0)
    pdf, fdf = lib.precursor_df, lib.fragment_df
    pdf["mz_library"] = _precursor_mz(spec, cycle, box["apex_s"], pdf["charge"].values, written, mz_table).astype(np.float32)
    pdf["mobility_library"] = mobility[box["apex_s"]].astype(np.float32)
    pdf["elution_group_idx"] = pdf["precursor_idx"].values.astype(np.uint32)  # one candidate, one score group
    start = pdf["flat_frag_start_idx"].values.astype(np.int64)
    pdf["flat_frag_stop_idx"] = (start + spec["nl"].values).astype(np.uint32)
    f_mz = fdf["mz_library"].values.copy()
    for j, i in enumerate(np.flatnonzero(written)):  # every fragment window of a written row holds exactly one TOF bin, its own
        bins = np.searchsorted(mz_table, 204.0 + 11.0 * np.arange(12) + 0.25 * j)
        f_mz[start[i]:start[i] + 12] = mz_table[bins].astype(np.float32)
    for j, i in enumerate(np.flatnonzero(design == "pairs_fit")):   # four fragments at the low end: the narrowest windows
        f_mz[start[i]:start[i] + 4] = (202.0 + 7.0 * np.arange(4) + 0.05 * j).astype(np.float32)
    fdf["mz_library"] = f_mz

    # ---- the events: planted peptides, then the written rows on TOF bins nothing else writes to, then noise
    ev = _Events(mz_table, n_frames)
    _planted_events(ev, np.flatnonzero(~written), box, cycle, lib, spec["nl"].values, np.isin(design, PAIR_DENSITIES))
    reserved = np.zeros(n_tof + 1, dtype=bool)
    for i in np.flatnonzero(written):
        for a, e in sum(_density_windows(i, lib, mz_table), []):
            reserved[a:e] = True
    ev.drop_bins(reserved)
    _density_events(ev, np.flatnonzero(written), design, spec, box, cycle, lib)
    rng = np.random.default_rng([seed, 7])   # (the only random events)
    n_push = n_frames * S_MAX
    n_noise = int(NOISE_PER_PUSH * (n_push - S_MAX))
    noise = (rng.integers(S_MAX, n_push, n_noise).astype(np.int64), rng.integers(0, n_tof, n_noise).astype(np.int64),
             np.clip(rng.lognormal(3.0, 1.0, n_noise), 1, 60000).astype(np.int64))
    ev.parts.append(tuple(a[~reserved[noise[1]]] for a in noise))
    dia = _assemble_run(ev, cycle, rt, mobility)

    score = np.random.default_rng([seed, 4]).uniform(0, 100, n).astype(np.float32)
    cands = pd.DataFrame(
        {
            "elution_group_idx": pdf["elution_group_idx"].values,
            "precursor_idx": pdf["precursor_idx"].values.astype(np.uint32),
            "rank": np.zeros(n, dtype=np.uint8),
            "scan_start": box["s0"].astype(np.int64),
            "scan_stop": (box["s0"] + box["S"]).astype(np.int64),
            "scan_center": box["scan_center"].astype(np.int64),
            "frame_start": box["frame_start"].astype(np.int64),
            "frame_stop": box["frame_stop"].astype(np.int64),
            "frame_center": box["frame_center"].astype(np.int64),
            "score": score,
        }
    )
    return syn.TimsTOFCase(dia, lib, cands)


# ---- the rules, restated ---------------------------------------------------------------------------------------

def plan_class_im(n_obs: int, k_cap: int, S: int, F: int, skipped: bool = False) -> int:
    """adh_plan_rec_im_kernel (adh_plan.hip:317-331)."""
    if skipped:
        return CLASS_GENERIC
    small = k_cap <= SMALL_K and S <= SMALL_S and F <= SMALL_F and S * F <= SMALL_SF
    if n_obs <= 1:
        return CLASS_SMALL if small else CLASS_ONE
    return CLASS_TWO if n_obs == 2 else CLASS_GENERIC


def _holds_axes(c, K, O, S, F, I):
    return c["k"] <= K and c["o"] <= O and c["s"] <= S and c["f"] <= F and c["i"] <= I


def _class_caps(caps: dict, cls: int) -> dict:
    cc = dict(caps)
    if cls in (CLASS_ONE, CLASS_SMALL):
        cc["o"] = 1
    if cls == CLASS_TWO:
        cc["o"] = min(cc["o"], 2)
    if cls == CLASS_SMALL:
        cc["k"], cc["s"], cc["f"] = min(cc["k"], SMALL_K), min(cc["s"], SMALL_S), min(cc["f"], SMALL_F)
    return cc


def instantiation_of(caps: dict, n_class: dict, cfg, env: dict | None = None) -> dict:
    """im_launch_routes (adh_score_host.hip), the rule launch_scoring_im follows, restated to be read: per plan class
    of a launch the layout of the feature kernel ('small', 'common', 'common2', 'dynamic') and the launch ('fused4':
    tile and profile phase in one kernel, four candidates per wavefront; 'tile4': the tile phase so, then the profile
    kernel; 'split1': one candidate per wavefront, then the profile kernel; 'one': the one-kernel path).  ``caps``: the
    launch maxima k, o, s, f and the isotope count i; ``n_class``: candidates per plan class; ``env``: the
    ADH_DEBUG_IM* switches that are set.  The library exports the rule itself as ``adh_im_launch_routes``
    (``runtime.im_launch_routes``); tests/test_kernel_classes_im.py holds this copy equal to it on both sides of
    every limit and under every switch."""
    env = env or {}
    stop = int(env.get("ADH_DEBUG_IM", 0))
    fixed = "ADH_DEBUG_IM_DYNAMIC_LAYOUT" not in env
    split_cfg = (fixed and bool(cfg.experimental_xic) and stop in (0, 8) and "ADH_DEBUG_IM_NO_SPLIT" not in env
                 and min(int(cfg.top_k_isotopes), N_ISOTOPE_COLUMNS) <= 3)
    tile4 = "ADH_DEBUG_IM_TILE1" not in env
    fuse4 = tile4 and "ADH_DEBUG_IM_NO_FUSE4" not in env and int(env.get("ADH_DEBUG_IM4", 0)) == 0  # (an ablation stop of tile4)
    tile4_two = tile4 and "ADH_DEBUG_IM_TILE1_TWO" not in env
    out = {}
    for cls, cnt in n_class.items():
        if cnt <= 0:
            continue
        cc = _class_caps(caps, cls)
        small_axes = _holds_axes(cc, SMALL_K, 1, SMALL_S, SMALL_F, 3)
        common = _holds_axes(cc, COMMON_K, 1, COMMON_S, COMMON_F, COMMON_I) and cc["s"] * cc["f"] <= COMMON_SF
        common2 = _holds_axes(cc, COMMON_K, 2, COMMON_S, COMMON_F, COMMON_I) and cc["s"] * cc["f"] <= COMMON_SF
        one4 = "fused4" if fuse4 else ("tile4" if tile4 else "split1")
        if cls == CLASS_SMALL and split_cfg and small_axes:
            out[cls] = ("small", one4)
        elif cls == CLASS_TWO and split_cfg and common2 and cc["f"] >= 3 and "ADH_DEBUG_IM_NO_SPLIT2" not in env:
            out[cls] = ("common2", "tile4" if tile4_two else "split1")
        elif cls == CLASS_ONE and split_cfg and common and cc["f"] >= 3:
            out[cls] = ("common", one4)
        elif cls == CLASS_SMALL and small_axes and fixed:
            out[cls] = ("small", "one")
        elif common and fixed:
            out[cls] = ("common", "one")
        else:
            out[cls] = ("dynamic", "one")
    return out


def quad_range(precursor_mz, charge, n_isotopes: int):
    """plan::quad_range: the float32 isotope m/z range -/+ 0.5 Th, rounded as the kernels round it."""
    mzs = [np.float32(np.float64(k) * syn.ISOTOPE_DELTA / np.float64(charge)) + np.float32(precursor_mz) for k in range(n_isotopes)]
    return np.float32(np.float64(min(mzs)) - 0.5), np.float32(np.float64(max(mzs)) + 0.5)


def observations(cycle: np.ndarray, scan_start: int, scan_stop: int, precursor_mz, charge, n_isotopes: int):
    """Frames of the cycle with a push in the scan range whose isolation window overlaps the quadrupole range, and the
    frames whose window is (-1, -1): the observation counts of adh_plan_rec_im_kernel (one cycle row per frame)."""
    q_lo, q_hi = (np.float64(x) for x in quad_range(precursor_mz, charge, n_isotopes))
    lo, hi = cycle[0, :, scan_start:scan_stop, 0], cycle[0, :, scan_start:scan_stop, 1]
    return int(((q_lo <= hi) & (q_hi >= lo)).any(axis=1).sum()), int(((-1.0 <= hi) & (-1.0 >= lo)).any(axis=1).sum())


def shape_table(case, soa: dict, cfg) -> pd.DataFrame:
    """S, F, the observation counts, nl and k_cap of every candidate of an assembled table under ``cfg``."""
    L = case.dia.cycle_len
    I = min(int(cfg.top_k_isotopes), N_ISOTOPE_COLUMNS)
    F = (soa["frame_stop"].astype(np.int64) - 1) // L - (soa["frame_start"].astype(np.int64) - 1) // L
    S = soa["scan_stop"].astype(np.int64) - soa["scan_start"].astype(np.int64)
    nl = soa["frag_stop_idx"].astype(np.int64) - soa["frag_start_idx"].astype(np.int64)
    obs = [observations(case.dia.cycle, int(a), int(b), m, z, I)
           for a, b, m, z in zip(soa["scan_start"], soa["scan_stop"], soa["precursor_mz"], soa["charge"])]
    return pd.DataFrame({"S": S, "F": F, "O": [o[0] for o in obs], "Op": [o[1] for o in obs], "nl": nl,
                         "k_cap": np.minimum(int(cfg.top_k_fragments), nl)})


def classes_of(table: pd.DataFrame) -> np.ndarray:
    return np.array([plan_class_im(int(o), int(k), int(s), int(f)) for o, k, s, f in
                     zip(table["O"], table["k_cap"], table["S"], table["F"])], dtype=np.int64)


def histogram(classes: np.ndarray) -> np.ndarray:
    return np.bincount(classes, minlength=N_CLASSES).astype(np.int64)


def batch_caps(table: pd.DataFrame, rows: np.ndarray, cfg) -> dict:
    """The launch maxima of the rows of one batch (PlanMeta all_k ... all_op, adh_plan.hip)."""
    t = table.iloc[rows]
    return dict(k=int(t["k_cap"].max()), o=int(t["O"].max()), s=int(t["S"].max()), f=int(t["F"].max()),
                i=max(min(int(cfg.top_k_isotopes), N_ISOTOPE_COLUMNS), 1), n_lib=int(t["nl"].max()), op=int(t["Op"].max()))


def routes_of(table: pd.DataFrame, batch: np.ndarray, cfg, env: dict | None = None):
    """(plan class, layout, launch) of every candidate when the table is scored batch by batch."""
    classes = classes_of(table)
    out = np.empty(len(table), dtype=object)
    for b in pd.unique(batch):
        rows = np.flatnonzero(batch == b)
        n_class = {int(c): int((classes[rows] == c).sum()) for c in np.unique(classes[rows])}
        inst = instantiation_of(batch_caps(table, rows, cfg), n_class, cfg, env)
        for r in rows:
            out[r] = (int(classes[r]),) + inst[int(classes[r])]
    return out


# ---- LDS of a launch (adh_features_im.hip LayoutT::bytes, adh_gather_im.hip) -----------------------------------

def _layout_bytes(K, O, S, F, I, SF):
    qtf = max(I * O * S, 4 * K + F)
    n_double = qtf + 4 * K * O + 2 * K * O + 2 * O + 2 * I
    smax = max(S, F)
    r1 = max(O * SF, K * O * (F + S))
    n_float = (K * O * smax + r1 + K * O * (F + S) + 2 * O * F + 2 * O * S + O * S + 8 * K + 4 * K * O + 4 * O + 3 * I + 2 * F
               + NUM_FEATURES)
    n_int = 4 * K + K * O + O
    return n_double * 8 + (n_float * 4 + 7) // 8 * 8 + (n_int * 4 + 7) // 8 * 8 + (5 * K + 7) // 8 * 8


def feature_lds_bytes(c: dict) -> int:
    """adh_feature_im_lds_bytes: the layout the launch maxima fit."""
    if _holds_axes(c, SMALL_K, 1, SMALL_S, SMALL_F, 3) and c["s"] * c["f"] <= SMALL_SF:
        return _layout_bytes(SMALL_K, 1, SMALL_S, SMALL_F, 3, SMALL_SF)
    if _holds_axes(c, COMMON_K, 1, COMMON_S, COMMON_F, COMMON_I) and c["s"] * c["f"] <= COMMON_SF:
        return _layout_bytes(COMMON_K, 1, COMMON_S, COMMON_F, COMMON_I, COMMON_SF)
    return _layout_bytes(c["k"], c["o"], c["s"], c["f"], c["i"], c["s"] * c["f"])


def gather_lds_bytes(c: dict) -> int:
    """adh_gather_im_lds_bytes."""
    b = (c["k"] + c["i"]) * 12 + (c["k"] + c["i"] + 1) * 4
    b = (b + 15) // 16 * 16
    b += (c["k"] + c["i"]) * 8
    b = (b + 15) // 16 * 16
    compact = PAIR_CAP * 4 + (PAIR_CAP + 1) * 4 + 4 + SORT_CAP * 7 + PAIR_CAP
    b += max(c["n_lib"] * 16, compact)
    return (b + 15) // 16 * 16


def entry_capacity(k_cap: int, O: int, S: int, F: int, I: int, Op: int) -> int:
    """Entries that fit where the tiles of a candidate would be: (adh_im_tiles_end - adh_scratch_frag_off) / 12."""
    frag_off = 32 + k_cap * 32
    end = (frag_off + k_cap * O * S * F * 8 + I * Op * S * F * 8 + 31) // 32 * 32
    return (end - frag_off) // 12


# ---- exact event counts of a candidate, from the run arrays ------------------------------------------------------

def window_events(case, soa: dict, cfg, row: int) -> dict:
    """What the gather kernel meets for candidate ``row`` (every fragment of its slice kept: nl <= top_k_fragments):
    events per fragment window and of the isotope windows together (inside the box, on a push whose isolation window
    passes the quadrupole test), non-zero cells of all planes, TOF bins of all windows."""
    dia = case.dia
    L, S_max = dia.cycle_len, dia.scan_max_index
    I = min(int(cfg.top_k_isotopes), N_ISOTOPE_COLUMNS)
    a, b = int(soa["frag_start_idx"][row]), int(soa["frag_stop_idx"][row])
    assert b - a <= int(cfg.top_k_fragments)
    f_mz = case.library.fragment_df["mz_library"].values.astype(np.float32)[a:b]
    pmz, z = np.float32(soa["precursor_mz"][row]), soa["charge"][row]
    q_lo, q_hi = (np.float64(x) for x in quad_range(pmz, z, I))
    iso = [np.float32(np.float64(k) * syn.ISOTOPE_DELTA / np.float64(z)) + pmz for k in range(I)]
    fs, fe = int(soa["frame_start"][row]), int(soa["frame_stop"][row])
    c_lo, c_hi = (fs - 1) // L, (fe - 1) // L
    ss, se = int(soa["scan_start"][row]), int(soa["scan_stop"][row])

    def count(mzq, tol, lo, hi):
        t0, t1 = _tof_range(dia.mz_values, mzq, tol)
        push = dia.push_indices[dia.tof_indptr[t0]:dia.tof_indptr[t1]].astype(np.int64)
        frame, scan = push // S_max, push % S_max
        cyc = (frame - 1) // L
        ok = (frame >= 1) & (cyc >= c_lo) & (cyc < c_hi) & (scan >= ss) & (scan < se)
        frame, scan, cyc = frame[ok], scan[ok], cyc[ok]
        w = dia.cycle[0, (frame - 1) % L, scan]
        ok = (lo <= w[:, 1]) & (hi >= w[:, 0])
        cells = np.unique((frame[ok] * S_max + scan[ok]))
        return int(ok.sum()), int(cells.size), t1 - t0

    frag = [count(m, float(cfg.fragment_mz_tolerance), q_lo, q_hi) for m in f_mz]
    prec = [count(m, float(cfg.precursor_mz_tolerance), -1.0, -1.0) for m in iso]
    return dict(fragment_windows=[f[0] for f in frag], isotope_group=sum(p[0] for p in prec),
                entries=sum(f[1] for f in frag) + sum(p[1] for p in prec), bins=sum(f[2] for f in frag) + sum(p[2] for p in prec),
                widest_window=max([f[2] for f in frag] + [p[2] for p in prec]))


# ---- the scoring configurations the sweep is run under ----------------------------------------------------------

# (HANDLER: above, next to the run it is made for)
CONFIGS = {
    "defaults": dict(),                           # HANDLER as it stands (the sweep's defaults, not the product's: 20 ppm)
    "no_xic": dict(experimental_xic=False),       # no split path: the one-kernel path of every layout
    "isotopes1": dict(top_k_isotopes=1),
    "isotopes4": dict(top_k_isotopes=4),          # no fixed layout holds four isotopes
    "top16": dict(top_k_fragments=16),            # 13 ... 16 kept fragments: neither small nor common
    "best_of_two": dict(quant_all=False),
    # the widest fragment tolerance the configuration takes.  On the run "fine" a window holds 33 ... 44 TOF bins: twelve
    # are 1.5 x ADH_IM_PAIR_CAP (window, bin) pairs and more, none has 256 bins (on 24 000 bins: 8 ... 11 a window)
    "wide_tolerance": dict(fragment_mz_tolerance=200.0),
}
_SPLIT = {(CLASS_SMALL, "small", "fused4"), (CLASS_ONE, "common", "fused4"), (CLASS_TWO, "common2", "tile4")}
_PAST = {(CLASS_ONE, "dynamic", "one"), (CLASS_TWO, "dynamic", "one")}   # batches (c), and two observations without a split
_DEFAULT = _SPLIT | _PAST | {(CLASS_ONE, "common", "one")}             # (the launch of two-cycle boxes: not split)
# the (class, layout, launch) triples of the base run a configuration must reach, and no other
REACHES = {
    "defaults": _DEFAULT, "best_of_two": _DEFAULT, "isotopes1": _DEFAULT, "wide_tolerance": _DEFAULT,
    "no_xic": _PAST | {(CLASS_SMALL, "small", "one"), (CLASS_ONE, "common", "one")},
    "isotopes4": _PAST | {(CLASS_SMALL, "dynamic", "one")},
    "top16": _PAST | {(CLASS_SMALL, "small", "fused4")},
}


def config_of(name: str):
    from alphadia_amd.scoring import CandidateScoringConfig

    cfg = CandidateScoringConfig()
    cfg.update(dict(HANDLER, **CONFIGS[name]))
    return cfg
