"""A deterministic sweep of candidate SHAPES, and the kernel-class rule restated in Python.

Candidate scoring on an AlphaRaw run is routed by the device plan (alphadia_amd/csrc/adh_plan.hip) into 37 kernel
classes by three numbers per candidate: the cycle count of its box, its observation count and the fragments it keeps.
``make_candidates`` draws boxes of 6 ... 29 cycles around their centre and libraries stop at 61 fragments; this module
crosses, on a small run that ends inside a cycle,

* the cycle count F = 2 ... 36 (both sides of every class edge; F = 1 is implementation-defined: the reference reads
  past a row of length 1 in ``_odd_center_envelope``, fragment_features.py:88),
* ``frame_center`` on the first, the middle and the last cycle of the box,
* boxes that touch cycle 0, that touch the last cycle (every other one with ``frame_stop`` clipped to the last
  spectrum, as the selection step leaves it) and interior ones,
* one and two observations (precursor mid-window / isotope range across a window boundary),
* and, in the ragged variant, library slices of 1 ... 200 fragments cut out of a 200-fragment library.

Every precursor is planted with its apex in the middle of its box.  ``golden=True`` gives a thinned sweep on a sparser
run, small enough for a fixture (tests/golden/make_golden.py, ``golden_boxes``).
"""

from __future__ import annotations

import numpy as np
import pandas as pd

import synthetic as syn

N_CLASSES = 37
CLASS_FUSED1, CLASS_FUSED2, CLASS_FAST2, CLASS_FAST1 = 0, 7, 14, 17
CLASS_WIDE2, CLASS_WIDE1, CLASS_MID2, CLASS_MID1, CLASS_GENERIC = 24, 27, 30, 33, 36

F_ALL = tuple(range(2, 37))
# class edges of the register shape: below / at 3, the FM steps of the one-observation classes, past 32
F_EDGES = ((2, 3), (8, 9), (12, 13), (16, 17), (20, 21), (24, 25), (28, 29), (32, 33))
F_EDGE_VALUES = tuple(sorted({f for e in F_EDGES for f in e} | {4, 5}))
NL_ALL = (1, 2, 3, 11, 12, 13, 16, 17, 32, 33, 61, 62, 63, 64, 65, 66, 80, 200)
# The generic kernel sizes its LDS tile by the MAXIMA of its class over a batch (kept fragments x observations x
# cycles, 160 KiB at most: 200 x 2 x 36 would need 230 KB and the plan refuses such a batch).  Slices of 200 fragments
# therefore go with boxes of at most 16 cycles and are scored as a batch of their own (column ``batch`` = 1); the
# longer boxes take 120 fragments in that place (120 x 2 x 36: 142 KB).
NL_LONG, NL_LONG_FMAX, NL_LONG_OTHERWISE = 200, 16, 120
NL_REGISTER = (12, 16, 17, 32, 33, 64, 65)   # the register axes are crossed with these slice lengths
N_CYCLES = 80
TRUNCATE = 4          # spectra cut off the end: the run ends inside its last cycle
N_WINDOWS = 8
SEED = 20261018
# The draws of the two fixtures.  diff_b_y_ion_intensity (feature 27) is the difference of the logarithms of two float32
# sums; NumPy (the fixtures' reference run) sums pairwise, Numba and the kernels in sequence, and where the two
# logarithms nearly cancel one ulp of a sum is more than the 1e-4 relative bound of the fixture tests (about one row
# in 200 of the sweep).  These draws hold no such row; the full sweep keeps its own (HIP against the oracle).
GOLDEN_SEED = {False: 2, True: 4}


def spec_rows(ragged: bool, golden: bool = False) -> pd.DataFrame:
    """One row per candidate: F, centre (0 first / 1 middle / 2 last), position (0 start / 1 interior / 2 end),
    observations, slice length, scoring batch.  Pure arithmetic: no random numbers."""
    rows = []
    i = 0
    for F in F_ALL:
        for ce in range(3):
            for pos in range(3):
                for O in (1, 2):
                    nl = NL_ALL[(i + 7 * (F - 2)) % len(NL_ALL)] if ragged else 12
                    if nl == NL_LONG and (F > NL_LONG_FMAX or golden):  # (a fixture is scored as one batch)
                        nl = NL_LONG_OTHERWISE
                    rows.append((F, ce, pos, O, nl))
                    i += 1
    if ragged:
        j = 0
        for rep in range(3):
            for F in F_EDGE_VALUES:
                for O in (1, 2):
                    for nl in NL_REGISTER:
                        rows.append((F, (j + rep) % 3, (j // 3 + rep) % 3, O, nl))
                        j += 1
    df = pd.DataFrame(rows, columns=["F", "centre", "position", "O", "nl"])
    df["batch"] = (df["nl"] == NL_LONG).astype(np.int64)
    if golden:  # every 7th / 13th row (coprime to the periods 2, 3, 18 of the axes), the rows of F = 30 ... 33 twice as dense
        stride, first = (13, 12) if ragged else (7, 0)
        at = np.arange(len(df)) % stride
        df = df[(at == first) | ((at == (first + 3) % stride) & df["F"].isin((30, 31, 32, 33)).values)].reset_index(drop=True)
    return df


def sweep_case(ragged: bool, golden: bool = False) -> syn.SyntheticCase:
    spec = spec_rows(ragged, golden)
    n = len(spec)
    cycle = syn.make_cycle(n_ms2=N_WINDOWS, mz_lo=400.0, mz_hi=400.0 + 10.0 * N_WINDOWS)
    L = cycle.shape[1]
    seed = SEED + (1 if ragged else 0) + (GOLDEN_SEED[ragged] if golden else 0)
    lib = syn.make_library(n, seed, k_fragments=(200, 200) if ragged else 12, mz_lo=400.0, mz_hi=480.0,
                           rt_max=N_CYCLES * 1.5, frag_mz_lo=200.0, frag_mz_hi=350.0)
    pdf = lib.precursor_df
    idx = np.arange(n)
    F = spec["F"].values.astype(np.int64)
    # one observation: the middle of a window; two: 0.4 Th below a window boundary (isotope range -0.5 ... +0.5 Th)
    mz = np.where(spec["O"].values == 1, 405.0 + 10.0 * (idx % N_WINDOWS), 409.6 + 10.0 * (idx % (N_WINDOWS - 1)))
    pdf["mz_library"] = mz.astype(np.float32)
    pdf["elution_group_idx"] = pdf["precursor_idx"].values.astype(np.uint32)  # one candidate, one score group
    start = pdf["flat_frag_start_idx"].values.astype(np.int64)
    pdf["flat_frag_stop_idx"] = (start + spec["nl"].values).astype(np.uint32)
    complete = (N_CYCLES * L - TRUNCATE) // L   # complete cycles of the truncated run
    n_spectra = N_CYCLES * L - TRUNCATE
    pos = spec["position"].values
    interior = 1 + (idx * 13) % np.maximum(complete - F - 1, 1)
    c0 = np.where(pos == 0, 0, np.where(pos == 2, complete - F, interior)).astype(np.int64)
    centre = c0 + np.where(spec["centre"].values == 0, 0, np.where(spec["centre"].values == 1, F // 2, F - 1))
    frame_stop = (c0 + F) * L
    clipped = (pos == 2) & (idx % 2 == 1)
    frame_stop = np.where(clipped, n_spectra, frame_stop)
    apex = c0 + F // 2
    planted = syn.plant_peptides(lib, cycle, N_CYCLES, seed, sigma_cycles=2.0, half_width=4 if golden else 5, apex=apex)
    dia = syn.make_thermo_run(N_CYCLES, seed, cycle=cycle, ms1_peaks=60 if golden else 400, ms2_peaks=20 if golden else 150,
                              planted=planted, threads=1, ms1_mz_range=(395.0, 500.0), ms2_mz_range=(195.0, 355.0))
    dia.rt_values = dia.rt_values[:-TRUNCATE]
    dia.peak_start_idx_list = dia.peak_start_idx_list[:-TRUNCATE]
    dia.peak_stop_idx_list = dia.peak_stop_idx_list[:-TRUNCATE]
    assert dia.n_spectra == n_spectra and (frame_stop <= n_spectra).all() and (c0 >= 0).all()
    rng = np.random.default_rng([seed, 4])
    cands = pd.DataFrame(
        {
            "elution_group_idx": pdf["elution_group_idx"].values,
            "precursor_idx": pdf["precursor_idx"].values.astype(np.uint32),
            "rank": np.zeros(n, dtype=np.uint8),
            "scan_start": np.zeros(n, dtype=np.int64),
            "scan_stop": np.ones(n, dtype=np.int64),
            "scan_center": np.zeros(n, dtype=np.int64),
            "frame_start": (c0 * L).astype(np.int64),
            "frame_stop": frame_stop.astype(np.int64),
            "frame_center": (centre * L).astype(np.int64),
            "score": rng.uniform(0, 100, n).astype(np.float32),
        }
    )
    return syn.SyntheticCase(dia, lib, cands, apex)


# ---- the class rule of adh_plan_rec_kernel (adh_plan.hip), restated ---------------------------------------------

def quad_range(precursor_mz, charge, n_isotopes: int):
    """plan::quad_range: the float32 isotope m/z range -/+ 0.5 Th, rounded as the kernels round it."""
    mzs = [np.float32(np.float64(k) * syn.ISOTOPE_DELTA / np.float64(charge)) + np.float32(precursor_mz) for k in range(n_isotopes)]
    mn, mx = min(mzs), max(mzs)
    return np.float32(np.float64(mn) - 0.5), np.float32(np.float64(mx) + 0.5)


def observations(cycle: np.ndarray, precursor_mz, charge, n_isotopes: int) -> int:
    """Cycle rows whose isolation window overlaps the quadrupole range (MS1 rows are (-1, -1) and never do)."""
    q_lo, q_hi = quad_range(precursor_mz, charge, n_isotopes)
    lo, hi = cycle[0, :, 0, 0], cycle[0, :, 0, 1]
    return int(((np.float64(q_lo) <= hi) & (np.float64(q_hi) >= lo)).sum())


def plan_class(F: int, O: int, k_cap: int, nl: int, I: int, experimental_xic: bool, quant_all: bool, n_ms1_rows: int = 1,
               no_fast: bool = False, no_fused: bool = False, no_fused2: bool = False, no_wide: bool = False) -> int:
    fast_cfg = bool(experimental_xic) and not no_fast
    wide_cfg = fast_cfg and not no_wide
    fused_obs = (1, 2) if (fast_cfg and not no_fused and n_ms1_rows == 1 and I <= 4) else ()
    if no_fused2:
        fused_obs = tuple(o for o in fused_obs if o == 1)
    shape_any_k = fast_cfg and 1 <= O <= 2 and 3 <= F <= 32 and I <= 4
    shape = shape_any_k and k_cap <= 16
    fast = shape and (O == 1 or quant_all)
    wide = shape_any_k and wide_cfg and 16 < k_cap <= 64 and (O == 1 or quant_all)
    fused = shape and O in fused_obs and k_cap <= 12 and nl <= 64
    third = 0 if F <= 16 else (1 if F <= 24 else 2)
    if fused:
        return (CLASS_FUSED1 if O == 1 else CLASS_FUSED2) + max(F - 5, 0) // 4
    if wide:
        if k_cap <= 32:
            return (CLASS_MID1 if O == 1 else CLASS_MID2) + third
        return (CLASS_WIDE1 if O == 1 else CLASS_WIDE2) + third
    if not fast:
        return CLASS_GENERIC
    return CLASS_FAST1 + max(F - 5, 0) // 4 if O == 1 else CLASS_FAST2 + third


def shape_table(case, soa: dict, cfg, n_isotope_columns: int = 4) -> pd.DataFrame:
    """F, O, nl and k_cap of every candidate of an assembled table under ``cfg``."""
    L = case.dia.cycle_len
    I = min(int(cfg.top_k_isotopes), n_isotope_columns)
    F = soa["frame_stop"].astype(np.int64) // L - soa["frame_start"].astype(np.int64) // L
    nl = soa["frag_stop_idx"].astype(np.int64) - soa["frag_start_idx"].astype(np.int64)
    O = np.array([observations(case.dia.cycle, m, z, I) for m, z in zip(soa["precursor_mz"], soa["charge"])], dtype=np.int64)
    return pd.DataFrame({"F": F, "O": O, "nl": nl, "k_cap": np.minimum(int(cfg.top_k_fragments), nl)})


def classes_of(case, soa: dict, cfg, **switches) -> np.ndarray:
    """The class of every candidate (rows flagged to be skipped stay in the generic class)."""
    t = shape_table(case, soa, cfg)
    I = min(int(cfg.top_k_isotopes), 4)
    n_ms1 = int(syn.ms1_rows_of(case.dia.cycle).size)
    cls = np.array([plan_class(int(F), int(O), int(k), int(nl), I, bool(cfg.experimental_xic), bool(cfg.quant_all), n_ms1, **switches)
                    for F, O, nl, k in zip(t["F"], t["O"], t["nl"], t["k_cap"])], dtype=np.int64)
    flags = np.asarray(soa.get("flags", np.zeros(len(cls), np.uint8)))
    return np.where((flags & 1) != 0, CLASS_GENERIC, cls)


def histogram(classes: np.ndarray) -> np.ndarray:
    return np.bincount(classes, minlength=N_CLASSES).astype(np.int64)


# ---- the scoring configurations the sweep is run under ----------------------------------------------------------

# ClassicExtractionHandler's settings (extraction_handler.py:370-376,400-409)
HANDLER = dict(score_grouped=False, top_k_isotopes=3, reference_channel=-1, precursor_mz_tolerance=10,
               fragment_mz_tolerance=15, exclude_shared_ions=True, quant_window=3, quant_all=True, experimental_xic=True,
               top_k_fragments=12)
# name: (ragged library, settings on top of the handler's)
CONFIGS = {
    "defaults": (False, dict()),                                   # the fused classes, one and two observations
    "best_of_two": (False, dict(quant_all=False)),                 # the fused kernel picks the observation itself
    "isotopes4": (False, dict(top_k_isotopes=4)),                  # the 16-column tile of the fused kernel
    "isotopes1": (False, dict(top_k_isotopes=1)),
    "window1": (False, dict(quant_window=1)),
    "window5": (False, dict(quant_window=5)),                      # wider than the boxes of 3 ... 8 cycles
    "top16": (True, dict(top_k_fragments=16)),                     # register classes behind the gather kernel
    "all_fragments": (True, dict(top_k_fragments=9999)),           # 32-lane, 64-lane and generic classes
    "all_fragments_best": (True, dict(top_k_fragments=9999, quant_all=False)),
    "no_xic": (False, dict(experimental_xic=False)),               # the generic kernel's K x K contraction
    "no_xic_all_fragments": (True, dict(top_k_fragments=9999, experimental_xic=False)),
}
# classes a configuration must reach (tests/test_kernel_classes.py holds the sweep to it on the CPU,
# tests/test_kernel_classes_gpu.py the device plan)
FUSED = set(range(0, 14))
REACHES = {
    "defaults": FUSED | {36}, "best_of_two": FUSED | {36}, "isotopes4": FUSED | {36}, "isotopes1": FUSED | {36},
    "window1": FUSED | {36}, "window5": FUSED | {36},
    "top16": FUSED | set(range(14, 24)) | {36},
    "all_fragments": set(range(37)),
    "all_fragments_best": FUSED | set(range(17, 24)) | {27, 28, 29, 33, 34, 35, 36},
    "no_xic": {36}, "no_xic_all_fragments": {36},
}


def config_of(name: str):
    from alphadia_amd.scoring import CandidateScoringConfig

    cfg = CandidateScoringConfig()
    cfg.update(dict(HANDLER, **CONFIGS[name][1]))
    return cfg
