"""Ion-mobility candidates whose tile does not fit the LDS of a CU: the inputs of tests/test_im_oversize.py and
tests/test_im_oversize_gpu.py, and the rules the device plan and the host apply to the DYNAMIC route of the
ion-mobility feature kernel (``adh_plan_rec_im_kernel``, ``launch_scoring_im``), restated in Python: the LDS layout
of ONE candidate, the launch group it sorts into, the spill layout with its spill block, and the bound that is left.

Input B ("oversize by fragments"): every 7th row of the base sweep of tests/box_sweep_im.py on a library of 200
fragments per precursor, every planted row with a slice of 200, scored with ``top_k_fragments = 9999``.
Input A ("ragged"): the rows of B whose own layout is within the limit, as ONE call: no candidate is too large, only the
product of the call's maxima.
Input C ("oversize by observations"): the run "obs3" (three and six observations) with every slice at 40 fragments and
``top_k_fragments = 40``.
"""

from __future__ import annotations

import functools

import numpy as np

import box_sweep_im as bi
import helpers as H
import synthetic as syn

# ---- adh_features_im.hip / adh_feature_layout.h, restated ---------------------------------------------------------
CU_LDS = bi.LDS_LIMIT
LDS_LIMIT = CU_LDS - bi.IM_STATIC_LDS                 # dynamic LDS a block of the feature kernel may ask for: 161 280
SMALL_LDS = 40 * 1024 - 2 * 16 * 17 * 4               # ADH_GENERIC_SMALL_LDS: the edge between the two LDS groups (untuned)
GROUP_SMALL, GROUP_LARGE, GROUP_SPILL, N_GROUPS = 0, 1, 2, 3
THIN = 7

VARIANTS = {"all_fragments": dict(), "no_xic_all_fragments": dict(experimental_xic=False),
            "all_fragments_best": dict(quant_all=False)}
CONFIG_NAMES = tuple(VARIANTS)
TOP_K = {"A": 9999, "B": 9999, "C": 40}


def config_of(name: str, which: str = "B"):
    from alphadia_amd.scoring import CandidateScoringConfig

    cfg = CandidateScoringConfig()
    cfg.update(dict(bi.HANDLER, **VARIANTS[name], top_k_fragments=TOP_K[which]))
    return cfg


def _work_floats(K, O, S, F, I):
    """The work region: centred profiles [K][O][max(S, F)]; the isotope scan sums of a materialised tile [I][S]."""
    return max(K * O * max(S, F), I * S)


def layout_bytes(K, O, S, F, I, spill=False):
    """featim::Layout / featim::LayoutSpill on a candidate's own capacities.  The spill layout leaves the work region
    and the profile regions R1 and R2 (ffp, fsp_raw / ffp_u, fsp_u, fsp, bp) to the spill block; R1 keeps the
    template [O][S][F]."""
    K, O, S, F, I = int(K), max(int(O), 1), int(S), int(F), max(int(I), 1)   # (featim::own_caps)
    qtf = max(I * O * S, 4 * K + F)
    n_double = qtf + 6 * K * O + 2 * O + 2 * I
    prof = K * O * (F + S)
    if spill:
        regions = O * S * F
    else:
        regions = _work_floats(K, O, S, F, I) + max(O * S * F, prof) + prof
    n_float = regions + 2 * O * F + 2 * O * S + O * S + 8 * K + 4 * K * O + 4 * O + 3 * I + 2 * F + bi.NUM_FEATURES
    n_int = 4 * K + K * O + O
    return n_double * 8 + (n_float * 4 + 7) // 8 * 8 + (n_int * 4 + 7) // 8 * 8 + (5 * K + 7) // 8 * 8


def spill_block_bytes(K, O, S, F, I):
    """featim::spill_bytes: work region, R1 and R2 behind the candidate's gather cells in the scratch slab."""
    K, O, S, F, I = int(K), max(int(O), 1), int(S), int(F), max(int(I), 1)   # (featim::own_caps)
    return ((_work_floats(K, O, S, F, I) + 2 * K * O * (F + S)) * 4 + 31) // 32 * 32


def launch_group(K, O, S, F, I, spill_all=False):
    """(group, dynamic LDS) of one candidate of the dynamic route, or (GROUP_SPILL, None) beyond the bound that is left."""
    own = layout_bytes(K, O, S, F, I)
    if own <= LDS_LIMIT and not spill_all:
        return (GROUP_SMALL if own <= SMALL_LDS else GROUP_LARGE), own
    sp = layout_bytes(K, O, S, F, I, spill=True)
    return GROUP_SPILL, (sp if sp <= LDS_LIMIT else None)


def spill_k_max(O, S, F, I):
    """The bound that is left: the most fragments a candidate of O observations in S scans x F cycles may keep."""
    lo, hi = 1, 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if layout_bytes(mid, O, S, F, I, spill=True) <= LDS_LIMIT:
            lo = mid
        else:
            hi = mid - 1
    return lo


def own_layouts(table, I, spill=False):
    return np.array([layout_bytes(k, o, s, f, I, spill) for k, o, s, f in zip(table["k_cap"], table["O"], table["S"], table["F"])],
                    dtype=np.int64)


def expected_stats(case, soa, cfg, env: dict | None = None):
    """What Context.im_launch_stats() must report after ONE plan over ``soa`` (one chunk), and the group of every row
    (-1: its class does not take the dynamic route).  The route of a class follows from the maxima of the call
    (``box_sweep_im.instantiation_of``); rows flagged to be skipped ask for no LDS."""
    env = env or {}
    t = bi.shape_table(case, soa, cfg)
    I = max(min(int(cfg.top_k_isotopes), bi.N_ISOTOPE_COLUMNS), 1)
    classes = bi.classes_of(t)
    n_class = {int(c): int((classes == c).sum()) for c in np.unique(classes)}
    inst = bi.instantiation_of(bi.batch_caps(t, np.arange(len(t)), cfg), n_class, cfg, env)
    flags = np.asarray(soa.get("flags", np.zeros(len(classes), np.uint8)))
    group = np.full(len(classes), -1, dtype=np.int64)
    cand, lds = np.zeros(N_GROUPS, np.int64), np.zeros(N_GROUPS, np.int64)
    for r in range(len(classes)):
        if inst[int(classes[r])][0] != "dynamic":
            continue
        g, need = launch_group(t["k_cap"][r], t["O"][r], t["S"][r], t["F"][r], I, "ADH_DEBUG_IM_SPILL" in env)
        if flags[r] & 1:
            need = 0
        assert need is not None, r
        group[r] = g
        cand[g] += 1
        lds[g] = max(lds[g], need)
    return {"candidates": cand, "lds_bytes": lds}, group


# ---- the inputs ---------------------------------------------------------------------------------------------------

def _sweep(run: str, spec, k_fragments: int, on_bins: bool = False):
    """``box_sweep_im.sweep_case(run)`` on another specification and library size.  The two module attributes are put
    back before this returns: other modules build their sweeps from them.  ``on_bins``: every library fragment sits on
    a TOF bin of the run (a 15 ppm window is narrower than a bin of this run at 200 ... 350 Th: about half the windows of
    a drawn library hold no bin, and a slice of 200 fills some 60 ... 120 fragment slots)."""
    make_library = syn.make_library

    def library(n, seed, k_fragments_=40, **kw):
        kw.pop("k_fragments", None)
        lib = make_library(n, seed, k_fragments=k_fragments, **kw)
        if on_bins:
            table = bi.mz_table_of(bi.RUNS[run].get("n_tof", bi.N_TOF))
            mz = lib.fragment_df["mz_library"].values.astype(np.float64)
            on = table[np.clip(np.searchsorted(table, mz), 0, len(table) - 1)]
            f32 = on.astype(np.float32)   # (never above its bin: the events of a fragment go to the first bin at or above it)
            f32 = np.where(f32.astype(np.float64) > on, np.nextafter(f32, np.float32(0)), f32)
            lib.fragment_df["mz_library"] = f32.astype(np.float32)
        return lib

    # (sweep_case takes its specification and its library from these two names and has no parameter for either)
    spec_rows = bi.spec_rows
    bi.spec_rows, syn.make_library = (lambda run_=run: spec.copy()), library
    try:
        case = bi.sweep_case(run)
    finally:
        bi.spec_rows, syn.make_library = spec_rows, make_library
    soa = H.soa_for(case, bi.config_of("defaults"))
    assert np.array_equal(soa["precursor_idx"], np.arange(len(spec)))  # (table order = sweep order)
    return case, soa, spec


@functools.lru_cache(maxsize=None)
def oversize_by_fragments(on_bins: bool = False):
    """Input B: (case, assembled table, specification).  ``on_bins``: the same boxes with every library fragment on a
    TOF bin, so that the long rows fill 150 and more fragment slots (the entry-point test)."""
    spec = bi.spec_rows("base").iloc[::THIN].reset_index(drop=True)
    spec.loc[spec["density"].values == "", "nl"] = 200
    return _sweep("base", spec, 200, on_bins)


@functools.lru_cache(maxsize=None)
def oversize_by_observations():
    """Input C."""
    spec = bi.spec_rows("obs3")
    spec["nl"] = 40
    return _sweep("obs3", spec, 40)


@functools.lru_cache(maxsize=None)
def ragged_rows():
    """The rows of B that make input A: own layout within the limit."""
    case, soa, spec = oversize_by_fragments()
    t = bi.shape_table(case, soa, config_of("all_fragments", "B"))
    return np.flatnonzero(own_layouts(t, 3) <= LDS_LIMIT)


def rows_of(soa: dict, idx) -> dict:
    n = len(soa["precursor_idx"])
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in soa.items()}


@functools.lru_cache(maxsize=None)
def ragged():
    """Input A: (case, assembled table, specification)."""
    case, soa, spec = oversize_by_fragments()
    idx = ragged_rows()
    return case, rows_of(soa, idx), spec.iloc[idx].reset_index(drop=True)


@functools.lru_cache(maxsize=None)
def bound_case(O: int, S: int, F: int):
    """(case, assembled table, specification, row) for the bound that is left: twelve interior boxes of S scans x F
    cycles on a library of 200 fragments per precursor, and the first row the plan gives exactly O observations.  (The
    test lengthens that row's library slice over the fragments of the rows behind it.)"""
    run, designed = {2: ("base", 2), 6: ("obs3", 2)}[O]
    rows = [(S, F, 1, i % 3, 1, 1, designed, 200, "k", "") for i in range(12)]
    spec = bi.pd.DataFrame(rows, columns=["S", "F", "pos_f", "pos_s", "ce_f", "ce_s", "O", "nl", "batch", "density"])
    case, soa, spec = _sweep(run, spec, 200)
    t = bi.shape_table(case, soa, config_of("all_fragments", "B"))
    hit = np.flatnonzero((t["O"].values == O) & (t["S"].values == S) & (t["F"].values == F))
    assert len(hit) and hit[0] < 6, t
    return case, soa, spec, int(hit[0])


def input_of(which: str):
    return {"A": ragged, "B": oversize_by_fragments, "C": oversize_by_observations}[which]()


_oracle_cache = {}


def oracle_tables(oracle_lib, which, name):
    """The oracle's tables of an input under a configuration: computed once, never written to.  (A: the rows of B's.)"""
    from alphadia_amd.scoring import fragment_columns, pack_assembled

    if which == "A":
        full = oracle_tables(oracle_lib, "B", name)
        return {k: v[ragged_rows()] for k, v in full.items()}
    if (which, name) not in _oracle_cache:
        case, soa, _ = input_of(which)
        _oracle_cache[which, name] = oracle_lib.score_timstof(
            case.dia, fragment_columns(case.library.fragment_df, "mz_library"), pack_assembled(soa),
            config_of(name, which).to_jitclass(), n_threads=8, with_stats=True)
    return _oracle_cache[which, name]
