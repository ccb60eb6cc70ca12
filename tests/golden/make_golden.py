"""Generate the golden vectors under tests/golden/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE.  Run in the build container only (``/root/reference`` is
mounted there):

    python tests/golden/make_golden.py

It imports the reference's own modules through ``ref_shim`` (which stubs the
missing third-party packages numba / alphatims / alpharaw, nothing else), feeds
them synthetic inputs from ``tests/synthetic.py`` and stores inputs AND
outputs as small ``.npz`` fixtures, so that the tests need neither the
reference nor bit-reproducible random streams on the GPU box.

Shim caveats (NumPy-2 promotion, pairwise sums, argsort ties) are listed in
``ref_shim.py`` and repeated in every fixture's ``caveat`` field.
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
# fixtures go to tests/golden/ unless --out DIR is given (tests/test_golden_regenerate.py writes to a temp dir)
OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))  # tests/: the synthetic generators
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402

ref_shim.install()

from alphadia.fragcomp.fragcomp import FragmentCompetition  # noqa: E402
from alphadia.search.jitclasses.alpharaw_jit import AlphaRawJIT  # noqa: E402
from alphadia.search.scoring import scoring as ref_scoring  # noqa: E402
from alphadia.search.scoring.config import CandidateScoringConfig  # noqa: E402
from alphadia.search.scoring.output import OutputPsmDF  # noqa: E402

import synthetic as syn  # noqa: E402

CAVEAT = (
    "reference executed as pure Python under a numba stub with NumPy "
    + np.__version__
    + ": float32-with-python-float stays float32 (Numba: float64), np.sum is "
    "pairwise (Numba: sequential), argsort tie order may differ"
)


def to_jit(dia: syn.AlphaRawArrays) -> AlphaRawJIT:
    return AlphaRawJIT(
        dia.cycle,
        dia.rt_values,
        dia.mobility_values,
        dia.zeroth_frame,
        dia.max_mz_value,
        dia.min_mz_value,
        np.float32(dia.cycle[0, 1:, :, 1].max()),
        np.float32(dia.cycle[0, 1:, :, 0].min()),
        dia.precursor_cycle_max_index,
        dia.peak_start_idx_list,
        dia.peak_stop_idx_list,
        dia.mz_values,
        dia.intensity_values,
        dia.scan_max_index,
        dia.frame_max_index,
    )


class DuckDia:
    def __init__(self, dia):
        self._dia = dia
        self.cycle = dia.cycle
        self._jit = to_jit(dia)

    def to_jitclass(self):
        return self._jit


def dia_to_dict(dia: syn.AlphaRawArrays) -> dict:
    return {
        "dia_cycle": dia.cycle,
        "dia_rt_values": dia.rt_values,
        "dia_mobility_values": dia.mobility_values,
        "dia_peak_start": dia.peak_start_idx_list,
        "dia_peak_stop": dia.peak_stop_idx_list,
        "dia_mz": dia.mz_values,
        "dia_intensity": dia.intensity_values,
    }


FRAG_COLS = [
    "mz_library",
    "intensity",
    "cardinality",
    "type",
    "loss_type",
    "charge",
    "number",
    "position",
]
PREC_NUM_COLS = [
    "elution_group_idx",
    "precursor_idx",
    "channel",
    "decoy",
    "flat_frag_start_idx",
    "flat_frag_stop_idx",
    "charge",
    "rt_library",
    "mobility_library",
    "mz_library",
    "i_0",
    "i_1",
    "i_2",
    "i_3",
]
CAND_COLS = [
    "elution_group_idx",
    "precursor_idx",
    "rank",
    "scan_start",
    "scan_stop",
    "scan_center",
    "frame_start",
    "frame_stop",
    "frame_center",
    "score",
]


# parameters of the fitted quadrupole calibration of the "fitted_quadrupole" golden (what SimpleQuadrupole.fit
# leaves in jit.sigma / jit.delta_mu, quadrupole.py:195-204)
FITTED_QUADRUPOLE = dict(sigma=(0.35, 0.12), delta_mu=(0.4, -0.25))


def run_scoring(case: syn.SyntheticCase, cfg_updates: dict, quadrupole: dict | None = None):
    cfg = CandidateScoringConfig()
    cfg.update(cfg_updates)
    dia = DuckDia(case.dia)
    cs = ref_scoring.CandidateScoring(
        dia_data=dia,
        precursors_flat=case.library.precursor_df.copy(),
        fragments_flat=case.library.fragment_df.copy(),
        rt_column="rt_library",
        mobility_column="mobility_library",
        precursor_mz_column="mz_library",
        fragment_mz_column="mz_library",
        config=cfg,
    )
    cands = case.candidates_df.copy()
    if quadrupole is not None:  # a fitted calibration: sigma / delta_mu as SimpleQuadrupole.fit sets them
        cs.quadrupole_calibration.jit.sigma = np.array(quadrupole["sigma"], dtype=np.float64)
        cs.quadrupole_calibration.jit.delta_mu = np.array(quadrupole["delta_mu"], dtype=np.float64)
    fragment_container = cs.assemble_fragments()
    sgc = cs.assemble_score_group_container(cands)
    n = sgc.get_candidate_count()
    out = OutputPsmDF(n, cs.config.top_k_fragments)
    ref_scoring._process_score_groups(
        range(len(sgc)),
        sgc,
        out,
        fragment_container,
        dia.to_jitclass(),
        cs.config.to_jitclass(),
        cs.quadrupole_calibration.jit,
        False,
    )
    features_df = cs.collect_candidates(cands, out)
    fragments_df = cs.collect_fragments(cands, out)
    # order of rows in `out` = order of candidates inside the score group container
    order_pidx = np.array(
        [c.precursor_idx for sg in sgc.score_groups for c in sg.candidates], dtype=np.uint32
    )
    order_rank = np.array(
        [c.rank for sg in sgc.score_groups for c in sg.candidates], dtype=np.uint8
    )
    return out, features_df, fragments_df, order_pidx, order_rank, cs.config


def out_to_dict(out: OutputPsmDF) -> dict:
    names = [
        "valid",
        "precursor_idx",
        "rank",
        "features",
        "fragment_precursor_idx",
        "fragment_rank",
        "fragment_mz_library",
        "fragment_mz",
        "fragment_mz_observed",
        "fragment_height",
        "fragment_intensity",
        "fragment_mass_error",
        "fragment_correlation",
        "fragment_position",
        "fragment_number",
        "fragment_type",
        "fragment_charge",
        "fragment_loss_type",
    ]
    return {"out_" + n: np.asarray(getattr(out, n)) for n in names}


def case_to_dict(case: syn.SyntheticCase) -> dict:
    d = dia_to_dict(case.dia)
    for c in FRAG_COLS:
        d["frag_" + c] = case.library.fragment_df[c].values
    for c in PREC_NUM_COLS:
        d["prec_" + c] = case.library.precursor_df[c].values
    for c in CAND_COLS:
        d["cand_" + c] = case.candidates_df[c].values
    return d


def small_case(config_id: int, **kw) -> syn.SyntheticCase:
    args = dict(
        n_precursors=300,
        n_cycles=60,
        config_id=config_id,
        per_precursor=2,
        n_ms2=8,
        ms1_peaks=400,
        ms2_peaks=150,
        mz_lo=400,
        mz_hi=480,
        frag_mz_lo=200,
        frag_mz_hi=350,
        ms1_mz_range=(395, 500),
        ms2_mz_range=(195, 355),
        few_fragment_fraction=0.05,
        even_fraction=0.3,
        planted_fraction=0.5,
        threads=1,
    )
    args.update(kw)
    return syn.make_case(**args)


SCORING_CONFIGS = {
    # what ClassicExtractionHandler passes (extraction_handler.py:370-376,400-409,460-468
    # with default.yaml:158-199 and target tolerances)
    "handler_default": dict(
        score_grouped=False,
        top_k_isotopes=3,
        reference_channel=-1,
        precursor_mz_tolerance=10,
        fragment_mz_tolerance=15,
        exclude_shared_ions=True,
        quant_window=3,
        quant_all=True,
        experimental_xic=True,
        top_k_fragments=12,
    ),
    # the handler's settings with a FITTED quadrupole calibration (FITTED_QUADRUPOLE above)
    "fitted_quadrupole": dict(
        score_grouped=False,
        top_k_isotopes=3,
        reference_channel=-1,
        precursor_mz_tolerance=10,
        fragment_mz_tolerance=15,
        exclude_shared_ions=True,
        quant_window=3,
        quant_all=True,
        experimental_xic=True,
        top_k_fragments=12,
    ),
    # CandidateScoringConfig() defaults (config.py:73-85); used by multiplex requant
    "class_default": dict(),
    # top-k filtering active + narrow tolerances
    "topk6": dict(
        top_k_isotopes=2,
        precursor_mz_tolerance=5,
        fragment_mz_tolerance=7,
        quant_window=2,
        quant_all=True,
        experimental_xic=True,
        top_k_fragments=6,
    ),
}


# libraries with 5..40 fragments per precursor (more than the 12 of a predicted library and than
# the 16 lanes of the register kernels): transfer-library requantification scores every fragment
# (transfer_library_requantification_handler.py:117-124, top_k_fragments = 9999), and a plain top-k
# of 24 with the class defaults exercises the K > 16 branch of the K x K contraction
MANYFRAG_CONFIGS = {
    "manyfrag": dict(SCORING_CONFIGS["handler_default"], top_k_fragments=9999),
    "manyfrag_class": dict(top_k_fragments=24),
}


def golden_scoring(which=None):
    configs = dict(SCORING_CONFIGS, **MANYFRAG_CONFIGS)
    for name, upd in configs.items():
        if which is not None and name not in which:
            continue
        if name in MANYFRAG_CONFIGS:
            case = small_case(131, n_precursors=160, k_fragments=(5, 40), frag_mz_hi=500, ms2_mz_range=(195, 505))
        else:
            case = small_case(101)
        if name == "topk6":
            # give some fragments cardinality 2 so exclude_shared_ions drops them
            rng = np.random.default_rng(7)
            card = case.library.fragment_df["cardinality"].values.copy()
            card[rng.random(card.size) < 0.15] = 2
            case.library.fragment_df["cardinality"] = card
        out, fdf, frdf, opidx, orank, cfg = run_scoring(case, upd, FITTED_QUADRUPOLE if name == "fitted_quadrupole" else None)
        d = case_to_dict(case)
        od = out_to_dict(out)
        if name == "fitted_quadrupole":
            d["cfg_quadrupole_sigma"] = np.asarray(FITTED_QUADRUPOLE["sigma"], dtype=np.float64)
            d["cfg_quadrupole_delta_mu"] = np.asarray(FITTED_QUADRUPOLE["delta_mu"], dtype=np.float64)
        if name in MANYFRAG_CONFIGS:
            # the reference allocates top_k_fragments (9999) columns; keep those a library slice can fill
            lens = (case.library.precursor_df["flat_frag_stop_idx"].values.astype(np.int64)
                    - case.library.precursor_df["flat_frag_start_idx"].values.astype(np.int64))
            width = int(min(int(cfg.top_k_fragments), lens.max()))
            for k, v in od.items():
                if v.ndim == 2 and k != "out_features":
                    assert not v[:, width:].any(), k
                    od[k] = np.ascontiguousarray(v[:, :width])
        d.update(od)
        d["order_precursor_idx"] = opidx
        d["order_rank"] = orank
        cfgj = cfg.to_jitclass()
        for k in (
            "collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
            "reference_channel quant_window quant_all precursor_mz_tolerance "
            "fragment_mz_tolerance experimental_xic"
        ).split():
            d["cfg_" + k] = np.asarray(getattr(cfgj, k))
        d["features_df_columns"] = np.array(list(fdf.columns), dtype="U")
        d["fragments_df_columns"] = np.array(list(frdf.columns), dtype="U")
        d["features_df_precursor_idx"] = fdf["precursor_idx"].values
        d["features_df_rank"] = fdf["rank"].values
        d["features_df_delta_rt"] = fdf["delta_rt"].values
        d["fragments_df_precursor_idx"] = frdf["precursor_idx"].values
        d["fragments_df_mz_observed"] = frdf["mz_observed"].values
        d["fragments_df_n"] = np.asarray(len(frdf))
        d["caveat"] = np.asarray(CAVEAT)
        path = os.path.join(OUT_DIR, f"scoring_{name}.npz")
        np.savez_compressed(path, **d)
        v = np.asarray(out.valid)
        print(
            f"{path}: {v.sum()}/{len(v)} valid, nan rows "
            f"{np.isnan(out.features[v]).any(axis=1).sum()}, {os.path.getsize(path)/1e6:.2f} MB"
        )


def multiplex_case(n_base: int = 120, n_cycles: int = 60):
    """Config 5 in small: 4 label channels per elution group, y-ions shifted, b-ions shared."""
    seed = syn.BASE_SEED + 105
    cycle = syn.make_cycle(n_ms2=8, mz_lo=400, mz_hi=480)
    base = syn.make_library(n_base, seed, mz_lo=400, mz_hi=465, rt_max=n_cycles * 1.5,
                            frag_mz_lo=200, frag_mz_hi=340)
    lib = syn.multiplex_library(base, channels=(0, 4, 8, 12), seed=seed)
    planted = syn.plant_peptides(lib, cycle, n_cycles, seed, fraction=0.6)
    dia = syn.make_thermo_run(n_cycles, seed, cycle=cycle, ms1_peaks=400, ms2_peaks=150,
                              planted=planted, threads=1, ms1_mz_range=(395, 500),
                              ms2_mz_range=(195, 355))
    # reference-channel candidates (one per target precursor of channel 0) ...
    pdf = lib.precursor_df
    ref = pdf[(pdf["channel"] == 0) & (pdf["decoy"] == 0)]
    ref_lib = syn.SyntheticLibrary(ref.reset_index(drop=True), lib.fragment_df)
    apex = planted.apex_cycle[ref.index.values]
    cands = syn.make_candidates(ref_lib, n_cycles, cycle.shape[1], seed, per_precursor=1,
                                apex_cycle=apex, even_fraction=0.3)
    cands["proba"] = np.linspace(0.0, 0.5, len(cands)).astype(np.float32)
    cands["decoy"] = np.uint8(0)
    # ... expanded to all channels by the reference (scoring/utils.py:114-200), as the
    # multiplexing handler does (multiplexing_requantification_handler.py:94-131)
    from alphadia.search.scoring.utils import multiplex_candidates

    mult = multiplex_candidates(cands, pdf, channels=[0, 4, 8, 12])
    mult["rank"] = np.uint8(0)
    # a few elution groups lose their reference channel: ScoreGroup.process skips them
    # (score_group.py:50-65)
    egs = np.unique(mult["elution_group_idx"].values)
    lost = egs[::7]
    mult = mult[~((mult["channel"] == 0) & mult["elution_group_idx"].isin(lost))].reset_index(drop=True)
    for c in ("scan_start", "scan_stop", "scan_center", "frame_start", "frame_stop", "frame_center"):
        mult[c] = mult[c].astype(np.int64)
    mult["elution_group_idx"] = mult["elution_group_idx"].astype(np.uint32)
    mult["precursor_idx"] = mult["precursor_idx"].astype(np.uint32)
    return syn.SyntheticCase(dia, lib, mult[CAND_COLS].copy(), planted.apex_cycle)


def golden_host_helpers():
    """Inputs and outputs of the reference's DataFrame helpers that the host layer restates in
    numpy: ``multiplex_candidates`` (scoring/utils.py:114-200, three settings) and
    ``calculate_score_groups`` (scoring/utils.py:269-410, grouped and not)."""
    from alphadia.search.scoring.utils import calculate_score_groups, multiplex_candidates

    rng = np.random.default_rng(20260928)
    n_eg, channels_all = 150, np.array([0, 4, 8, 12])
    rows = []
    for eg in range(n_eg):
        for decoy in (0, 1):
            for ch in channels_all[: rng.integers(2, 5)]:
                rows.append((eg, decoy, int(ch)))
    lib = pd.DataFrame(rows, columns=["elution_group_idx", "decoy", "channel"])
    lib = lib.sample(frac=1.0, random_state=3).reset_index(drop=True)  # library order is arbitrary
    lib["precursor_idx"] = rng.permutation(len(lib)).astype(np.uint32)
    lib["elution_group_idx"] = lib["elution_group_idx"].astype(np.uint32)
    lib["decoy"] = lib["decoy"].astype(np.uint8)
    lib["channel"] = lib["channel"].astype(np.uint32)
    # the columns precursors_flat_schema asks for (validation/schemas.py:11-32)
    for c in ("flat_frag_start_idx", "flat_frag_stop_idx"):
        lib[c] = np.zeros(len(lib), dtype=np.uint32)
    lib["charge"] = np.full(len(lib), 2, dtype=np.uint8)
    for c in ("rt_library", "mobility_library", "mz_library"):
        lib[c] = rng.random(len(lib)).astype(np.float32)
    lib["proteins"] = np.full(len(lib), "P", dtype=object)
    lib["genes"] = np.full(len(lib), "G", dtype=object)
    # candidates: several per elution group (different precursors, ranks), ties in proba, some groups absent
    pick = lib[lib["elution_group_idx"] % 5 != 0].sample(frac=0.7, random_state=9)
    cand = pick[["elution_group_idx", "precursor_idx", "decoy", "channel"]].copy().reset_index(drop=True)
    cand = pd.concat([cand, cand.iloc[::3]], ignore_index=True)
    cand["channel"] = cand["channel"].astype(np.uint8)  # candidates_schema: uint8
    cand["rank"] = rng.integers(0, 3, len(cand)).astype(np.uint8)
    cand["proba"] = np.round(rng.random(len(cand)), 1).astype(np.float32)  # many ties
    for c in ("scan_start", "scan_stop", "scan_center", "frame_start", "frame_stop", "frame_center"):
        cand[c] = rng.integers(0, 5000, len(cand)).astype(np.int64)
    cand["score"] = rng.random(len(cand)).astype(np.float32)
    d = {"lib_" + c: lib[c].values for c in lib.columns if lib[c].dtype != object}
    d.update({"cand_" + c: cand[c].values for c in cand.columns})
    settings = {"default": dict(), "with_decoys": dict(remove_decoys=False), "two_channels": dict(channels=[0, 8])}
    for name, kw in settings.items():
        out = multiplex_candidates(cand.copy(), lib.copy(), **kw)
        d[f"mult_{name}_columns"] = np.array(list(out.columns), dtype="U")
        for c in out.columns:
            d[f"mult_{name}_{c}"] = out[c].values
        print(f"multiplex_candidates[{name}]: {len(out)} rows")
    for name, grouped in (("plain", False), ("grouped", True)):
        out = calculate_score_groups(cand.copy(), group_channels=grouped)
        for c in ("precursor_idx", "rank", "score_group_idx"):
            d[f"groups_{name}_{c}"] = out[c].values
    path = os.path.join(OUT_DIR, "host_helpers.npz")
    np.savez_compressed(path, **d)
    print(f"{path}: {os.path.getsize(path)/1e3:.0f} kB")


def _spectrum_tables(rng, n_cycles, n_windows, prefix, ms1_every_cycle=True, peaks=(3, 9)):
    """An AlphaRaw-style spectrum_df / peak_df pair: ``prefix`` non-DIA spectra, then cycles of one MS1
    + ``n_windows`` MS2 spectra (rt in minutes, as alpharaw delivers it)."""
    edges = np.linspace(400.0, 400.0 + 10.0 * n_windows, n_windows + 1)
    lower, upper, level, prec = [], [], [], []
    for _ in range(prefix):  # calibration / settling scans before the method starts cycling
        lo = float(rng.uniform(300, 900))
        lower.append(lo)
        upper.append(lo + float(rng.uniform(1, 30)))
        level.append(2)
        prec.append(lo + 1)
    for c in range(n_cycles):
        if ms1_every_cycle or c % 3 != 1:
            lower.append(-1.0)
            upper.append(-1.0)
            level.append(1)
            prec.append(-1.0)
        for w in range(n_windows):
            lower.append(edges[w])
            upper.append(edges[w + 1])
            level.append(2)
            prec.append(0.5 * (edges[w] + edges[w + 1]))
    n = len(lower)
    counts = rng.integers(peaks[0], peaks[1], n)
    stop = np.cumsum(counts)
    spectrum_df = pd.DataFrame({
        "spec_idx": np.arange(n, dtype=np.int64), "rt": np.cumsum(rng.uniform(0.0008, 0.0012, n)),
        "ms_level": np.array(level, dtype=np.int64), "precursor_mz": np.array(prec, dtype=np.float64),
        "isolation_lower_mz": np.array(lower, dtype=np.float64), "isolation_upper_mz": np.array(upper, dtype=np.float64),
        "peak_start_idx": (stop - counts).astype(np.int64), "peak_stop_idx": stop.astype(np.int64),
    })
    mz = np.concatenate([np.sort(rng.uniform(150, 1500, c)) for c in counts])
    peak_df = pd.DataFrame({"mz": mz, "intensity": rng.lognormal(5, 1, mz.size)})
    return spectrum_df, peak_df


def golden_staging():
    """f-4: what the reference derives from a spectrum table before anything is scored -
    ``determine_dia_cycle`` (raw_data/dia_cycle.py:18-82) and ``AlphaRaw._preprocess_raw_data``
    (raw_data/alpharaw_wrapper.py:72-117) - on tables with a non-DIA prefix and with an MS1 that
    does not follow the cycle."""
    import types as _types

    from alphadia.raw_data.alpharaw_wrapper import AlphaRaw
    from alphadia.raw_data.dia_cycle import determine_dia_cycle

    rng = np.random.default_rng(77)
    cases = {
        "plain": dict(n_cycles=40, n_windows=12, prefix=0),
        "prefix": dict(n_cycles=35, n_windows=9, prefix=7),
        "irregular_ms1": dict(n_cycles=45, n_windows=6, prefix=0, ms1_every_cycle=False),
    }
    d = {}
    for name, kw in cases.items():
        sdf, pdf = _spectrum_tables(rng, **kw)
        for c in sdf.columns:
            d[f"{name}_spec_{c}"] = sdf[c].values
        for c in pdf.columns:
            d[f"{name}_peak_{c}"] = pdf[c].values
        obj = _types.SimpleNamespace(spectrum_df=sdf.copy(), peak_df=pdf.copy(), has_ms1=True)
        obj._is_ms1_dia = _types.MethodType(AlphaRaw._is_ms1_dia, obj)
        AlphaRaw._preprocess_raw_data(obj)
        cycle, start, length = determine_dia_cycle(obj.spectrum_df if not obj.has_ms1 else sdf)
        d[f"{name}_cycle_direct"] = cycle
        for attr in ("cycle", "rt_values", "_peak_start_idx_list", "_peak_stop_idx_list", "_mz_values", "_intensity_values"):
            d[f"{name}_{attr.lstrip('_')}"] = np.asarray(getattr(obj, attr))
        for attr in ("_cycle_start", "_cycle_length", "_precursor_cycle_max_index", "_max_mz_value", "_min_mz_value",
                     "_quad_max_mz_value", "_quad_min_mz_value", "frame_max_index", "has_ms1"):
            d[f"{name}_{attr.lstrip('_')}"] = np.asarray(getattr(obj, attr))
        print(name, "cycle length", obj._cycle_length, "start", obj._cycle_start, "has_ms1", obj.has_ms1,
              "spectra", len(obj.rt_values))
    path = os.path.join(OUT_DIR, "staging.npz")
    np.savez_compressed(path, **d)
    print(f"{path}: {os.path.getsize(path)/1e3:.0f} kB")


def golden_multiplex():
    case = multiplex_case()
    upd = dict(score_grouped=True, exclude_shared_ions=True, reference_channel=0, experimental_xic=True)
    out, fdf, frdf, opidx, orank, cfg = run_scoring(case, upd)
    d = case_to_dict(case)
    d.update(out_to_dict(out))
    d["order_precursor_idx"] = opidx
    d["order_rank"] = orank
    cfgj = cfg.to_jitclass()
    for k in (
        "collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
        "reference_channel quant_window quant_all precursor_mz_tolerance "
        "fragment_mz_tolerance experimental_xic"
    ).split():
        d["cfg_" + k] = np.asarray(getattr(cfgj, k))
    d["features_df_columns"] = np.array(list(fdf.columns), dtype="U")
    d["fragments_df_columns"] = np.array(list(frdf.columns), dtype="U")
    d["features_df_precursor_idx"] = fdf["precursor_idx"].values
    d["features_df_rank"] = fdf["rank"].values
    d["features_df_delta_rt"] = fdf["delta_rt"].values
    d["fragments_df_precursor_idx"] = frdf["precursor_idx"].values
    d["fragments_df_mz_observed"] = frdf["mz_observed"].values
    d["fragments_df_n"] = np.asarray(len(frdf))
    d["caveat"] = np.asarray(CAVEAT)
    path = os.path.join(OUT_DIR, "scoring_multiplex.npz")
    np.savez_compressed(path, **d)
    v = np.asarray(out.valid)
    print(f"{path}: {v.sum()}/{len(v)} valid, {os.path.getsize(path)/1e6:.2f} MB")


def edges_case():
    """Hand-made edge cases on top of a small run: precursors at the edge of the isolation scheme,
    windows of 1-4 cycles, boxes at the first / last cycle, libraries of 0-4 fragments,
    fragments outside the m/z range of the run, precursors on a window boundary."""
    case = small_case(103, n_precursors=60, per_precursor=1, few_fragment_fraction=0.0,
                      even_fraction=0.0, planted_fraction=0.8)
    pdf = case.library.precursor_df.copy()
    fdf = case.library.fragment_df.copy()
    L = case.dia.cycle_len
    n_cycles = case.dia.n_cycles
    cands = case.candidates_df.copy().reset_index(drop=True)
    n = len(pdf)
    mz = pdf["mz_library"].values.copy()
    # (a precursor outside EVERY window makes the reference raise inside
    # quadrupole_transfer_function_single; that case is implementation-defined)
    mz[0] = 400.2   # isotope range starts below the first window
    mz[1] = 479.4   # ... and ends above the last one
    mz[2] = 410.0   # exactly on a window boundary (windows are 10 Th wide from 400)
    mz[3] = 409.6   # isotopes straddle the boundary -> two observations
    pdf["mz_library"] = mz.astype(np.float32)
    # fragment counts 0..4 for precursors 4..8
    start = pdf["flat_frag_start_idx"].values.astype(np.int64).copy()
    stop = pdf["flat_frag_stop_idx"].values.astype(np.int64).copy()
    for j, cnt in zip(range(4, 9), (0, 1, 2, 3, 4)):
        stop[j] = start[j] + cnt
    pdf["flat_frag_stop_idx"] = stop.astype(np.uint32)
    # precursor 9: all fragments outside the acquired m/z range
    f = fdf["mz_library"].values.copy()
    f[start[9]:stop[9]] = np.linspace(50.0, 60.0, stop[9] - start[9], dtype=np.float32)
    # precursor 10: half of them above it
    f[start[10]:start[10] + 6] = np.linspace(2000.0, 2100.0, 6, dtype=np.float32)
    fdf["mz_library"] = f.astype(np.float32)

    def box(i, c, h_lo, h_hi):
        cands.loc[i, "frame_start"] = (c - h_lo) * L
        cands.loc[i, "frame_stop"] = (c + h_hi + 1) * L
        cands.loc[i, "frame_center"] = c * L

    box(11, 20, 0, 0)   # one cycle
    box(12, 20, 0, 1)   # two cycles
    box(13, 20, 1, 1)   # three
    box(14, 20, 1, 2)   # four
    box(15, 3, 3, 3)    # touches the first cycle
    box(16, n_cycles - 4, 3, 3)  # touches the last cycle
    box(17, 30, 14, 14)  # 29 cycles
    box(18, 30, 16, 17)  # 34 cycles: beyond the register kernels
    case.library.precursor_df = pdf
    case.library.fragment_df = fdf
    case.candidates_df = cands
    return case


def golden_edges():
    case = edges_case()
    out, fdf, frdf, opidx, orank, cfg = run_scoring(case, SCORING_CONFIGS["handler_default"])
    d = case_to_dict(case)
    d.update(out_to_dict(out))
    d["order_precursor_idx"] = opidx
    d["order_rank"] = orank
    cfgj = cfg.to_jitclass()
    for k in (
        "collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
        "reference_channel quant_window quant_all precursor_mz_tolerance "
        "fragment_mz_tolerance experimental_xic"
    ).split():
        d["cfg_" + k] = np.asarray(getattr(cfgj, k))
    d["features_df_columns"] = np.array(list(fdf.columns), dtype="U")
    d["fragments_df_columns"] = np.array(list(frdf.columns), dtype="U")
    d["features_df_precursor_idx"] = fdf["precursor_idx"].values
    d["features_df_rank"] = fdf["rank"].values
    d["features_df_delta_rt"] = fdf["delta_rt"].values
    d["fragments_df_precursor_idx"] = frdf["precursor_idx"].values
    d["fragments_df_mz_observed"] = frdf["mz_observed"].values
    d["fragments_df_n"] = np.asarray(len(frdf))
    d["caveat"] = np.asarray(CAVEAT)
    path = os.path.join(OUT_DIR, "scoring_edges.npz")
    np.savez_compressed(path, **d)
    v = np.asarray(out.valid)
    print(f"{path}: {v.sum()}/{len(v)} valid; first 20 valid flags {v[:20].astype(int)}; "
          f"n_obs of 0..3: {np.asarray(out.features)[:4, 17]}")


class _ScalarExpThroughLibm:
    """The numpy module with ``exp`` of a float64 SCALAR evaluated by libm, as Numba compiles it.  NumPy's own float64
    exp differs from libm's in the last bit for 2 - 3 % of its arguments; in ``weighted_center_mean``
    (features_utils.py:21) that moves a float64 mean m/z by 1e-16 relative, and the float32 rounding of the mass
    error in ppm by one ulp on about one fragment in 15 000."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def exp(x):
        import math

        return np.float64(math.exp(float(x))) if np.ndim(x) == 0 else np.exp(x)


def golden_boxes():
    """Candidate shapes at the limits of the scoring kernel classes (tests/box_sweep.py, the thinned sweep): boxes of
    2 ... 36 cycles with the centre on their first / middle / last cycle, at both ends of a run that ends inside a
    cycle, one and two observations - on a 12-fragment library under the handler's settings with quant_window = 5,
    and on library slices of 1 ... 200 fragments with every fragment kept and quant_all off."""
    import alphadia.search.scoring.features.features_utils as features_utils
    import box_sweep as bs

    features_utils.np = _ScalarExpThroughLibm()  # (this recipe only: the other fixtures were made with NumPy's exp)
    variants = (
        ("boxes", False, dict(SCORING_CONFIGS["handler_default"], quant_window=5)),
        ("boxes_ragged", True, dict(SCORING_CONFIGS["handler_default"], top_k_fragments=9999, quant_all=False)),
    )
    for name, ragged, upd in variants:
        case = bs.sweep_case(ragged, golden=True)
        out, fdf, frdf, opidx, orank, cfg = run_scoring(case, upd)
        d = case_to_dict(case)
        od = out_to_dict(out)
        # the reference allocates top_k_fragments columns; keep those a library slice can fill (as "manyfrag")
        lens = (case.library.precursor_df["flat_frag_stop_idx"].values.astype(np.int64)
                - case.library.precursor_df["flat_frag_start_idx"].values.astype(np.int64))
        width = int(min(int(cfg.top_k_fragments), lens.max()))
        for k, v in od.items():
            if v.ndim == 2 and k != "out_features":
                assert not v[:, width:].any(), k
                od[k] = np.ascontiguousarray(v[:, :width])
        d.update(od)
        d["order_precursor_idx"] = opidx
        d["order_rank"] = orank
        cfgj = cfg.to_jitclass()
        for k in (
            "collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
            "reference_channel quant_window quant_all precursor_mz_tolerance "
            "fragment_mz_tolerance experimental_xic"
        ).split():
            d["cfg_" + k] = np.asarray(getattr(cfgj, k))
        # (no features_df_columns / fragments_df_columns here: their order follows a set and changes from run to run)
        d["features_df_precursor_idx"] = fdf["precursor_idx"].values
        d["features_df_rank"] = fdf["rank"].values
        d["features_df_delta_rt"] = fdf["delta_rt"].values
        d["fragments_df_precursor_idx"] = frdf["precursor_idx"].values
        d["fragments_df_mz_observed"] = frdf["mz_observed"].values
        d["fragments_df_n"] = np.asarray(len(frdf))
        d["caveat"] = np.asarray(CAVEAT)
        path = os.path.join(OUT_DIR, f"scoring_{name}.npz")
        np.savez_compressed(path, **d)
        v = np.asarray(out.valid)
        print(f"{path}: {v.sum()}/{len(v)} valid, {os.path.getsize(path)/1e6:.2f} MB")
    features_utils.np = np


def golden_selection():
    """Next-row golden: CandidateSelection.__call__ on a small AlphaRaw run.

    Produced with the FFT stand-in of ref_shim.install_selection_glue (np.fft instead of
    rocket_fft/pocketfft; float32 results): scores agree with any other exact convolution to
    ~1e-5 relative, so a candidate whose score ties another one within that margin may swap or
    move by a cycle.  The golden stores the smoothed score row of every precursor as well."""
    import ref_shim

    ref_shim.install_selection_glue()
    from alphadia.search.selection import selection as ref_sel
    from alphadia.search.selection.config_df import CandidateSelectionConfig

    case = small_case(104, n_precursors=240, n_cycles=120, per_precursor=1, planted_fraction=0.7)
    cfgs = {
        "default": dict(rt_tolerance=30.0, candidate_count=3, min_size_rt=3),
        "wide": dict(rt_tolerance=70.0, candidate_count=5, min_size_rt=2, exclude_shared_ions=False,
                     join_close_candidates=False, precursor_mz_tolerance=20.0, fragment_mz_tolerance=30.0),
    }
    d = case_to_dict(case)
    d["caveat"] = np.asarray(CAVEAT)
    for name, upd in cfgs.items():
        cfg = CandidateSelectionConfig()
        cfg.update(upd)
        dia = DuckDia(case.dia)
        cs = ref_sel.CandidateSelection(
            dia, case.library.precursor_df.copy(), case.library.fragment_df.copy(), cfg,
            rt_column="rt_library", mobility_column="mobility_library",
            precursor_mz_column="mz_library", fragment_mz_column="mz_library",
            fwhm_rt=cfg.peak_len_rt, fwhm_mobility=cfg.peak_len_mobility,
        )
        df = cs(thread_count=1)
        d[f"{name}_kernel"] = np.asarray(cs.kernel, dtype=np.float32)
        cj = cs.config_jit
        for k in ("rt_tolerance precursor_mz_tolerance fragment_mz_tolerance candidate_count "
                  "top_k_precursors exclude_shared_ions kernel_size f_mobility f_rt center_fraction "
                  "min_size_mobility min_size_rt max_size_mobility max_size_rt use_weighted_score "
                  "join_close_candidates join_close_candidates_scan_threshold "
                  "join_close_candidates_cycle_threshold").split():
            d[f"{name}_cfg_{k}"] = np.asarray(getattr(cj, k))
        for k in ("feature_mean", "feature_std", "feature_weight"):
            d[f"{name}_cfg_{k}"] = np.asarray(getattr(cj, k), dtype=np.float64)
        for c in ("precursor_idx rank score scan_center scan_start scan_stop frame_center frame_start "
                  "frame_stop elution_group_idx decoy").split():
            d[f"{name}_out_{c}"] = df[c].values
        print(name, len(df), "candidates for", df["precursor_idx"].nunique(), "precursors;",
              "ranks", np.bincount(df["rank"].values))
    path = os.path.join(OUT_DIR, "selection.npz")
    np.savez_compressed(path, **d)
    print(path, f"{os.path.getsize(path)/1e6:.2f} MB")


def golden_transpose():
    """Staging-format golden: the reference's `_transpose`
    (alphadia/raw_data/bruker.py:201-280) on a small frame-major event list."""
    from alphadia.raw_data.bruker import _transpose

    rng = np.random.default_rng(17)
    n_push, n_tof = 3000, 700
    counts = rng.poisson(12, n_push)
    counts[rng.random(n_push) < 0.1] = 0  # empty pushes
    push_indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(push_indptr[-1])
    # inside a push the tof indices are ascending and may repeat across pushes
    tof = np.concatenate([np.sort(rng.integers(0, n_tof, c)) for c in counts]).astype(np.uint32)
    values = rng.integers(1, 4000, n).astype(np.uint16)
    push_indices, tof_indptr, new_values = _transpose(tof, push_indptr, n_tof, values)
    path = os.path.join(OUT_DIR, "transpose.npz")
    np.savez_compressed(path, tof_indices=tof, push_indptr=push_indptr, n_tof=np.asarray(n_tof), values=values,
                        out_push_indices=push_indices, out_tof_indptr=tof_indptr, out_values=new_values)
    print(path, n, "events", f"{os.path.getsize(path)/1e6:.2f} MB")


def golden_selection_kats():
    """Known answers of the small selection functions, produced by the reference functions
    (selection/utils.py:49-77,218-280): random inputs -> outputs."""
    import ref_shim

    ref_shim.install_selection_glue()
    from alphadia.search.selection.utils import _symetric_limits_1d, find_peaks_1d

    rng = np.random.default_rng(23)
    lim_in, lim_out = [], []
    for _ in range(400):
        n = int(rng.integers(0, 40))
        x = rng.random(n)
        if n and rng.random() < 0.5:  # a real peak shape
            c0 = rng.integers(0, n)
            x = np.exp(-0.5 * ((np.arange(n) - c0) / rng.uniform(1, 6)) ** 2) + 0.05 * rng.random(n)
        center = int(rng.integers(-2, 42))
        f, cf = float(rng.random() * 1.5), float(rng.random())
        mn, mx = int(rng.integers(0, 12)), int(rng.integers(0, 25))
        out = _symetric_limits_1d(x, center, f=f, center_fraction=cf, min_size=mn, max_size=mx)
        pad = np.full(40, np.nan)
        pad[:n] = x
        lim_in.append(np.concatenate([pad, [n, center, f, cf, mn, mx]]))
        lim_out.append(np.asarray(out, dtype=np.int32))
    pk_in, pk_cyc, pk_val, pk_n = [], [], [], []
    for _ in range(200):
        n = int(rng.integers(3, 60))
        row = np.cumsum(rng.normal(size=n))  # random walk: plenty of strict 5-point maxima
        if rng.random() < 0.3:
            row = np.round(row, 1)  # ties
        top_n = int(rng.integers(1, 7))
        scan, cyc, val = find_peaks_1d(np.stack([row, row]), top_n=top_n)
        pad = np.full(60, np.nan)
        pad[:n] = row
        pk_in.append(np.concatenate([pad, [n, top_n]]))
        c = np.full(6, -1, dtype=np.int32)
        v = np.full(6, np.nan)
        c[: len(cyc)] = cyc
        v[: len(val)] = val
        pk_cyc.append(c)
        pk_val.append(v)
        pk_n.append(len(cyc))
    path = os.path.join(OUT_DIR, "selection_kats.npz")
    np.savez_compressed(path, limits_in=np.stack(lim_in), limits_out=np.stack(lim_out), peaks_in=np.stack(pk_in),
                        peaks_cycle=np.stack(pk_cyc), peaks_score=np.stack(pk_val), peaks_n=np.asarray(pk_n))
    print(path, f"{os.path.getsize(path)/1e6:.2f} MB")


def golden_get_dense():
    """G1: AlphaRawJIT.get_dense on hand-picked query lists (incl. overlapping windows)."""
    case = small_case(102, n_precursors=40)
    jit = to_jit(case.dia)
    rng = np.random.default_rng(11)
    L = case.dia.cycle_len
    d = dia_to_dict(case.dia)
    n_cases = 32
    for i in range(n_cases):
        c0 = int(rng.integers(0, 40))
        nc = int(rng.integers(1, 18))
        frame_limits = np.array([[c0 * L, (c0 + nc) * L, 1]], dtype=np.uint64)
        k = int(rng.integers(2, 13))
        ms1 = i % 3 == 0
        if ms1:
            mzq = np.sort(rng.uniform(400, 480, k)).astype(np.float32)
            quad = np.array([[-1.0, -1.0]])
            tol = np.float32(10)
        else:
            mzq = np.sort(rng.uniform(200, 350, k)).astype(np.float32)
            lo = rng.uniform(400, 478)
            quad = np.array([[lo, lo + rng.uniform(0.5, 12.0)]], dtype=np.float32)
            tol = np.float32(15)
        if i % 4 == 1:
            # overlapping windows: duplicate / near-duplicate queries, huge tolerance
            mzq[1] = mzq[0] * np.float32(1 + 5e-6)
            tol = np.float32(200)
            mzq = np.sort(mzq)
        if i % 5 == 4 and nc > 0:
            # use the real m/z of peaks so windows are hit for sure
            s = int(rng.integers(0, case.dia.n_spectra))
            a, b = case.dia.peak_start_idx_list[s], case.dia.peak_stop_idx_list[s]
            mzq = np.sort(rng.choice(case.dia.mz_values[a:b], size=k, replace=False)).astype(
                np.float32
            )
        absolute = i % 2 == 0
        dense, pidx = jit.get_dense(
            frame_limits,
            np.array([[0, 1, 1]], dtype=np.uint64),
            mzq,
            tol,
            quad,
            absolute_masses=absolute,
        )
        d[f"q{i}_frame_limits"] = frame_limits
        d[f"q{i}_mz"] = mzq
        d[f"q{i}_tol"] = np.asarray(tol)
        d[f"q{i}_quad"] = np.asarray(quad, dtype=np.float64)
        d[f"q{i}_absolute"] = np.asarray(absolute)
        d[f"q{i}_dense"] = dense
        d[f"q{i}_pidx"] = np.asarray(pidx, dtype=np.int64)
    d["n_cases"] = np.asarray(n_cases)
    d["caveat"] = np.asarray(CAVEAT)
    path = os.path.join(OUT_DIR, "get_dense_alpharaw.npz")
    np.savez_compressed(path, **d)
    print(path, f"{os.path.getsize(path)/1e6:.2f} MB")


def golden_fragcomp():
    """G6: FragmentCompetition.__call__ on a synthetic PSM / fragment table."""
    rng = np.random.default_rng(13)
    n_psm = 5000
    cycle = syn.make_cycle(n_ms2=8, mz_lo=400, mz_hi=480)
    precursor_idx = rng.permutation(n_psm).astype(np.uint32)
    rank = rng.integers(0, 2, n_psm).astype(np.uint8)
    mz_observed = rng.uniform(400, 480, n_psm).astype(np.float32)
    rt_observed = rng.uniform(0, 120, n_psm).astype(np.float32)
    proba = rng.random(n_psm).astype(np.float32)
    nfrag = rng.integers(3, 13, n_psm)
    # a pool of shared fragment m/z values so that overlaps >= 3 really happen
    pool = np.sort(rng.uniform(200, 350, 160)).astype(np.float32)
    f_pidx, f_rank, f_mz = [], [], []
    for i in range(n_psm):
        mz = rng.choice(pool, nfrag[i], replace=False) * (
            1 + rng.normal(0, 4e-6, nfrag[i])
        ).astype(np.float32)
        f_pidx.append(np.full(nfrag[i], precursor_idx[i], np.uint32))
        f_rank.append(np.full(nfrag[i], rank[i], np.uint8))
        f_mz.append(np.sort(mz).astype(np.float32))
    psm_df = pd.DataFrame(
        {
            "precursor_idx": precursor_idx,
            "rank": rank,
            "mz_observed": mz_observed,
            "rt_observed": rt_observed,
            "proba": proba,
        }
    )
    frag_df = pd.DataFrame(
        {
            "precursor_idx": np.concatenate(f_pidx),
            "rank": np.concatenate(f_rank),
            "mz_observed": np.concatenate(f_mz),
        }
    )
    d = {
        "psm_precursor_idx": precursor_idx,
        "psm_rank": rank,
        "psm_mz_observed": mz_observed,
        "psm_rt_observed": rt_observed,
        "psm_proba": proba,
        "frag_precursor_idx": frag_df["precursor_idx"].values,
        "frag_rank": frag_df["rank"].values,
        "frag_mz_observed": frag_df["mz_observed"].values,
        "cycle": cycle,
    }
    fc = FragmentCompetition(rt_tol_seconds=3, mass_tol_ppm=15, thread_count=1)
    res = fc(psm_df.copy(), frag_df.copy(), cycle)
    d["surviving_precursor_idx"] = res["precursor_idx"].values
    d["surviving_rank"] = res["rank"].values
    d["caveat"] = np.asarray(CAVEAT)
    path = os.path.join(OUT_DIR, "fragcomp.npz")
    np.savez_compressed(path, **d)
    print(path, f"{len(res)}/{n_psm} survive, {os.path.getsize(path)/1e6:.2f} MB")


def timstof_to_jit(dia):
    from alphadia.search.jitclasses.bruker_jit import TimsTOFTransposeJIT

    n_frames = dia.rt_values.shape[0]
    return TimsTOFTransposeJIT(
        np.ones(n_frames),                      # accumulation_times
        dia.cycle,
        dia.dia_mz_cycle,
        dia.dia_precursor_cycle,
        dia.frame_max_index,
        np.ones(dia.mz_values.shape[0]),        # intensity_corrections
        60000, 0,                               # intensity max / min
        dia.intensity_values,
        1.0,                                    # max_accumulation_time
        float(dia.mobility_values.max()), float(dia.mobility_values.min()),
        dia.mobility_values,
        dia.mz_values,
        np.zeros(1, np.int64), 0,               # precursor_indices, precursor_max_index
        np.zeros(1, np.int64),                  # quad_indptr
        float(dia.cycle.max()), float(dia.cycle[dia.cycle > 0].min()),
        np.zeros((1, 2)),                       # quad_mz_values
        np.zeros(1, np.int64),                  # raw_quad_indptr
        dia.rt_values,
        dia.scan_max_index,
        dia.mz_values.shape[0],                 # tof_max_index
        0,                                      # use_calibrated_mz_values_as_default
        dia.zeroth_frame,
        dia.push_indices,
        dia.tof_indptr,
    )


class DuckTims:
    def __init__(self, dia):
        self.cycle = dia.cycle
        self._jit = timstof_to_jit(dia)

    def to_jitclass(self):
        return self._jit


TIMS_COLS = ["cycle", "dia_precursor_cycle", "rt_values", "mobility_values", "mz_values",
             "tof_indptr", "push_indices", "intensity_values"]


def golden_selection_timstof():
    """CandidateSelection.__call__ on a small ion-mobility run (2-D tiles, find_peaks_2d); same FFT
    stand-in and caveats as golden_selection."""
    import ref_shim

    ref_shim.install_selection_glue()
    from alphadia.search.selection import selection as ref_sel
    from alphadia.search.selection.config_df import CandidateSelectionConfig

    case = syn.make_timstof_case(n_precursors=90, n_cycles=70, config_id=46, per_precursor=1,
                                 scan_max_index=96, planted_fraction=0.7, n_tof=24000, events_per_push=20.0)
    d = {"tims_" + c: getattr(case.dia, c) for c in TIMS_COLS}
    d["tims_scan_max_index"] = np.asarray(case.dia.scan_max_index)
    d["tims_zeroth_frame"] = np.asarray(case.dia.zeroth_frame)
    for c in FRAG_COLS:
        d["frag_" + c] = case.library.fragment_df[c].values
    for c in PREC_NUM_COLS:
        d["prec_" + c] = case.library.precursor_df[c].values
    d["caveat"] = np.asarray(CAVEAT)
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=2.0, mobility_tolerance=0.22, candidate_count=3, min_size_rt=2,
                    peak_len_rt=1.5, sigma_scale_rt=0.5, peak_len_mobility=0.06, sigma_scale_mobility=1.0,
                    max_size_mobility=20))
    dia = DuckTims(case.dia)
    dia.has_mobility = True
    cs = ref_sel.CandidateSelection(
        dia, case.library.precursor_df.copy(), case.library.fragment_df.copy(), cfg,
        rt_column="rt_library", mobility_column="mobility_library",
        precursor_mz_column="mz_library", fragment_mz_column="mz_library",
        fwhm_rt=cfg.peak_len_rt, fwhm_mobility=cfg.peak_len_mobility,
    )
    df = cs(thread_count=1)
    d["kernel"] = np.asarray(cs.kernel, dtype=np.float32)
    cj = cs.config_jit
    for k in ("rt_tolerance mobility_tolerance precursor_mz_tolerance fragment_mz_tolerance candidate_count "
              "top_k_precursors exclude_shared_ions kernel_size f_mobility f_rt center_fraction "
              "min_size_mobility min_size_rt max_size_mobility max_size_rt use_weighted_score "
              "join_close_candidates join_close_candidates_scan_threshold "
              "join_close_candidates_cycle_threshold sigma_scale_rt sigma_scale_mobility peak_len_rt "
              "peak_len_mobility").split():
        d[f"cfg_{k}"] = np.asarray(getattr(cj, k))
    for k in ("feature_mean", "feature_std", "feature_weight"):
        d[f"cfg_{k}"] = np.asarray(getattr(cj, k), dtype=np.float64)
    for c in ("precursor_idx rank score scan_center scan_start scan_stop frame_center frame_start "
              "frame_stop elution_group_idx decoy").split():
        d[f"out_{c}"] = df[c].values
    print(len(df), "candidates for", df["precursor_idx"].nunique(), "precursors; ranks", np.bincount(df["rank"].values),
          "kernel", cs.kernel.shape, "scan width", np.unique(df["scan_stop"] - df["scan_start"]))
    path = os.path.join(OUT_DIR, "selection_timstof.npz")
    np.savez_compressed(path, **d)
    print(path, f"{os.path.getsize(path)/1e6:.2f} MB")


def golden_timstof():
    """G2 + G4 for ion-mobility data: TimsTOFTransposeJIT.get_dense and full scoring."""
    case = syn.make_timstof_case(n_precursors=160, n_cycles=36)
    d = {"tims_" + c: getattr(case.dia, c) for c in TIMS_COLS}
    d["tims_scan_max_index"] = np.asarray(case.dia.scan_max_index)
    d["tims_zeroth_frame"] = np.asarray(case.dia.zeroth_frame)
    for c in FRAG_COLS:
        d["frag_" + c] = case.library.fragment_df[c].values
    for c in PREC_NUM_COLS:
        d["prec_" + c] = case.library.precursor_df[c].values
    for c in CAND_COLS:
        d["cand_" + c] = case.candidates_df[c].values

    # direct get_dense cases
    jit = timstof_to_jit(case.dia)
    rng = np.random.default_rng(17)
    L, S = case.dia.cycle_len, case.dia.scan_max_index
    n_cases = 16
    for i in range(n_cases):
        c0 = int(rng.integers(0, 20)); nc = int(rng.integers(3, 12))
        s0 = int(rng.integers(0, S - 24)); ns = int(rng.integers(4, 24))
        frame_limits = np.array([[c0 * L + 1, (c0 + nc) * L + 1, 1]], dtype=np.uint64)
        scan_limits = np.array([[s0, s0 + ns, 1]], dtype=np.uint64)
        k = int(rng.integers(2, 10))
        if i % 3 == 0:
            mzq = np.sort(rng.uniform(400, 480, k)).astype(np.float32)
            quad = np.array([[-1.0, -1.0]])
        else:
            mzq = np.sort(rng.uniform(200, 350, k)).astype(np.float32)
            lo = rng.uniform(400, 470)
            quad = np.array([[lo, lo + rng.uniform(1.0, 25.0)]], dtype=np.float32)
        tol = np.float32(30 if i % 2 else 80)
        dense, pidx = jit.get_dense(frame_limits, scan_limits, mzq, tol, quad, absolute_masses=True)
        d[f"q{i}_frame_limits"] = frame_limits
        d[f"q{i}_scan_limits"] = scan_limits
        d[f"q{i}_mz"] = mzq
        d[f"q{i}_tol"] = np.asarray(tol)
        d[f"q{i}_quad"] = np.asarray(quad, dtype=np.float64)
        d[f"q{i}_dense"] = dense
        d[f"q{i}_pidx"] = np.asarray(pidx, dtype=np.int64)
    d["n_cases"] = np.asarray(n_cases)

    # full scoring (handler defaults)
    cfg = CandidateScoringConfig()
    cfg.update(SCORING_CONFIGS["handler_default"])
    dia = DuckTims(case.dia)
    cs = ref_scoring.CandidateScoring(
        dia_data=dia,
        precursors_flat=case.library.precursor_df.copy(),
        fragments_flat=case.library.fragment_df.copy(),
        rt_column="rt_library", mobility_column="mobility_library",
        precursor_mz_column="mz_library", fragment_mz_column="mz_library", config=cfg,
    )
    cands = case.candidates_df.copy()
    fragment_container = cs.assemble_fragments()
    sgc = cs.assemble_score_group_container(cands)
    out = OutputPsmDF(sgc.get_candidate_count(), cs.config.top_k_fragments)
    ref_scoring._process_score_groups(range(len(sgc)), sgc, out, fragment_container, dia.to_jitclass(),
                                      cs.config.to_jitclass(), cs.quadrupole_calibration.jit, False)
    d.update(out_to_dict(out))
    cfgj = cfg.to_jitclass()
    for kk in ("collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
               "reference_channel quant_window quant_all precursor_mz_tolerance "
               "fragment_mz_tolerance experimental_xic").split():
        d["cfg_" + kk] = np.asarray(getattr(cfgj, kk))
    d["caveat"] = np.asarray(CAVEAT)
    path = os.path.join(OUT_DIR, "scoring_timstof.npz")
    np.savez_compressed(path, **d)
    v = np.asarray(out.valid)
    print(f"{path}: {v.sum()}/{len(v)} valid, {os.path.getsize(path)/1e6:.2f} MB, "
          f"mean f29 {np.nanmean(out.features[v][:, 29]):.3f}")


# --------------------------------------------------------------------------- general cycles
# Cycles that the touching windows of syn.make_cycle cannot express: overlapping and staggered windows, several MS1
# rows per cycle (also none at row 0), a stretch of m/z no window covers.  Runs are sized so that a fixture stays
# below 1 MiB: more cycle rows, fewer noise peaks per row.
# The config_ids (seeds) are chosen so that no row of a fixture sits on a knife edge of the shim: NumPy's exp differs
# from libm's in the last bit for one argument in twenty, which now and then moves a float32 mass error by an ulp; a
# tie of two observation importances (quant_all off) or of two candidate scores is broken by the summation order.  With
# such a row the Numba-typed and the NumPy-typed restatement cannot both equal the fixture.
CYCLE_GEOMETRIES = {
    "staggered": dict(cycle=lambda: syn.make_staggered_cycle(400.0, 480.0, 10.0), config_id=141, ms1_peaks=400, ms2_peaks=70),
    "multi_ms1": dict(cycle=lambda: syn.make_multi_ms1_cycle(8, 400.0, 480.0, ms1_first=True), config_id=142,
                      ms1_peaks=300, ms2_peaks=110),
    "multi_ms1_twin": dict(cycle=lambda: syn.make_multi_ms1_cycle(8, 400.0, 480.0, ms1_first=False), config_id=153,
                           ms1_peaks=300, ms2_peaks=110, n_precursors=200),
    "dense_overlap": dict(cycle=lambda: syn.make_dense_overlap_cycle(400.0, 480.0), config_id=154, ms1_peaks=200,
                          ms2_peaks=28),
    # both at once, for candidate selection: two rows in each of its groups of cycle rows
    "staggered_multi_ms1": dict(cycle=lambda: staggered_multi_ms1_cycle(), config_id=148, ms1_peaks=150, ms2_peaks=35,
                                amplitude=0.5),
}
# fixture -> (geometry, scoring settings, extra arguments of small_case)
CYCLE_SCORING = {
    "staggered": ("staggered", SCORING_CONFIGS["handler_default"], {}),
    "multi_ms1": ("multi_ms1", SCORING_CONFIGS["handler_default"], {}),
    "multi_ms1_twin": ("multi_ms1_twin", SCORING_CONFIGS["handler_default"], {}),
    "dense_overlap": ("dense_overlap", SCORING_CONFIGS["handler_default"], {}),
    "dense_overlap_class": ("dense_overlap", SCORING_CONFIGS["class_default"], {}),
    "multi_ms1_manyfrag": ("multi_ms1", MANYFRAG_CONFIGS["manyfrag"],
                           dict(config_id=145, n_precursors=140, k_fragments=(5, 40), frag_mz_hi=500, ms2_mz_range=(195, 505))),
}


def staggered_multi_ms1_cycle() -> np.ndarray:
    """The staggered windows with a second MS1 row in the middle of the cycle."""
    rows = syn.make_staggered_cycle(400.0, 480.0, 10.0)[0, :, 0, :]
    half = 1 + (len(rows) - 1) // 2
    return syn.cycle_from_rows(np.concatenate([rows[:half], [[-1.0, -1.0]], rows[half:]]))


def geometry_case(geometry: str, **kw) -> syn.SyntheticCase:
    args = dict(CYCLE_GEOMETRIES[geometry])
    args["cycle"] = args["cycle"]()
    args.update(kw)
    return small_case(**args)


def run_scoring_tolerant(case, cfg_updates):
    """run_scoring, one score group at a time: a candidate whose precursor range no window overlaps makes the
    reference raise (quadrupole_transfer_function_single on an empty observation list); such a row stays
    ``valid = False`` in the output and is listed in ``raised``."""
    cfg = CandidateScoringConfig()
    cfg.update(cfg_updates)
    dia = DuckDia(case.dia)
    cs = ref_scoring.CandidateScoring(
        dia_data=dia, precursors_flat=case.library.precursor_df.copy(), fragments_flat=case.library.fragment_df.copy(),
        rt_column="rt_library", mobility_column="mobility_library", precursor_mz_column="mz_library",
        fragment_mz_column="mz_library", config=cfg,
    )
    cands = case.candidates_df.copy()
    fragment_container = cs.assemble_fragments()
    sgc = cs.assemble_score_group_container(cands)
    out = OutputPsmDF(sgc.get_candidate_count(), cs.config.top_k_fragments)
    raised = []
    for g in range(len(sgc)):
        try:
            ref_scoring._process_score_groups(range(g, g + 1), sgc, out, fragment_container, dia.to_jitclass(),
                                              cs.config.to_jitclass(), cs.quadrupole_calibration.jit, False)
        except Exception as e:  # noqa: BLE001
            raised.append((g, type(e).__name__))
    opidx = np.array([c.precursor_idx for sg in sgc.score_groups for c in sg.candidates], dtype=np.uint32)
    orank = np.array([c.rank for sg in sgc.score_groups for c in sg.candidates], dtype=np.uint8)
    return out, opidx, orank, cs.config, raised


def n_windows_of(case, top_k_isotopes: int) -> np.ndarray:
    """Cycle rows the quadrupole range of every candidate overlaps (candidate.py:151-163,203-205 with
    alpharaw_jit.py:46-48), in candidate order."""
    pdf = case.library.precursor_df.set_index("precursor_idx")
    mz = pdf.loc[case.candidates_df["precursor_idx"].values, "mz_library"].values.astype(np.float32)
    ch = pdf.loc[case.candidates_df["precursor_idx"].values, "charge"].values.astype(np.float64)
    iso = (np.arange(min(int(top_k_isotopes), 4))[None, :] * 1.0033548350700006 / ch[:, None]).astype(np.float32) + mz[:, None]
    lo = (iso.min(axis=1) - 0.5).astype(np.float32)
    hi = (iso.max(axis=1) + 0.5).astype(np.float32)
    flat = case.dia.cycle.reshape(-1, 2)
    return ((lo[:, None] <= flat[None, :, 1]) & (hi[:, None] >= flat[None, :, 0])).sum(axis=1)


def golden_scoring_cycles(which=None):
    for name, (geometry, upd, kw) in CYCLE_SCORING.items():
        if which is not None and name not in which:
            continue
        case = geometry_case(geometry, **kw)
        out, opidx, orank, cfg, raised = run_scoring_tolerant(case, upd)
        d = case_to_dict(case)
        od = out_to_dict(out)
        lens = (case.library.precursor_df["flat_frag_stop_idx"].values.astype(np.int64)
                - case.library.precursor_df["flat_frag_start_idx"].values.astype(np.int64))
        width = int(min(int(cfg.top_k_fragments), lens.max()))
        for k, v in od.items():
            if v.ndim == 2 and k != "out_features" and v.shape[1] > width:
                assert not v[:, width:].any(), k
                od[k] = np.ascontiguousarray(v[:, :width])
        d.update(od)
        d["order_precursor_idx"] = opidx
        d["order_rank"] = orank
        d["raised_groups"] = np.array([g for g, _ in raised], dtype=np.int64)
        cfgj = cfg.to_jitclass()
        for k in (
            "collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
            "reference_channel quant_window quant_all precursor_mz_tolerance "
            "fragment_mz_tolerance experimental_xic"
        ).split():
            d["cfg_" + k] = np.asarray(getattr(cfgj, k))
        d["caveat"] = np.asarray(CAVEAT)
        # ---- what the fixture is for
        v = np.asarray(out.valid).astype(bool)
        nobs = np.asarray(out.features)[v][:, 17]
        nwin = n_windows_of(case, cfg.top_k_isotopes)
        n_ms1 = len(syn.ms1_rows_of(case.dia.cycle))
        hist = {int(o): int((nobs == o).sum()) for o in np.unique(nobs)}
        if geometry == "staggered":
            assert hist.get(2, 0) >= 20 and hist.get(3, 0) >= 20 and set(hist) <= {2, 3}, hist
        if geometry.startswith("multi_ms1"):
            assert n_ms1 == 2 and hist.get(1, 0) >= 20, (n_ms1, hist)
        if geometry == "dense_overlap":
            assert n_ms1 == 3 and hist.get(3, 0) >= 20 and sum(c for o, c in hist.items() if o >= 4) >= 20, hist
            assert (nwin == 0).sum() >= 1, "no candidate outside every window"
        # the reference raises on the candidates no window overlaps, and only on them (those with three fragments or
        # fewer leave before): such rows stay valid = False
        key_in = case.candidates_df["precursor_idx"].values.astype(np.int64) * 256 + case.candidates_df["rank"].values
        key_out = opidx.astype(np.int64) * 256 + orank
        outside = np.isin(key_out, key_in[nwin == 0])
        assert outside[[g for g, _ in raised]].all() and not np.asarray(out.valid)[outside].any(), raised
        assert len(raised) >= 1 or geometry != "dense_overlap"
        d["cand_n_windows"] = nwin.astype(np.int64)
        path = os.path.join(OUT_DIR, f"scoring_{name}.npz")
        np.savez_compressed(path, **d)
        print(f"{path}: {v.sum()}/{len(v)} valid, n_observations {hist}, MS1 rows {n_ms1}, windows==0: {(nwin == 0).sum()}, "
              f"raised {raised[:3]}{'...' if len(raised) > 3 else ''} ({len(raised)}), {os.path.getsize(path)/2**20:.2f} MiB")


def golden_get_dense_cycles():
    """AlphaRawJIT.get_dense on the general cycles: per geometry a small run and, alternating, fragment queries
    (quadrupole ranges as wide as a precursor's isotope range +- 0.5) and MS1 queries (quadrupole (-1, -1))."""
    d = {"caveat": np.asarray(CAVEAT)}
    names = ["staggered", "multi_ms1", "multi_ms1_twin", "dense_overlap"]
    d["geometries"] = np.array(names, dtype="U")
    n_cases = 10
    frag_lens, ms1_lens = [], []
    for gi, name in enumerate(names):
        case = geometry_case(name, n_precursors=40, n_cycles=30, ms1_peaks=120, ms2_peaks=30, config_id=150 + gi)
        jit = to_jit(case.dia)
        rng = np.random.default_rng(31 + gi)
        L = case.dia.cycle_len
        for k, v in dia_to_dict(case.dia).items():
            d[f"{name}_{k}"] = v
        for i in range(n_cases):
            c0 = int(rng.integers(0, 14))
            nc = int(rng.integers(1, 16))
            frame_limits = np.array([[c0 * L, (c0 + nc) * L, 1]], dtype=np.uint64)
            k = int(rng.integers(2, 13))
            if i % 2 == 1:
                mzq = np.sort(rng.uniform(400, 480, k)).astype(np.float32)
                quad = np.array([[-1.0, -1.0]])
                tol = np.float32(10)
            else:
                mzq = np.sort(rng.uniform(200, 350, k)).astype(np.float32)
                lo = 441.0 if (name == "dense_overlap" and i == 0) else rng.uniform(399, 478)  # (441..442.5: no window)
                quad = np.array([[lo, lo + (1.5 if i == 0 else rng.uniform(1.5, 2.6))]], dtype=np.float32)
                tol = np.float32(15)
            if i % 5 == 4:  # the real m/z of peaks, so that windows are hit for sure
                rows = jit.get_dense(frame_limits, np.array([[0, 1, 1]], dtype=np.uint64), mzq, tol, quad, absolute_masses=True)[1]
                if len(rows):
                    sp = int(rows[0]) + c0 * L
                    a, b = case.dia.peak_start_idx_list[sp], case.dia.peak_stop_idx_list[sp]
                    mzq = np.sort(rng.choice(case.dia.mz_values[a:b], size=min(k, b - a), replace=False)).astype(np.float32)
            dense, pidx = jit.get_dense(frame_limits, np.array([[0, 1, 1]], dtype=np.uint64), mzq, tol, quad,
                                        absolute_masses=True)
            (ms1_lens if i % 2 == 1 else frag_lens).append(len(pidx))
            q = f"{name}_q{i}_"
            d[q + "frame_limits"] = frame_limits
            d[q + "mz"] = mzq
            d[q + "tol"] = np.asarray(tol)
            d[q + "quad"] = np.asarray(quad, dtype=np.float64)
            d[q + "dense"] = dense
            d[q + "pidx"] = np.asarray(pidx, dtype=np.int64)
    d["n_cases"] = np.asarray(n_cases)
    # what the fixture is for: MS1 lists of 2 and 3 rows, fragment lists of 0, 2, 3 and 4 or more rows
    assert {2, 3} <= set(ms1_lens) and {0, 2, 3} <= set(frag_lens) and max(frag_lens) >= 4, (ms1_lens, frag_lens)
    path = os.path.join(OUT_DIR, "get_dense_cycles.npz")
    np.savez_compressed(path, **d)
    print(path, "MS1 lists", sorted(set(ms1_lens)), "fragment lists", sorted(set(frag_lens)), f"{os.path.getsize(path)/2**20:.2f} MiB")


def golden_get_dense_mz_edges():
    """AlphaRawJIT.get_dense(absolute_masses=True) and TimsTOFTransposeJIT.get_dense on the designed-edge runs of
    tests/mz_edges.py: peaks on the float32 bounds of the tolerance windows, on the edges of the transposed run's m/z
    bins, on powers of two and on the ends of the run; TOF bins on the bounds and on the edges of the lookup buckets.
    The runs' arrays, the queries and the dense outputs.  (The shim keeps ``float32 > 1e-26`` and ``float32 + 1e-36``
    in float32 where Numba computes them in float64: float32(1e-26) lies below 1e-26, so the cut falls between the
    same two float32 values either way, and in the E7 cells 1e-36 is the whole sum (intensity zeroed), or below half
    an ulp of both sums in both types, or - intensity 1e-30 - moves the quotient alike: the oracle, which follows
    Numba's typing, reproduces every cell bit for bit, tests/test_mz_edges.py.)"""
    import mz_edges

    d = {"caveat": np.asarray(CAVEAT)}
    scan = np.array([[0, 1, 1]], dtype=np.uint64)
    hits = 0
    for run in mz_edges.RUNS:
        dia, cases = mz_edges.build_alpharaw(0, run)
        jit = to_jit(dia)
        for k, v in dia_to_dict(dia).items():
            d[f"{run}_{k}"] = v
        d[f"{run}_cases"] = np.array([c.name for c in cases], dtype="U")
        for c in cases:
            dense, pidx = jit.get_dense(c.frame_limits, scan, c.mz_query, c.tol, c.quad, absolute_masses=True)
            q = f"{run}_{c.name}_"
            d[q + "frame_limits"] = c.frame_limits
            d[q + "mz"] = c.mz_query
            d[q + "tol"] = np.asarray(c.tol)
            d[q + "quad"] = c.quad
            d[q + "dense"] = dense
            d[q + "pidx"] = np.asarray(pidx, dtype=np.int64)
            hits += int((dense[0] > 0).sum())
    dia, cases = mz_edges.build_timstof(0)
    jit = timstof_to_jit(dia)
    for c in TIMS_COLS:
        d["tims_" + c] = getattr(dia, c)
    d["tims_scan_max_index"] = np.asarray(dia.scan_max_index)
    d["tims_zeroth_frame"] = np.asarray(dia.zeroth_frame)
    d["tims_cases"] = np.array([c.name for c in cases], dtype="U")
    for c in cases:
        dense, pidx = jit.get_dense(c.frame_limits, c.scan_limits, c.mz_query, c.tol, c.quad, absolute_masses=True)
        q = f"tims_{c.name}_"
        d[q + "frame_limits"] = c.frame_limits
        d[q + "scan_limits"] = c.scan_limits
        d[q + "mz"] = c.mz_query
        d[q + "tol"] = np.asarray(c.tol)
        d[q + "quad"] = c.quad
        d[q + "dense"] = dense
        d[q + "pidx"] = np.asarray(pidx, dtype=np.int64)
        hits += int((dense[0] > 0).sum())
    path = os.path.join(OUT_DIR, "get_dense_mz_edges.npz")
    np.savez_compressed(path, **d)
    print(path, hits, "cells hit", f"{os.path.getsize(path)/2**20:.2f} MiB")


def golden_selection_cycles():
    """CandidateSelection.__call__ (as golden_selection, same FFT stand-in) on staggered windows with two MS1 rows:
    every precursor sums two or three fragment rows and two MS1 rows per cycle."""
    import ref_shim

    ref_shim.install_selection_glue()
    from alphadia.search.selection import selection as ref_sel
    from alphadia.search.selection.config_df import CandidateSelectionConfig

    case = geometry_case("staggered_multi_ms1", n_precursors=200, n_cycles=100, per_precursor=1, planted_fraction=0.7)
    d = case_to_dict(case)
    d["caveat"] = np.asarray(CAVEAT)
    name = "cycles"
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=30.0, candidate_count=3, min_size_rt=3))
    dia = DuckDia(case.dia)
    cs = ref_sel.CandidateSelection(
        dia, case.library.precursor_df.copy(), case.library.fragment_df.copy(), cfg,
        rt_column="rt_library", mobility_column="mobility_library",
        precursor_mz_column="mz_library", fragment_mz_column="mz_library",
        fwhm_rt=cfg.peak_len_rt, fwhm_mobility=cfg.peak_len_mobility,
    )
    df = cs(thread_count=1)
    d[f"{name}_kernel"] = np.asarray(cs.kernel, dtype=np.float32)
    cj = cs.config_jit
    for k in ("rt_tolerance precursor_mz_tolerance fragment_mz_tolerance candidate_count "
              "top_k_precursors exclude_shared_ions kernel_size f_mobility f_rt center_fraction "
              "min_size_mobility min_size_rt max_size_mobility max_size_rt use_weighted_score "
              "join_close_candidates join_close_candidates_scan_threshold "
              "join_close_candidates_cycle_threshold").split():
        d[f"{name}_cfg_{k}"] = np.asarray(getattr(cj, k))
    for k in ("feature_mean", "feature_std", "feature_weight"):
        d[f"{name}_cfg_{k}"] = np.asarray(getattr(cj, k), dtype=np.float64)
    for c in ("precursor_idx rank score scan_center scan_start scan_stop frame_center frame_start "
              "frame_stop elution_group_idx decoy").split():
        d[f"{name}_out_{c}"] = df[c].values
    assert len(syn.ms1_rows_of(case.dia.cycle)) == 2 and len(df) > 300
    path = os.path.join(OUT_DIR, "selection_cycles.npz")
    np.savez_compressed(path, **d)
    print(path, len(df), "candidates for", df["precursor_idx"].nunique(), "precursors; ranks", np.bincount(df["rank"].values),
          f"{os.path.getsize(path)/2**20:.2f} MiB")


SELECTION_CFG_KEYS = ("rt_tolerance precursor_mz_tolerance fragment_mz_tolerance candidate_count "
                      "top_k_precursors exclude_shared_ions kernel_size f_mobility f_rt center_fraction "
                      "min_size_mobility min_size_rt max_size_mobility max_size_rt use_weighted_score "
                      "join_close_candidates join_close_candidates_scan_threshold "
                      "join_close_candidates_cycle_threshold").split()
SELECTION_CFG_KEYS_IM = SELECTION_CFG_KEYS + ("mobility_tolerance sigma_scale_rt sigma_scale_mobility peak_len_rt "
                                              "peak_len_mobility").split()
SELECTION_OUT_COLS = ("precursor_idx rank score scan_center scan_start scan_stop frame_center frame_start "
                      "frame_stop elution_group_idx decoy").split()


def _run_reference_selection(d, name, dia, library, updates, cfg_keys):
    """CandidateSelection.__call__ of the reference with `updates` on its default config; kernel, config fields and
    output columns go to d under `name`_kernel / `name`_cfg_* / `name`_out_*.  -> the candidate table."""
    from alphadia.search.selection import selection as ref_sel
    from alphadia.search.selection.config_df import CandidateSelectionConfig

    cfg = CandidateSelectionConfig()
    cfg.update(updates)
    cs = ref_sel.CandidateSelection(
        dia, library.precursor_df.copy(), library.fragment_df.copy(), cfg,
        rt_column="rt_library", mobility_column="mobility_library",
        precursor_mz_column="mz_library", fragment_mz_column="mz_library",
        fwhm_rt=cfg.peak_len_rt, fwhm_mobility=cfg.peak_len_mobility,
    )
    df = cs(thread_count=1)
    d[f"{name}_kernel"] = np.asarray(cs.kernel, dtype=np.float32)
    cj = cs.config_jit
    for k in cfg_keys:
        d[f"{name}_cfg_{k}"] = np.asarray(getattr(cj, k))
    for k in ("feature_mean", "feature_std", "feature_weight"):
        d[f"{name}_cfg_{k}"] = np.asarray(getattr(cj, k), dtype=np.float64)
    for c in SELECTION_OUT_COLS:
        d[f"{name}_out_{c}"] = df[c].values
    return df


def share_fragments(library, fraction: float, seed: int) -> None:
    """Cardinality 2 for that share of the fragments (exclude_shared_ions drops them), from a stream of its own."""
    card = library.fragment_df["cardinality"].values.copy()
    card[np.random.default_rng([seed, 23]).random(card.size) < fraction] = 2
    library.fragment_df["cardinality"] = card


# candidate selection at the limits of the selection kernels (tests/test_selection_limits_gpu.py): libraries of 4 ... 60
# fragments per precursor (the reference takes every fragment of the slice, selection.py:120-137), a fifth of them
# shared, up to 16 candidates per precursor, a smoothing kernel of 16 cycles
# (tolerances of 50 ppm on a narrow m/z range: no tile has a stretch of cycles without any signal, in which only the
# noise of the reference's float32 FFT would make peaks - equal scores, ordered by an unstable sort)
SELECTION_LIMITS = {
    # every precursor's tile is the whole run: far more than 16 peaks compete for the 16 ranks
    "many": dict(rt_tolerance=500.0, candidate_count=16, top_k_precursors=4, exclude_shared_ions=True, min_size_rt=2,
                 join_close_candidates=False, precursor_mz_tolerance=50.0, fragment_mz_tolerance=50.0),
    "k16": dict(rt_tolerance=40.0, kernel_size=16, candidate_count=8, top_k_precursors=1, min_size_rt=2,
                join_close_candidates=True, precursor_mz_tolerance=50.0, fragment_mz_tolerance=50.0),
}


def selection_limits_case() -> syn.SyntheticCase:
    case = small_case(129, n_precursors=120, n_cycles=260, per_precursor=1, n_ms2=4, ms1_peaks=110, ms2_peaks=55,
                      frag_mz_hi=260, ms2_mz_range=(195, 265), planted_fraction=0.7, amplitude=0.3,
                      few_fragment_fraction=0.0, k_fragments=(4, 60))
    share_fragments(case.library, 0.2, 129)
    return case


def golden_selection_limits():
    """CandidateSelection.__call__ (as golden_selection, same FFT stand-in) on a run of 260 cycles with 4 ... 60
    fragments per precursor, the settings of SELECTION_LIMITS."""
    import ref_shim

    ref_shim.install_selection_glue()
    case = selection_limits_case()
    d = case_to_dict(case)
    d["caveat"] = np.asarray(CAVEAT)
    for name, upd in SELECTION_LIMITS.items():
        df = _run_reference_selection(d, name, DuckDia(case.dia), case.library, upd, SELECTION_CFG_KEYS)
        per = df.groupby("precursor_idx").size()
        print(name, len(df), "candidates for", len(per), "precursors;", int((per == upd["candidate_count"]).sum()),
              "with every rank filled")
        assert len(df) > 300
    n_frag = (case.library.precursor_df.flat_frag_stop_idx - case.library.precursor_df.flat_frag_start_idx).values
    assert n_frag.min() == 4 and n_frag.max() == 60 and (n_frag > 16).sum() > 60
    path = os.path.join(OUT_DIR, "selection_limits.npz")
    np.savez_compressed(path, **d)
    print(path, f"{os.path.getsize(path)/2**20:.2f} MiB")


# ion mobility: 4 ... 60 fragments and 4 isotopes give 8 ... 64 m/z windows per precursor.  A coarse TOF axis (1 200
# bins) and windows of +-300 ppm: every tile (the whole scan range, 32 cycles) is full enough that no stretch of it is
# without signal (see SELECTION_LIMITS).  "wide": fragment windows of +-800 ppm, with which about half the precursors
# queue more events in one window than its sort list takes (512), and the other half do not
_TIMSTOF_LIMITS = dict(rt_tolerance=3.0, mobility_tolerance=0.6, candidate_count=16, top_k_precursors=4, min_size_rt=2,
                       peak_len_rt=1.2, sigma_scale_rt=0.5, peak_len_mobility=0.05, sigma_scale_mobility=1.0,
                       max_size_mobility=20, precursor_mz_tolerance=300.0, fragment_mz_tolerance=300.0)
SELECTION_TIMSTOF_LIMITS = {
    "many": dict(_TIMSTOF_LIMITS, join_close_candidates=False),
    "wide": dict(_TIMSTOF_LIMITS, fragment_mz_tolerance=800.0),
}


def selection_timstof_limits_case() -> syn.TimsTOFCase:
    return syn.make_timstof_case(n_precursors=60, n_cycles=34, config_id=132, per_precursor=1, n_ms2_frames=3,
                                 windows_per_frame=2, scan_max_index=64, planted_fraction=0.4, n_tof=1200,
                                 events_per_push=17.0, k_fragments=(4, 60))


def golden_selection_timstof_limits():
    """CandidateSelection.__call__ on a small ion-mobility run (as golden_selection_timstof) with 4 ... 60 fragments
    per precursor, the settings of SELECTION_TIMSTOF_LIMITS."""
    import ref_shim

    ref_shim.install_selection_glue()
    case = selection_timstof_limits_case()
    d = {"tims_" + c: getattr(case.dia, c) for c in TIMS_COLS}
    d["tims_scan_max_index"] = np.asarray(case.dia.scan_max_index)
    d["tims_zeroth_frame"] = np.asarray(case.dia.zeroth_frame)
    for c in FRAG_COLS:
        d["frag_" + c] = case.library.fragment_df[c].values
    for c in PREC_NUM_COLS:
        d["prec_" + c] = case.library.precursor_df[c].values
    d["caveat"] = np.asarray(CAVEAT)
    for name, upd in SELECTION_TIMSTOF_LIMITS.items():
        dia = DuckTims(case.dia)
        dia.has_mobility = True
        df = _run_reference_selection(d, name, dia, case.library, upd, SELECTION_CFG_KEYS_IM)
        per = df.groupby("precursor_idx").size()
        print(name, len(df), "candidates for", len(per), "precursors; per precursor", np.bincount(per.values),
              "kernel", d[f"{name}_kernel"].shape)
        assert len(df) > 150
    n_frag = (case.library.precursor_df.flat_frag_stop_idx - case.library.precursor_df.flat_frag_start_idx).values
    assert n_frag.min() == 4 and n_frag.max() == 60 and (n_frag > 28).sum() >= 20  # (W = 8 ... 64 with four isotopes)
    path = os.path.join(OUT_DIR, "selection_timstof_limits.npz")
    np.savez_compressed(path, **d)
    print(path, f"{os.path.getsize(path)/2**20:.2f} MiB")


def golden_timstof_cycles():
    """Full scoring (handler defaults) on an ion-mobility run with two MS1 frames per cycle and every MS2 frame
    three times per cycle: two unfragmented observations, three and more fragment observations per candidate."""
    S = 64
    cycle = syn.make_timstof_cycle(3, 2, S, 400.0, 480.0, n_ms1_frames=2, repeats=3)
    case = syn.make_timstof_case(n_precursors=90, n_cycles=30, config_id=49, scan_max_index=S, n_tof=24000,
                                 events_per_push=6.0, candidates_on_window=True, cycle=cycle)
    d = {"tims_" + c: getattr(case.dia, c) for c in TIMS_COLS}
    d["tims_scan_max_index"] = np.asarray(case.dia.scan_max_index)
    d["tims_zeroth_frame"] = np.asarray(case.dia.zeroth_frame)
    for c in FRAG_COLS:
        d["frag_" + c] = case.library.fragment_df[c].values
    for c in PREC_NUM_COLS:
        d["prec_" + c] = case.library.precursor_df[c].values
    for c in CAND_COLS:
        d["cand_" + c] = case.candidates_df[c].values
    cfg = CandidateScoringConfig()
    cfg.update(SCORING_CONFIGS["handler_default"])
    dia = DuckTims(case.dia)
    cs = ref_scoring.CandidateScoring(
        dia_data=dia, precursors_flat=case.library.precursor_df.copy(), fragments_flat=case.library.fragment_df.copy(),
        rt_column="rt_library", mobility_column="mobility_library", precursor_mz_column="mz_library",
        fragment_mz_column="mz_library", config=cfg,
    )
    cands = case.candidates_df.copy()
    fragment_container = cs.assemble_fragments()
    sgc = cs.assemble_score_group_container(cands)
    out = OutputPsmDF(sgc.get_candidate_count(), cs.config.top_k_fragments)
    ref_scoring._process_score_groups(range(len(sgc)), sgc, out, fragment_container, dia.to_jitclass(),
                                      cs.config.to_jitclass(), cs.quadrupole_calibration.jit, False)
    d.update(out_to_dict(out))
    cfgj = cfg.to_jitclass()
    for kk in ("collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
               "reference_channel quant_window quant_all precursor_mz_tolerance "
               "fragment_mz_tolerance experimental_xic").split():
        d["cfg_" + kk] = np.asarray(getattr(cfgj, kk))
    d["caveat"] = np.asarray(CAVEAT)
    v = np.asarray(out.valid).astype(bool)
    nobs = np.asarray(out.features)[v][:, 17]
    hist = {int(o): int((nobs == o).sum()) for o in np.unique(nobs)}
    assert sum(c for o, c in hist.items() if o >= 3) >= 20 and v.sum() >= 40, hist
    path = os.path.join(OUT_DIR, "scoring_timstof_cycles.npz")
    np.savez_compressed(path, **d)
    print(f"{path}: {v.sum()}/{len(v)} valid, n_observations {hist}, {os.path.getsize(path)/2**20:.2f} MiB")


def golden_boxes_timstof():
    """Full scoring (the settings of tests/box_sweep_im.py) of the thinned ion-mobility shape sweep: boxes of 2 ... 36
    cycles x 2 ... 48 scans at every edge of the run, centres on the first, middle and last cycle / scan, one to four
    observations (box_sweep_im.golden_spec, cycle "mixed").  The path of golden_timstof()."""
    import box_sweep_im as bi

    case = bi.sweep_case(golden=True)
    d = {"tims_" + c: getattr(case.dia, c) for c in TIMS_COLS}
    d["tims_scan_max_index"] = np.asarray(case.dia.scan_max_index)
    d["tims_zeroth_frame"] = np.asarray(case.dia.zeroth_frame)
    for c in FRAG_COLS:
        d["frag_" + c] = case.library.fragment_df[c].values
    for c in PREC_NUM_COLS:
        d["prec_" + c] = case.library.precursor_df[c].values
    for c in CAND_COLS:
        d["cand_" + c] = case.candidates_df[c].values
    cfg = CandidateScoringConfig()
    cfg.update(bi.HANDLER)
    dia = DuckTims(case.dia)
    cs = ref_scoring.CandidateScoring(
        dia_data=dia, precursors_flat=case.library.precursor_df.copy(), fragments_flat=case.library.fragment_df.copy(),
        rt_column="rt_library", mobility_column="mobility_library", precursor_mz_column="mz_library",
        fragment_mz_column="mz_library", config=cfg,
    )
    cands = case.candidates_df.copy()
    fragment_container = cs.assemble_fragments()
    sgc = cs.assemble_score_group_container(cands)
    out = OutputPsmDF(sgc.get_candidate_count(), cs.config.top_k_fragments)
    ref_scoring._process_score_groups(range(len(sgc)), sgc, out, fragment_container, dia.to_jitclass(),
                                      cs.config.to_jitclass(), cs.quadrupole_calibration.jit, False)
    d.update(out_to_dict(out))
    cfgj = cfg.to_jitclass()
    for kk in ("collect_fragments score_grouped exclude_shared_ions top_k_fragments top_k_isotopes "
               "reference_channel quant_window quant_all precursor_mz_tolerance "
               "fragment_mz_tolerance experimental_xic").split():
        d["cfg_" + kk] = np.asarray(getattr(cfgj, kk))
    d["caveat"] = np.asarray(CAVEAT)
    v = np.asarray(out.valid).astype(bool)
    nobs = np.asarray(out.features)[v][:, 17]
    path = os.path.join(OUT_DIR, "scoring_boxes_timstof.npz")
    np.savez_compressed(path, **d)
    print(f"{path}: {v.sum()}/{len(v)} valid, n_observations {dict(zip(*np.unique(nobs, return_counts=True)))}, "
          f"{os.path.getsize(path)/2**20:.2f} MiB")


if __name__ == "__main__":
    if "--mz-edges-only" in sys.argv:
        golden_get_dense_mz_edges()
        sys.exit(0)
    if "--boxes-timstof-only" in sys.argv:
        golden_boxes_timstof()
        sys.exit(0)
    if "--timstof-only" in sys.argv:
        golden_timstof()
        sys.exit(0)
    if "--selection-timstof-only" in sys.argv:
        golden_selection_timstof()
        sys.exit(0)
    if "--selection-kats-only" in sys.argv:
        golden_selection_kats()
        sys.exit(0)
    if "--transpose-only" in sys.argv:
        golden_transpose()
        sys.exit(0)
    if "--selection-only" in sys.argv:
        golden_selection()
        sys.exit(0)
    if "--selection-limits-only" in sys.argv:
        golden_selection_limits()
        sys.exit(0)
    if "--selection-timstof-limits-only" in sys.argv:
        golden_selection_timstof_limits()
        sys.exit(0)
    if "--small-only" in sys.argv:
        golden_get_dense()
        golden_fragcomp()
        golden_timstof()
        sys.exit(0)
    if "--edges-only" in sys.argv:
        golden_edges()
        sys.exit(0)
    if "--boxes-only" in sys.argv:
        golden_boxes()
        sys.exit(0)
    if "--multiplex-only" in sys.argv:
        golden_multiplex()
        sys.exit(0)
    if "--staging-only" in sys.argv:
        golden_staging()
        sys.exit(0)
    if "--host-helpers-only" in sys.argv:
        golden_host_helpers()
        sys.exit(0)
    if "--cycles-only" in sys.argv:  # optionally followed by the fixtures to make
        rest = [a for a in sys.argv[sys.argv.index("--cycles-only") + 1:] if not a.startswith("--") and a != OUT_DIR]
        scoring = [a for a in rest if a in CYCLE_SCORING]
        if not rest or scoring:
            golden_scoring_cycles(which=scoring or None)
        if not rest or "get_dense" in rest:
            golden_get_dense_cycles()
        if not rest or "selection" in rest:
            golden_selection_cycles()
        if not rest or "timstof" in rest:
            golden_timstof_cycles()
        sys.exit(0)
    if "--manyfrag-only" in sys.argv:
        golden_scoring(which=MANYFRAG_CONFIGS)
        sys.exit(0)
    golden_get_dense()
    golden_fragcomp()
    golden_scoring()
    golden_multiplex()
    golden_host_helpers()
    golden_staging()
    golden_edges()
    golden_boxes()
    golden_selection()
    golden_selection_kats()
    golden_selection_timstof()
    golden_transpose()
    golden_timstof()
    golden_scoring_cycles()
    golden_get_dense_cycles()
    golden_selection_cycles()
    golden_timstof_cycles()
    golden_boxes_timstof()
    golden_selection_limits()
    golden_selection_timstof_limits()
    golden_get_dense_mz_edges()
