"""The candidate library of transfer-library requantification built in HBM (``adh_stage_candidate_library``) against
the NumPy restatement byte for byte, calibrated against ``stage_fragments_calibrated`` bit for bit, its refusals, and
``HipTransferLibraryRequantificationHandler.requantify`` against the host route on a small AlphaRaw run, whose frames
then feed the transfer-learning accumulator."""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import candidate_library_cases as G
import synthetic as syn
from alphadia_amd import _abi, runtime
from alphadia_amd import calibration as cal
from alphadia_amd import transfer_requantification as trq
from alphadia_amd.fragcomp import candidate_hash
from test_calibration import CASES, golden_model

pytestmark = pytest.mark.gpu

BYTE_COLUMNS = ("type", "loss_type", "charge", "number", "position", "cardinality")


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


def both(ctx) -> np.ndarray:
    """The device records, which the host mirror must repeat byte for byte."""
    dev, mirror = ctx.staged_fragment_records(), ctx.staged_fragment_records(host_mirror=True)
    assert dev.shape == mirror.shape and dev.tobytes() == mirror.tobytes()
    return dev


def eight(cols: dict) -> tuple:
    return (cols["mz_library"], cols["intensity"], *(cols[k] for k in BYTE_COLUMNS))


@functools.lru_cache(maxsize=None)
def mix():
    """~400 precursors: every length of ``G.LENGTHS``, charges 1-4, every modification pattern.  Read-only."""
    return G.draw_precursors(400, seed=11)


@functools.lru_cache(maxsize=None)
def restated(max_charge: int):
    arrays, series, args = G.tables_of(mix(), max_charge=max_charge)
    start, stop, cols = trq.host_candidate_library(*args)
    for c in cols.values():
        c.setflags(write=False)
    return arrays, series, args, start, stop, cols


def by_hand(frame: pd.DataFrame, p: int, series) -> list[tuple]:
    """The rows of precursor p in Python floats: (mz_library as float32, type, charge, number, position)."""
    table = G.aa_mass_table()
    m = [float(table[ord(a)]) for a in frame["sequence"].iloc[p]]
    if frame["mods"].iloc[p]:
        for name, site in zip(frame["mods"].iloc[p].split(";"), frame["mod_sites"].iloc[p].split(";")):
            s = int(site)
            j = 0 if s == 0 else len(m) - 1 if s == -1 else s - 1
            m[j] = m[j] + G.MOD_MASS[name]
    prefix = [m[0]]
    for v in m[1:]:
        prefix.append(prefix[-1] + v)
    pep = prefix[-1] + G.MASS_H2O
    rows = []
    for i in range(len(m) - 1):
        for kind, from_nterm, z in zip(*series[1:]):
            v = prefix[i] if from_nterm else pep - prefix[i]
            rows.append((np.float32(v / float(z) + G.MASS_PROTON), int(kind), int(z),
                         i + 1 if from_nterm else len(m) - 1 - i, i))
    return rows


# ---- 1. records equal the restatement -------------------------------------------------------------------------------

@pytest.mark.parametrize("max_charge", [1, 2, 3])
def test_records_equal_the_restatement(ctx, max_charge):
    arrays, series, args, start, stop, cols = restated(max_charge)
    S = 2 * max_charge
    lengths = np.diff(arrays["seq_offset"])
    assert set(lengths.tolist()) == set(G.LENGTHS) and lengths[0] == 2 and lengths[-1] == 255
    assert int(stop[-1]) > 8 * 1024  # several blocks of the kernel
    got_start, got_stop, mz_library, mz_calibrated = ctx.stage_candidate_library(_abi.pack_candidate_library(*args))
    assert ctx.calibration_time_ms() >= 0.0
    assert mz_calibrated is None
    assert got_start.dtype == np.uint32 and np.array_equal(got_start, start)
    assert got_stop.dtype == np.uint32 and np.array_equal(got_stop, stop)
    dev = both(ctx)
    want = G.records_of(cols)
    assert dev.shape == want.shape == (int(stop[-1]),)
    for name in want.dtype.names:
        assert dev[name].tobytes() == want[name].tobytes(), name
    assert dev.tobytes() == want.tobytes()
    assert mz_library.dtype == np.float32 and np.array_equal(mz_library.view(np.uint32), cols["mz_library"].view(np.uint32))
    # the first precursor (two residues: one position) and the last (255: number and position at the uint8 edge)
    for p in (0, len(start) - 1):
        rows = by_hand(mix(), p, series)
        rec = dev[int(start[p]):int(stop[p])]
        assert len(rec) == len(rows) == (lengths[p] - 1) * S
        assert np.array_equal(rec["mz_library"].view(np.uint32), np.array([r[0] for r in rows], np.float32).view(np.uint32))
        assert np.array_equal(rec["mz"].view(np.uint32), rec["mz_library"].view(np.uint32))
        for k, name in enumerate(("type", "charge", "number", "position"), start=1):
            assert rec[name].tolist() == [r[k] for r in rows], name
        assert (rec["intensity"] == 1).all() and not rec["loss_type"].any() and not rec["cardinality"].any()
    assert dev["position"][-1] == 253 and dev["number"][int(stop[-1]) - S] == 254 and dev["number"][-1] == 1
    assert not ctx.staged_from(*eight(cols))  # the staged library equals no host column set yet


# ---- 2. calibrated --------------------------------------------------------------------------------------------------

def fragment_mz_model() -> cal.HipLOESSRegression:
    model = golden_model(CASES["mz_f32"])
    assert model.beta.shape[1] == 2  # two kernels, as the fragment m/z estimator
    return model


@pytest.mark.parametrize("max_charge", [1, 2, 3])
def test_calibrated_records_equal_the_calibrated_staging(ctx, max_charge):
    _, _, args, start, stop, cols = restated(max_charge)
    model = fragment_mz_model()
    got_start, got_stop, mz_library, y = ctx.stage_candidate_library(_abi.pack_candidate_library(*args), model)
    dev = both(ctx).copy()
    assert np.array_equal(got_start, start) and np.array_equal(got_stop, stop)
    assert np.array_equal(mz_library.view(np.uint32), cols["mz_library"].view(np.uint32))
    want_y = ctx.stage_fragments_calibrated(model, *eight(cols))
    want = both(ctx)
    assert y.dtype == np.float64 and np.array_equal(y.view(np.uint64), want_y.view(np.uint64))
    assert dev.tobytes() == want.tobytes()
    assert np.array_equal(dev["mz"].view(np.uint32), y.astype(np.float32).view(np.uint32))
    assert (dev["mz"] != dev["mz_library"]).mean() > 0.5 and np.isfinite(y).all()


def test_past_one_pipeline_chunk(ctx):
    """More rows than one chunk of the pipeline: the second chunk runs on the other slot and stream."""
    n = 700
    frame = pd.DataFrame({"sequence": np.array(["".join(np.roll(G.LETTERS, p)[np.arange(255) % 20]) for p in range(n)], dtype=object),
                          "mods": np.full(n, "", dtype=object), "mod_sites": np.full(n, "", dtype=object)})
    _, _, args = G.tables_of(frame, max_charge=3)
    start, stop, cols = trq.host_candidate_library(*args)
    total = int(stop[-1])
    assert _abi.CALIBRATION_CHUNK_ROWS < total < 2 * _abi.CALIBRATION_CHUNK_ROWS
    model = fragment_mz_model()
    ctx.d2h_bytes(reset=True)
    _, got_stop, mz_library, y = ctx.stage_candidate_library(_abi.pack_candidate_library(*args), model)
    assert ctx.d2h_bytes(reset=True) == 12 * total  # mz_library and the predictions, nothing else
    dev = both(ctx).copy()
    want_y = ctx.stage_fragments_calibrated(model, *eight(cols))
    assert np.array_equal(got_stop, stop)
    assert np.array_equal(mz_library.view(np.uint32), cols["mz_library"].view(np.uint32))
    assert np.array_equal(y.view(np.uint64), want_y.view(np.uint64))
    assert dev.tobytes() == both(ctx).tobytes()


# ---- 3. the empty table and the refusals ----------------------------------------------------------------------------

def _args(sequence, mods=None, sites=None, max_charge=2):
    n = len(sequence)
    frame = pd.DataFrame({"sequence": np.array(sequence, dtype=object),
                          "mods": np.array(mods if mods is not None else [""] * n, dtype=object),
                          "mod_sites": np.array(sites if sites is not None else [""] * n, dtype=object)})
    return list(G.tables_of(frame, max_charge=max_charge)[2])


def test_empty_table(ctx):
    start, stop, mz_library, y = ctx.stage_candidate_library(_abi.pack_candidate_library(*_args([])), fragment_mz_model())
    assert start.shape == stop.shape == mz_library.shape == y.shape == (0,)
    assert both(ctx).shape == (0,)


def test_refusals_leave_the_staged_library(ctx):
    good = _args(["PEPTIDEK", "AG", "GASP"])
    ctx.stage_candidate_library(_abi.pack_candidate_library(*good))
    before = both(ctx).tobytes()
    n_before, key_before = ctx._n_lib, ctx._lib_source
    ctx.d2h_bytes(reset=True)

    def refused(args, match):
        with pytest.raises(runtime.HipBackendError, match=match):
            ctx.stage_candidate_library(_abi.pack_candidate_library(*args), fragment_mz_model())

    refused(_args(["PEPTIDEK", "K", "GASP"]), r"1 residues")                      # L < 2
    refused(_args(["PEPTIDEK", "G" * 256]), r"256 residues")                      # L > 255
    high = _args(["PEPTIDEK", "AG"])
    high[1] = high[1].copy()
    high[1][9] = 128
    refused(high, r"128 or above")                                                # a residue byte >= 128
    refused(_args(["PEPTIDEK", "AG"], ["", "Oxidation@M"], ["", "3"]), r"site 3 outside")       # site > L
    refused(_args(["PEPTIDEK", "AG"], ["Oxidation@M", ""], ["-2", ""]), r"site -2 outside")     # site < -1
    none = _args(["PEPTIDEK"])
    none[8:] = [np.zeros(0, np.uint8)] * 3
    refused(none, r"no fragment series")                                          # n_series = 0
    many = _args(["PEPTIDEK"])
    many[8:] = [np.full(65, 98, np.uint8), np.ones(65, np.uint8), np.ones(65, np.uint8)]
    refused(many, r"more than 64")
    # 2^32 rows: 264 300 precursors of 255 residues in 64 series (254 * 64 rows each)
    n = 264_300
    assert n * 254 * 64 >= 2**32 > (n - 100) * 254 * 64
    big = _args(["AG"])
    big[0] = np.arange(n + 1, dtype=np.int64) * 255
    big[1] = np.full(n * 255, ord("G"), dtype=np.uint8)
    big[2] = np.zeros(n + 1, dtype=np.int64)
    big[8:] = [np.full(64, 121, np.uint8), np.zeros(64, np.uint8), np.ones(64, np.uint8)]
    refused(big, r"2\^32 rows")
    assert ctx.d2h_bytes() == 0  # nothing ran
    assert both(ctx).tobytes() == before
    assert (ctx._n_lib, ctx._lib_source) == (n_before, key_before)


# ---- 4. the handler against the host route --------------------------------------------------------------------------

CONFIG = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                     "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
          "general": {"thread_count": 4},
          "fdr": {"fdr": 0.01, "competitive_scoring": True, "channel_wise_fdr": False},
          "transfer_library": {"fragment_types": ["b", "y"], "max_charge": 2}}
NAMES = SimpleNamespace(get_rt_column=lambda: "rt_library", get_mobility_column=lambda: "mobility_library",
                        get_precursor_mz_column=lambda: "mz_library", get_fragment_mz_column=lambda: "mz_calibrated")
OPT = SimpleNamespace(ms1_error=10, ms2_error=15, rt_error=30.0, mobility_error=0.1, num_candidates=1, fwhm_rt=5.0,
                      fwhm_mobility=0.01, score_cutoff=0.0, classifier_version=-1)
REPORTER = SimpleNamespace(log_string=lambda *a, **k: None)
N_CYCLES = 100
PLANTED_FRACTION = 0.9


def calibration_manager() -> cal.HipCalibrationManager:
    """The fragment m/z estimator fitted (two kernels, a shift of 2-3 ppm), the precursor estimators not."""
    m = cal.HipCalibrationManager(path=None, load_from_file=False, has_ms1=True, has_mobility=False)
    e = m.get_estimator("fragment", "mz")
    shift = cal.HipLOESSRegression(n_kernels=2, polynomial_degree=1)
    shift.scale_mean, shift.scale_max = np.array([400.0, 1600.0]), np.array([1500.0, 1500.0])
    shift.beta = np.array([[0.0, 0.0], [1 + 2e-6, 1 + 3e-6]])
    for k in ("scale_mean", "scale_max", "beta", "n_kernels", "polynomial_degree"):
        setattr(e.model, k, getattr(shift, k))
    e.is_fitted = True
    return m


@pytest.fixture(scope="module")
def requant_case():
    """~300 identified precursors of 7-30 residues, their b / y library at charge 1-2 planted into a small run."""
    n, seed = 300, 4242
    frame = G.draw_precursors(n, seed=seed, lengths=tuple(range(7, 31)))
    frame["charge"] = np.random.default_rng(seed).integers(2, 4, n).astype(np.uint8)
    _, series, args = G.tables_of(frame, max_charge=2)
    start, stop, cols = trq.host_candidate_library(*args)
    first = cols["mz_library"].astype(np.float64)[start.astype(np.int64)]       # b1 of every precursor
    y_first = cols["mz_library"].astype(np.float64)[start.astype(np.int64) + 2]  # ... and its complement
    peptide = first + y_first - 2 * G.MASS_PROTON
    z = frame["charge"].to_numpy().astype(np.float64)
    rng = np.random.default_rng([seed, 1])
    precursor_df = pd.DataFrame({
        "elution_group_idx": np.arange(n, dtype=np.uint32), "precursor_idx": np.arange(n, dtype=np.uint32),
        "channel": np.zeros(n, dtype=np.uint32), "decoy": np.zeros(n, dtype=np.uint8),
        "flat_frag_start_idx": start, "flat_frag_stop_idx": stop, "charge": frame["charge"].to_numpy(),
        "rt_library": rng.uniform(0, N_CYCLES * 1.5, n).astype(np.float32),
        "mobility_library": np.zeros(n, dtype=np.float32), "mz_library": (peptide / z + G.MASS_PROTON).astype(np.float32),
        "proteins": np.full(n, "P", dtype=object), "genes": np.full(n, "G", dtype=object),
        "sequence": frame["sequence"].to_numpy(), "mods": frame["mods"].to_numpy(), "mod_sites": frame["mod_sites"].to_numpy()})
    for i, share in enumerate((0.5, 0.3, 0.2)):
        precursor_df[f"i_{i}"] = np.float32(share)
    lib = syn.SyntheticLibrary(precursor_df, pd.DataFrame(cols))
    lo, hi = float(precursor_df["mz_library"].min()) - 1, float(precursor_df["mz_library"].max()) + 1
    cycle = syn.make_cycle(n_ms2=12, mz_lo=lo, mz_hi=hi)
    planted = syn.plant_peptides(lib, cycle, N_CYCLES, seed, fraction=PLANTED_FRACTION)
    dia = syn.make_thermo_run(N_CYCLES, seed, cycle=cycle, ms1_peaks=300, ms2_peaks=100, planted=planted, threads=4,
                              ms1_mz_range=(lo, hi), ms2_mz_range=(50.0, 4000.0))
    cands = syn.make_candidates(lib, N_CYCLES, cycle.shape[1], seed, per_precursor=1, apex_cycle=planted.apex_cycle)
    psm = cands.copy()
    for c in ("channel", "rt_library", "mz_library", "mobility_library", "genes", "proteins", "decoy", "mods", "mod_sites",
              "sequence", "charge"):
        psm[c] = precursor_df[c].to_numpy()
    psm["proba"] = rng.random(n).astype(np.float32)
    psm["qval"] = np.float64(0.001)
    psm["rt_observed"], psm["mobility_observed"], psm["mz_observed"] = psm["rt_library"], psm["mobility_library"], psm["mz_library"]
    psm["n_b_ions"] = np.float32(3)  # (a features column the candidate frame does not take over)
    psm = psm.sample(frac=1.0, random_state=3)  # the identifications come in no particular order, with their index
    return SimpleNamespace(dia=dia, psm=psm, planted=np.flatnonzero(planted.apex_cycle >= 0), args=args, series=series)


def _reference_index(scored, frag):
    """Handler :128-135 with fragcomp/utils.py:38-45 as the reference writes them."""
    scored["_candidate_idx"] = candidate_hash(scored["precursor_idx"].values, scored["rank"].values)
    frag["_candidate_idx"] = candidate_hash(frag["precursor_idx"].values, frag["rank"].values)
    frag["frag_idx"] = np.arange(len(frag))
    index_df = frag.groupby("_candidate_idx", as_index=False).agg(
        _frag_start_idx=pd.NamedAgg("frag_idx", "min"), _frag_stop_idx=pd.NamedAgg("frag_idx", "max"))
    index_df["_frag_stop_idx"] += 1
    return scored.merge(index_df, "inner", on="_candidate_idx"), frag


def host_route(case, manager):
    """The restatement's frames, calibrated by the manager's own predict, scored and indexed."""
    from alphadia_amd.extraction_handler import HipExtractionHandler

    scored = trq.candidate_features_to_candidates(case.psm, trq.OPTIONAL_CANDIDATE_COLUMNS)
    arrays = trq.candidate_library_tables(scored["sequence"].to_numpy(), scored["mods"].to_numpy(),
                                          scored["mod_sites"].to_numpy(), G.MOD_MASS)
    start, stop, cols = trq.host_candidate_library(arrays["seq_offset"], arrays["residues"], arrays["mod_offset"],
                                                   arrays["mod_site"], arrays["mod_mass"], G.aa_mass_table(),
                                                   G.MASS_PROTON, G.MASS_H2O, *case.series[1:])
    scored["nAA"] = np.diff(arrays["seq_offset"])
    scored["flat_frag_start_idx"], scored["flat_frag_stop_idx"] = start, stop
    manager.predict(scored, "precursor")
    fragment_df = trq.fragment_frame(cols)
    manager.predict(fragment_df, "fragment")
    handler = HipExtractionHandler(CONFIG, OPT, None, REPORTER, NAMES, device=0)
    _, frag = handler.quantify_candidates(scored, None, case.dia, SimpleNamespace(precursor_df=scored, fragment_df=fragment_df),
                                          top_k_fragments=9999)
    return _reference_index(scored, frag)


@pytest.fixture(scope="module")
def requantified(requant_case):
    manager = calibration_manager()
    want = host_route(requant_case, manager)
    handler = trq.HipTransferLibraryRequantificationHandler(CONFIG, manager, OPT, None, NAMES, REPORTER, G.aa_mass_table(),
                                                            G.MOD_MASS, G.MASS_PROTON, G.MASS_H2O, device=0)
    psm_before = requant_case.psm.copy()
    got = handler.requantify(requant_case.dia, requant_case.psm)
    pd.testing.assert_frame_equal(requant_case.psm, psm_before, check_exact=True)  # the caller's frame is left alone
    return got, want, handler


def test_requantify_equals_the_host_route(requant_case, requantified):
    (got_scored, got_frag), (want_scored, want_frag), handler = requantified
    with_rows = np.intersect1d(np.unique(want_frag["precursor_idx"].to_numpy()), requant_case.planted)
    print(f"host route: {len(with_rows)} of {len(requant_case.planted)} planted precursors return fragment rows, "
          f"{len(want_frag)} rows")
    assert len(requant_case.planted) > 200 and 2 * len(with_rows) > len(requant_case.planted)
    for got, want, what in ((got_scored, want_scored, "scored_candidates"), (got_frag, want_frag, "frag_df")):
        assert list(got.columns) == list(want.columns), what
        for c in want.columns:
            a, b = got[c].to_numpy(), want[c].to_numpy()
            assert a.dtype == b.dtype and a.shape == b.shape, (what, c)
            same = a.tobytes() == b.tobytes() if a.dtype != object else (a == b).all()
            assert same, (what, c)
        pd.testing.assert_frame_equal(got, want, check_exact=True, obj=what)
    # every b / y ion at both charges of a precursor that was scored: 4 per position
    counts = got_frag.groupby("precursor_idx").size()
    n_aa = got_scored.set_index("precursor_idx")["nAA"]
    assert (counts == 4 * (n_aa[counts.index] - 1)).mean() > 0.5
    assert (got_frag["mz"].to_numpy() != got_frag["mz_library"].to_numpy()).mean() > 0.9  # scored on the calibrated m/z
    assert {"_candidate_idx", "_frag_start_idx", "_frag_stop_idx", "nAA", "flat_frag_start_idx"} <= set(got_scored.columns)
    assert handler.last_timings["fragments"] == int(4 * (requant_case.psm["sequence"].str.len() - 1).sum())


def test_requantify_without_a_fitted_model(requant_case, requantified):
    """No fitted estimator: the library is staged uncalibrated and scored on mz_library."""
    manager = cal.HipCalibrationManager(path=None, load_from_file=False, has_ms1=True, has_mobility=False)
    names = SimpleNamespace(**{**vars(NAMES), "get_fragment_mz_column": lambda: "mz_library"})
    handler = trq.HipTransferLibraryRequantificationHandler(CONFIG, manager, OPT, None, names, REPORTER, G.aa_mass_table(),
                                                            G.MOD_MASS, G.MASS_PROTON, G.MASS_H2O, device=0)
    scored, frag = handler.requantify(requant_case.dia, requant_case.psm)
    assert len(frag) > 0 and (frag["mz"].to_numpy() == frag["mz_library"].to_numpy()).all()
    assert set(scored["precursor_idx"]) <= set(requant_case.psm["precursor_idx"])
    with pytest.raises(ValueError, match="not fitted"):
        trq.HipTransferLibraryRequantificationHandler(CONFIG, manager, OPT, None, NAMES, REPORTER, G.aa_mass_table(),
                                                      G.MOD_MASS, G.MASS_PROTON, G.MASS_H2O, device=0
                                                      ).requantify(requant_case.dia, requant_case.psm)


# ---- 5. the chain closes --------------------------------------------------------------------------------------------

def test_frames_feed_the_transfer_learning_accumulator(requant_case, requantified):
    from alphadia_amd.transfer_library import HipTransferLearningAccumulator

    (scored, frag), _, _ = requantified
    psm = scored.copy()
    psm["mod_seq_hash"] = psm["precursor_idx"].to_numpy().astype(np.int64) + 1000  # (the output stage hashes the sequences)
    names = requant_case.series[0]
    acc = HipTransferLearningAccumulator(keep_top=2, device=0)
    try:
        acc.add_run(psm, frag, names)
        lib = acc.consensus_speclibase
        assert len(lib.precursor_df) == len(psm)
        dense = lib._fragment_mz_df
        assert list(dense.columns) == names and len(dense) == int((psm["sequence"].str.len() - 1).sum())
        assert np.count_nonzero(dense.to_numpy()) == len(frag)
    finally:
        acc.close()
