"""The library staged from its columns and calibrated in HBM, on the GPU: ``adh_stage_fragments_columns`` against
``adh_stage_fragments`` byte for byte, the calibrated records against ``adh_calibration_predict`` bit for bit and
against the reference's predictions (tests/golden/calibration.npz), the in-place path, the staging keys, a search
over a library calibrated in place, and the optimisation lock."""

from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import synthetic as syn
from alphadia_amd import _abi, runtime
from alphadia_amd import calibration as cal
from alphadia_amd.scoring import fragment_columns
from test_calibration import CASES, FITTED, golden_model, np_predict
from test_calibration_gpu import _psms, check_against, f32_knife_edge
from test_optimization_resident_gpu import CONFIG, _handler
from test_optimization_resident_gpu import _manager as _fdr_manager

pytestmark = pytest.mark.gpu

CHUNK = _abi.CALIBRATION_CHUNK_ROWS
SIZES = [0, 1, 255, 256, 257, 1000, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
BYTE_COLUMNS = ("type", "loss_type", "charge", "number", "position", "cardinality")


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


def one_kernel_model() -> cal.HipLOESSRegression:
    """One kernel (weight 1 everywhere, NaN inputs included), degree 0: the constant beta."""
    m = cal.HipLOESSRegression(n_kernels=1, polynomial_degree=0)
    m.scale_mean, m.scale_max, m.beta = np.array([700.0]), np.array([500.0]), np.array([[431.2197265625 + 2.0**-20]])
    return m


MODELS = {"mz_f32": lambda: golden_model(CASES["mz_f32"]), "rt_f64": lambda: golden_model(CASES["rt_f64"]),
          "one_kernel": one_kernel_model}


def test_the_models_have_the_kernel_counts_the_cases_need():
    assert [MODELS[k]().beta.shape[1] for k in ("mz_f32", "rt_f64", "one_kernel")] == [2, 6, 1]
    assert MODELS["one_kernel"]().beta.shape[0] == 1


@functools.lru_cache(maxsize=None)
def library(n: int) -> dict:
    """Nine columns of n rows.  mz_library starts with NaN, 0, values far below the first and above the last kernel of
    every model and one at a kernel centre; every byte column holds 0 and 255.  Read-only: shared by the tests."""
    rng = np.random.default_rng(1000 + n % 9973)
    cols = {"mz_library": rng.uniform(-900.0, 9000.0, n).astype(np.float32),
            "mz": rng.uniform(100.0, 2500.0, n).astype(np.float32),
            "intensity": rng.random(n).astype(np.float32)}
    special = np.array([np.nan, 0.0, -1e6, 1e7, CASES["mz_f32"]["scale_mean"][0], -0.0, np.inf], dtype=np.float32)
    cols["mz_library"][: min(n, special.size)] = special[:n]
    for j, name in enumerate(BYTE_COLUMNS):
        c = rng.integers(0, 256, n).astype(np.uint8)
        if n >= 2:
            c[(j + 1) % n], c[(j + 3) % n] = 0, 255
        cols[name] = c
    for c in cols.values():
        c.setflags(write=False)
    return cols


def nine(cols: dict, mz: str = "mz") -> tuple:
    return (cols["mz_library"], cols[mz], cols["intensity"], *(cols[k] for k in BYTE_COLUMNS))


def eight(cols: dict) -> tuple:
    return (cols["mz_library"], cols["intensity"], *(cols[k] for k in BYTE_COLUMNS))


def raw(records: np.ndarray) -> np.ndarray:
    assert records.dtype == _abi.LIB_RECORD_DTYPE
    return records.view(np.uint8).reshape(-1, 32)


def both(ctx) -> tuple[np.ndarray, np.ndarray]:
    """The device records and the host mirror, which must be the same bytes."""
    dev, mirror = ctx.staged_fragment_records(), ctx.staged_fragment_records(host_mirror=True)
    assert dev.shape == mirror.shape and dev.tobytes() == mirror.tobytes()
    return dev, mirror


@functools.lru_cache(maxsize=None)
def expected(n: int, model_name: str) -> tuple[np.ndarray, np.ndarray]:
    """Today's path: the float64 column of adh_calibration_predict and its float32."""
    y = runtime.get_context(0).calibration_predict(MODELS[model_name](), library(n)["mz_library"])
    y.setflags(write=False)
    return y, y.astype(np.float32)


def assert_calibrated(records: np.ndarray, n: int, model_name: str, returned: np.ndarray | None):
    y, y32 = expected(n, model_name)
    cols = library(n)
    assert records.shape == (n,)
    assert np.array_equal(records["mz"].view(np.uint32), y32.view(np.uint32))
    if returned is not None:
        assert returned.dtype == np.float64 and np.array_equal(returned.view(np.uint64), y.view(np.uint64))
    assert np.array_equal(records["mz_library"].view(np.uint32), cols["mz_library"].view(np.uint32))
    assert np.array_equal(records["intensity"].view(np.uint32), cols["intensity"].view(np.uint32))
    for k in BYTE_COLUMNS:
        assert np.array_equal(records[k], cols[k]), k
    assert not records["pad"].any()


# ---- 1. columns equal records ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_columns_equal_records(ctx, n):
    cols = library(n)
    assert ctx.stage_fragments(*nine(cols), force=True)
    want_dev, want_mirror = both(ctx)
    assert want_dev.shape == (n,)
    ctx.stage_fragments(*nine(cols, "mz_library"), force=True)  # (something else in between)
    ctx.stage_fragments_columns(*nine(cols))
    got_dev, got_mirror = both(ctx)
    assert got_dev.tobytes() == want_dev.tobytes()
    assert got_mirror.tobytes() == want_mirror.tobytes()
    assert not got_dev["pad"].any()
    assert np.array_equal(got_dev["mz"].view(np.uint32), cols["mz"].view(np.uint32))
    assert not ctx.stage_fragments(*nine(cols))  # the key is that of the columns


# ---- 2. calibrated staging against today's path ---------------------------------------------------------------------

@pytest.mark.parametrize("model_name", list(MODELS))
@pytest.mark.parametrize("n", SIZES)
def test_calibrated_staging_is_bit_exact(ctx, n, model_name):
    y = ctx.stage_fragments_calibrated(MODELS[model_name](), *eight(library(n)))
    assert ctx.calibration_time_ms() >= 0.0
    for records in both(ctx):
        assert_calibrated(records, n, model_name, y)
    if n >= 7:  # NaN in, NaN out - except through the single kernel, whose weight is 1 whatever the input
        assert np.isnan(y[0]) == (model_name != "one_kernel")
        assert np.isfinite(y[1:4]).all()


# ---- 3. in place ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, model_a, model_b", [(n, "mz_f32", "rt_f64") for n in SIZES] +
                         [(257, "one_kernel", "mz_f32"), (CHUNK + 1, "rt_f64", "one_kernel")])
def test_in_place_calibration(ctx, n, model_a, model_b):
    cols = library(n)
    ctx.stage_fragments(*nine(cols, "mz_library"), force=True)
    before, _ = both(ctx)
    y = ctx.calibrate_staged_fragments(MODELS[model_a]())
    assert ctx.calibration_time_ms() >= 0.0
    for records in both(ctx):
        assert_calibrated(records, n, model_a, y)
        masked, want = raw(records).copy(), raw(before).copy()
        masked[:, 4:8] = 0
        want[:, 4:8] = 0
        assert masked.tobytes() == want.tobytes()  # every byte but mz: mz_library and the pads included
    # a second calibration starts from mz_library again, not from the calibrated mz
    y_b = ctx.calibrate_staged_fragments(MODELS[model_b]())
    got_dev, got_mirror = both(ctx)
    fresh = ctx.stage_fragments_calibrated(MODELS[model_b](), *eight(cols))
    want_dev, want_mirror = both(ctx)
    assert np.array_equal(y_b.view(np.uint64), fresh.view(np.uint64))
    assert got_dev.tobytes() == want_dev.tobytes() and got_mirror.tobytes() == want_mirror.tobytes()
    assert_calibrated(got_dev, n, model_b, y_b)


def test_in_place_counts_the_copy_back_as_predict_does(ctx):
    n = CHUNK + 1
    cols = library(n)
    ctx.stage_fragments(*nine(cols, "mz_library"), force=True)
    ctx.d2h_bytes(reset=True)
    ctx.calibration_predict(MODELS["mz_f32"](), cols["mz_library"])
    predict_bytes = ctx.d2h_bytes(reset=True)
    ctx.calibrate_staged_fragments(MODELS["mz_f32"]())
    assert ctx.d2h_bytes(reset=True) == predict_bytes == 8 * n
    ctx.stage_fragments_calibrated(MODELS["mz_f32"](), *eight(cols))
    assert ctx.d2h_bytes(reset=True) == 8 * n
    ctx.stage_fragments_columns(*nine(cols))
    assert ctx.d2h_bytes(reset=True) == 0


# ---- 4. against the reference ---------------------------------------------------------------------------------------

F32_CASES = [n for n in FITTED if CASES[n]["meta"]["dtype"] == "float32"]


@pytest.mark.parametrize("name", F32_CASES)
def test_staged_library_matches_reference_predictions(ctx, name):
    c = CASES[name]
    model = golden_model(c)
    for q, want in ((c["query"], c["pred"]), (c["query_nan"], c["pred_nan"])):
        assert q.dtype == np.float32
        n = q.shape[0]
        rng = np.random.default_rng(n)
        others = [rng.random(n).astype(np.float32)] + [rng.integers(0, 256, n).astype(np.uint8) for _ in BYTE_COLUMNS]
        _, scale = np_predict(model.scale_mean, model.scale_max, model.beta, q)
        scale = np.where(np.isnan(scale), 0, scale)
        for path in ("staged", "in_place"):
            if path == "staged":
                y = ctx.stage_fragments_calibrated(model, q, *others)
            else:
                ctx.stage_fragments(q, q, *others, force=True)
                y = ctx.calibrate_staged_fragments(model)
            check_against(y, want, scale)
            dev, _ = both(ctx)
            finite = ~np.isnan(want)
            assert np.array_equal(np.isnan(dev["mz"]), ~finite)
            same = dev["mz"][finite] == want[finite].astype(np.float32)
            edge = f32_knife_edge(want[finite], 1e-13 * scale[finite])
            assert (same | edge).all()
            assert edge.sum() <= max(2, 1e-4 * finite.sum())


# ---- 5. keys --------------------------------------------------------------------------------------------------------

def fitted_manager(model=None) -> cal.HipCalibrationManager:
    m = cal.HipCalibrationManager(path=None, load_from_file=False, has_ms1=True, has_mobility=False)
    e = m.get_estimator("fragment", "mz")
    g = golden_model(CASES["mz_f32"]) if model is None else model
    for k in ("scale_mean", "scale_max", "beta", "n_kernels", "polynomial_degree"):
        setattr(e.model, k, getattr(g, k))
    e.is_fitted = True
    return m


def frame(n: int) -> pd.DataFrame:
    cols = library(n)
    return pd.DataFrame({k: cols[k].copy() for k in ("mz_library", "intensity", *BYTE_COLUMNS)})


def test_keys(ctx):
    n = 1000
    cols = nine(library(n))
    assert ctx.stage_fragments(*cols, force=True)
    uncalibrated, _ = both(ctx)
    assert not ctx.stage_fragments(*cols)
    ctx.calibrate_staged_fragments(MODELS["mz_f32"]())
    assert ctx.staged_from(*eight(library(n)))
    assert ctx.stage_fragments(*cols)  # the key was cleared: staged again, and the records are the uncalibrated ones
    again, _ = both(ctx)
    assert again.tobytes() == uncalibrated.tobytes()

    manager = fitted_manager()
    for first in ("staged", "in_place"):
        df = frame(n)
        if first == "in_place":
            ctx.stage_fragments(*fragment_columns(df, "mz_library"))
        from_frame = fragment_columns(df, "mz_library")
        assert ctx.staged_from(from_frame[0], *from_frame[2:]) == (first == "in_place")
        assert manager.predict_staged(df) == first
        assert not ctx.stage_fragments(*fragment_columns(df, "mz_calibrated"))
        by_predict = frame(n)
        manager.predict(by_predict, "fragment")
        assert df["mz_calibrated"].dtype == np.float64
        assert np.array_equal(df["mz_calibrated"].to_numpy().view(np.uint64),
                              by_predict["mz_calibrated"].to_numpy().view(np.uint64))
        assert_calibrated(both(ctx)[0], n, "mz_f32", df["mz_calibrated"].to_numpy())
        assert manager.predict_staged(df, only_if_staged=True) == "in_place"  # the adopted columns are this frame's
        assert manager.predict_staged(frame(n), only_if_staged=True) == "host"  # another frame: nothing staged from it
        assert not ctx.stage_fragments(*fragment_columns(df, "mz_calibrated"))


# ---- 6. nothing stale survives --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def search_case():
    case = syn.make_case(n_precursors=600, n_cycles=120, config_id=77, per_precursor=2, n_ms2=8, ms1_peaks=400,
                         ms2_peaks=150, mz_lo=400, mz_hi=480, frag_mz_lo=200, frag_mz_hi=350,
                         ms1_mz_range=(395, 500), ms2_mz_range=(195, 355), planted_fraction=0.5, threads=4)
    lib_p, lib_f, _, psm_f = _psms(case, np.random.default_rng(5))
    manager = cal.HipCalibrationManager(path=None, load_from_file=False, has_ms1=True, has_mobility=False)
    manager.fit(psm_f, "fragment", plot=False)
    assert manager.get_estimator("fragment", "mz").is_fitted
    return case, lib_p, lib_f, manager


def _search(case, pdf, fdf, fragment_mz):
    from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring
    from alphadia_amd.selection import CandidateSelectionConfig, HipCandidateSelection

    scfg = CandidateSelectionConfig()
    scfg.update(dict(rt_tolerance=60.0, precursor_mz_tolerance=10.0, fragment_mz_tolerance=15.0))
    sel = HipCandidateSelection(case.dia, pdf, fdf, scfg, rt_column="rt_library", mobility_column="mobility_library",
                                precursor_mz_column="mz_library", fragment_mz_column=fragment_mz, device=0)()
    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15))
    scorer = HipCandidateScoring(dia_data=case.dia, precursors_flat=pdf, fragments_flat=fdf, rt_column="rt_library",
                                 mobility_column="mobility_library", precursor_mz_column="mz_library",
                                 fragment_mz_column=fragment_mz, config=cfg, device=0)
    features, fragments = scorer(sel)
    return sel, features, fragments


def _both_paths(ctx, search_case):
    case, lib_p, lib_f, manager = search_case
    # A: staged and scored uncalibrated, calibrated in place, searched
    df_a = lib_f.copy()
    _, feat_0, _ = _search(case, lib_p, df_a, "mz_library")
    assert manager.predict_staged(df_a) == "in_place"
    out_a = _search(case, lib_p, df_a, "mz_calibrated")
    # B: the host-calibrated frame staged the way it is today
    df_b = lib_f.copy()
    manager.predict(df_b, "fragment")
    assert ctx.stage_fragments(*fragment_columns(df_b, "mz_calibrated"), force=True)
    out_b = _search(case, lib_p, df_b, "mz_calibrated")
    assert np.array_equal(df_a["mz_calibrated"].to_numpy().view(np.uint64), df_b["mz_calibrated"].to_numpy().view(np.uint64))
    for a, b, what in zip(out_a, out_b, ("candidates", "features", "fragments")):
        assert len(a) > 0, what
        pd.testing.assert_frame_equal(a, b, check_exact=True, obj=what)
    # the calibration moves the staged m/z of most fragments: a library left as it was would not score the same
    moved = df_a["mz_calibrated"].to_numpy().astype(np.float32) != df_a["mz_library"].to_numpy()
    assert moved.mean() > 0.9 and len(feat_0) > 0


def test_nothing_stale_survives(ctx, search_case):
    _both_paths(ctx, search_case)


def test_nothing_stale_survives_without_the_host_rebuild(ctx, search_case, monkeypatch):
    """ADH_DEBUG_COPY_ALL=1: the library columns of the fragment table come from the device records instead of being
    rebuilt from the host mirror."""
    monkeypatch.setenv("ADH_DEBUG_COPY_ALL", "1")
    _both_paths(ctx, search_case)


# ---- 7. the optimisation lock ---------------------------------------------------------------------------------------

LOCK_CONFIG = copy.deepcopy(CONFIG)
LOCK_CONFIG["calibration"]["batch_size"] = 1200  # (each of the two batches scores half of the batch library's candidates)


@pytest.fixture(scope="module")
def lock_case():
    """The case of tests/test_optimization_resident_gpu.py."""
    c = syn.make_case(5000, 260, config_id=78, per_precursor=2, planted_fraction=0.5, threads=4)
    pre, frag = c.library.precursor_df, c.library.fragment_df
    pre["mz_calibrated"] = pre["mz_library"]
    pre["rt_calibrated"] = pre["rt_library"]
    frag["mz_calibrated"] = frag["mz_library"]
    return c


def _lock_run(case, hide: bool):
    """Two batches over one batch library with a calibration update between them."""
    from alphadia_amd.optimization import HipOptimizationLock

    shift = cal.HipLOESSRegression(n_kernels=1, polynomial_degree=1)
    shift.scale_mean, shift.scale_max, shift.beta = np.array([300.0]), np.array([200.0]), np.array([[0.0], [1 + 3e-6]])
    manager = fitted_manager(shift)
    calibration = SimpleNamespace(predict=manager.predict) if hide else manager
    assert hasattr(calibration, "predict_staged") != hide
    fdr_manager = _fdr_manager(case.dia)
    lib = SimpleNamespace(_precursor_df=case.library.precursor_df.copy(), _fragment_df=case.library.fragment_df.copy())
    lock = HipOptimizationLock(lib, LOCK_CONFIG, device=0)
    even = (case.candidates_df["precursor_idx"] % 2 == 0).to_numpy()
    out = {}
    handler = _handler(case.candidates_df[even], fdr_manager)
    out["psm_1"] = handler.process_optimization_batch(case.dia, lock)
    out["lock_1"] = (lock.features_df, lock.fragments_df)
    lock.update_with_calibration(calibration)  # (no lock.update(): the batch library just scored is the one staged)
    out["path"] = lock.last_fragment_calibration
    out["mz_calibrated"] = lock.batch_library.fragment_df["mz_calibrated"].to_numpy().copy()
    lock._precursor_target_count = 1
    handler = _handler(case.candidates_df[~even], fdr_manager)
    out["psm_2"] = handler.process_optimization_batch(case.dia, lock)
    assert lock.has_target_num_precursors
    out["filtered"] = handler.filter_for_calibration(out["psm_2"], LOCK_CONFIG)
    out["lock_2"] = (lock.features_df, lock.fragments_df)
    return out


def test_optimisation_lock_recalibrates_in_place(lock_case):
    staged = _lock_run(lock_case, hide=False)
    hidden = _lock_run(lock_case, hide=True)
    assert staged["path"] == "in_place" and hidden["path"] == "host"
    assert staged["mz_calibrated"].dtype == np.float64
    assert np.array_equal(staged["mz_calibrated"].view(np.uint64), hidden["mz_calibrated"].view(np.uint64))
    for key in ("psm_1", "psm_2"):
        pd.testing.assert_frame_equal(staged[key], hidden[key], check_exact=True, obj=key)
    for got, exp, what in zip(staged["filtered"], hidden["filtered"], ("calibration precursors", "calibration fragments")):
        assert len(got) > 0, what
        pd.testing.assert_frame_equal(got, exp, check_exact=True, obj=what)
    for i, what in enumerate(("features", "fragments")):
        pd.testing.assert_frame_equal(staged["lock_2"][i], hidden["lock_2"][i], check_exact=True, obj=f"lock {what}")
        # the rows accumulated before the update keep the values they were scored with
        first = staged["lock_1"][i]
        assert len(staged["lock_2"][i]) > len(first) > 0
        pd.testing.assert_frame_equal(staged["lock_2"][i].iloc[: len(first)], first, check_exact=True, obj=f"first {what}")
    # ... and the second batch was scored with the recalibrated library
    frags = staged["lock_2"][1].iloc[len(staged["lock_1"][1]):]
    assert len(frags) > 0 and (frags["mz_library"].to_numpy() != frags["mz"].to_numpy()).mean() > 0.9
    first = staged["lock_1"][1]
    assert (first["mz_library"].to_numpy() == first["mz"].to_numpy()).all()


# ---- 8. errors ------------------------------------------------------------------------------------------------------

def test_errors():
    fresh = runtime.Context(0)
    try:
        with pytest.raises(runtime.HipBackendError, match="no fragment library staged"):
            fresh.calibrate_staged_fragments(MODELS["mz_f32"]())
        with pytest.raises(runtime.HipBackendError, match="no fragment library staged"):
            fresh.staged_fragment_records()
        with pytest.raises(runtime.HipBackendError, match="no fragment library staged"):
            fresh.adopt_fragment_columns(*nine(library(256)))
        assert not fresh.staged_from(*eight(library(256)))
        cols = library(256)
        fresh.stage_fragments_columns(*nine(cols))
        before = fresh.staged_fragment_records().tobytes()
        fresh.d2h_bytes(reset=True)
        wide = cal.HipLOESSRegression(n_kernels=33)
        wide.scale_mean, wide.scale_max, wide.beta = np.zeros(33), np.ones(33), np.zeros((3, 33))
        with pytest.raises(ValueError, match="at most 32"):
            fresh.calibrate_staged_fragments(wide)
        with pytest.raises(ValueError, match="at most 32"):
            fresh.stage_fragments_calibrated(wide, *eight(cols))
        short = list(eight(cols))
        short[3] = short[3][:-1]
        with pytest.raises(ValueError, match="differ in length"):
            fresh.stage_fragments_calibrated(MODELS["mz_f32"](), *short)
        short = list(nine(cols))
        short[1] = short[1][:-1]
        with pytest.raises(ValueError, match="differ in length"):
            fresh.stage_fragments_columns(*short)
        with pytest.raises(ValueError, match="staged library's 256 rows"):
            fresh.adopt_fragment_columns(*nine(library(255)))
        with pytest.raises(ValueError, match="nine"):
            fresh.adopt_fragment_columns(*eight(cols))
        # none of these launched a kernel: no prediction came back, the library is as it was and keeps its key
        assert fresh.d2h_bytes() == 0
        assert fresh.staged_fragment_records().tobytes() == before
        assert not fresh.stage_fragments(*nine(cols))
    finally:
        fresh.close()


def test_model_limits_of_the_c_entries():
    """The limits the C entries check themselves (the Python packer refuses such a model before the call)."""
    import ctypes as C

    fresh = runtime.Context(0)
    try:
        cols = library(256)
        fresh.stage_fragments_columns(*nine(cols))
        before = fresh.staged_fragment_records().tobytes()
        packed = _abi.pack_loess_model(*(getattr(MODELS["mz_f32"](), k) for k in ("scale_mean", "scale_max", "beta")))
        packed.n_kernels = 33
        y = np.zeros(256)
        rc = runtime.lib.adh_calibrate_staged_fragments(fresh._h, C.byref(packed), y.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == -4 and b"n_kernels" in runtime.lib.adh_last_error()
        packed.n_kernels, packed.degree = 2, 5
        m = _abi.pack_fragments_calibrated(*eight(cols))
        rc = runtime.lib.adh_stage_fragments_columns(fresh._h, m.ref(), C.byref(packed), y.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == -4 and b"degree" in runtime.lib.adh_last_error()
        m = _abi.pack_fragments_calibrated(*eight(cols))  # no model and no m/z column
        assert runtime.lib.adh_stage_fragments_columns(fresh._h, m.ref(), None, None) == -1
        assert fresh.staged_fragment_records().tobytes() == before and not y.any()
    finally:
        fresh.close()
