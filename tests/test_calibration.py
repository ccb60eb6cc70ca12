"""Library calibration on the host: the LOESS fit against the reference's (tests/golden/calibration.npz, written by
tests/golden/make_golden_calibration.py from alphadia/calibration/models.py and estimator.py), the estimator and the
manager.  The prediction itself runs on the GPU (tests/test_calibration_gpu.py); here a small NumPy evaluator of the
reference's arithmetic stands in for it."""

from __future__ import annotations

import json
import logging
import os

import numpy as np
import pandas as pd
import pytest

from alphadia_amd import calibration as cal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calibration.npz")


def load_golden():
    z = np.load(GOLDEN)
    cases = {}
    for name in z["cases"]:
        name = str(name)
        c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        c["meta"] = json.loads(str(c["meta"]))
        cases[name] = c
    return cases


CASES = load_golden()
FITTED = [n for n, c in CASES.items() if c["meta"]["fit_ok"]]
# a singular normal-equation system (two rows left for a cubic): its beta is noise, only the decisions are compared
ILL_POSED = {"rt_f64_reduce_degree"}


def np_predict(scale_mean, scale_max, beta, x):
    """LOESSRegression.predict in plain NumPy: (prediction, forward-error scale sum_k w_k sum_d |x^d beta_dk|)."""
    col = np.asarray(x).reshape(-1)
    if col.dtype not in (np.float32, np.float64):
        col = col.astype(np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    d1, k = beta.shape
    design = np.empty((col.shape[0], d1), dtype=col.dtype)
    design[:, 0] = 1
    for d in range(1, d1):
        design[:, d] = col if d == 1 else design[:, d - 1] * col
    design = design.astype(np.float64)
    v = (col.astype(np.float64)[:, None] - np.asarray(scale_mean, dtype=np.float64)) / np.asarray(scale_max, np.float64)
    if k == 1:
        w = np.ones(v.shape)
    else:
        a = np.abs(v)
        w = (a <= 1) * ((1 - a**3) ** 3 + 1e-6)
        w[:, 0] = np.where(v[:, 0] < 0, 1, w[:, 0])
        w[:, -1] = np.where(v[:, -1] > 0, 1, w[:, -1])
    w = w / w.sum(axis=1, keepdims=True)
    return (design @ beta * w).sum(axis=1), (np.abs(design) @ np.abs(beta) * np.abs(w)).sum(axis=1)


def golden_model(c) -> cal.HipLOESSRegression:
    args = c["meta"]["model_args"]
    m = cal.HipLOESSRegression(**args)
    m.n_kernels = c["meta"]["n_kernels"]
    m.polynomial_degree = c["meta"]["polynomial_degree"]
    m.scale_mean, m.scale_max, m.beta = c["scale_mean"].copy(), c["scale_max"].copy(), c["beta"].copy()
    return m


@pytest.fixture
def numpy_predict(monkeypatch):
    """HipLOESSRegression.predict through the NumPy evaluator (no GPU)."""
    monkeypatch.setattr(cal.HipLOESSRegression, "predict",
                        lambda self, x, device=None: np_predict(self.scale_mean, self.scale_max, self.beta, x)[0])


def test_golden_covers_the_cases():
    meta = {n: c["meta"] for n, c in CASES.items()}
    assert {m["dtype"] for m in meta.values()} == {"float32", "float64"}
    assert {1, 2, 6} <= {m["n_kernels"] for m in meta.values() if m["fit_ok"]}
    assert meta["rt_f64_uniform"]["uniform_used"] and not meta["gap_f64_uniform_fallback"]["uniform_used"]
    assert meta["mz_f64_reduce_kernels"]["n_kernels"] < meta["mz_f64_reduce_kernels"]["model_args"]["n_kernels"]
    assert meta["rt_f64_reduce_degree"]["polynomial_degree"] < meta["rt_f64_reduce_degree"]["model_args"]["polynomial_degree"]
    assert not meta["rt_f64_two_points"]["fit_ok"]
    c = CASES["mz_f32_outliers"]
    assert c["x_train"].max() > 4000 and meta["mz_f32_outliers"]["n_trimmed"] < c["x_train"].size
    assert all(meta[n]["reference_rejects_nan"] for n in FITTED)


@pytest.mark.parametrize("name", list(CASES))
def test_host_fit_matches_reference(name):
    """Decisions exact, scales to 1e-12, predictions of the fitted model to 1e-8 of the target range."""
    c = CASES[name]
    meta = c["meta"]
    model = cal.HipLOESSRegression(**meta["model_args"])
    x, y = c["x_train"][:, None], c["y_train"][:, None]
    if not meta["fit_ok"]:
        with pytest.raises((ValueError, np.linalg.LinAlgError)):
            model.fit(x, y)
        assert (model.n_kernels, model.polynomial_degree) == (meta["n_kernels"], meta["polynomial_degree"])
        return
    model.fit(x, y)
    assert int(model.n_kernels) == meta["n_kernels"]
    assert model.polynomial_degree == meta["polynomial_degree"]
    assert model.uniform_used_ == meta["uniform_used"]
    assert model.n_trimmed_ == meta["n_trimmed"]
    assert model.beta.shape == c["beta"].shape
    np.testing.assert_allclose(model.scale_mean, c["scale_mean"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(model.scale_max, c["scale_max"], rtol=1e-12, atol=0)
    if name in ILL_POSED:
        return
    got, _ = np_predict(model.scale_mean, model.scale_max, model.beta, c["query"])
    tol = 1e-8 * np.abs(c["y_train"].astype(np.float64)).max()
    assert np.abs(got - c["pred"]).max() <= tol, (name, np.abs(got - c["pred"]).max(), tol)


@pytest.mark.parametrize("name", FITTED)
def test_numpy_evaluator_reproduces_reference(name):
    """The test's evaluator (the yardstick of the device) against the reference's own predictions."""
    c = CASES[name]
    got, scale = np_predict(c["scale_mean"], c["scale_max"], c["beta"], c["query"])
    assert (np.abs(got - c["pred"]) <= 1e-13 * scale).all()
    got_nan, _ = np_predict(c["scale_mean"], c["scale_max"], c["beta"], c["query_nan"])
    assert np.array_equal(np.isnan(got_nan), np.isnan(c["query_nan"]))
    assert np.array_equal(np.isnan(c["pred_nan"]), np.isnan(c["query_nan"]))


@pytest.mark.parametrize("has_ms1,has_mobility", [(True, True), (True, False), (False, True), (False, False)])
def test_manager_groups(has_ms1, has_mobility):
    m = cal.HipCalibrationManager(has_ms1=has_ms1, has_mobility=has_mobility, load_from_file=False)
    assert set(m.estimator_groups) == {"fragment", "precursor"}
    assert set(m.estimator_groups["fragment"]) == {"mz"}
    want = {"rt"} | ({"mz"} if has_ms1 else set()) | ({"mobility"} if has_mobility else set())
    assert set(m.estimator_groups["precursor"]) == want
    assert m.get_estimator("fragment", "mz").model.n_kernels == 2
    assert m.get_estimator("precursor", "rt").model.n_kernels == 6
    assert m.get_estimator("precursor", "nothing") is None and m.get_estimator("none", "mz") is None
    assert m.get_estimator("fragment", "mz").transform_deviation == 1e6
    assert not m.all_fitted


def test_other_models_are_not_implemented():
    config = {"precursor": {"rt": dict(cal.CALIBRATION_GROUPS_CONFIG["precursor"]["rt"], model="LinearRegression")}}
    with pytest.raises(NotImplementedError, match="LinearRegression"):
        cal.HipCalibrationManager(load_from_file=False, calibration_config=config)


def test_unfitted_estimator_skips(caplog):
    m = cal.HipCalibrationManager(load_from_file=False)
    df = pd.DataFrame({"mz_library": np.array([500.0, 600.0], np.float32)})
    est = m.get_estimator("fragment", "mz")
    with caplog.at_level(logging.WARNING):
        assert est.predict(df, inplace=False) is None
        m.predict(df, "fragment")
    assert "mz_calibrated" not in df.columns
    assert "not been fitted" in caplog.text
    assert est.ci(df.assign(mz_observed=df.mz_library), 0.95) == 0
    with pytest.raises(ValueError):
        est.ci(df, 1.5)


def test_failed_fit_leaves_estimator_unfitted(caplog):
    c = CASES["rt_f64_two_points"]
    m = cal.HipCalibrationManager(has_ms1=False, has_mobility=False, load_from_file=False)
    df = pd.DataFrame({"rt_library": c["x_train"], "rt_observed": c["y_train"]})
    with caplog.at_level(logging.WARNING):
        m.fit(df, "precursor", plot=False)
    est = m.get_estimator("precursor", "rt")
    assert not est.is_fitted and est.metrics is None and not m.all_fitted
    assert "Could not fit estimator rt" in caplog.text
    with pytest.raises(ValueError, match="failed input validation"):
        m.fit(pd.DataFrame({"rt_library": c["x_train"]}), "precursor")


@pytest.mark.parametrize("name", FITTED)
def test_ci_and_metrics_from_golden_parameters(name, numpy_predict):
    c = CASES[name]
    meta = c["meta"]
    est = cal.HipCalibrationEstimator(name, golden_model(c), ["x"], ["y"], ["x_calibrated"], meta["transform_deviation"])
    est.is_fitted = True
    df = pd.DataFrame({"x": c["x_train"], "y": c["y_train"]})
    metrics = est._get_metrics(df)
    for k, v in meta["metrics"].items():
        assert metrics[k] == pytest.approx(v, rel=1e-6, abs=1e-9 * max(abs(v), 1.0)), k
    assert est.ci(df, 0.95) == pytest.approx(meta["ci95"], rel=1e-6)
    dev = est.calc_deviation(df)
    assert dev.shape == (len(df), 4)
    est.predict(df)
    assert df["x_calibrated"].dtype == np.float64


def test_fit_computes_metrics(numpy_predict):
    c = CASES["mz_f32"]
    m = cal.HipCalibrationManager(has_ms1=True, has_mobility=False, load_from_file=False)
    df = pd.DataFrame({"mz_library": c["x_train"], "mz_observed": c["y_train"]})
    m.fit(df, "fragment", plot=True)
    est = m.get_estimator("fragment", "mz")
    assert est.is_fitted and not m.all_fitted
    for k, v in c["meta"]["metrics"].items():
        assert est.metrics[k] == pytest.approx(v, rel=1e-4), k


def _manager_with_golden_parameters(**kwargs):
    m = cal.HipCalibrationManager(has_ms1=True, has_mobility=True, load_from_file=False, **kwargs)
    for (g, n), case in {("fragment", "mz"): "mz_f32", ("precursor", "mz"): "mz_f64", ("precursor", "rt"): "rt_f32",
                         ("precursor", "mobility"): "mobility_f32"}.items():
        est = m.get_estimator(g, n)
        est._model = golden_model(CASES[case])
        est.is_fitted = True
        est.metrics = dict(CASES[case]["meta"]["metrics"])
    m.all_fitted = True
    return m


def test_save_load_round_trip(tmp_path, numpy_predict):
    path = str(tmp_path / "calibration_manager.pkl")
    m = _manager_with_golden_parameters(path=path)
    m.save()
    loaded = cal.HipCalibrationManager(path=path, load_from_file=True)
    assert loaded.is_loaded_from_file and loaded.all_fitted
    fresh = cal.HipCalibrationManager(path=str(tmp_path / "missing.pkl"), load_from_file=True)
    assert not fresh.is_loaded_from_file
    for g, group in m.estimator_groups.items():
        for n, est in group.items():
            other = loaded.get_estimator(g, n)
            assert other.is_fitted and other.metrics == est.metrics
            for k in ("scale_mean", "scale_max", "beta"):
                assert np.array_equal(getattr(other.model, k), getattr(est.model, k))
            assert other.model.get_params() == est.model.get_params()
    df = pd.DataFrame({"mz_library": CASES["mz_f32"]["query"]})
    a, b = df.copy(), df.copy()
    m.predict(a, "fragment")
    loaded.predict(b, "fragment")
    assert np.array_equal(a["mz_calibrated"].to_numpy(), b["mz_calibrated"].to_numpy())


class LOESSRegression:  # the reference's class name: what from_reference recognises
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _RefEstimator:
    def __init__(self, name, model, input_columns, target, output, transform, is_fitted, metrics):
        self.name, self._model, self.input_columns = name, model, input_columns
        self._target_columns, self._output_columns = target, output
        self.transform_deviation, self.is_fitted, self.metrics = transform, is_fitted, metrics


class _RefManager:
    def __init__(self, groups, has_ms1, has_mobility):
        self.estimator_groups, self._has_ms1, self._has_mobility = groups, has_ms1, has_mobility
        self.all_fitted, self.path = True, None


def _reference_like_manager(model_type=LOESSRegression):
    def est(name, case, col):
        c = CASES[case]
        model = model_type(n_kernels=c["meta"]["n_kernels"], kernel_size=2.0,
                           polynomial_degree=c["meta"]["polynomial_degree"], uniform=False,
                           scale_mean=c["scale_mean"], scale_max=c["scale_max"], beta=c["beta"])
        return _RefEstimator(name, model, [f"{col}_library"], [f"{col}_observed"], [f"{col}_calibrated"],
                             c["meta"]["transform_deviation"], True, c["meta"]["metrics"])

    return _RefManager({"fragment": {"mz": est("mz", "mz_f32", "mz")},
                        "precursor": {"rt": est("rt", "rt_f64", "rt")}}, has_ms1=False, has_mobility=False)


def test_from_reference(numpy_predict):
    ref = _reference_like_manager()
    m = cal.HipCalibrationManager.from_reference(ref)
    assert m.all_fitted and set(m.estimator_groups["precursor"]) == {"rt"}
    est = m.get_estimator("precursor", "rt")
    c = CASES["rt_f64"]
    assert est.is_fitted and est.metrics == c["meta"]["metrics"] and est.transform_deviation is None
    assert np.array_equal(est.model.beta, c["beta"]) and est.model.n_kernels == 6
    df = pd.DataFrame({"rt_library": c["query"]})
    m.predict(df, "precursor")
    assert np.abs(df["rt_calibrated"].to_numpy() - c["pred"]).max() <= 1e-9 * np.abs(c["pred"]).max()

    class LinearRegression:
        def __init__(self, **kw):
            pass

    with pytest.raises(NotImplementedError, match="LinearRegression"):
        cal.HipCalibrationManager.from_reference(_reference_like_manager(LinearRegression))


def test_saved_state_is_recognised(tmp_path, numpy_predict):
    """What the run statistics of the reference read back after a search: the manager class is
    picked by ``is_saved_state``, and the loaded estimators carry the metrics."""
    import pickle

    path = str(tmp_path / "calibration_manager.pkl")
    _manager_with_golden_parameters(path=path).save()
    assert cal.HipCalibrationManager.is_saved_state(path)
    other = str(tmp_path / "other.pkl")
    with open(other, "wb") as f:
        pickle.dump({"something": "else"}, f)
    assert not cal.HipCalibrationManager.is_saved_state(other)
    with open(other, "wb") as f:
        f.write(b"not a pickle")
    assert not cal.HipCalibrationManager.is_saved_state(other)
    stats = cal.HipCalibrationManager(path=path)
    for group, case in (("fragment", "mz_f32"), ("precursor", "mz_f64")):
        metrics = stats.get_estimator(group, "mz").metrics
        assert metrics == CASES[case]["meta"]["metrics"]
        assert {"median_accuracy", "median_precision"} <= set(metrics)


def test_loess_model_struct_matches_header():
    """_abi.LoessModel / its limits against adh_loess_model_t and the #defines of include/alphadia_hip.h: a drift
    would make the device read beta at the wrong offsets."""
    import ctypes as C
    import re

    from alphadia_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "alphadia_hip.h")).read()

    def define(name):
        m = re.search(rf"#define\s+{name}\s+\(?([0-9]+)(?:\s*<<\s*([0-9]+))?\)?", header)
        assert m, name
        return int(m.group(1)) << int(m.group(2) or 0)

    k, d = define("ADH_LOESS_MAX_KERNELS"), define("ADH_LOESS_MAX_DEGREE")
    assert (_abi.LOESS_MAX_KERNELS, _abi.LOESS_MAX_DEGREE) == (k, d)
    assert _abi.CALIBRATION_CHUNK_ROWS == define("ADH_CALIBRATION_CHUNK_ROWS")
    body = re.search(r"typedef struct adh_loess_model \{(.*?)\} adh_loess_model_t;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+)", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in _abi.LoessModel._fields_]
    assert C.sizeof(_abi.LoessModel) == 4 + 4 + 8 * (2 * k + (d + 1) * k)
    assert _abi.LoessModel.scale_mean.offset == 8
    assert _abi.LoessModel.scale_max.offset == 8 + 8 * k
    assert _abi.LoessModel.beta.offset == 8 + 16 * k
    m = _abi.pack_loess_model(np.arange(3.0), np.ones(3), np.arange(9.0).reshape(3, 3))
    assert (m.n_kernels, m.degree) == (3, 2) and list(m.beta[:9]) == list(range(9))  # beta[d * n_kernels + k]
