"""Golden vectors of the library calibration, produced by RUNNING THE REFERENCE's ``LOESSRegression``
(alphadia/calibration/models.py) and ``CalibrationEstimator`` (alphadia/calibration/estimator.py) in the build
container:

    python tests/golden/make_golden_calibration.py

TEST INFRASTRUCTURE, same rules as make_golden.py: the reference is imported from /root/reference (it needs numpy
and sklearn only), fed seeded synthetic calibration data, and inputs + outputs are stored in
``tests/golden/calibration.npz``.  Per case ``<c>``:

    <c>/x_train, <c>/y_train        training columns (float32 or float64, the case's dtype)
    <c>/query, <c>/query_nan        query columns: 10 % beyond the training range on both sides; with NaN rows
    <c>/scale_mean, scale_max, beta the reference's fitted parameters (fit_ok cases)
    <c>/pred, <c>/pred_nan          the reference's predictions of the queries
    <c>/meta                        JSON: model arguments, the fit's decisions (n_kernels, degree, uniform or
                                    density intervals, rows left by the trim), fit_ok, metrics, ci(0.95)

The reference's ``predict`` rejects NaN inputs (sklearn's input check of PolynomialFeatures); ``pred_nan`` holds its
prediction of the finite rows and NaN at the NaN rows, which is what its arithmetic gives them.
"""

from __future__ import annotations

import json
import logging
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
REFERENCE_ROOT = "/root/reference"
sys.path.insert(0, REFERENCE_ROOT)

from alphadia.calibration.estimator import CalibrationEstimator  # noqa: E402
from alphadia.calibration.models import LOESSRegression  # noqa: E402


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.messages: list[str] = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def _data(kind: str, rng, n: int, dtype):
    if kind == "mz":
        x = rng.uniform(150.0, 2000.0, n)
        y = x * (1 + 8e-6 + 3e-6 * np.sin(x / 300.0)) + rng.normal(0, 1, n) * x * 2e-6
    elif kind == "rt":
        x = rng.uniform(0.0, 7200.0, n)
        y = x * 1.02 + 60.0 * np.sin(x / 1500.0) + rng.normal(0, 10.0, n)
    elif kind == "mobility":
        x = rng.uniform(0.6, 1.6, n)
        y = x * 1.01 + 0.005 + rng.normal(0, 0.005, n)
    elif kind == "gap":  # two clusters: uniform kernels in the gap hold no points
        x = np.concatenate([rng.uniform(0.0, 100.0, n // 2), rng.uniform(900.0, 1000.0, n - n // 2)])
        y = x + 5.0 + rng.normal(0, 0.5, n)
    else:
        raise ValueError(kind)
    return x.astype(dtype), y.astype(dtype)


# name: (data kind, rows, dtype, LOESSRegression arguments, transform_deviation, outliers)
CASES = {
    "mz_f32": ("mz", 5000, np.float32, dict(n_kernels=2), 1e6, False),
    "mz_f64": ("mz", 5000, np.float64, dict(n_kernels=2), 1e6, False),
    "mz_f32_outliers": ("mz", 4000, np.float32, dict(n_kernels=2), 1e6, True),
    "rt_f32": ("rt", 5000, np.float32, dict(n_kernels=6), None, False),
    "rt_f64": ("rt", 5000, np.float64, dict(n_kernels=6), None, False),
    "mobility_f32": ("mobility", 3000, np.float32, dict(n_kernels=2), None, False),
    "rt_f64_one_kernel": ("rt", 2000, np.float64, dict(n_kernels=1), None, False),
    "rt_f64_uniform": ("rt", 3000, np.float64, dict(n_kernels=6, uniform=True), None, False),
    "rt_f32_uniform": ("rt", 3000, np.float32, dict(n_kernels=6, uniform=True), None, False),
    "gap_f64_uniform_fallback": ("gap", 2000, np.float64, dict(n_kernels=6, uniform=True), None, False),
    "mz_f64_reduce_kernels": ("mz", 10, np.float64, dict(n_kernels=6), 1e6, False),
    "rt_f64_reduce_degree": ("rt", 4, np.float64, dict(n_kernels=6, polynomial_degree=4), None, False),
    "rt_f64_two_points": ("rt", 2, np.float64, dict(n_kernels=6), None, False),
}


def run_case(name, spec, rng, out):
    kind, n, dtype, args, transform, outliers = spec
    x, y = _data(kind, rng, n, dtype)
    if outliers:  # three rows beyond each end, with wild targets: the 0.1 / 99.9 percentile trim removes them
        x = np.concatenate([x, np.array([20.0, 25.0, 30.0, 5000.0, 5100.0, 5200.0], dtype=dtype)])
        y = np.concatenate([y, np.array([500.0, -200.0, 40.0, 1.0, 9000.0, 7000.0], dtype=dtype)])
    lo, hi = float(np.nanmin(x)), float(np.nanmax(x))
    span = hi - lo
    query = np.concatenate([np.linspace(lo - 0.1 * span, hi + 0.1 * span, 1500), rng.uniform(lo, hi, 500)]).astype(dtype)
    query_nan = query[:64].copy()
    query_nan[::5] = np.nan

    model = LOESSRegression(**args)
    trimmed: list[int] = []
    weight_matrix = model._get_weight_matrix  # noqa: SLF001
    model._get_weight_matrix = lambda v: (trimmed.append(v.shape[0]) if not trimmed else None, weight_matrix(v))[1]  # noqa: SLF001
    cap = _Capture()
    root = logging.getLogger()
    root.addHandler(cap)
    root.setLevel(logging.INFO)
    df = pd.DataFrame({"x": x, "y": y})
    est = CalibrationEstimator(name=name, model=model, input_columns=["x"], target_columns=["y"],
                               output_columns=["x_calibrated"], transform_deviation=transform)
    try:
        est.fit(df, plot=False)
    finally:
        root.removeHandler(cap)
    model._get_weight_matrix = weight_matrix  # noqa: SLF001
    fit_ok = bool(est.is_fitted)
    meta = dict(
        model_args=args,
        transform_deviation=transform,
        dtype=np.dtype(dtype).name,
        fit_ok=fit_ok,
        n_kernels=int(model.n_kernels),
        polynomial_degree=int(model.polynomial_degree),
        uniform_used=bool(args.get("uniform", False)) and not any("Uniform kernels will be replaced" in m for m in cap.messages),
        n_trimmed=int(trimmed[0]) if trimmed else None,
    )
    out[f"{name}/x_train"] = x
    out[f"{name}/y_train"] = y
    out[f"{name}/query"] = query
    out[f"{name}/query_nan"] = query_nan
    if fit_ok:
        meta["metrics"] = est.metrics
        meta["ci95"] = est.ci(df, 0.95)
        out[f"{name}/scale_mean"] = np.asarray(model.scale_mean, dtype=np.float64)
        out[f"{name}/scale_max"] = np.asarray(model.scale_max, dtype=np.float64)
        out[f"{name}/beta"] = np.asarray(model.beta, dtype=np.float64)
        out[f"{name}/pred"] = model.predict(query)
        finite = ~np.isnan(query_nan)
        pred_nan = np.full(query_nan.shape[0], np.nan)
        pred_nan[finite] = model.predict(query_nan[finite])
        try:
            model.predict(query_nan)
            meta["reference_rejects_nan"] = False
        except ValueError:
            meta["reference_rejects_nan"] = True
        out[f"{name}/pred_nan"] = pred_nan
    out[f"{name}/meta"] = np.array(json.dumps(meta))
    print(f"{name}: {json.dumps(meta)}")


def main():
    rng = np.random.default_rng(20261015)
    out: dict[str, np.ndarray] = {}
    for name, spec in CASES.items():
        run_case(name, spec, rng, out)
    out["cases"] = np.array(list(CASES))
    path = os.path.join(OUT_DIR, "calibration.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
