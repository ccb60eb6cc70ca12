"""Calibration of the spectral library with the prediction on the GPU.

Drop-in for the reference's ``CalibrationManager`` (alphadia/workflow/managers/calibration_manager.py:34-297),
``CalibrationEstimator`` (alphadia/calibration/estimator.py:19-328) and ``LOESSRegression``
(alphadia/calibration/models.py:24-366).  The fit sees at most ``calibration.max_fragments`` fragments or the
1 %-FDR precursors of a batch and stays on the host, in NumPy, taking every decision the reference takes (kernel and
degree reduction, the 0.1 / 99.9 percentile trim, uniform or density intervals, the design matrix in the input's
dtype).  The prediction touches every library row - the batch library at every optimisation step, the whole library
once the loop ends - and runs in a HIP kernel (``adh_calibration_predict``, csrc/adh_calibration.hip).
``HipCalibrationManager.predict_staged`` also leaves the calibrated fragment m/z in the library staged in HBM.

Only ``LOESSRegression`` models are supported, the only model the default configuration names; any other model name
raises ``NotImplementedError`` when the estimators are set up.  Plots are not drawn.
"""

from __future__ import annotations

import copy
import logging
import os
import pickle

import numpy as np
import pandas as pd

logger = logging.getLogger(__name__)

MZ_LIBRARY, MZ_OBSERVED, MZ_CALIBRATED = "mz_library", "mz_observed", "mz_calibrated"
RT_LIBRARY, RT_OBSERVED, RT_CALIBRATED = "rt_library", "rt_observed", "rt_calibrated"
MOBILITY_LIBRARY, MOBILITY_OBSERVED, MOBILITY_CALIBRATED = "mobility_library", "mobility_observed", "mobility_calibrated"

# CALIBRATION_GROUPS_CONFIG of the reference (calibration_manager.py:36-76)
CALIBRATION_GROUPS_CONFIG: dict = {
    "fragment": {
        "mz": {
            "input_columns": [MZ_LIBRARY],
            "target_columns": [MZ_OBSERVED],
            "output_columns": [MZ_CALIBRATED],
            "model": "LOESSRegression",
            "model_args": {"n_kernels": 2},
            "transform_deviation": "1e6",
        }
    },
    "precursor": {
        "mz": {
            "input_columns": [MZ_LIBRARY],
            "target_columns": [MZ_OBSERVED],
            "output_columns": [MZ_CALIBRATED],
            "model": "LOESSRegression",
            "model_args": {"n_kernels": 2},
            "transform_deviation": "1e6",
        },
        "rt": {
            "input_columns": [RT_LIBRARY],
            "target_columns": [RT_OBSERVED],
            "output_columns": [RT_CALIBRATED],
            "model": "LOESSRegression",
            "model_args": {"n_kernels": 6},
        },
        "mobility": {
            "input_columns": [MOBILITY_LIBRARY],
            "target_columns": [MOBILITY_OBSERVED],
            "output_columns": [MOBILITY_CALIBRATED],
            "model": "LOESSRegression",
            "model_args": {"n_kernels": 2},
        },
    },
}

_LOESS_PARAMS = ("n_kernels", "kernel_size", "polynomial_degree", "uniform")
_LOESS_FITTED = ("scale_mean", "scale_max", "beta")


def _tricube(v: np.ndarray) -> np.ndarray:
    """(1 - |v|^3)^3 + 1e-6 inside |v| <= 1, else 0 - as a product with the mask, so that NaN stays NaN."""
    a = np.abs(v)
    return (a <= 1) * ((1 - a**3) ** 3 + 1e-6)


class HipLOESSRegression:
    """``LOESSRegression`` (models.py:24-366): local polynomials of ``polynomial_degree`` on ``n_kernels`` tricubic
    kernels.  Same constructor, same attribute names (``scale_mean``, ``scale_max``, ``beta[d, k]``), so fitted
    parameters pass between the two classes.  ``fit`` runs on the host, ``predict`` on the GPU."""

    def __init__(self, n_kernels: int = 6, kernel_size: float = 2.0, polynomial_degree: int = 2, *,
                 uniform: bool = False):
        self.n_kernels = n_kernels
        self.kernel_size = kernel_size
        self.polynomial_degree = polynomial_degree
        self.uniform = uniform

    def get_params(self) -> dict:
        return {k: getattr(self, k) for k in _LOESS_PARAMS}

    @property
    def is_fitted(self) -> bool:
        return all(hasattr(self, k) for k in _LOESS_FITTED)

    # -- kernel placement (models.py:62-148) --------------------------------
    def _uniform_intervals(self, xs: np.ndarray) -> np.ndarray:
        """(start, stop) of kernels spread evenly over [xs[0], xs[-1]], widened by ``kernel_size``."""
        width = (xs[-1] - xs[0]) / self.n_kernels
        start = np.arange(xs[0], xs[-1], width) - (width / 2) * (self.kernel_size - 1)
        stop = start + width + width * (self.kernel_size - 1)
        return np.column_stack([start, stop])

    def _density_rows(self, n: int) -> np.ndarray:
        """[start, stop) rows of kernels holding equal numbers of the sorted points, widened by ``kernel_size``."""
        size = n // self.n_kernels
        start = np.arange(0, self.n_kernels) * size
        grow = (size * self.kernel_size - size) // 2
        return np.column_stack([np.maximum(0, start - grow), np.minimum(n, start + size + grow)]).astype(int)

    def _weights(self, x: np.ndarray) -> np.ndarray:
        """Normalised kernel weights of the column ``x`` (n, 1): (n, n_kernels) (models.py:302-366)."""
        v = np.tile(x, (1, self.n_kernels)) - self.scale_mean
        v = v / self.scale_max
        k = v.shape[1]
        if k == 1:
            w = np.ones(v.shape)
        else:
            w = np.empty_like(v)
            w[:, :] = _tricube(v)
            w[:, 0] = np.where(v[:, 0] < 0, 1, w[:, 0])  # first kernel open to the left
            w[:, -1] = np.where(v[:, -1] > 0, 1, w[:, -1])  # last kernel open to the right
        return w / np.sum(w, axis=1, keepdims=True)

    def _design(self, x: np.ndarray) -> np.ndarray:
        """[1, x, x^2, ...] in the column's floating dtype, each power the previous one times x (as sklearn's
        PolynomialFeatures builds it)."""
        col = x[:, 0]
        if col.dtype not in (np.float32, np.float64):
            col = col.astype(np.float64)
        out = np.empty((col.shape[0], self.polynomial_degree + 1), dtype=col.dtype)
        out[:, 0] = 1
        for d in range(1, self.polynomial_degree + 1):
            out[:, d] = col if d == 1 else out[:, d - 1] * col
        return out

    def fit(self, x, y) -> "HipLOESSRegression":
        """Fit on a single input column (models.py:150-274); the decisions are the reference's."""
        x, y = np.asarray(x), np.asarray(y)
        self.n_features_in_ = 1
        if x.ndim > 1 and x.shape[1] > 1:
            raise ValueError("Input arrays with more than one feature not yet supported.")
        n = x.size
        if n < 2:
            raise ValueError("At least two datapoints required for fitting.")
        if n < (1 + self.polynomial_degree) * self.n_kernels:
            # (a NumPy integer, as in the reference: it decides the dtype of the uniform intervals)
            self.n_kernels = np.int64(max(n // (1 + self.polynomial_degree), 1))
            logger.info("Too few points for the kernels: reduced to %d kernels.", self.n_kernels)
        if n < (1 + self.polynomial_degree) * self.n_kernels:
            self.polynomial_degree = n - 1
            logger.info("Polynomial degree reduced to %d.", self.polynomial_degree)
        if x.ndim == 1:
            x = x[:, np.newaxis]
        if y.ndim == 1:
            y = y[:, np.newaxis]

        lo, hi = np.percentile(x, [0.1, 99.9])
        inside = (lo < x[:, 0]) & (x[:, 0] < hi)
        x, y = x[inside], y[inside]
        self.n_trimmed_ = int(x.shape[0])
        xs = np.sort(x.ravel())

        uniform = bool(self.uniform)
        if uniform:
            rows = np.searchsorted(xs, self._uniform_intervals(xs)).astype(int)
            if np.any(np.diff(rows) < 1 + self.polynomial_degree):
                logger.info("Too few points per kernel: density kernels instead of uniform ones.")
                uniform = False
        self.uniform_used_ = uniform

        if uniform:
            bounds = self._uniform_intervals(xs)
            self.scale_mean = np.mean(bounds, axis=1)
            self.scale_max = np.max(bounds, axis=1) - self.scale_mean
        else:
            self.scale_mean = np.zeros(self.n_kernels)
            self.scale_max = np.zeros(self.n_kernels)
            for k, (a, b) in enumerate(self._density_rows(xs.shape[0])):
                part = xs[a:b]
                self.scale_mean[k] = part.mean()
                self.scale_max[k] = np.max(np.abs(part - self.scale_mean[k]))

        w = self._weights(x)
        design = self._design(x)
        beta = np.zeros((design.shape[1], self.n_kernels))
        for k in range(w.shape[1]):
            wk = w[:, k]
            # weighted least squares of the kernel: (X^T W X)^-1 X^T W y, the reference's normal equations
            gram = design.T * wk @ design
            beta[:, k] = np.ravel((np.linalg.inv(gram) @ design.T * wk) @ y)
        self.beta = beta
        return self

    def predict(self, x, device: int | None = None) -> np.ndarray:
        """The fitted model over ``x`` on the GPU (``adh_calibration_predict``); float64, NaN where ``x`` is NaN."""
        if not self.is_fitted:
            raise ValueError("HipLOESSRegression is not fitted")
        from alphadia_amd import runtime

        return runtime.get_context(device).calibration_predict(self, x)


def _supported_model(name: str) -> type:
    if name != "LOESSRegression":
        raise NotImplementedError(
            f"calibration model '{name}' is not supported by the HIP backend: only LOESSRegression predicts on the GPU"
        )
    return HipLOESSRegression


class HipCalibrationEstimator:
    """``CalibrationEstimator`` (estimator.py:19-328) of one property (m/z, RT, mobility) with a
    :class:`HipLOESSRegression` model."""

    def __init__(self, name: str, model: HipLOESSRegression, input_columns: list[str], target_columns: list[str],
                 output_columns: list[str], transform_deviation: None | str | float = None):
        if len(output_columns) != 1 or len(target_columns) != 1:
            raise ValueError(f"{name} calibration: only one output and target column is supported")
        self.name = name
        self._model = model
        self.input_columns = list(input_columns)
        self._target_columns = list(target_columns)
        self._output_columns = list(output_columns)
        self.transform_deviation = float(transform_deviation) if transform_deviation is not None else None
        self.is_fitted = False
        self.metrics = None

    def __repr__(self) -> str:
        return f"<HipCalibration {self.name}, is_fitted: {self.is_fitted}>"

    @property
    def model(self) -> HipLOESSRegression:
        return self._model

    def _has_columns(self, df: pd.DataFrame, columns: list[str]) -> bool:
        if not set(columns).issubset(df.columns):
            logger.warning("%s, at least one column %s not found in dataframe", self.name, set(columns))
            return False
        return True

    def fit(self, df: pd.DataFrame, *, plot: bool = False, figure_path: str | None = None) -> None:
        """Fit on the rows of ``df``; a model that cannot be fitted is logged and leaves ``is_fitted`` False."""
        if not self._has_columns(df, self.input_columns + self._target_columns):
            raise ValueError(f"{self.name} calibration fitting: failed input validation")
        try:
            self._model.fit(df[self.input_columns].to_numpy(), df[self._target_columns].to_numpy())
        except Exception as e:  # noqa: BLE001 (the reference logs any failure and goes on unfitted)
            logger.warning("Could not fit estimator %s: %s", self.name, e)
            return
        self.is_fitted = True
        self.metrics = self._get_metrics(df)

    def predict(self, df: pd.DataFrame, *, inplace: bool = True) -> np.ndarray | None:
        """Calibrated values of ``df`` (float64): written to the output column, or returned with ``inplace=False``.
        Skipped with a warning while the estimator is not fitted."""
        if not self.is_fitted:
            logger.warning("%s prediction was skipped as it has not been fitted yet", self.name)
            return None
        if not self._has_columns(df, self.input_columns):
            raise ValueError(f"{self.name} calibration prediction: failed input validation")
        values = self._model.predict(df[self.input_columns[0]].to_numpy())
        if inplace:
            df[self._output_columns[0]] = values
            return None
        return values

    def calc_deviation(self, df: pd.DataFrame) -> np.ndarray:
        """(n, 3 + inputs): observed, calibrated and residual deviation, then the input columns (estimator.py:228-291);
        deviations in ppm where ``transform_deviation`` is set."""
        inputs = df[self.input_columns].to_numpy()
        uncalibrated = inputs[:, [0]]
        target = df[self._target_columns].to_numpy()[:, [0]]
        calibrated = self.predict(df, inplace=False)
        if calibrated is None:
            raise ValueError(f"{self.name}: deviation of an estimator that is not fitted")
        calibrated = calibrated.reshape(-1, 1)
        observed_dev = target - uncalibrated
        calibrated_dev = calibrated - uncalibrated
        if self.transform_deviation is not None:
            observed_dev = observed_dev / uncalibrated * self.transform_deviation
            calibrated_dev = calibrated_dev / uncalibrated * self.transform_deviation
        return np.concatenate([observed_dev, calibrated_dev, observed_dev - calibrated_dev, inputs], axis=1)

    def _get_metrics(self, df: pd.DataFrame) -> dict[str, float]:
        dev = self.calc_deviation(df)
        return {
            "median_accuracy": float(np.median(np.abs(dev[:, 1]))),
            "median_precision": float(np.median(np.abs(dev[:, 2]))),
        }

    def ci(self, df: pd.DataFrame, ci: float = 0.95) -> float:
        """Mean absolute residual deviation at the two ends of the ``ci`` interval (estimator.py:301-327); 0 while
        not fitted."""
        if not 0 < ci < 1:
            raise ValueError("Confidence interval must be between 0 and 1")
        if not self.is_fitted:
            return 0
        residual = self.calc_deviation(df)[:, 2]
        return float(np.mean(np.abs(np.percentile(residual, [100 * (1 - ci) / 2, 100 * (1 + ci) / 2]))))

    # -- parameters --------------------------------------------------------
    def state(self) -> dict:
        m = self._model
        return {
            "params": m.get_params(),
            "fitted": {k: np.array(getattr(m, k)) for k in _LOESS_FITTED} if m.is_fitted else None,
            "is_fitted": self.is_fitted,
            "metrics": copy.deepcopy(self.metrics),
        }

    def set_state(self, state: dict) -> None:
        for k, v in state["params"].items():
            setattr(self._model, k, v)
        for k in _LOESS_FITTED:
            if hasattr(self._model, k):
                delattr(self._model, k)
        if state["fitted"] is not None:
            for k, v in state["fitted"].items():
                setattr(self._model, k, np.array(v))
        self.is_fitted = bool(state["is_fitted"])
        self.metrics = copy.deepcopy(state["metrics"])


class _LogReporter:
    """Stands in for the reference's reporting pipeline when none is given."""

    _levels = {"debug": logging.DEBUG, "info": logging.INFO, "progress": logging.INFO, "warning": logging.WARNING,
               "error": logging.ERROR, "critical": logging.CRITICAL}

    def log_string(self, value: str, verbosity: str = "info") -> None:
        logger.log(self._levels.get(verbosity, logging.INFO), value)

    def log_event(self, name: str, value: object) -> None:
        pass

    def log_metric(self, name: str, value: object) -> None:
        pass


class HipCalibrationManager:
    """``CalibrationManager`` (calibration_manager.py:79-297) whose estimators predict on the GPU.

    Constructor as the reference's at workflow/base.py:147-153.  ``save`` / ``load`` pickle the parameters of every
    estimator (not the objects) to ``path``."""

    _STATE_VERSION = 1

    def __init__(self, path: None | str = None, load_from_file: bool = True, has_ms1: bool = True,
                 has_mobility: bool = True, reporter=None, figure_path: None | str = None,
                 calibration_config: dict | None = None):
        self._path = path
        self.figure_path = figure_path
        self.reporter = _LogReporter() if reporter is None else reporter
        self._has_ms1 = has_ms1
        self._has_mobility = has_mobility
        self._plot_logged = False
        self.is_loaded_from_file = False
        self.all_fitted = False
        self.reporter.log_string(f"Initializing {self.__class__.__name__}")
        self.estimator_groups = self.setup_estimator_groups(
            CALIBRATION_GROUPS_CONFIG if calibration_config is None else calibration_config)
        if load_from_file:
            self.load()

    @property
    def path(self) -> None | str:
        return self._path

    def setup_estimator_groups(self, calibration_config: dict) -> dict[str, dict[str, HipCalibrationEstimator]]:
        """One estimator per configured property; mobility without mobility data and precursor m/z without MS1 are
        skipped (calibration_manager.py:170-191).  A model other than LOESSRegression raises NotImplementedError."""
        groups: dict[str, dict[str, HipCalibrationEstimator]] = {}
        for group_name, estimators in calibration_config.items():
            group: dict[str, HipCalibrationEstimator] = {}
            for name, params in estimators.items():
                if not self._has_mobility and name == "mobility":
                    self.reporter.log_string(f"Skipping estimator 'mobility' in group '{group_name}': no mobility data")
                    continue
                if not self._has_ms1 and group_name == "precursor" and name == "mz":
                    self.reporter.log_string(f"Skipping estimator 'mz' in group '{group_name}': no MS1 data")
                    continue
                model_type = _supported_model(params["model"])
                group[name] = HipCalibrationEstimator(
                    name=name,
                    model=model_type(**params.get("model_args", {})),
                    input_columns=params["input_columns"],
                    target_columns=params["target_columns"],
                    output_columns=params["output_columns"],
                    transform_deviation=params.get("transform_deviation", None),
                )
            groups[group_name] = group
        return groups

    def get_estimator(self, group_name: str, estimator_name: str) -> HipCalibrationEstimator | None:
        try:
            return self.estimator_groups[group_name][estimator_name]
        except KeyError:
            return None

    def fit(self, df: pd.DataFrame, group_name: str, plot: bool = True, figure_path: None | str = None) -> None:
        """Fit every estimator of ``group_name`` on ``df`` (host)."""
        if plot and not self._plot_logged:
            self.reporter.log_string("Calibration plots are not drawn by the HIP calibration manager.")
            self._plot_logged = True
        for estimator in self.estimator_groups[group_name].values():
            self.reporter.log_string(f"Fitting estimator '{estimator.name}' in calibration group '{group_name}' ..")
            estimator.fit(df)
        self.all_fitted = all(e.is_fitted for g in self.estimator_groups.values() for e in g.values())

    def predict(self, df: pd.DataFrame, group_name: str) -> None:
        """Write the calibrated columns of every estimator of ``group_name`` into ``df`` (GPU)."""
        for estimator in self.estimator_groups[group_name].values():
            self.reporter.log_string(f"Predicting estimator '{estimator.name}' in calibration group '{group_name}' ..")
            estimator.predict(df, inplace=True)

    def predict_staged(self, fragment_df: pd.DataFrame, group_name: str = "fragment", device: int | None = None,
                       only_if_staged: bool = False) -> str:
        """``predict(fragment_df, group_name)`` for the fragment m/z, with the calibrated column also put where the
        next selection or scoring constructor looks for it: in the library staged in HBM.  Returns the path taken:

        ``"skipped"``   the estimator is not fitted: as ``predict`` (a warning, nothing written, nothing staged);
        ``"in_place"``  the library staged on the context was staged from this frame's other eight columns: its
                        ``mz`` is rewritten in HBM (``adh_calibrate_staged_fragments``), nothing is uploaded;
        ``"staged"``    otherwise: the library is staged from the frame's columns and calibrated while its records are
                        packed (``adh_stage_fragments_columns``);
        ``"host"``      otherwise, with ``only_if_staged``: plain ``predict``, nothing staged.

        In every case the frame gets the ``mz_calibrated`` column ``predict`` gives it, bit for bit; after
        ``"in_place"`` and ``"staged"`` the context has adopted ``fragment_columns(fragment_df, "mz_calibrated")``, so
        staging those columns again is skipped."""
        from alphadia_amd import runtime
        from alphadia_amd.scoring import fragment_columns

        estimator = self.get_estimator(group_name, "mz")
        if estimator is None or not estimator.is_fitted:
            self.predict(fragment_df, group_name)
            return "skipped"
        if not estimator._has_columns(fragment_df, estimator.input_columns):  # noqa: SLF001
            raise ValueError(f"{estimator.name} calibration prediction: failed input validation")
        self.reporter.log_string(f"Predicting estimator '{estimator.name}' in calibration group '{group_name}' ..")
        source, output = estimator.input_columns[0], estimator._output_columns[0]  # noqa: SLF001
        ctx = runtime.get_context(device)
        columns = fragment_columns(fragment_df, source)
        eight = columns[:1] + columns[2:]
        if ctx.staged_from(*eight):
            values, path = ctx.calibrate_staged_fragments(estimator.model), "in_place"
        elif only_if_staged:
            estimator.predict(fragment_df, inplace=True)
            return "host"
        else:
            values, path = ctx.stage_fragments_calibrated(estimator.model, *eight), "staged"
        fragment_df[output] = values  # (before the columns are adopted: the key is taken from the frame's own column)
        ctx.adopt_fragment_columns(*fragment_columns(fragment_df, output))
        return path

    # -- persistence -------------------------------------------------------
    def _state(self) -> dict:
        return {
            "version": self._STATE_VERSION,
            "all_fitted": self.all_fitted,
            "groups": {g: {n: e.state() for n, e in est.items()} for g, est in self.estimator_groups.items()},
        }

    def _set_state(self, state: dict) -> None:
        for g, est in state["groups"].items():
            for n, s in est.items():
                e = self.get_estimator(g, n)
                if e is not None:
                    e.set_state(s)
        self.all_fitted = bool(state["all_fitted"])

    def save(self) -> None:
        if self.path is None:
            return
        try:
            with open(self.path, "wb") as f:
                pickle.dump(self._state(), f)
        except Exception as e:  # noqa: BLE001 (as the reference: a failed save is logged)
            self.reporter.log_string(f"Failed to save {self.__class__.__name__} to {self.path}: {e}", verbosity="error")

    @classmethod
    def is_saved_state(cls, path: str) -> bool:
        """Whether ``path`` holds what :meth:`save` writes (a parameter dict, not the pickled manager object the
        reference's ``BaseManager.load`` expects): readers of the calibration pickle, such as the run statistics
        (alphadia/outputtransform/df_builders.py:113-145), pick the manager class by it."""
        try:
            with open(path, "rb") as f:
                state = pickle.load(f)  # noqa: S301 (the caller's own calibration file)
        except Exception:  # noqa: BLE001 (a reference pickle whose classes do not import here is not ours)
            return False
        return isinstance(state, dict) and state.get("version") == cls._STATE_VERSION and "groups" in state

    def load(self) -> None:
        if self.path is None or not os.path.exists(self.path):
            self.reporter.log_string(f"{self.__class__.__name__}: no saved state, will be initialized.")
            return
        try:
            with open(self.path, "rb") as f:
                state = pickle.load(f)  # noqa: S301 (a file this class wrote)
            if not isinstance(state, dict) or state.get("version") != self._STATE_VERSION:
                self.reporter.log_string(f"{self.__class__.__name__}: {self.path} is not a saved state of this version",
                                         verbosity="warning")
                return
            self._set_state(state)
            self.is_loaded_from_file = True
            self.reporter.log_string(f"Loaded {self.__class__.__name__} from {self.path}")
        except Exception:  # noqa: BLE001
            self.reporter.log_string(f"Failed to load {self.__class__.__name__} from {self.path}", verbosity="error")

    @classmethod
    def from_reference(cls, manager, path: None | str = None, reporter=None) -> "HipCalibrationManager":
        """Adopt the LOESS parameters of a reference ``CalibrationManager`` (e.g. one loaded with
        ``reuse_calibration``): same groups, fitted flags and metrics, the models' parameters copied."""
        has_ms1 = getattr(manager, "_has_ms1", True)
        has_mobility = getattr(manager, "_has_mobility", True)
        out = cls(path=path if path is not None else getattr(manager, "path", None), load_from_file=False,
                  has_ms1=has_ms1, has_mobility=has_mobility,
                  reporter=reporter if reporter is not None else getattr(manager, "reporter", None))
        groups = {}
        for g, estimators in manager.estimator_groups.items():
            groups[g] = {}
            for n, ref in estimators.items():
                model = ref._model  # noqa: SLF001
                if type(model).__name__ != "LOESSRegression":
                    raise NotImplementedError(
                        f"estimator '{n}' of group '{g}' uses {type(model).__name__}: only LOESSRegression is supported")
                mine = HipLOESSRegression(n_kernels=model.n_kernels, kernel_size=model.kernel_size,
                                          polynomial_degree=model.polynomial_degree, uniform=model.uniform)
                for k in _LOESS_FITTED:
                    if hasattr(model, k):
                        setattr(mine, k, np.array(getattr(model, k)))
                e = HipCalibrationEstimator(name=ref.name, model=mine, input_columns=ref.input_columns,
                                            target_columns=ref._target_columns,  # noqa: SLF001
                                            output_columns=ref._output_columns,  # noqa: SLF001
                                            transform_deviation=ref.transform_deviation)
                e.is_fitted = bool(ref.is_fitted)
                e.metrics = copy.deepcopy(ref.metrics)
                groups[g][n] = e
        out.estimator_groups = groups
        out.all_fitted = bool(getattr(manager, "all_fitted", False))
        return out
