"""Protein-group FDR on the GPU: group features, the target/decoy classifier, q-values and their way back to the rows.

Drop-in for ``perform_protein_fdr`` (alphadia/outputtransform/protein_fdr.py:15-112) and the short chain of
``SearchPlanOutput._build_precursor_table`` (outputtransform/search_plan_output.py:273-334) around it.  The reference
loops in Python over ``groupby(["pg", "decoy"])`` and fits an sklearn ``MLPClassifier(random_state=0)``; here

* the host factorises ``pg`` (sorted, the way pandas sorts the group keys), ``sequence`` and ``run`` to int32 codes -
  strings never reach the device - and uploads them with ``decoy``, ``precursor_idx`` and ``proba``;
* ``adh_pfdr_features`` sorts the rows by (pg, decoy), keeping table order inside a group, and computes per group the
  row count, the distinct precursors / sequences / runs, the best and worst score and the mean score.  The mean is
  NumPy's sum in the column's own dtype - pairwise inside chunks of 8 192 elements, the chunks added in order;
  ``pairwise_sum`` states the association - so it is bit-equal to pandas' in float32 and float64;
* the train / test split and the ``StandardScaler`` are restated in NumPy on the host (a few hundred to a few
  thousand groups);
* the classifier - float64, 7 -> 100 (ReLU) -> 1 (logistic), Adam, sklearn's defaults - trains on the device, one
  launch per epoch (``adh_pfdr_epoch``), from initial weights and per-epoch permutations the host draws from
  ``np.random.RandomState(0)`` exactly as sklearn does; the host applies sklearn's stopping rule between launches;
* ``adh_fdr_q_values`` gives the q-values (ties broken by decoy, then by the sorted rank of ``pg``), scaled by
  ``n_targets / n_decoys``, and ``adh_pfdr_gather`` hands every row its group's value.

sklearn is not imported.  ``host_perform_protein_fdr`` restates the same semantics in NumPy; it is the comparator of
the tests and the benchmark, not a fallback: ``perform_protein_fdr`` needs the GPU.

Stated divergences from the reference:

* a non-finite ``proba`` in a row that belongs to a group raises ``ValueError``;
* a table whose groups hold no target, or no decoy, raises ``ValueError`` (the reference divides by zero there);
* a ``decoy`` value other than 0 or 1 in a row with a ``pg`` raises ``ValueError`` (the reference would train a
  multi-class network);
* ``figure_path`` is accepted and no plot is drawn.

Rows with a NaN ``pg`` belong to no group and come back with a NaN ``pg_qval``; the same ``pg`` string in both decoy
classes gives two groups.
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass

import numpy as np
import pandas as pd

from alphadia_amd.fdr import TooFewPSMError, train_test_indices

logger = logging.getLogger()

FEATURE_COLUMNS = ["count", "mean_score", "n_peptides", "n_precursor", "n_runs", "best_score", "worst_score"]
N_FEATURES = 7
N_HIDDEN = 100
N_PARAMS = N_FEATURES * N_HIDDEN + N_HIDDEN + N_HIDDEN + 1  # W1 [7, 100], b1 [100], W2 [100], b2

# sklearn.neural_network.MLPClassifier defaults
ALPHA = 1e-4
LEARNING_RATE = 1e-3
BETA_1, BETA_2, EPSILON = 0.9, 0.999, 1e-8
MAX_ITER = 200
TOL = 1e-4
N_ITER_NO_CHANGE = 10
BATCH = 200

# seconds / milliseconds of the stages of the last call (the benchmark reads them)
last_timing: dict[str, float] = {}
# the intermediate results of the last call (the tests read them)
last_fit: dict[str, object] = {}


class TooFewProteinsError(ValueError):
    """alphadia.exceptions.TooFewProteinsError: the train/test split of the protein groups is empty."""


# --------------------------------------------------------------------------------------------
# the mean score: NumPy's pairwise sum
# --------------------------------------------------------------------------------------------
def _pairwise_block(a: np.ndarray):
    t = a.dtype.type
    n = len(a)
    if n < 8:
        res = t(0)
        for x in a:
            res = t(res + x)
        return res
    m = n - n % 8
    r = a[:8].copy()  # eight strided accumulators
    for row in a[8:m].reshape(-1, 8):
        r += row
    res = t(t(t(r[0] + r[1]) + t(r[2] + r[3])) + t(t(r[4] + r[5]) + t(r[6] + r[7])))
    for x in a[m:]:
        res = t(res + x)
    return res


NUMPY_CHUNK = 8192  # NumPy's default buffer size (np.getbufsize()): a longer vector is summed chunk after chunk


def _pairwise(a: np.ndarray):
    if len(a) <= 128:
        return _pairwise_block(a)
    half = len(a) // 2
    half -= half % 8
    return a.dtype.type(_pairwise(a[:half]) + _pairwise(a[half:]))


def pairwise_sum(values: np.ndarray):
    """``np.add.reduce`` of a contiguous float32 / float64 vector, with its association spelled out: chunks of 8 192
    elements added one after the other, starting from zero; inside a chunk sequential below 8 elements, eight strided
    accumulators per block of up to 128, above that a split at ``n // 2`` rounded down to a multiple of 8.
    ``adh_pfdr_features`` sums in this order."""
    a = np.ascontiguousarray(values)
    t = a.dtype.type
    res = t(0)
    for start in range(0, len(a), NUMPY_CHUNK):
        res = t(res + _pairwise(a[start:start + NUMPY_CHUNK]))
    return res


# --------------------------------------------------------------------------------------------
# inputs and group features
# --------------------------------------------------------------------------------------------
@dataclass
class Inputs:
    """The columns the device works on."""

    pg: np.ndarray             # [rows] int32: rank of the row's pg among the sorted distinct pgs, -1: NaN
    pg_names: np.ndarray       # [distinct pgs] object, sorted
    decoy: np.ndarray          # [rows] uint8 (0 wherever pg is -1)
    precursor_idx: np.ndarray  # [rows] int64
    sequence: np.ndarray       # [rows] int32 codes (-1: NaN, a value like any other)
    run: np.ndarray            # [rows] int32 codes
    proba: np.ndarray          # [rows] float32 or float64


def prepare_inputs(psm_df: pd.DataFrame) -> Inputs:
    pg, names = pd.factorize(psm_df["pg"], sort=True)
    pg = pg.astype(np.int32)
    grouped = pg >= 0
    d = psm_df["decoy"].to_numpy()
    if not np.isin(d[grouped], (0, 1)).all():
        raise ValueError("protein FDR: decoy must be 0 or 1 in every row that has a pg")
    decoy = np.where(grouped, d == 1, False).astype(np.uint8)
    proba = psm_df["proba"].to_numpy()
    if proba.dtype != np.float32:
        proba = proba.astype(np.float64)
    if not np.isfinite(proba[grouped]).all():
        raise ValueError("protein FDR: proba is not finite in every row that has a pg")
    seq = pd.factorize(psm_df["sequence"])[0].astype(np.int32)
    run = pd.factorize(psm_df["run"])[0].astype(np.int32)
    return Inputs(pg, np.asarray(names, dtype=object), decoy, psm_df["precursor_idx"].to_numpy().astype(np.int64), seq,
                  run, np.ascontiguousarray(proba))


def _distinct_per_segment(values: np.ndarray, seg: np.ndarray, n_seg: int) -> np.ndarray:
    order = np.lexsort((values, seg))
    v, s = values[order], seg[order]
    new = np.ones(len(v), dtype=bool)
    new[1:] = (v[1:] != v[:-1]) | (s[1:] != s[:-1])
    return np.bincount(s[new], minlength=n_seg)


def host_group_features(inp: Inputs):
    """``(group_pg, group_decoy, features [groups, 7] float64, row_group)``: what ``adh_pfdr_features`` returns."""
    rows = np.flatnonzero(inp.pg >= 0)
    key = inp.pg[rows].astype(np.int64) * 2 + inp.decoy[rows]
    order = np.argsort(key, kind="stable")
    rows, key = rows[order], key[order]
    head = np.ones(len(rows), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    start = np.flatnonzero(head)
    n_seg = len(start)
    seg = np.cumsum(head) - 1
    row_group = np.full(len(inp.pg), -1, dtype=np.int32)
    row_group[rows] = seg
    x = np.zeros((n_seg, N_FEATURES), dtype=np.float64)
    if n_seg:
        count = np.diff(np.append(start, len(rows)))
        p = inp.proba[rows]
        t = p.dtype.type
        x[:, 0] = count
        x[:, 1] = [t(pairwise_sum(p[s:s + c]) / t(c)) for s, c in zip(start.tolist(), count.tolist())]
        x[:, 2] = _distinct_per_segment(inp.sequence[rows], seg, n_seg)
        x[:, 3] = _distinct_per_segment(inp.precursor_idx[rows], seg, n_seg)
        x[:, 4] = _distinct_per_segment(inp.run[rows], seg, n_seg)
        x[:, 5] = np.minimum.reduceat(p, start)
        x[:, 6] = np.maximum.reduceat(p, start)
    return (key[start] // 2).astype(np.int32), (key[start] % 2).astype(np.uint8), x, row_group


# --------------------------------------------------------------------------------------------
# StandardScaler
# --------------------------------------------------------------------------------------------
def standard_scaler(x_train: np.ndarray):
    """``(mean_, scale_)`` of ``sklearn.preprocessing.StandardScaler().fit``: column sums over the rows in order, the
    corrected two-pass variance, and scale 1 for a column that cannot be told from a constant."""
    x = np.asarray(x_train, dtype=np.float64)
    n = x.shape[0]
    total = np.sum(x, axis=0)
    mean = total / n
    temp = x - mean
    correction = np.sum(temp, axis=0)
    temp **= 2
    var = np.sum(temp, axis=0)
    var -= correction**2 / n
    var = var / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return mean, scale


# --------------------------------------------------------------------------------------------
# the classifier: sklearn's MLPClassifier(random_state=0), its draws on the host
# --------------------------------------------------------------------------------------------
def initial_parameters(rng: np.random.RandomState) -> np.ndarray:
    """The 901 parameters as sklearn draws them (``_init_coef``): per layer the coefficients, then the intercepts,
    uniform within ``sqrt(6 / (fan_in + fan_out))``.  Packed as W1 [7, 100] row-major, b1, W2, b2."""
    out = []
    for fan_in, fan_out in ((N_FEATURES, N_HIDDEN), (N_HIDDEN, 1)):
        bound = np.sqrt(6.0 / (fan_in + fan_out))
        coef = rng.uniform(-bound, bound, (fan_in, fan_out))
        intercept = rng.uniform(-bound, bound, fan_out)
        out.append((coef, intercept))
    (w1, b1), (w2, b2) = out
    return np.concatenate([w1.ravel(), b1, w2.ravel(), b2]).astype(np.float64)


def learning_rates(t0: int, steps: int) -> np.ndarray:
    """Adam's step size at steps ``t0 + 1 .. t0 + steps`` as sklearn computes it."""
    return np.array([LEARNING_RATE * np.sqrt(1 - BETA_2**t) / (1 - BETA_1**t) for t in range(t0 + 1, t0 + steps + 1)],
                    dtype=np.float64)


class StoppingRule:
    """``_update_no_improvement_count`` on the training loss: stop after more than ``N_ITER_NO_CHANGE`` consecutive
    epochs with ``loss > best - TOL``."""

    def __init__(self):
        self.best = np.inf
        self.stalled = 0

    def stop(self, loss: float) -> bool:
        self.stalled = self.stalled + 1 if loss > self.best - TOL else 0
        if loss < self.best:
            self.best = loss
        return self.stalled > N_ITER_NO_CHANGE


def _train(n_train: int, begin, epoch, finish):
    """The epoch loop both backends share: draws, Adam step sizes and the stopping rule on the host."""
    rng = np.random.RandomState(0)
    begin(initial_parameters(rng))
    sample_idx = np.arange(n_train)
    n_batches = -(-n_train // min(BATCH, n_train))
    rule = StoppingRule()
    curve = []
    for it in range(MAX_ITER):
        indices = np.arange(n_train)
        rng.shuffle(indices)  # sklearn.utils.shuffle: a permutation of the previous epoch's order
        sample_idx = sample_idx[indices]
        loss = float(epoch(sample_idx, learning_rates(it * n_batches, n_batches)))
        if not np.isfinite(loss):
            raise ValueError("protein FDR: the training loss is not finite")
        curve.append(loss)
        if rule.stop(loss):
            break
    return finish(), len(curve), np.asarray(curve, dtype=np.float64)


def _unpack(params):
    w1 = params[: N_FEATURES * N_HIDDEN].reshape(N_FEATURES, N_HIDDEN)
    b1 = params[N_FEATURES * N_HIDDEN: N_FEATURES * N_HIDDEN + N_HIDDEN]
    w2 = params[N_FEATURES * N_HIDDEN + N_HIDDEN: N_PARAMS - 1].reshape(N_HIDDEN, 1)
    b2 = params[N_PARAMS - 1:]
    return w1, b1, w2, b2


def _expit(z):
    return 1.0 / (1.0 + np.exp(-z))


def host_predict(params: np.ndarray, x: np.ndarray, dot=np.matmul) -> np.ndarray:
    w1, b1, w2, b2 = _unpack(params)
    h = np.maximum(dot(x, w1) + b1, 0)
    return _expit(dot(h, w2) + b2)[:, 0]


def host_fit_predict(x_train: np.ndarray, y_train: np.ndarray, x_all: np.ndarray, dot=np.matmul):
    """sklearn's ``MLPClassifier(random_state=0).fit(x_train, y_train).predict_proba(x_all)[:, 1]`` in NumPy float64:
    ``(proba, n_iter, loss_curve)``.  ``dot`` is the matrix product (the golden recipe swaps its association)."""
    x_train = np.ascontiguousarray(x_train, dtype=np.float64)
    y = np.asarray(y_train, dtype=np.float64).reshape(-1, 1)
    n = x_train.shape[0]
    batch = min(BATCH, n)
    state: dict[str, np.ndarray] = {}
    eps = np.finfo(np.float64).eps

    def begin(params):
        state["p"] = params.copy()
        state["m"] = np.zeros(N_PARAMS)
        state["v"] = np.zeros(N_PARAMS)

    def epoch(sample_idx, lrs):
        accumulated = 0.0
        for k, start in enumerate(range(0, n, batch)):
            idx = sample_idx[start:start + batch]
            xb, yb = x_train[idx], y[idx]
            nb = len(idx)
            w1, b1, w2, b2 = _unpack(state["p"])
            h = np.maximum(dot(xb, w1) + b1, 0)
            p = _expit(dot(h, w2) + b2)
            pc = np.clip(p, eps, 1 - eps)
            with np.errstate(divide="ignore", invalid="ignore"):
                ll = np.where(yb != 0, yb * np.log(pc), 0.0) + np.where(yb != 1, (1 - yb) * np.log(1 - pc), 0.0)
            loss = -np.mean(ll, axis=0).sum()
            loss += (0.5 * ALPHA) * (np.dot(w1.ravel(), w1.ravel()) + np.dot(w2.ravel(), w2.ravel())) / nb
            accumulated += loss * nb
            delta2 = p - yb
            g_w2 = (dot(h.T, delta2) + ALPHA * w2) / nb
            g_b2 = np.mean(delta2, 0)
            delta1 = dot(delta2, w2.T)
            delta1[h == 0] = 0
            g_w1 = (dot(xb.T, delta1) + ALPHA * w1) / nb
            g_b1 = np.mean(delta1, 0)
            g = np.concatenate([g_w1.ravel(), g_b1, g_w2.ravel(), g_b2])
            state["m"] = BETA_1 * state["m"] + (1 - BETA_1) * g
            state["v"] = BETA_2 * state["v"] + (1 - BETA_2) * (g**2)
            state["p"] = state["p"] + (-lrs[k] * state["m"] / (np.sqrt(state["v"]) + EPSILON))
        return accumulated / n

    def finish():
        return host_predict(state["p"], np.ascontiguousarray(x_all, dtype=np.float64), dot)

    return _train(n, begin, epoch, finish)


def device_fit_predict(x_train: np.ndarray, y_train: np.ndarray, x_all: np.ndarray, device: int | None = None,
                       session=None):
    """The same training with every epoch on the GPU (``adh_pfdr_fit_begin`` / ``_epoch`` / ``_predict``)."""
    from alphadia_amd import runtime

    own = session is None
    s = runtime.get_context(device).protein_fdr() if own else session
    try:
        return _train(len(x_train), lambda params: s.fit_begin(x_train, y_train, params), s.epoch,
                      lambda: s.predict(x_all))
    finally:
        if own:
            s.close()


# --------------------------------------------------------------------------------------------
# q-values
# --------------------------------------------------------------------------------------------
def host_q_values(score: np.ndarray, decoy: np.ndarray, tiebreak: np.ndarray):
    """``(order, qval)`` as ``adh_fdr_q_values`` returns them."""
    order = np.lexsort((tiebreak, decoy, score))
    d = decoy[order].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fdr = np.cumsum(d) / np.cumsum(1 - d)
    return order, np.flip(np.minimum.accumulate(np.flip(fdr)))


# --------------------------------------------------------------------------------------------
# the chain
# --------------------------------------------------------------------------------------------
class _HostBackend:
    def features(self, inp):
        *out, self._row_group = host_group_features(inp)
        return out

    def fit_predict(self, x_train, y_train, x_all):
        return host_fit_predict(x_train, y_train, x_all)

    def q_values(self, score, decoy, rank):
        return host_q_values(score, decoy, rank)

    def gather(self, group_qval):
        out = np.full(len(self._row_group), np.nan)
        has = self._row_group >= 0
        out[has] = group_qval[self._row_group[has]]
        return out

    def timing(self):
        return {}

    def close(self):
        pass


class _DeviceBackend:
    def __init__(self, device):
        from alphadia_amd import runtime

        self._ctx = runtime.get_context(device)
        self._s = self._ctx.protein_fdr()

    def features(self, inp):
        return self._s.features(inp.pg, inp.decoy, inp.precursor_idx, inp.sequence, inp.run, inp.proba)

    def fit_predict(self, x_train, y_train, x_all):
        return device_fit_predict(x_train, y_train, x_all, session=self._s)

    def q_values(self, score, decoy, rank):
        return self._ctx.fdr_q_values(score, decoy, rank)

    def gather(self, group_qval):
        return self._s.gather(group_qval)

    def timing(self):
        features_ms, epochs_ms, predict_ms, gather_ms = self._s.time_ms()
        return dict(features_ms=features_ms, epochs_ms=epochs_ms, predict_ms=predict_ms, gather_ms=gather_ms)

    def close(self):
        self._s.close()


def _perform(psm_df: pd.DataFrame, backend) -> pd.DataFrame:
    last_timing.clear()
    last_fit.clear()
    try:
        t0 = time.perf_counter()
        inp = prepare_inputs(psm_df)
        if not (inp.pg >= 0).any():
            raise TooFewProteinsError("protein FDR: no row of the table has a pg")
        t1 = time.perf_counter()
        group_pg, group_decoy, x = backend.features(inp)
        t2 = time.perf_counter()
        n_groups = len(group_pg)
        try:
            idx_train, idx_test = train_test_indices(n_groups, 0.2, 42)
        except TooFewPSMError as e:
            raise TooFewProteinsError(str(e)) from e
        n_decoys = int(group_decoy.sum())
        n_targets = n_groups - n_decoys
        if n_targets == 0 or n_decoys == 0:
            raise ValueError(f"protein FDR: the table holds {n_targets} target and {n_decoys} decoy protein groups")
        mean, scale = standard_scaler(x[idx_train])
        x_scaled = (x - mean) / scale
        t3 = time.perf_counter()
        proba, n_iter, curve = backend.fit_predict(x_scaled[idx_train], group_decoy[idx_train], x_scaled)
        t4 = time.perf_counter()
        order, qval = backend.q_values(proba, group_decoy, group_pg.astype(np.int64))
        group_qval = np.empty(n_groups, dtype=np.float64)
        group_qval[order] = qval * np.int64(n_targets) / np.int64(n_decoys)
        t5 = time.perf_counter()
        row_qval = backend.gather(group_qval)
        parts = []
        d = psm_df["decoy"].to_numpy()
        for c in (0, 1):
            mask = d == c
            part = psm_df[mask].reset_index(drop=True)
            part["pg_qval"] = row_qval[mask]
            parts.append(part)
        out = pd.concat(parts)
        t6 = time.perf_counter()
        logger.info(f"Normalizing q-values using {n_targets:,} targets and {n_decoys:,} decoys")
        last_timing.update(prepare_s=t1 - t0, features_s=t2 - t1, scale_s=t3 - t2, train_s=t4 - t3, qvalues_s=t5 - t4,
                           gather_s=t6 - t5, total_s=t6 - t0, rows=len(psm_df), groups=n_groups, epochs=n_iter,
                           epoch_s=(t4 - t3) / max(n_iter, 1), **backend.timing())
        last_fit.update(group_pg=group_pg, group_decoy=group_decoy, features=x, idx_train=idx_train, idx_test=idx_test,
                        mean=mean, scale=scale, x_scaled=x_scaled, n_iter=n_iter, loss_curve=curve, proba=proba,
                        group_qval=group_qval, pg_names=inp.pg_names)
        return out
    finally:
        backend.close()


def perform_protein_fdr(psm_df: pd.DataFrame, figure_path: str | None = None, device: int | None = None):
    """``perform_protein_fdr`` with the group features, the classifier, the q-values and the gather on the GPU.

    Parameters
    ----------
    psm_df : pd.DataFrame
        Precursor table with ``pg``, ``decoy``, ``precursor_idx``, ``sequence``, ``run`` and ``proba`` (float32 or
        float64).
    figure_path : str | None
        Accepted; no plot is drawn.
    device : int | None
        GPU ordinal (default: the process's, ``runtime.default_device``).

    Returns the target rows in table order, then the decoy rows, each part with its own RangeIndex, and ``pg_qval``
    (float64) as the last column.
    """
    return _perform(psm_df, _DeviceBackend(device))


def host_perform_protein_fdr(psm_df: pd.DataFrame, figure_path: str | None = None):
    """``perform_protein_fdr`` restated on the host in NumPy, for comparison."""
    return _perform(psm_df, _HostBackend())


def build_precursor_table(psm_df: pd.DataFrame, inference_strategy: str, group_level: str, fdr: float,
                          keep_decoys: bool, device: int | None = None) -> pd.DataFrame:
    """The device stages of ``_build_precursor_table`` (search_plan_output.py:309-325): protein inference, protein
    FDR, the ``pg_qval <= fdr`` filter and the decoy drop.  ``prepare_psm_dataframe`` stays with the caller."""
    from alphadia_amd.grouping import apply_protein_inference

    psm_df = apply_protein_inference(psm_df, inference_strategy, group_level, device=device)
    psm_df = perform_protein_fdr(psm_df, None, device=device)
    psm_df = psm_df[psm_df["pg_qval"] <= fdr]
    if not keep_decoys:
        psm_df = psm_df[psm_df["decoy"] == 0]
    return psm_df
