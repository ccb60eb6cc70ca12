"""Label-free quantification (directLFQ) on the matrices in HBM.

A drop-in for ``QuantBuilder.direct_lfq`` (alphadia/outputtransform/quantification/quant_builder.py:184-245): the
filtered intensity frame of ``quant.filter_frag_df`` goes in, one row per ``quant_level`` group and one float64 column
per run comes out.  ``directlfq`` itself is not at hand, so nothing here is pinned to that package:

    ``host_direct_lfq`` restates the published directLFQ method once in NumPy, with the corner decisions written out
    (DESIGN.md section 8); ``direct_lfq`` runs the same procedure on the device (alphadia_amd/csrc/adh_lfq.hip) and is
    pinned to the restatement; the restatement is pinned to hand-computed answers and invariants (tests/test_lfq.py).

Where the package turns out to differ, the restatement changes and the device follows.

The procedure, all in float64 over ``x = log2(v)`` of the float32 intensities (``v <= 0`` and NaN are missing):
rows in (group, original row) order, rows without a value removed; optionally one shift per run from ``normalize``
over the runs as traces; per group the summed intensity ``S``, ``normalize`` over the ions as traces, the per-run
median ``p`` of at least ``min_nonan`` values, and ``out = 2**(p + log2(S / sum 2**p))``.  ``normalize`` of up to
``num_samples_quadratic`` traces is ``normfacts`` - pairwise median and variance of the differences, then merging
the closest pair n-1 times; beyond that the fullest ``num_samples_quadratic`` traces are normalised that way and
every other trace is shifted onto their median trace.
"""

from __future__ import annotations

import weakref

import numpy as np
import pandas as pd

from alphadia_amd.quant import NON_RUN_COLUMNS

INF = float("inf")


# ---- the restatement ---------------------------------------------------------------------------------------------

def _log2(values: np.ndarray) -> np.ndarray:
    v = values.astype(np.float32, copy=False).astype(np.float64)
    x = np.full(v.shape, np.nan)
    pos = v > 0
    x[pos] = np.log2(v[pos])
    return x


def _median(d: np.ndarray) -> float:
    """The median of a non-empty array: the mean of the two middle values of an even count."""
    s = np.sort(d)
    c = len(s)
    return (s[(c - 1) // 2] + s[c // 2]) / 2


def _pair(a: np.ndarray, b: np.ndarray) -> tuple[float, float]:
    """Median and population variance of ``a - b`` over the positions where both are valid; ``+inf`` without one."""
    ok = ~(np.isnan(a) | np.isnan(b))
    c = int(ok.sum())
    if c == 0:
        return INF, INF
    d = a[ok] - b[ok]
    mean = d.sum() / c
    return _median(d), ((d - mean) ** 2).sum() / c


def _normfacts(T: np.ndarray, trace: list | None) -> np.ndarray:
    """One total shift per trace of ``T[m][L]``."""
    m = T.shape[0]
    dist, var = np.full((m, m), INF), np.full((m, m), INF)
    for i in range(m):
        for j in range(i + 1, m):
            dist[i, j], var[i, j] = _pair(T[i], T[j])
    merged = T.copy()
    counts = np.ones(m, dtype=np.int64)
    shift = np.zeros(m)
    anchor_of = np.full(m, -1, dtype=np.int64)
    for _ in range(m - 1):
        i, j = divmod(int(np.argmin(var)), m)  # the first minimum in row-major order
        if dist[i, j] == INF:
            break
        if trace is not None:
            two = np.partition(var.ravel(), 1)[:2] if m * m > 1 else np.array([var[i, j], INF])
            trace.append((float(two[0]), float(two[1])))
        if counts[i] >= counts[j]:
            a, s, sh = i, j, dist[i, j]
        else:
            a, s, sh = j, i, -dist[i, j]
        anchor_of[s], shift[s] = a, sh
        shifted = T[s] + sh  # the original trace
        ma = merged[a]
        new = np.where(np.isnan(ma), shifted, ma)
        both = ~np.isnan(ma) & ~np.isnan(shifted)
        new[both] = (ma[both] * counts[a] + shifted[both] * counts[s]) / (counts[a] + counts[s])
        merged[a] = new
        for k in range(m):
            lo, hi = min(a, k), max(a, k)
            if k == a or k == s or dist[lo, hi] == INF:
                continue
            dist[lo, hi], var[lo, hi] = _pair(merged[lo], merged[hi])
        dist[s, :] = dist[:, s] = INF
        var[s, :] = var[:, s] = INF
        counts[a] += 1
    total = np.zeros(m)
    for k in range(m):
        t, a = shift[k], anchor_of[k]
        while a >= 0:
            t, a = t + shift[a], anchor_of[a]
        total[k] = t
    return total


def _normalize_shifts(T: np.ndarray, q: int, trace: list | None) -> np.ndarray:
    """The shift ``normalize`` adds to every trace of ``T[m][L]``."""
    m = T.shape[0]
    if m <= q:
        return _normfacts(T, trace)
    order = np.argsort(-(~np.isnan(T)).sum(axis=1), kind="stable")
    sel = order[:q]
    shifts = np.zeros(m)
    shifts[sel] = _normfacts(T[sel], trace)
    N = T[sel] + shifts[sel][:, None]
    ref = np.full(T.shape[1], np.nan)
    for pos in range(T.shape[1]):
        col = N[:, pos]
        col = col[~np.isnan(col)]
        if len(col):
            ref[pos] = _median(col)
    for t in order[q:]:
        ok = ~(np.isnan(ref) | np.isnan(T[t]))
        if ok.any():  # (a trace without overlap stays where it is)
            shifts[t] = _median(ref[ok] - T[t][ok])
    return shifts


def run_columns(intensity_df: pd.DataFrame) -> list[str]:
    return [c for c in intensity_df.columns if c not in NON_RUN_COLUMNS]


def _frame(quant_level: str, values, runs: list[str], table: np.ndarray) -> pd.DataFrame:
    out = pd.DataFrame({quant_level: values})
    for r, name in enumerate(runs):
        out[name] = table[:, r] if len(table) else np.zeros(0)
    return out


def host_direct_lfq(intensity_df: pd.DataFrame, quant_level: str, min_nonan: int = 3,
                    num_samples_quadratic: int = 50, normalize: bool = True, trace: list | None = None) -> pd.DataFrame:
    """The directLFQ procedure of this module's docstring in NumPy: the contract of ``direct_lfq`` and the benchmark's
    baseline.  ``trace``: a list that receives, per merge step, the best and the runner-up variance."""
    runs = run_columns(intensity_df)
    R, q = len(runs), int(num_samples_quadratic)
    codes, uniques = pd.factorize(intensity_df[quant_level], sort=True)
    vals = np.empty((len(intensity_df), R), dtype=np.float32)
    for r, c in enumerate(runs):
        vals[:, r] = intensity_df[c].to_numpy()
    X = _log2(vals)
    keep = (codes >= 0) & ~np.isnan(X).all(axis=1) if R else np.zeros(len(codes), dtype=bool)
    order = np.argsort(codes, kind="stable")
    order = order[keep[order]]
    X, g = X[order], codes[order]
    if normalize and len(X):
        X = X + _normalize_shifts(np.ascontiguousarray(X.T), q, trace)[None, :]
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]]) if len(g) else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], len(g)]
    kept, rows = [], []
    for lo, hi in zip(starts, ends):
        Xg = X[lo:hi]
        S = np.exp2(Xg[~np.isnan(Xg)]).sum()
        if hi - lo > 1:
            Xg = Xg + _normalize_shifts(Xg, q, trace)[:, None]
        p = np.full(R, np.nan)
        for r in range(R):
            col = Xg[:, r]
            col = col[~np.isnan(col)]
            if len(col) and len(col) >= min_nonan:
                p[r] = _median(col)
        valid = ~np.isnan(p)
        if not valid.any():
            continue
        s = np.exp2(p[valid]).sum()
        out = np.zeros(R)
        out[valid] = np.exp2(p[valid] + np.log2(S / s))
        kept.append(g[lo])
        rows.append(out)
    table = np.array(rows).reshape(len(rows), R)
    return _frame(quant_level, uniques[np.array(kept, dtype=np.int64)], runs, table)


# ---- the device ----------------------------------------------------------------------------------------------------

class _Filtered:
    """What ``quant.filter_frag_df`` remembers of an intensity frame it returned: the resident matrices it was cut
    from and the kept rows."""

    def __init__(self, frame: pd.DataFrame, quant, column: int, runs: list[str], mask: np.ndarray):
        self.ref = weakref.ref(frame, self._drop)
        self.key = id(frame)
        self.quant, self.column, self.runs, self.mask = quant, column, runs, mask

    def _drop(self, _ref):
        if _FILTERED.get(self.key) is self:
            del _FILTERED[self.key]


_FILTERED: dict[int, _Filtered] = {}


def remember_filtered(frame: pd.DataFrame, quant, column: int, runs: list[str], mask: np.ndarray) -> None:
    f = _Filtered(frame, quant, column, runs, np.ascontiguousarray(mask, dtype=np.bool_))
    _FILTERED[f.key] = f


def _filtered(frame: pd.DataFrame, runs: list[str]) -> _Filtered | None:
    f = _FILTERED.get(id(frame))
    if (f is None or f.ref() is not frame or f.runs != runs or len(f.mask) != f.quant.n_keys
            or int(f.mask.sum()) != len(frame)):
        return None
    return f


def direct_lfq(intensity_df: pd.DataFrame, quant_level: str, *, min_nonan: int = 3, num_samples_quadratic: int = 50,
               normalize: bool = True, device: int | None = None) -> pd.DataFrame:
    """``QuantBuilder.direct_lfq`` on the GPU; returns what ``host_direct_lfq`` returns.  A frame that
    ``quant.filter_frag_df`` cut out of a resident matrix is computed in place from HBM: the row mask, the group
    codes and the result cross PCIe.  Any other frame is uploaded first."""
    from alphadia_amd import runtime

    runs = run_columns(intensity_df)
    if not runs:
        raise ValueError("direct_lfq: no run columns")
    if int(num_samples_quadratic) < 2:
        raise ValueError("direct_lfq: num_samples_quadratic must be at least 2")
    codes, uniques = pd.factorize(intensity_df[quant_level], sort=True)
    codes = codes.astype(np.int32, copy=False)
    res = _filtered(intensity_df, runs)
    if res is not None:
        quant, column, mask = res.quant, res.column, res.mask
        full = np.full(len(mask), -1, dtype=np.int32)
        full[mask] = codes
        codes = full
    else:
        quant = runtime.get_context(device).quant_matrices(1, [])
        quant.set_matrix([intensity_df[c].to_numpy().astype(np.float32, copy=False) for c in runs])
        column, mask = 0, None
    groups, table = quant.lfq(column, mask, codes, len(uniques), int(min_nonan), int(num_samples_quadratic),
                              bool(normalize))
    return _frame(quant_level, uniques[groups], runs, table)
