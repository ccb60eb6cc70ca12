"""The transfer-learning library of the output stage on the GPU: top-k runs per peptide, RT normalisation, MS2 QC.

Drop-in for ``TransferLearningAccumulator``, ``normalize_rt_max``, ``normalize_rt_delta_max`` and
``ms2_quality_control`` (alphadia/outputtransform/outputaccumulator.py:272-540) and, through ``add_run``, for
``build_speclibflat_from_quant`` (:42-159) without alphabase.  The reference re-sorts the whole consensus frame once
per run and walks the precursors one at a time in the quality control; here

* ``HipTransferLearningAccumulator.update`` uploads the new run's key columns (``mod_seq_hash``, ``proba``,
  ``precursor_idx``, ``frag_start_idx``, ``frag_stop_idx``) and dense matrices; ``adh_tl_update`` orders "consensus,
  then the new run" by (mod_seq_hash, proba, precursor_idx) with stable radix passes, keeps the first ``keep_top``
  rows of every hash, drops the dense rows of the others and renumbers the kept blocks.  The consensus' keys and
  matrices stay in HBM; the host gets the kept rows as an index and truncates its own frame (strings and every other
  column) with it;
* ``add_run`` builds a run's dense matrices on the device from the flat fragment table (``adh_tl_scatter``);
* ``ms2_quality_control`` is one kernel over all precursors (``adh_tl_qc``): a wavefront per precursor, the masked
  median by rank counting in an LDS slice of ``QC_LDS_SLICE`` values, the product ``intensity * (correlation >
  median * ratio)``; blocks with more masked cells take a workgroup path of any size;
* ``normalize_rt_max`` / ``normalize_rt_delta_max`` are two max reductions and the elementwise formula in the dtype
  NumPy's promotion gives (``adh_tl_rt_norm``).

alphabase is not imported.  ``consensus_speclibase`` is a ``ConsensusLibrary``: ``precursor_df``, the dense frames
under alphabase's names and ``available_dense_fragment_dfs()``.  Its index is a RangeIndex after every update.

``host_update``, ``host_ms2_quality_control``, ``host_normalize_rt_max`` / ``_delta_max`` and ``host_scatter_dense``
restate the same semantics in NumPy; they are the comparators of the tests and the benchmark, not fallbacks: the
public classes and functions need the GPU.

Pinned to these restatements only (alphabase's source is not at hand): the dropping and renumbering of unused fragment
rows (``remove_unused_fragments``: the kept blocks in the order of their old ``frag_start_idx``, one block per
precursor) and the flat-to-dense mapping of ``add_run`` (``to_speclib_base``).

The blocks ``[frag_start_idx, frag_stop_idx)`` of a library must not overlap (they do not after an update); the
quality control raises ``ValueError`` otherwise, where the reference would let a later precursor see the intensities
an earlier one masked.
"""

from __future__ import annotations

import logging
import time

import numpy as np
import pandas as pd

from alphadia_amd import _abi

logger = logging.getLogger()

QC_LDS_SLICE = _abi.TL_QC_SLICE  # masked cells of a block the wavefront path of adh_tl_qc holds
KEY_COLUMNS = ("mod_seq_hash", "proba", "precursor_idx")
FLAT_DENSE = ("_fragment_mz_df", "_fragment_intensity_df", "_fragment_correlation_df")  # the matrices add_run builds
RT_OBSERVED, RT_CALIBRATED, RT_LIBRARY = "rt_observed", "rt_calibrated", "rt_library"

# alphabase's codes of the flat fragment table: the series letter's code point, the mass of the neutral loss
LOSS_NAMES = {0: "", 18: "H2O", 17: "NH3", 1: "lossH", 2: "addH", 98: "modloss"}

# seconds / milliseconds of the stages of the last call (the benchmark reads them)
last_timing: dict[str, float] = {}


# --------------------------------------------------------------------------------------------
# the light library object
# --------------------------------------------------------------------------------------------
class ConsensusLibrary:
    """What the accumulator hands out as ``consensus_speclibase``: ``_precursor_df`` / ``precursor_df``, the dense
    frames under alphabase's names (``_fragment_mz_df``, ``fragment_mz_df``, ...) and
    ``available_dense_fragment_dfs()``.  A dense frame that is still in HBM is fetched when it is first read."""

    def __init__(self, precursor_df: pd.DataFrame, names, columns, frames=None, fetch=None):
        self._precursor_df = precursor_df
        self._names = list(names)
        self._columns = list(columns)
        self._fetch = fetch
        for name, frame in (frames or {}).items():
            setattr(self, name, frame)

    def __getattr__(self, name):  # (only reached when the attribute is not set)
        d = self.__dict__
        if name in d.get("_names", ()) and d.get("_fetch") is not None:
            frame = pd.DataFrame(d["_fetch"](d["_names"].index(name)), columns=d["_columns"])
            setattr(self, name, frame)
            return frame
        if not name.startswith("_") and name.startswith("fragment_") and "_" + name in d.get("_names", ()):
            return getattr(self, "_" + name)
        raise AttributeError(name)

    @property
    def precursor_df(self) -> pd.DataFrame:
        return self._precursor_df

    @precursor_df.setter
    def precursor_df(self, df: pd.DataFrame):
        self._precursor_df = df

    def available_dense_fragment_dfs(self) -> list[str]:
        return list(self._names)


def _run_parts(speclibase):
    """``(precursor_df, names, columns, matrices)`` of a library object, checked."""
    if hasattr(speclibase, "hash_precursor_df"):
        speclibase.hash_precursor_df()
    df = speclibase.precursor_df
    missing = [c for c in (*KEY_COLUMNS, "frag_start_idx", "frag_stop_idx") if c not in df.columns]
    if missing:
        raise ValueError(f"transfer library: precursor_df lacks {missing}")
    names = list(speclibase.available_dense_fragment_dfs())
    if not 1 <= len(names) <= _abi.TL_MAX_MATRICES:
        raise ValueError(f"transfer library: 1 to {_abi.TL_MAX_MATRICES} dense fragment frames, not {len(names)}")
    frames = [getattr(speclibase, n) for n in names]
    columns = list(frames[0].columns)
    mats = []
    for n, f in zip(names, frames):
        if list(f.columns) != columns or f.shape != frames[0].shape:
            raise ValueError(f"transfer library: {n} differs from {names[0]} in shape or columns")
        m = f.to_numpy()
        if m.dtype != np.float32:
            raise TypeError(f"transfer library: {n} must be float32, not {m.dtype}")
        mats.append(np.ascontiguousarray(m))
    return df, names, columns, mats


def _same_layout(cons: ConsensusLibrary, names, columns):
    if cons._names != list(names) or cons._columns != list(columns):
        raise ValueError("transfer library: the run's dense frames differ from the consensus' in names or columns")


def _truncate(cons_df, run_df, kept, start, stop) -> pd.DataFrame:
    """The kept rows of "consensus, then the new run" with their renumbered blocks and a RangeIndex."""
    df = run_df.reset_index(drop=True) if cons_df is None else pd.concat([cons_df, run_df], ignore_index=True)
    out = df.iloc[kept].reset_index(drop=True)
    out["frag_start_idx"] = start.astype(df["frag_start_idx"].dtype)
    out["frag_stop_idx"] = stop.astype(df["frag_stop_idx"].dtype)
    return out


# --------------------------------------------------------------------------------------------
# host restatements
# --------------------------------------------------------------------------------------------
def host_top_k(mod_seq_hash, proba, precursor_idx, keep_top: int) -> np.ndarray:
    """The rows ``sort_values([mod_seq_hash, proba, precursor_idx])`` + ``_get_top_indices_from_freq`` keep, in their
    sorted order: a stable sort (NaN proba last), the first ``keep_top`` rows of every hash."""
    order = np.lexsort((np.asarray(precursor_idx), np.asarray(proba), np.asarray(mod_seq_hash)))
    h = np.asarray(mod_seq_hash)[order]
    pos = np.arange(len(h))
    head = np.ones(len(h), dtype=bool)
    head[1:] = h[1:] != h[:-1]
    seg_start = np.maximum.accumulate(np.where(head, pos, 0))
    return order[pos - seg_start < keep_top]


def host_drop_unused(start, stop, matrices):
    """``(new_start, new_stop, matrices)``: the blocks ``[start, stop)`` by ascending old start (ties in row order),
    renumbered by an exclusive scan of their lengths; every other dense row leaves."""
    start, stop = np.asarray(start, np.int64), np.asarray(stop, np.int64)
    order = np.argsort(start, kind="stable")
    length = (stop - start)[order]
    ns = np.cumsum(length) - length
    new_start = np.empty_like(start)
    new_start[order] = ns
    new_stop = new_start + (stop - start)
    src = np.repeat(start[order] - ns, length) + np.arange(int(length.sum()))
    return new_start, new_stop, [m[src] for m in matrices]


def host_update(consensus: ConsensusLibrary | None, speclibase, keep_top: int = 3) -> ConsensusLibrary:
    """``TransferLearningAccumulator.update`` in NumPy: the new consensus (``consensus`` None: the first run)."""
    run_df, names, columns, mats = _run_parts(speclibase)
    if consensus is None:
        cons_df, key_df, rows0 = None, run_df, 0
    else:
        _same_layout(consensus, names, columns)
        cons_df = consensus.precursor_df
        rows0 = len(getattr(consensus, names[0]))
        mats = [np.concatenate([getattr(consensus, n).to_numpy(), m]) for n, m in zip(names, mats)]
        key_df = pd.concat([cons_df[list(KEY_COLUMNS)], run_df[list(KEY_COLUMNS)]], ignore_index=True)
    start = run_df["frag_start_idx"].to_numpy().astype(np.int64) + rows0
    stop = run_df["frag_stop_idx"].to_numpy().astype(np.int64) + rows0
    if consensus is not None:
        start = np.concatenate([cons_df["frag_start_idx"].to_numpy().astype(np.int64), start])
        stop = np.concatenate([cons_df["frag_stop_idx"].to_numpy().astype(np.int64), stop])
    kept = host_top_k(key_df["mod_seq_hash"].to_numpy(), key_df["proba"].to_numpy(), key_df["precursor_idx"].to_numpy(),
                      keep_top)
    new_start, new_stop, mats = host_drop_unused(start[kept], stop[kept], mats)
    frames = {n: pd.DataFrame(m, columns=columns) for n, m in zip(names, mats)}
    return ConsensusLibrary(_truncate(cons_df, run_df, kept, new_start, new_stop), names, columns, frames)


def host_normalize_rt_max(lib):
    df = lib.precursor_df
    df["rt_norm"] = df[RT_OBSERVED] / df[RT_OBSERVED].max()
    return lib


def host_normalize_rt_delta_max(lib):
    df = lib.precursor_df
    obs, cal, library = df[RT_OBSERVED].values, df[RT_CALIBRATED].values, df[RT_LIBRARY].values
    with np.errstate(invalid="ignore", divide="ignore"):
        max_norm = obs / np.max(obs)
        deviation_from_calib = (obs - cal) / cal
        calibrated_norm = library * (1 + deviation_from_calib)
        calibrated_norm = calibrated_norm / calibrated_norm.max()
        df["rt_norm"] = (1 - max_norm) * calibrated_norm + max_norm * max_norm
    return lib


def _qc_parts(lib):
    df = lib.precursor_df
    start = df["frag_start_idx"].to_numpy().astype(np.int64)
    stop = df["frag_stop_idx"].to_numpy().astype(np.int64)
    inten, corr = lib.fragment_intensity_df, lib._fragment_correlation_df
    if inten.shape != corr.shape:
        raise ValueError("ms2_quality_control: intensity and correlation frames differ in shape")
    if len(start) and (start.min() < 0 or (stop < start).any() or stop.max() > len(inten)):
        raise ValueError("ms2_quality_control: fragment rows outside the dense frames")
    order = np.argsort(start, kind="stable")
    if (stop[order][:-1] > start[order][1:]).any():
        raise ValueError("ms2_quality_control: the fragment blocks of two precursors overlap")
    return df, start, stop, inten, corr


def host_ms2_quality_control(lib, precursor_correlation_cutoff: float = 0.5, fragment_correlation_ratio: float = 0.75,
                             looped: bool = False):
    """``ms2_quality_control`` in NumPy.  ``looped``: one precursor at a time with ``np.median``, as the reference
    walks them (on array slices, not through ``DataFrame.iloc``); otherwise the same values from one segmented pass
    (sort the masked correlations by (block, value), take the middle ones)."""
    df, start, stop, inten_df, corr_df = _qc_parts(lib)
    cutoff, ratio = precursor_correlation_cutoff, fragment_correlation_ratio
    inten, corr = inten_df.to_numpy(), corr_df.to_numpy()
    use = np.zeros(len(df), dtype=bool)
    out = inten.copy()
    if looped:
        with np.errstate(invalid="ignore"):
            for i, (a, b) in enumerate(zip(start.tolist(), stop.tolist())):
                fc, fi = corr[a:b], inten[a:b]
                mask = fi.flatten() > 0.0
                median = np.median(fc.flatten()[mask]) if mask.any() else 0.0
                use[i] = median > cutoff
                out[a:b] = fi * (fc > median * ratio)
    else:
        C = inten.shape[1]
        n_cell = (stop - start) * C
        seg = np.repeat(np.arange(len(df)), n_cell)
        first = np.cumsum(n_cell) - n_cell
        cell = np.arange(int(n_cell.sum())) - np.repeat(first, n_cell) + np.repeat(start * C, n_cell)
        fi, fc = inten.reshape(-1)[cell], corr.reshape(-1)[cell]
        with np.errstate(invalid="ignore"):
            masked = fi > 0.0
        ms, mc = seg[masked], fc[masked]
        order = np.lexsort((mc, ms))  # NaN last inside its block
        ms, mc = ms[order], mc[order]
        n = np.bincount(ms, minlength=len(df))
        lo = np.cumsum(n) - n
        has = n > 0
        t = corr.dtype.type
        median = np.zeros(len(df), dtype=corr.dtype)
        a, b = mc[(lo + (n - 1) // 2)[has]], mc[(lo + n // 2)[has]]
        with np.errstate(invalid="ignore", over="ignore"):
            median[has] = np.where(n[has] % 2 == 1, a, (a + b) / t(2))
            median[has] = np.where(np.isnan(mc[(lo + n - 1)[has]]), t(np.nan), median[has])
            use = np.where(has, median > t(cutoff), 0.0 > cutoff)
            thr = np.where(has, median * t(ratio), t(0.0 * ratio))
            out.reshape(-1)[cell] = fi * (fc > np.repeat(thr, n_cell))
    inten_df.iloc[:, :] = out
    df["use_for_ms2"] = use
    return lib


def fragment_column_index(frag_type, loss_type, charge, charged_frag_types) -> np.ndarray:
    """The column of every flat fragment row in ``charged_frag_types`` (-1: none): ``type`` is the series letter's code
    point, ``loss_type`` one of ``LOSS_NAMES``; the names read ``b_z1``, ``y_H2O_z2``, ``b_modloss_z1``."""
    table = {}
    for k, name in enumerate(charged_frag_types):
        parts = name.split("_")
        if len(parts) not in (2, 3) or len(parts[0]) != 1 or not parts[-1].startswith("z"):
            raise ValueError(f"charged fragment type {name!r} is not <series>[_<loss>]_z<charge>")
        table[(ord(parts[0]), parts[1] if len(parts) == 3 else "", int(parts[-1][1:]))] = k
    ft, lt, ch = (np.asarray(x).astype(np.int64) for x in (frag_type, loss_type, charge))
    out = np.full(len(ft), -1, dtype=np.int32)
    combos, inverse = np.unique(np.stack([ft, lt, ch], axis=1), axis=0, return_inverse=True) if len(ft) else ([], None)
    for u, (t, l, c) in enumerate(np.asarray(combos).tolist()):
        k = table.get((t, LOSS_NAMES.get(l), c), -1)
        if k >= 0:
            out[np.asarray(inverse).reshape(-1) == u] = k
    return out


def flat_run(psm_df: pd.DataFrame, frag_df: pd.DataFrame, charged_frag_types):
    """The host half of ``add_run``: ``(precursor_df, n_rows, row, col, mz, intensity, correlation)`` - the target
    rows with ``len(sequence) - 1`` dense rows each, and the flat rows that have a precursor and a column."""
    psm = psm_df[psm_df["decoy"].astype(int) == 0].reset_index(drop=True)
    if psm["precursor_idx"].duplicated().any():
        raise ValueError("add_run: a precursor_idx occurs twice among the target rows")
    n_rows_each = psm["sequence"].str.len().to_numpy().astype(np.int64) - 1
    stop = np.cumsum(n_rows_each)
    psm["frag_start_idx"], psm["frag_stop_idx"] = stop - n_rows_each, stop
    owner = pd.Index(psm["precursor_idx"]).get_indexer(frag_df["precursor_idx"])
    col = fragment_column_index(frag_df["type"], frag_df["loss_type"], frag_df["charge"], charged_frag_types)
    take = (owner >= 0) & (col >= 0)
    owner, col = owner[take], col[take]
    position = frag_df["position"].to_numpy()[take].astype(np.int64)
    if (position >= n_rows_each[owner]).any():
        raise ValueError("add_run: a fragment position lies beyond its peptide")
    row = psm["frag_start_idx"].to_numpy()[owner] + position
    values = [frag_df[c].to_numpy()[take].astype(np.float32) for c in ("mz", "intensity", "correlation")]
    return psm, int(stop[-1]) if len(stop) else 0, row, col, *values


def host_scatter_dense(n_rows: int, n_columns: int, row, col, mz, intensity, correlation):
    """``(mz, intensity, correlation)`` matrices [n_rows, n_columns], zero but for the flat rows at (row, col); a cell
    written twice raises ``ValueError``."""
    cell = np.asarray(row, np.int64) * n_columns + np.asarray(col, np.int64)
    if len(np.unique(cell)) != len(cell):
        raise ValueError("transfer library: two flat fragment rows fall into one cell of the dense matrices")
    out = []
    for v in (mz, intensity, correlation):
        m = np.zeros(n_rows * n_columns, dtype=np.float32)
        m[cell] = v
        out.append(m.reshape(n_rows, n_columns))
    return tuple(out)


class _FlatLibrary:
    """A run built from flat tables, shaped as ``update`` takes it."""

    def __init__(self, precursor_df, columns, mats):
        self.precursor_df = precursor_df
        for name, m in zip(FLAT_DENSE, mats):
            setattr(self, name, pd.DataFrame(m, columns=list(columns)))

    def available_dense_fragment_dfs(self):
        return list(FLAT_DENSE)


def host_add_run(consensus, psm_df, frag_df, charged_frag_types, keep_top: int = 3) -> ConsensusLibrary:
    """``add_run`` in NumPy: ``host_scatter_dense`` followed by ``host_update``."""
    psm, n_rows, row, col, mz, inten, corr = flat_run(psm_df, frag_df, charged_frag_types)
    mats = host_scatter_dense(n_rows, len(charged_frag_types), row, col, mz, inten, corr)
    return host_update(consensus, _FlatLibrary(psm, charged_frag_types, mats), keep_top)


# --------------------------------------------------------------------------------------------
# the device path
# --------------------------------------------------------------------------------------------
def _context(device):
    from alphadia_amd import runtime

    return runtime.get_context(device)


def normalize_rt_max(spec_lib_base, device: int | None = None):
    """``normalize_rt_max``: ``rt_norm = rt_observed / rt_observed.max()`` on the GPU."""
    df = spec_lib_base.precursor_df
    t0 = time.perf_counter()
    out, ms = _context(device).tl_rt_norm(df[RT_OBSERVED].to_numpy())
    df["rt_norm"] = out
    last_timing.update(rt_norm_s=time.perf_counter() - t0, rt_norm_ms=ms)
    return spec_lib_base


def normalize_rt_delta_max(spec_lib_base, device: int | None = None):
    """``normalize_rt_delta_max`` on the GPU."""
    df = spec_lib_base.precursor_df
    t0 = time.perf_counter()
    out, ms = _context(device).tl_rt_norm(df[RT_OBSERVED].to_numpy(), df[RT_CALIBRATED].to_numpy(),
                                          df[RT_LIBRARY].to_numpy())
    df["rt_norm"] = out
    last_timing.update(rt_norm_s=time.perf_counter() - t0, rt_norm_ms=ms)
    return spec_lib_base


def ms2_quality_control(spec_lib_base, precursor_correlation_cutoff: float = 0.5,
                        fragment_correlation_ratio: float = 0.75, device: int | None = None):
    """``ms2_quality_control`` on the GPU: ``use_for_ms2`` and the masked ``fragment_intensity_df`` (in place).  The
    two frames are float32; cutoff and ratio are rounded to float32 as NumPy's comparison with a float32 does."""
    t0 = time.perf_counter()
    df, start, stop, inten_df, corr_df = _qc_parts(spec_lib_base)
    inten, corr = inten_df.to_numpy(), corr_df.to_numpy()
    if inten.dtype != np.float32 or corr.dtype != np.float32:
        raise TypeError("ms2_quality_control: the intensity and correlation frames must be float32")
    use, out, n_large, ms = _context(device).tl_qc(start, stop, inten, corr, precursor_correlation_cutoff,
                                                   fragment_correlation_ratio,
                                                   0.0 > precursor_correlation_cutoff)
    inten_df.iloc[:, :] = out
    df["use_for_ms2"] = use
    last_timing.update(qc_s=time.perf_counter() - t0, qc_ms=ms, qc_large_blocks=n_large)
    return spec_lib_base


class HipTransferLearningAccumulator:
    """``TransferLearningAccumulator`` with the consensus in HBM.  Subscribes to the reference's
    ``AccumulationBroadcaster`` unchanged (``update`` per run, ``post_process`` at the end); ``add_run`` takes a run's
    flat tables instead of a library object."""

    def __init__(self, keep_top: int = 3, norm_delta_max: bool = True, precursor_correlation_cutoff: float = 0.5,
                 fragment_correlation_ratio: float = 0.75, device: int | None = None):
        self._keep_top = keep_top
        self.consensus_speclibase: ConsensusLibrary | None = None
        self._norm_delta_max = norm_delta_max
        self._precursor_correlation_cutoff = precursor_correlation_cutoff
        self._fragment_correlation_ratio = fragment_correlation_ratio
        self._device = device
        self._tl = None
        self.timing = dict(update_s=0.0, scatter_s=0.0, topk_ms=0.0, gather_ms=0.0, scatter_ms=0.0, runs=0)

    def _session(self, names, columns):
        if self._tl is None:
            self._tl = _context(self._device).transfer_library(len(columns), len(names))
        elif self.consensus_speclibase is not None:
            _same_layout(self.consensus_speclibase, names, columns)
        elif (self._tl.n_columns, self._tl.n_matrices) != (len(columns), len(names)):
            self._tl.close()  # (nothing was accumulated yet)
            self._tl = _context(self._device).transfer_library(len(columns), len(names))
        return self._tl

    def _finish(self, s, run_df, names, columns, n_rows, mats, t0):
        cons = self.consensus_speclibase
        kept, start, stop = s.update(self._keep_top, run_df["mod_seq_hash"].to_numpy(), run_df["proba"].to_numpy(),
                                     run_df["precursor_idx"].to_numpy(), run_df["frag_start_idx"].to_numpy(),
                                     run_df["frag_stop_idx"].to_numpy(), n_rows, mats)
        df = _truncate(None if cons is None else cons.precursor_df, run_df, kept, start, stop)
        if cons is not None:
            cons._fetch = None  # its matrices have left HBM
        self.consensus_speclibase = ConsensusLibrary(df, names, columns, fetch=s.matrix)
        topk_ms, gather_ms, scatter_ms = s.time_ms()
        t = self.timing
        t["update_s"] += time.perf_counter() - t0
        t["topk_ms"] += topk_ms
        t["gather_ms"] += gather_ms
        t["scatter_ms"] += scatter_ms if mats is None else 0.0
        t["runs"] += 1

    def update(self, speclibase) -> None:
        """Takes one run: ``precursor_df`` with ``mod_seq_hash``, ``proba``, ``precursor_idx``, ``frag_start_idx`` and
        ``frag_stop_idx``, and the float32 dense frames ``available_dense_fragment_dfs()`` names."""
        t0 = time.perf_counter()
        run_df, names, columns, mats = _run_parts(speclibase)
        self._finish(self._session(names, columns), run_df, names, columns, len(mats[0]), mats, t0)

    def add_run(self, psm_df: pd.DataFrame, frag_df: pd.DataFrame, charged_frag_types) -> None:
        """``build_speclibflat_from_quant`` + ``update`` from a run's PSM table and ``frag.transfer`` table: the
        dense m/z, intensity and correlation matrices are built on the device."""
        t0 = time.perf_counter()
        columns = list(charged_frag_types)
        psm, n_rows, row, col, mz, inten, corr = flat_run(psm_df, frag_df, columns)
        s = self._session(list(FLAT_DENSE), columns)
        if s.scatter(n_rows, row, col, mz, inten, corr):
            raise ValueError("transfer library: two flat fragment rows fall into one cell of the dense matrices")
        self.timing["scatter_s"] += time.perf_counter() - t0
        self._finish(s, psm, list(FLAT_DENSE), columns, n_rows, None, t0)

    def post_process(self) -> None:
        """RT normalisation (delta-max, or max when asked for or when ``rt_calibrated`` is absent) and the MS2
        quality control of the consensus."""
        norm_delta_max = self._norm_delta_max
        lib = self.consensus_speclibase
        if RT_CALIBRATED not in lib.precursor_df.columns:
            logger.warning(f"Column '{RT_CALIBRATED}' not found in the precursor_df, delta-max normalization will not "
                           "be performed")
            norm_delta_max = False
        logger.info("Performing quality control for transfer learning.")
        logger.info(f"Normalize by delta: {norm_delta_max}")
        logger.info(f"Precursor correlation cutoff: {self._precursor_correlation_cutoff}")
        logger.info(f"Fragment correlation cutoff: {self._fragment_correlation_ratio}")
        if norm_delta_max:
            lib = normalize_rt_delta_max(lib, device=self._device)
        else:
            lib = normalize_rt_max(lib, device=self._device)
        self.consensus_speclibase = ms2_quality_control(lib, self._precursor_correlation_cutoff,
                                                        self._fragment_correlation_ratio, device=self._device)

    def close(self) -> None:
        """Frees the consensus in HBM; dense frames not read so far are fetched first."""
        if self._tl is not None:
            if self.consensus_speclibase is not None:
                for name in self.consensus_speclibase.available_dense_fragment_dfs():
                    getattr(self.consensus_speclibase, name)
            self._tl.close()
            self._tl = None
