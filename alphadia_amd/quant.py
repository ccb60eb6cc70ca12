"""Cross-run fragment quantity matrices of label-free quantification on the GPU.

Drop-ins for ``FragmentQuantLoader`` (alphadia/outputtransform/quantification/fragment_accumulator.py:13-160) and
``QuantBuilder.filter_frag_df`` (quant_builder.py:132-182).  The reference builds one frame per quantity column with
one pandas outer merge per run, each of which copies the whole frame accumulated so far; here the kept frag rows of
every run go to HBM, one radix sort gives the union of ion keys, and each column is scattered into a dense
column-major ``n_keys x n_runs`` matrix (alphadia_amd/csrc/adh_quant.hip).  The frames handed back equal the
reference's: columns, column order, dtypes, row order and values.  The matrices stay in HBM, and
``filter_frag_df`` ranks the quality matrix there for every grouping level.

A run that holds the same ``(ion, precursor_idx)`` key twice makes the reference's merge a cartesian product; the
device detects it and the frames are then merged on the host exactly as the reference does (``merge_runs``).
"""

from __future__ import annotations

import logging
import os
import weakref
from collections.abc import Iterable, Iterator

import numpy as np
import pandas as pd

logger = logging.getLogger()

DEFAULT_COLUMNS = ["intensity", "correlation"]
KEY_COLUMNS = ("number", "type", "charge", "loss_type")
METADATA_COLUMNS = ["pg", "mod_seq_hash", "mod_seq_charge_hash"]
# columns of an accumulated frame that are not runs (quant_builder.py:160-166)
NON_RUN_COLUMNS = ["precursor_idx", "ion", *METADATA_COLUMNS]

_duplicate_logged = False


def ion_hash(precursor_idx, number, type_, charge, loss_type) -> np.ndarray:
    """The ion key of quant_builder.py:52-81 in int64, as Numba types it (the frag columns are uint8)."""
    i64 = lambda a: np.asarray(a).astype(np.int64)  # noqa: E731
    return i64(precursor_idx) + (i64(number) << 32) + (i64(type_) << 40) + (i64(charge) << 48) + (i64(loss_type) << 56)


def precursor_metadata(psm_df: pd.DataFrame) -> pd.DataFrame:
    """The first pg / mod_seq_hash / mod_seq_charge_hash of every precursor of the PSM table."""
    return psm_df.groupby("precursor_idx", as_index=False).agg({c: "first" for c in METADATA_COLUMNS})


def prepare_run(df: pd.DataFrame, psm_df: pd.DataFrame, columns: list[str]) -> pd.DataFrame:
    """One run's rows of PSM precursors with their ion key: ``precursor_idx, ion, *columns``."""
    df = df[df["precursor_idx"].isin(psm_df["precursor_idx"])]
    out = pd.DataFrame({"precursor_idx": df["precursor_idx"].values,
                        "ion": ion_hash(*(df[c].values for c in ("precursor_idx", *KEY_COLUMNS)))})
    for c in columns:
        out[c] = df[c].values
    return out


def merge_runs(runs: Iterable[tuple[str, pd.DataFrame]], psm_df: pd.DataFrame, columns: list[str]):
    """The reference's accumulation on the host, from prepared runs (``prepare_run``): per quantity column, the first
    run's rows, then one outer merge on ``(ion, precursor_idx)`` per further run, ``fillna(0)``, precursor_idx as
    uint32, the precursor metadata joined on the left.  The duplicate-key path and the benchmark's baseline."""
    frames = None
    for name, run in runs:
        if frames is None:
            frames = [run[["precursor_idx", "ion", c]].rename(columns={c: name}) for c in columns]
            continue
        frames = [f.merge(run[["ion", c, "precursor_idx"]], on=["ion", "precursor_idx"], how="outer")
                  .rename(columns={c: name}) for f, c in zip(frames, columns)]
    if frames is None:
        return None
    meta = precursor_metadata(psm_df)
    out = {}
    for c, f in zip(columns, frames):
        f = f.fillna(0)
        f["precursor_idx"] = f["precursor_idx"].astype(np.uint32)
        out[c] = f.merge(meta, on="precursor_idx", how="left")
    return out


def host_accumulate(df_iterable: Iterator[tuple[str, pd.DataFrame]], psm_df: pd.DataFrame, columns=None):
    """``FragmentQuantLoader.accumulate`` restated on the host (pandas merges), for comparison."""
    columns = DEFAULT_COLUMNS if columns is None else list(columns)
    return merge_runs(((n, prepare_run(df, psm_df, columns)) for n, df in df_iterable), psm_df, columns)


def host_filter_frag_df(intensity_df: pd.DataFrame, quality_df: pd.DataFrame, min_correlation: float = 0.5,
                        top_n: int = 3, group_column: str = "pg"):
    """``filter_frag_df`` restated on the host with NumPy and pandas, for comparison."""
    runs = [c for c in intensity_df.columns if c not in NON_RUN_COLUMNS]
    mean = quality_df[runs].to_numpy().mean(axis=1)
    quality_df["total"] = mean
    quality_df["rank"] = quality_df.groupby(group_column)["total"].rank(method="first", ascending=False)
    keep = (quality_df["rank"].to_numpy() <= top_n) | (mean > min_correlation)
    return intensity_df[keep], quality_df[keep]


def _key_column(df: pd.DataFrame, name: str, dtype, hi: int) -> np.ndarray:
    v = df[name].to_numpy()
    if v.dtype == dtype:
        return v
    if not np.issubdtype(v.dtype, np.integer) or (len(v) and (v.min() < 0 or v.max() > hi)):
        raise ValueError(f"frag column {name!r}: integers in [0, {hi}] expected, got {v.dtype}")
    return v.astype(dtype)


def _quantity_column(df: pd.DataFrame, name: str) -> tuple[np.ndarray, np.dtype]:
    """A quantity column as float32 for the device and the dtype the frame gives it back in.  float32 columns and
    integer columns of up to 16 bits (exact in float32) are supported."""
    v = df[name].to_numpy()
    if v.dtype == np.float32:
        return v, v.dtype
    if np.issubdtype(v.dtype, np.integer) and v.dtype.itemsize <= 2:
        return v.astype(np.float32), v.dtype
    raise TypeError(f"frag column {name!r}: float32 or an integer type of up to 16 bits expected, got {v.dtype}")


class _Resident:
    """The device matrices behind an accumulated frame."""

    def __init__(self, frame: pd.DataFrame, quant, column: int, runs: list[str]):
        self.ref = weakref.ref(frame, self._drop)
        self.key = id(frame)
        self.quant, self.column, self.runs = quant, column, runs

    def _drop(self, _ref):
        if _RESIDENT.get(self.key) is self:
            del _RESIDENT[self.key]


_RESIDENT: dict[int, _Resident] = {}


def _resident(quality_df: pd.DataFrame, run_columns: list[str]) -> _Resident | None:
    r = _RESIDENT.get(id(quality_df))
    if r is None or r.ref() is not quality_df or r.runs != run_columns or len(quality_df) != r.quant.n_keys:
        return None
    return r


class HipFragmentQuantLoader:
    """``FragmentQuantLoader`` with the accumulation on the GPU.

    Parameters
    ----------
    psm_df : pd.DataFrame
        PSMs; only frag rows of their precursors are kept.  Needs precursor_idx, pg, mod_seq_hash and
        mod_seq_charge_hash.
    columns : list[str] | None
        Quantity columns, by default ``["intensity", "correlation"]``: float32 or integers of up to 16 bits.
    device : int | None
        GPU ordinal (default: the process's, ``runtime.default_device``).

    The frames returned by ``accumulate`` keep their matrices in HBM for ``filter_frag_df``; they are treated as
    read-only in their run columns (``filter_frag_df`` adds its ``total`` / ``rank`` columns as the reference does).
    """

    def __init__(self, psm_df: pd.DataFrame, columns: list[str] | None = None, device: int | None = None):
        self.psm_df = psm_df
        self.columns = list(DEFAULT_COLUMNS) if columns is None else list(columns)
        self.device = device
        self.last_device_ms = (0.0, 0.0)

    def accumulate_from_folders(self, folder_list: list[str]) -> dict[str, pd.DataFrame] | None:
        """``accumulate`` over the ``frag.parquet`` of every folder (run name: the folder's base name)."""
        return self.accumulate(self._frag_df_generator(folder_list))

    def accumulate(self, df_iterable: Iterator[tuple[str, pd.DataFrame]]) -> dict[str, pd.DataFrame] | None:
        """One frame per quantity column: ``precursor_idx, ion, <run>..., pg, mod_seq_hash, mod_seq_charge_hash``;
        ``None`` if the iterator is empty."""
        from alphadia_amd import runtime

        logger.info("Accumulating fragment data")
        df_iterable = iter(df_iterable)
        raw_name, df = next(df_iterable, (None, None))
        if df is None:
            logger.warning(f"No frag file found for {raw_name}")
            return None
        psm = pd.unique(self.psm_df["precursor_idx"].to_numpy())
        psm = psm[(psm >= 0) & (psm <= np.iinfo(np.uint32).max)]
        psm = np.unique(psm.astype(np.uint32))
        quant = runtime.get_context(self.device).quant_matrices(len(self.columns), psm)
        names, kept, pidx_dtypes, col_dtypes = [], [], [], []
        while df is not None:
            pidx = df["precursor_idx"].to_numpy()
            cols = [_quantity_column(df, c) for c in self.columns]
            kept.append(quant.add_run(_key_column(df, "precursor_idx", np.uint32, np.iinfo(np.uint32).max),
                                      *[_key_column(df, c, np.uint8, 255) for c in KEY_COLUMNS], [v for v, _ in cols]))
            names.append(raw_name)
            pidx_dtypes.append(pidx.dtype)
            col_dtypes.append([t for _, t in cols])
            raw_name, df = next(df_iterable, (None, None))
        n_keys, duplicate = quant.build()
        self.last_device_ms = quant.time_ms()
        if duplicate or len(set(names)) != len(names):
            return self._host_path(quant, names, pidx_dtypes, col_dtypes)
        ion, pidx = quant.keys()
        meta = precursor_metadata(self.psm_df)
        pos = np.searchsorted(meta["precursor_idx"].to_numpy(), pidx)
        meta_cols = {c: meta[c].take(pos).reset_index(drop=True) for c in METADATA_COLUMNS}
        out = {}
        for j, col in enumerate(self.columns):
            m = quant.matrix(j)  # (n_runs, n_keys), C order: the block pandas keeps for the run columns
            dts = [d[j] for d in col_dtypes]
            if all(d == np.float32 for d in dts):
                frame = pd.DataFrame(m.T, columns=names, copy=False)
            else:  # an integer column keeps its dtype where the run has every key, float64 where the merge left gaps
                frame = pd.DataFrame({
                    n: m[r].astype(d if d == np.float32 or len(names) == 1 or kept[r] == n_keys else np.float64)
                    for r, (n, d) in enumerate(zip(names, dts))
                })
            frame.insert(0, "ion", ion)
            frame.insert(0, "precursor_idx", pidx)
            for c in METADATA_COLUMNS:
                frame[c] = meta_cols[c]
            r = _Resident(frame, quant, j, names)
            _RESIDENT[r.key] = r
            out[col] = frame
        return out

    def _host_path(self, quant, names, pidx_dtypes, col_dtypes):
        global _duplicate_logged
        if not _duplicate_logged:
            logger.warning("fragment quantities: a run holds an (ion, precursor_idx) key twice (or two runs share a "
                           "name); merging these runs on the host as the reference does")
            _duplicate_logged = True
        ion, pidx, run, cols = quant.rows()
        quant.close()

        def runs():
            for r, name in enumerate(names):
                sel = run == r
                f = pd.DataFrame({"precursor_idx": pidx[sel].astype(pidx_dtypes[r]), "ion": ion[sel]})
                for c, (col, dt) in enumerate(zip(self.columns, col_dtypes[r])):
                    f[col] = cols[c][sel].astype(dt)
                yield name, f

        return merge_runs(runs(), self.psm_df, self.columns)

    @staticmethod
    def _frag_df_generator(folder_list: list[str]) -> Iterator[tuple[str, pd.DataFrame]]:
        import pyarrow.parquet as pq

        for folder in folder_list:
            raw_name = os.path.basename(folder)
            frag_path = os.path.join(folder, "frag.parquet")
            if not os.path.exists(frag_path):
                logger.warning(f"no frag file found for {raw_name}")
                continue
            try:
                logger.info(f"reading frag file for {raw_name}")
                run_df = pq.read_table(frag_path).to_pandas()
            except Exception as e:  # noqa: BLE001 (an unreadable file is skipped, as the reference does)
                logger.warning(f"Error reading frag file for {raw_name}")
                logger.warning(e)
            else:
                yield raw_name, run_df


def _threshold(min_correlation) -> float:
    """``total > min_correlation`` compares in the dtype NumPy picks for a float32 column and that scalar (float32 for
    a Python number); the device compares in float64, so the threshold is rounded to that dtype first."""
    dt = np.result_type(np.float32, min_correlation)
    return float(np.asarray(min_correlation).astype(dt))


def filter_frag_df(intensity_df: pd.DataFrame, quality_df: pd.DataFrame, min_correlation: float = 0.5,
                   top_n: int = 3, group_column: str = "pg", device: int | None = None):
    """``QuantBuilder.filter_frag_df`` on the GPU: keeps, per ``group_column`` group, the ``top_n`` fragments by mean
    quality over the runs and every fragment whose mean is above ``min_correlation``.  Writes ``total`` and ``rank``
    into ``quality_df`` and returns the kept rows of both frames, as the reference does.  A frame from
    ``HipFragmentQuantLoader.accumulate`` is ranked from its matrix in HBM; any other is uploaded first."""
    from alphadia_amd import runtime

    logger.info("Filtering fragments by quality")
    run_columns = [c for c in intensity_df.columns if c not in NON_RUN_COLUMNS]
    res = _resident(quality_df, run_columns)
    if res is not None:
        quant, column = res.quant, res.column
    else:
        if not run_columns:
            raise ValueError("filter_frag_df: no run columns")
        vals = [quality_df[c].to_numpy() for c in run_columns]
        if any(v.dtype != np.float32 for v in vals):
            raise TypeError("filter_frag_df: the run columns of quality_df must be float32")
        quant = runtime.get_context(device).quant_matrices(1, [])
        quant.set_matrix(vals)
        column = 0
    codes, uniques = pd.factorize(quality_df[group_column])
    total, rank, mask = quant.filter(column, codes.astype(np.int32, copy=False), len(uniques), float(top_n),
                                     _threshold(min_correlation))
    quality_df["total"] = total
    quality_df["rank"] = rank
    kept_intensity = intensity_df[mask]
    ires = _resident(intensity_df, run_columns)
    if res is not None and ires is not None and ires.quant is quant:
        # (alphadia_amd.lfq.direct_lfq quantifies this frame from the matrix in HBM)
        from alphadia_amd import lfq

        lfq.remember_filtered(kept_intensity, quant, ires.column, run_columns, mask)
    return kept_intensity, quality_df[mask]
