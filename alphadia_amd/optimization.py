"""The optimisation lock of the search-parameter optimisation with its rows kept in HBM.

The reference's ``OptimizationLock`` (alphadia/workflow/optimizers/optimization_lock.py) collects the features and
fragments frames of every batch it extracts and hands their concatenation to the FDR stage at every step
(``OptimizationHandler._process_batch``, workflow/peptidecentric/optimization_handler.py:381-456).
``HipOptimizationLock`` has the same constructor, batch plan, elution-group order, properties and methods; when
``HipExtractionHandler.process_optimization_batch`` drives it, the batches are scored into the device tables one
behind the other (``AccumulatedScores``) and the frames are only built on demand (``features_df`` /
``fragments_df``).  Driven by the chained calls (``update_with_extraction``), it keeps host frames as the reference
does.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

# workflow/peptidecentric/optimization_handler.py (MAX_FRAGMENT_MZ_TOLERANCE of _filter_dfs)
MAX_FRAGMENT_MZ_TOLERANCE = 200


class NoOptimizationLockTargetError(Exception):
    """alphadia.exceptions.NoOptimizationLockTargetError: the batch plan is exhausted."""


def remove_unused_fragments(precursor_df: pd.DataFrame, fragment_dfs: tuple, frag_start_col: str = "flat_frag_start_idx",
                            frag_stop_col: str = "flat_frag_stop_idx"):
    """alphabase.peptide.fragment.remove_unused_fragments: the fragment rows of ``precursor_df``'s slices, in the
    order of the slices' starts, renumbered from 0; the precursors keep their order and index."""
    precursor_df = precursor_df.sort_values([frag_start_col], ascending=True)
    frag_idx = precursor_df[[frag_start_col, frag_stop_col]].to_numpy()
    lengths = frag_idx[:, 1] - frag_idx[:, 0]
    new_idx = np.zeros_like(frag_idx)
    new_idx[:, 1] = np.cumsum(lengths)
    new_idx[1:, 0] = new_idx[:-1, 1]
    total = int(lengths.sum()) if len(lengths) else 0
    pointer = np.repeat(frag_idx[:, 0].astype(np.int64) - new_idx[:, 0].astype(np.int64), lengths) + np.arange(total)
    precursor_df = precursor_df.copy()
    precursor_df[[frag_start_col, frag_stop_col]] = new_idx
    precursor_df = precursor_df.sort_index()
    return precursor_df, tuple(df.iloc[pointer].copy().reset_index(drop=True) for df in fragment_dfs)


class BatchLibrary:
    """The batch library of the lock (the reference uses an alphabase ``SpecLibFlat`` with only the two frames set)."""

    def __init__(self, precursor_df: pd.DataFrame, fragment_df: pd.DataFrame):
        self._precursor_df = precursor_df
        self._fragment_df = fragment_df

    @property
    def precursor_df(self) -> pd.DataFrame:
        return self._precursor_df

    @property
    def fragment_df(self) -> pd.DataFrame:
        return self._fragment_df


def _library_frames(library) -> tuple[pd.DataFrame, pd.DataFrame]:
    pre = getattr(library, "_precursor_df", None)
    frag = getattr(library, "_fragment_df", None)
    return (library.precursor_df if pre is None else pre), (library.fragment_df if frag is None else frag)


class HipOptimizationLock:
    """Drop-in for the reference's ``OptimizationLock`` (same constructor, batch plan, seed-772 shuffle, properties and
    methods).  The accumulated rows live in the device tables when ``HipExtractionHandler.process_optimization_batch``
    extracts the batches (``resident``), or in host frames when the chained calls do (``update_with_extraction``).
    ``features_df`` / ``fragments_df`` build the concatenated frames on demand; ``n_features`` / ``n_fragments``
    count their rows without building them."""

    def __init__(self, library, config, device: int | None = None):
        self._library = library
        self._device = device

        self.previously_calibrated = False
        self.has_target_num_precursors = False

        precursor_df, _ = _library_frames(library)
        self._elution_group_order = precursor_df["elution_group_idx"].unique()
        rng = np.random.default_rng(seed=772)
        rng.shuffle(self._elution_group_order)

        self._precursor_target_count = config["calibration"]["optimization_lock_target"]
        self._batch_size = config["calibration"]["batch_size"]

        self.batch_idx = 0
        self.batch_plan = self._get_batch_plan(len(self._elution_group_order), self._batch_size)

        eg_idxes = self._elution_group_order[self.start_idx : self.stop_idx]

        self.batch_library: BatchLibrary | None = None
        self.set_batch_dfs(eg_idxes)

        self._feature_dfs: list[pd.DataFrame] = []
        self._fragment_dfs: list[pd.DataFrame] = []
        self.resident = None  # AccumulatedScores of the rows since the last reset, when they are on the device
        self._resident_groups = np.zeros(0, dtype=np.int64)  # elution groups of its valid rows
        self.total_elution_groups = 0
        self.fallbacks_logged: set[str] = set()  # (the workflow creates an extraction handler per step)
        self.last_fragment_calibration: str | None = None  # path of the last update_with_calibration (predict_staged)

    # ------------------------------------------------------------------ accumulated rows
    def _clear(self):
        self._feature_dfs = []
        self._fragment_dfs = []
        self.resident = None  # (the next resident append empties the device tables)
        self._resident_groups = np.zeros(0, dtype=np.int64)

    @property
    def features_df(self) -> pd.DataFrame:
        if self.resident is not None:
            return pd.concat(self.resident.batch_frames()[0])
        return pd.concat(self._feature_dfs)

    @property
    def fragments_df(self) -> pd.DataFrame:
        if self.resident is not None:
            return pd.concat(self.resident.batch_frames()[1])
        return pd.concat(self._fragment_dfs)

    @property
    def n_features(self) -> int:
        """``len(features_df)`` without building it."""
        if self.resident is not None:
            return self.resident.counts()[0]
        return sum(len(df) for df in self._feature_dfs)

    @property
    def n_fragments(self) -> int:
        """``len(fragments_df)`` without building it."""
        if self.resident is not None:
            return self.resident.counts()[1]
        return sum(len(df) for df in self._fragment_dfs)

    def append_resident(self, scorer, candidates_df: pd.DataFrame) -> int:
        """Score ``candidates_df`` (of the current batch library) behind the rows accumulated on the device; returns
        the table row of its first candidate.  The resident counterpart of ``update_with_extraction``."""
        from alphadia_amd.scoring import AccumulatedScores

        if self._feature_dfs:
            raise RuntimeError("the lock holds host frames of the chained calls: it cannot accumulate on the device too")
        if self.resident is None:
            self.resident = AccumulatedScores(self._device)
        first = self.resident.append(scorer, candidates_df)
        # features_df["elution_group_idx"].nunique(): the elution groups of the valid rows, this batch's added to
        # those of the batches before (one valid byte per row of this batch crosses PCIe)
        batch = self.resident.batches[-1]
        groups = batch.metadata["elution_group_idx"].to_numpy()[self.resident.valid(first, first + batch.n_table)]
        self._resident_groups = np.union1d(self._resident_groups, groups.astype(np.int64))
        self.total_elution_groups = int(self._resident_groups.size)
        return first

    # ------------------------------------------------------------------ the reference's interface
    @property
    def start_idx(self) -> int:
        if self.has_target_num_precursors:
            return 0
        elif self.batch_idx >= len(self.batch_plan):
            raise NoOptimizationLockTargetError()
        else:
            return self.batch_plan[self.batch_idx][0]

    @property
    def stop_idx(self) -> int:
        return self.batch_plan[self.batch_idx][1]

    @staticmethod
    def _get_batch_plan(num_items: int, batch_size: int, *, fixed_start_idx: bool = False) -> list[tuple[int, int]]:
        """optimization_lock.py: an exponential batch plan, each step twice the elution groups of the one before."""
        plan = []
        step = 0
        start_idx = 0
        stop_idx = 0
        while stop_idx < num_items:
            n_batches = int(2**step)
            stop_idx = min(stop_idx + n_batches * batch_size, num_items)
            plan.append((start_idx, stop_idx))
            step += 1
            if not fixed_start_idx:
                start_idx = stop_idx
        return plan

    def batches_remaining(self):
        return self.batch_idx + 1 < len(self.batch_plan)

    def update_with_extraction(self, feature_df: pd.DataFrame, fragment_df: pd.DataFrame):
        """The chained calls' frames of the current batch (host accumulation, as the reference's lock)."""
        if self.resident is not None:
            raise RuntimeError("the lock accumulates on the device: it cannot take host frames too")
        self._feature_dfs += [feature_df]
        self._fragment_dfs += [fragment_df]
        self.total_elution_groups = self.features_df["elution_group_idx"].nunique()

    def update_with_fdr(self, precursor_df: pd.DataFrame):
        self._precursor_at_fdr_count = np.sum((precursor_df["qval"] < 0.01) & (precursor_df["decoy"] == 0))
        self.has_target_num_precursors = self._precursor_at_fdr_count >= self._precursor_target_count

    def update_with_calibration(self, calibration_manager):
        """Recalibrate the batch library.  Rows accumulated before keep the values they were scored with."""
        calibration_manager.predict(self.batch_library._precursor_df, "precursor")  # (CalibrationGroups.PRECURSOR)
        # (CalibrationGroups.FRAGMENT) the batch that was just scored is staged: its m/z is recalibrated in HBM
        predict_staged = getattr(calibration_manager, "predict_staged", None)
        if predict_staged is not None:
            self.last_fragment_calibration = predict_staged(self.batch_library._fragment_df, "fragment",
                                                            device=self._device, only_if_staged=True)
        else:
            calibration_manager.predict(self.batch_library._fragment_df, "fragment")
            self.last_fragment_calibration = "host"

    def increase_batch_idx(self):
        self.batch_idx += 1

    def decrease_batch_idx(self):
        batch_plan_diff = np.array(
            [stop_at_given_idx - self.stop_idx * self._precursor_target_count / self._precursor_at_fdr_count
             for _, stop_at_given_idx in self.batch_plan]
        )
        self.batch_idx = np.where(batch_plan_diff >= 0)[0][0]

    def update(self):
        if self.has_target_num_precursors:
            self.decrease_batch_idx()
            self._clear()
        else:
            self.increase_batch_idx()
        eg_idxes = self._elution_group_order[self.start_idx : self.stop_idx]
        self.set_batch_dfs(eg_idxes)

    def reset_after_convergence(self, calibration_manager):
        self.has_target_num_precursors = True
        self._clear()
        self.set_batch_dfs()
        self.update_with_calibration(calibration_manager)

    def set_batch_dfs(self, eg_idxes: None | np.ndarray = None):
        if eg_idxes is None:
            eg_idxes = self._elution_group_order[self.start_idx : self.stop_idx]
        precursor_df, fragment_df = _library_frames(self._library)
        pre, (frag,) = remove_unused_fragments(
            precursor_df[precursor_df["elution_group_idx"].isin(eg_idxes)], (fragment_df,),
            frag_start_col="flat_frag_start_idx", frag_stop_col="flat_frag_stop_idx")
        self.batch_library = BatchLibrary(pre, frag)


def filter_fragments_for_calibration(fragments_df: pd.DataFrame, precursor_idx, min_correlation: float,
                                     max_fragments: int) -> pd.DataFrame:
    """The fragment half of ``OptimizationHandler._filter_dfs`` (optimization_handler.py:518-574): the fragments of
    ``precursor_idx`` with ``|mass_error| <= 200``, by (correlation, precursor_idx) descending, the first
    ``min(#correlation > min_correlation, max_fragments)``."""
    precursor_idx_mask = fragments_df["precursor_idx"].isin(precursor_idx)
    mass_error_mask = np.abs(fragments_df["mass_error"]) <= MAX_FRAGMENT_MZ_TOLERANCE
    filtered = fragments_df[precursor_idx_mask & mass_error_mask].sort_values(
        by=["correlation", "precursor_idx"], ascending=False)
    high_corr_count = (filtered["correlation"] > min_correlation).sum()
    stop_rank = min(high_corr_count, max_fragments)
    return filtered.head(stop_rank)


def append_geometry(live: int, cap: int, top_k: int, n: int, width: int) -> tuple[int, int, bool]:
    """The layout of the accumulated device tables after appending a batch of ``n`` rows of slot width ``width`` to
    ``live`` rows laid out for ``cap`` rows of ``top_k`` slots: ``(capacity, width, whether the live rows move)``.
    The rule of ``acc::grow`` (adh_resident_append.hip): an empty table takes the batch's layout; otherwise the
    capacity at least doubles when it is exceeded and the width is the larger one."""
    if live == 0:
        return max(n, 1), width, False
    need = live + n
    new_cap = max(need, 2 * cap) if need > cap else cap
    new_w = max(top_k, width)
    return new_cap, new_w, (new_cap != cap or new_w != top_k)


def relayout_rows(src: np.ndarray, ws: int, dst: np.ndarray, wd: int, n: int, row0: int) -> None:
    """Host model of ``acc::relayout_kernel`` on flat arrays: rows [0, n) of width ``ws`` into rows
    [row0, row0 + n) of width ``wd``, the slots from ``ws`` on zeroed."""
    e = np.arange(n * wd, dtype=np.int64)
    r, j = e // wd, e % wd
    out = np.zeros(n * wd, dtype=dst.dtype)
    inside = j < ws
    out[inside] = src[r[inside] * ws + j[inside]]
    dst[row0 * wd : (row0 + n) * wd] = out
