"""Host-side mirror of the reference's candidate selection operator (the step before scoring).

``HipCandidateSelection`` has the constructor and call signature of
``alphadia.search.selection.selection.CandidateSelection`` (selection.py:529-660) and returns the
same candidate DataFrame; the per-precursor work runs in ``adh_select_kernel`` behind the C ABI
(``adh_select_candidates``), for AlphaRaw runs and for ion-mobility (timsTOF) runs.

``HipCandidateSelection.select_resident`` leaves the table in HBM instead (``adh_select_candidates_resident``), where
it is filtered, ordered and joined with the library columns for scoring (``adh_assemble_selected``):
``HipCandidateScoring.score_resident`` takes the ``ResidentCandidates`` it returns.  ``host_assemble_selected`` is the
NumPy restatement of that device step.
"""

from __future__ import annotations

import re

import numpy as np
import pandas as pd

from . import _abi, runtime

CANDIDATE_COLUMNS = [name for name, _ in _abi.CANDIDATE_TABLE_FIELDS]


class CandidateSelectionConfig:
    """Field names and defaults of the reference's ``CandidateSelectionConfig``
    (search/selection/config_df.py:113-224)."""

    _DEFAULTS = dict(
        rt_tolerance=60.0, precursor_mz_tolerance=10.0, fragment_mz_tolerance=15.0,
        mobility_tolerance=0.1, isotope_tolerance=0.01, peak_len_rt=10.0, sigma_scale_rt=0.1,
        peak_len_mobility=0.013, sigma_scale_mobility=1.0, candidate_count=5, top_k_precursors=3,
        top_k_fragments=12, exclude_shared_ions=True, kernel_size=30, f_mobility=1.0, f_rt=0.99,
        center_fraction=0.5, min_size_mobility=8, min_size_rt=3, max_size_mobility=30, max_size_rt=15,
        group_channels=False, use_weighted_score=True, join_close_candidates=True,
        join_close_candidates_scan_threshold=0.01, join_close_candidates_cycle_threshold=0.6,
    )

    def __init__(self):
        for k, v in self._DEFAULTS.items():
            setattr(self, k, v)
        self.feature_std = np.array([1.0])
        self.feature_mean = np.array([0.0])
        self.feature_weight = np.array([1.0])

    def update(self, values: dict) -> None:
        for k, v in values.items():
            if not hasattr(self, k):
                raise KeyError(f"unknown candidate selection setting {k!r}")
            setattr(self, k, v)

    def validate(self) -> None:
        assert self.rt_tolerance >= 0 and self.precursor_mz_tolerance >= 0 and self.fragment_mz_tolerance >= 0
        assert self.candidate_count > 0 and self.top_k_precursors > 0 and self.kernel_size > 0
        assert np.size(self.feature_std) == np.size(self.feature_mean) == np.size(self.feature_weight) == 1, (
            "only the single-feature score of the reference is implemented"
        )

    def to_jitclass(self):
        self.validate()
        return self


def gaussian_kernel(dia, fwhm_rt: float, sigma_scale_rt: float, kernel_size: int,
                    fwhm_mobility: float = 0.012, sigma_scale_mobility: float = 1.0) -> np.ndarray:
    """The smoothing kernel of ``GaussianKernel.get_dense_matrix`` (selection/kernel.py:37-218):
    float32, shape (kernel_height, kernel_width).

    Restated literally, including the reference's use of sigma (not sigma squared) on the
    diagonal of the covariance matrix and its normalisation constant."""
    cycle = np.asarray(dia.cycle)
    rt_datapoints = cycle.shape[1]
    rt_values = np.asarray(dia.rt_values)
    rt_resolution = np.mean(np.diff(rt_values[::rt_datapoints]))
    sigma_rt = fwhm_rt / 2.3548 * sigma_scale_rt / rt_resolution
    if getattr(dia, "has_mobility", False):
        mobility_resolution = np.mean(np.diff(np.asarray(dia.mobility_values)[::-1]))
        sigma_mob = fwhm_mobility / 2.3548 * sigma_scale_mobility / mobility_resolution
    else:
        sigma_mob = 1.0  # determine_mobility_sigma without a mobility dimension (kernel.py:126-128)
    width = int(np.ceil(kernel_size / 2) * 2)
    height = int(np.ceil(min(kernel_size, int(dia.scan_max_index) + 1) / 2) * 2)
    x, y = np.meshgrid(np.arange(-width // 2, width // 2), np.arange(-height // 2, height // 2))
    xy = np.column_stack((x.flatten(), y.flatten())).astype("float32")
    sigma = np.array([[sigma_rt, 0.0], [0.0, sigma_mob]])
    dx = xy - np.array([[0.0, 0.0]])
    a = np.exp(-1 / 2 * np.einsum("ij,jk,ik->i", dx, np.linalg.inv(sigma), dx))
    b = (np.pi * 2) ** (-1 / 2) * np.linalg.det(sigma) ** (-1 / 2)  # mu.shape[0] == 1 in the reference
    return (a * b).reshape(height, width).astype(np.float32)


def isotope_columns(columns) -> list:
    """Sorted ``i_<n>`` columns (alphadia/utils.py get_isotope_columns)."""
    found = []
    for c in columns:
        m = re.fullmatch(r"i_(\d+)", str(c))
        if m:
            found.append(int(m.group(1)))
    return [f"i_{i}" for i in sorted(found)]


def select_sharded(n_precursors: int, candidate_count: int, rank: int, world: int, select, gather_rows) -> dict:
    """Candidate selection of one run on ``world`` GPUs: precursors are independent (selection.py:620-660 hands
    them to threads one by one), so rank r selects for the range ``precursor_bounds(n, r, world)`` of the table
    sorted by precursor_idx and the candidate columns - ``candidate_count`` rows per precursor - are gathered
    once, in rank order = precursor order: every rank ends with the table one GPU would have produced.

    ``select(a, b)`` -> the candidate columns of precursors [a, b); ``gather_rows(local, rows_per_rank)`` ->
    concatenation in rank order (``runtime.Context.all_gather_rows``; the CPU tests pass the gloo transport)."""
    from alphadia_amd.distributed import precursor_bounds

    if world <= 1:
        return select(0, n_precursors)
    a, b = precursor_bounds(n_precursors, rank, world)
    local = select(a, b)
    rows = [(precursor_bounds(n_precursors, r, world)[1] - precursor_bounds(n_precursors, r, world)[0]) * candidate_count
            for r in range(world)]
    return {k: gather_rows(np.ascontiguousarray(v), rows) for k, v in local.items()}


class HipCandidateSelection:
    def __init__(self, dia_data, precursors_flat: pd.DataFrame, fragments_flat: pd.DataFrame,
                 config: CandidateSelectionConfig, rt_column: str, mobility_column: str,
                 precursor_mz_column: str, fragment_mz_column: str, fwhm_rt: float = 5.0,
                 fwhm_mobility: float = 0.012, device: int | None = None, rank: int | None = None,
                 world: int | None = None) -> None:
        self.dia_data = dia_data.to_jitclass() if hasattr(dia_data, "to_jitclass") else dia_data
        self.precursors_flat = precursors_flat.sort_values("precursor_idx").reset_index(drop=True)
        self.fragments_flat = fragments_flat
        self.config = config
        self.config_jit = config.to_jitclass()
        self.rt_column = rt_column
        self.mobility_column = mobility_column
        self.precursor_mz_column = precursor_mz_column
        self.fragment_mz_column = fragment_mz_column
        self.kernel = gaussian_kernel(self.dia_data, fwhm_rt, self.config_jit.sigma_scale_rt,
                                      self.config_jit.kernel_size, fwhm_mobility,
                                      self.config_jit.sigma_scale_mobility)
        self._device = device
        # several GPUs: every rank selects for its own contiguous range of the precursor table and the candidate
        # columns are gathered once (default: the communicator attached to the context)
        self.rank, self.world = rank, world

    def _pack_precursors(self, a: int = 0, b: int | None = None) -> _abi.Marshalled:
        df = self.precursors_flat if (a == 0 and b is None) else self.precursors_flat.iloc[a:b]
        iso = df[isotope_columns(df.columns)].values
        return _abi.pack_precursors(
            df["precursor_idx"].values, df["flat_frag_start_idx"].values, df["flat_frag_stop_idx"].values,
            df["charge"].values, df[self.rt_column].values, df[self.mobility_column].values,
            df[self.precursor_mz_column].values, iso,
        )

    def __call__(self, thread_count: int = 10, debug: bool = False) -> pd.DataFrame:
        from .scoring import fragment_columns

        ctx = runtime.get_context(self._device)
        ctx.stage_run(self.dia_data)
        if "cardinality" not in self.fragments_flat.columns:
            self.fragments_flat["cardinality"] = np.ones(len(self.fragments_flat), dtype=np.uint8)
        ctx.stage_fragments(*fragment_columns(self.fragments_flat, self.fragment_mz_column))
        rank, world = ctx.comm_info() if self.world is None else (int(self.rank or 0), int(self.world))
        if world > 1 and ctx.comm_info()[1] != world:
            raise runtime.HipBackendError(f"HipCandidateSelection(world={world}) needs a communicator of {world} ranks "
                                          "on the context (Context.comm_init)")
        arrays = select_sharded(len(self.precursors_flat), int(self.config_jit.candidate_count), rank, world,
                                lambda a, b: ctx.select_candidates(self._pack_precursors(a, b), self.config_jit, self.kernel),
                                ctx.all_gather_rows)
        return candidate_frame(arrays, self.precursors_flat)

    def _id_columns(self) -> tuple:
        """``elution_group_idx``, ``decoy``, ``channel`` per precursor, in the dtypes ``assemble_candidates`` gives them."""
        df = self.precursors_flat
        channel = df["channel"].values if "channel" in df.columns else np.zeros(len(df), dtype=np.uint8)
        return (np.ascontiguousarray(df["elution_group_idx"].values, dtype=np.uint32),
                np.ascontiguousarray(df["decoy"].values, dtype=np.uint8), np.ascontiguousarray(channel, dtype=np.uint8))

    def select_resident(self, apply_cutoff: bool = False, score_cutoff: float = 0.0, score_grouped: bool = False,
                        reference_channel: int = -1) -> "ResidentCandidates":
        """``__call__`` plus the cutoff filter of the extraction handler (``score > score_cutoff``) with the table left
        in HBM (``adh_select_candidates_resident``) and assembled there for scoring (``adh_assemble_selected``):
        ``HipCandidateScoring.score_resident`` takes the result as it is, ``to_frame()`` copies it back.  The two
        scoring settings are those of the scorer the table goes to (it assembles again where they differ)."""
        from .scoring import fragment_columns

        ctx = runtime.get_context(self._device)
        world = ctx.comm_info()[1] if self.world is None else int(self.world)
        if world > 1 or getattr(ctx, "_comm_attached", False):
            raise runtime.HipBackendError("select_resident keeps one GPU's table in HBM: not with several ranks or a "
                                          "communicator attached")
        ctx.stage_run(self.dia_data)
        if "cardinality" not in self.fragments_flat.columns:
            self.fragments_flat["cardinality"] = np.ones(len(self.fragments_flat), dtype=np.uint8)
        ctx.stage_fragments(*fragment_columns(self.fragments_flat, self.fragment_mz_column))
        ctx.select_resident(self._pack_precursors(), self.config_jit, self.kernel, *self._id_columns())
        res = ResidentCandidates(self, ctx, ctx.select_serial, bool(apply_cutoff), score_cutoff)
        res.assemble(score_grouped, reference_channel)
        return res


def candidate_frame(arrays: dict, precursors_flat: pd.DataFrame, keep=None) -> pd.DataFrame:
    """The frame of the CandidateContainer columns ``arrays``: rows with a candidate (``score > 0``,
    candidate_container_to_df, config_df.py:270-298; ``keep`` where the caller has filtered already), the elution group
    and decoy columns merged in from the library (selection.py:651-660)."""
    if keep is None:
        keep = arrays["score"] > 0
    candidate_df = pd.DataFrame({c: arrays[c][keep] for c in CANDIDATE_COLUMNS})
    return candidate_df.merge(
        precursors_flat[["precursor_idx", "elution_group_idx", "decoy"]], on="precursor_idx", how="left"
    )


def cutoff_threshold(score_cutoff) -> float:
    """``score > score_cutoff`` compares in the dtype NumPy picks for a float32 column and that number (float32 for a
    Python number): the threshold in that dtype, as a float64 comparison needs it."""
    return float(np.asarray(score_cutoff).astype(np.result_type(np.float32, score_cutoff)))


def host_assemble_selected(table: dict, precursors: dict, candidate_count: int, apply_cutoff: bool = False,
                           score_cutoff: float = 0.0, score_grouped: bool = False, reference_channel: int = -1) -> dict:
    """NumPy restatement of ``adh_assemble_selected``, the parity reference of the device.

    ``table``: the nine CandidateContainer columns, ``n_precursors x candidate_count`` rows, row
    ``p * candidate_count + slot``; ``precursors``: per precursor row ``frag_start_idx``, ``frag_stop_idx``,
    ``charge``, ``precursor_mz``, ``isotope_intensity`` [n, I], ``elution_group_idx``, ``decoy``, ``channel``.  The join
    is the division ``table_row // candidate_count``.  Returns the struct of arrays of ``scoring.assemble_candidates``
    (``order`` refers to the kept rows in (precursor, slot) order, ``prec_row`` to the precursor rows) plus
    ``table_row``, ``selected_pos`` (position among the ``score > 0`` rows), ``n_selected``, ``n_kept`` and
    ``was_sorted``."""
    cc = int(candidate_count)
    score = np.asarray(table["score"], dtype=np.float32)
    selected = score > 0
    keep = selected.copy()
    if apply_cutoff:
        keep &= score.astype(np.float64) > cutoff_threshold(score_cutoff)
    selected_pos = np.cumsum(selected) - selected  # exclusive scan
    rows = np.flatnonzero(keep).astype(np.uint32)  # the flagged select: (precursor, slot) order
    n = len(rows)
    pr = (rows // cc).astype(np.intp)
    eg0 = np.asarray(precursors["elution_group_idx"], dtype=np.uint32)[pr]
    dc0 = np.asarray(precursors["decoy"], dtype=np.uint8)[pr]
    rk0 = np.asarray(table["rank"], dtype=np.uint8)[rows]
    pi0 = np.asarray(table["precursor_idx"], dtype=np.uint32)[rows]
    # the check kernel: every row orders at or behind the row before it
    hi = (eg0.astype(np.uint64) << np.uint64(8)) | dc0.astype(np.uint64)
    lo = (rk0.astype(np.uint64) << np.uint64(32)) | pi0.astype(np.uint64)
    was_sorted = bool(n < 2 or not ((hi[:-1] > hi[1:]) | ((hi[:-1] == hi[1:]) & (lo[:-1] > lo[1:]))).any())
    order = np.arange(n, dtype=np.intp)
    if not was_sorted:
        # two stable LSD passes: (precursor_idx | rank << 32 | decoy << 40), then elution_group_idx
        order = np.argsort(lo | (dc0.astype(np.uint64) << np.uint64(40)), kind="stable")
        order = order[np.argsort(eg0[order], kind="stable")]
    rows, pr = rows[order], pr[order]
    eg, dc, rk, pi = eg0[order], dc0[order], rk0[order], pi0[order]
    if score_grouped and n:
        head = np.ones(n, dtype=np.uint32)
        head[1:] = (eg[1:] != eg[:-1]) | (dc[1:] != dc[:-1]) | (rk[1:] != rk[:-1])
        score_group_idx = (np.cumsum(head, dtype=np.uint32) - 1).astype(np.uint32)
    else:
        score_group_idx = np.arange(n, dtype=np.uint32)
    if n > 1 and ((pi[1:] == pi[:-1]) & (score_group_idx[1:] == score_group_idx[:-1])).any():
        raise ValueError("precursor_idx must be unique within a score group")
    ch = np.asarray(precursors["channel"], dtype=np.uint8)[pr]
    flags = np.zeros(n, dtype=np.uint8)
    if reference_channel >= 0 and n:
        has_ref = np.zeros(n, dtype=bool)
        has_ref[score_group_idx[ch == reference_channel]] = True
        flags[~has_ref[score_group_idx]] = _abi.FLAG_SKIP
    out = {
        "order": order, "prec_row": pr, "score_group_idx": score_group_idx, "elution_group_idx": eg, "decoy": dc,
        "channel": ch, "precursor_idx": pi, "rank": rk, "flags": flags,
        "frag_start_idx": np.asarray(precursors["frag_start_idx"], dtype=np.uint32)[pr],
        "frag_stop_idx": np.asarray(precursors["frag_stop_idx"], dtype=np.uint32)[pr],
        "charge": np.asarray(precursors["charge"], dtype=np.uint8)[pr],
        "precursor_mz": np.asarray(precursors["precursor_mz"], dtype=np.float32)[pr],
        "isotope_intensity": np.ascontiguousarray(np.asarray(precursors["isotope_intensity"], dtype=np.float32)[pr]),
        "table_row": rows, "selected_pos": selected_pos[rows].astype(np.uint32),
        "n_selected": int(selected.sum()), "n_kept": n, "was_sorted": was_sorted,
    }
    for c in ("scan_start", "scan_stop", "scan_center", "frame_start", "frame_stop", "frame_center"):
        out[c] = np.asarray(table[c])[rows].astype(np.int64)
    return out


class ResidentCandidates:
    """The result of ``HipCandidateSelection.select_resident``: the candidate table of one selection call, filtered,
    ordered and joined with the library columns in HBM, ready for ``HipCandidateScoring.score_resident``.

    ``n_selected`` rows had a candidate (``score > 0``), ``n_kept`` of them passed the cutoff and form the table;
    ``was_sorted`` tells whether they were in score-group order as selected (no sort ran).  Valid until the next
    selection or staging call on the same GPU."""

    def __init__(self, selection: HipCandidateSelection, ctx, serial: int, apply_cutoff: bool, score_cutoff: float):
        self.selection = selection
        self._ctx = ctx
        self._serial = serial
        self.apply_cutoff = apply_cutoff
        self.score_cutoff = score_cutoff
        self.candidate_count = int(selection.config_jit.candidate_count)
        self.n_selected = self.n_kept = 0
        self.was_sorted = True
        self.score_grouped, self.reference_channel = False, -1
        self._ids = None

    def _check_current(self):
        if self._ctx.select_serial != self._serial:
            raise runtime.HipBackendError("the selection in HBM was replaced by a later selection or staging call")

    def assemble(self, score_grouped: bool = False, reference_channel: int = -1) -> None:
        """(Re-)assemble the table for a scorer with these two settings (``adh_assemble_selected``)."""
        self._check_current()
        self.n_selected, self.n_kept, self.was_sorted = self._ctx.assemble_selected(
            self.apply_cutoff, self.score_cutoff, score_grouped, reference_channel)
        self.score_grouped, self.reference_channel = bool(score_grouped), int(reference_channel)
        self._ids = None

    def ids(self) -> tuple[np.ndarray, np.ndarray]:
        """(row in the selection table, rank) of every row of the assembled table: 5 bytes per row cross PCIe."""
        self._check_current()
        if self._ids is None:
            self._ids = self._ctx.selected_ids(self.n_kept)
        return self._ids

    def frame_of(self, table_rows) -> tuple[pd.DataFrame, np.ndarray]:
        """The candidate frame of the listed rows of the assembled table (the columns of ``__call__``, a fresh
        RangeIndex) and their positions among the ``score > 0`` rows."""
        self._check_current()
        arrays, pos = self._ctx.take_selected(table_rows)
        return candidate_frame(arrays, self.selection.precursors_flat, keep=slice(None)), pos

    def to_frame(self) -> pd.DataFrame:
        """The frame ``HipCandidateSelection.__call__`` returns, filtered by ``score > score_cutoff`` where the cutoff
        applies: the same columns, dtypes, row order ((precursor, slot), not the processing order) and index."""
        rows, _ = self.ids()
        listed = np.arange(self.n_kept, dtype=np.int64) if self.was_sorted else np.argsort(rows, kind="stable")
        df, pos = self.frame_of(listed)
        if self.apply_cutoff:
            # the labels the boolean filter leaves of the RangeIndex of the score > 0 rows
            mask = np.zeros(self.n_selected, dtype=bool)
            mask[pos] = True
            df.index = pd.DataFrame(index=pd.RangeIndex(self.n_selected))[pd.Series(mask)].index
        return df
