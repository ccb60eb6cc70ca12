"""The "hip" extraction backend: the plug-in point of this repository.

The reference dispatches on ``config["search"]["extraction_backend"]`` in
``ExtractionHandler.create_handler``
(alphadia/workflow/peptidecentric/extraction_handler.py:70-119, with the
comment "add implementations for other backends here" at :114).
``HipExtractionHandler`` has the interface of ``ClassicExtractionHandler``
(extraction_handler.py:344-507): the same constructor arguments and the three
methods ``select_candidates`` / ``score_and_quantify_candidates`` /
``quantify_candidates``.  Candidate selection (``HipCandidateSelection``,
SURVEY.md section 8f-1), scoring and quantification all run on the GPU, for runs
with and without ion mobility; an optional ``selection_handler`` (e.g. the
reference's own ``ClassicExtractionHandler``) can take over the selection step.

``extract`` is the whole per-file extraction of ``PeptideCentricWorkflow.extraction``
(alphadia/workflow/peptidecentric/peptidecentric.py:183-263) on one GPU: the scores and the FDR stage stay in
HBM and only the surviving PSMs and their fragments cross PCIe.

INTEGRATION.md shows the three-line patch that registers the backend.
"""

from __future__ import annotations

import logging
import os
import time

import numpy as np
import pandas as pd

from alphadia_amd.fragcomp import candidate_hash
from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring
from alphadia_amd.selection import CandidateSelectionConfig, HipCandidateSelection

logger = logging.getLogger(__name__)


class HipExtractionHandler:
    """MI355X backend with the ``ClassicExtractionHandler`` method surface."""

    # the values ClassicExtractionHandler passes to the two config classes
    # (extraction_handler.py:348-376)
    _base_selection_config = dict(
        peak_len_rt=10.0, sigma_scale_rt=0.5, peak_len_mobility=0.01, sigma_scale_mobility=1.0,
        top_k_precursors=3, kernel_size=30, f_mobility=1.0, f_rt=0.99, center_fraction=0.5,
        min_size_mobility=8, min_size_rt=3, max_size_mobility=20, max_size_rt=15, group_channels=False,
        use_weighted_score=True, join_close_candidates=False, join_close_candidates_scan_threshold=0.6,
        join_close_candidates_cycle_threshold=0.6,
    )
    _base_scoring_config = dict(score_grouped=False, top_k_isotopes=3, reference_channel=-1,
                                precursor_mz_tolerance=10, fragment_mz_tolerance=15)

    def __init__(self, config, optimization_manager, fdr_manager, reporter, column_name_handler,
                 selection_handler=None, device: int | None = None):
        self._config = config
        self._optimization_manager = optimization_manager
        self._fdr_manager = fdr_manager
        self._reporter = reporter
        self._column_name_handler = column_name_handler
        self._selection_handler = selection_handler
        self._device = device
        self._fallbacks_logged: set[str] = set()
        self._optlock = None  # the lock of the last process_optimization_batch (filter_for_calibration)
        # extraction_handler.py:390-398
        self._selection_config = CandidateSelectionConfig()
        search = config["search"]
        self._selection_config.update(dict(
            self._base_selection_config, top_k_fragments=search["top_k_fragments_selection"],
            exclude_shared_ions=search["exclude_shared_ions"], min_size_rt=search["quant_window"]))
        # extraction_handler.py:400-409
        self._scoring_config = CandidateScoringConfig()
        self._scoring_config.update(dict(
            self._base_scoring_config, exclude_shared_ions=search["exclude_shared_ions"],
            quant_window=search["quant_window"], quant_all=search["quant_all"],
            experimental_xic=search["experimental_xic"]))

    def _select_candidates(self, dia_data, spectral_library) -> pd.DataFrame:
        """extraction_handler.py:411-446 with ``CandidateSelection`` replaced by the GPU operator."""
        return self._candidate_selection(dia_data, spectral_library)(thread_count=self._config["general"]["thread_count"])

    def _candidate_selection(self, dia_data, spectral_library) -> HipCandidateSelection:
        """The selection operator of extraction_handler.py:411-446, configured by the optimisation manager."""
        om = self._optimization_manager
        self._selection_config.update(dict(
            rt_tolerance=om.rt_error, mobility_tolerance=om.mobility_error, candidate_count=om.num_candidates,
            precursor_mz_tolerance=om.ms1_error, fragment_mz_tolerance=om.ms2_error))
        return HipCandidateSelection(
            dia_data,
            spectral_library.precursor_df,
            spectral_library.fragment_df,
            self._selection_config,
            rt_column=self._column_name_handler.get_rt_column(),
            mobility_column=self._column_name_handler.get_mobility_column(),
            precursor_mz_column=self._column_name_handler.get_precursor_mz_column(),
            fragment_mz_column=self._column_name_handler.get_fragment_mz_column(),
            fwhm_rt=om.fwhm_rt,
            fwhm_mobility=om.fwhm_mobility,
            device=self._device,
        )

    def select_candidates(self, dia_data, spectral_library, apply_cutoff: bool = False) -> pd.DataFrame:
        """extraction_handler.py:121-154; both run layouts are selected on the GPU.  A selection
        handler passed in by the integration (``selection_handler=``) takes precedence."""
        if self._selection_handler is not None:
            return self._selection_handler.select_candidates(dia_data, spectral_library, apply_cutoff)
        self._reporter.log_string(
            f"Extracting batch of {len(spectral_library.precursor_df)} precursors", verbosity="progress"
        )
        candidates_df = self._select_candidates(dia_data, spectral_library)
        if apply_cutoff:
            # extraction_handler.py:177-203 ("filter 1")
            num_before = len(candidates_df)
            candidates_df = candidates_df[candidates_df["score"] > self._optimization_manager.score_cutoff]
            num_after = len(candidates_df)
            num_removed = num_before - num_after
            self._reporter.log_string(
                f"Removed {num_removed} precursors with score below cutoff "
                f"{self._optimization_manager.score_cutoff}. {num_after} precursors remain.",
                verbosity="info",
            )
        return candidates_df

    def score_and_quantify_candidates(self, candidates_df, dia_data, spectral_library,
                                      top_k_fragments: int | None = None):
        """extraction_handler.py:449-486 with ``CandidateScoring`` replaced by the GPU operator."""
        candidate_scoring = self._candidate_scoring(dia_data, spectral_library, top_k_fragments)
        return candidate_scoring(
            candidates_df,
            thread_count=self._config["general"]["thread_count"],
            include_decoy_fragment_features=True,
        )

    def _candidate_scoring(self, dia_data, spectral_library, top_k_fragments: int | None = None) -> HipCandidateScoring:
        """The scoring operator of extraction_handler.py:449-486, configured by the optimisation manager."""
        om = self._optimization_manager
        k = top_k_fragments if top_k_fragments is not None else self._config["search"]["top_k_fragments_scoring"]
        self._scoring_config.update(dict(precursor_mz_tolerance=om.ms1_error, fragment_mz_tolerance=om.ms2_error,
                                         top_k_fragments=k))
        return HipCandidateScoring(
            dia_data=dia_data,
            precursors_flat=spectral_library.precursor_df,
            fragments_flat=spectral_library.fragment_df,
            config=self._scoring_config,
            rt_column=self._column_name_handler.get_rt_column(),
            mobility_column=self._column_name_handler.get_mobility_column(),
            precursor_mz_column=self._column_name_handler.get_precursor_mz_column(),
            fragment_mz_column=self._column_name_handler.get_fragment_mz_column(),
            device=self._device,
        )

    def resident_refusal(self) -> str | None:
        """Why ``extract`` cannot keep the tables in HBM for this run (it then takes the chained calls), or None."""
        return resident_refusal(self._config, self._fdr_manager, self._comm_attached)

    def _comm_attached(self) -> bool:
        from alphadia_amd import runtime

        return bool(getattr(runtime.get_context(self._device), "_comm_attached", False))

    def extract(self, dia_data, spectral_library) -> tuple[pd.DataFrame, pd.DataFrame]:
        """``PeptideCentricWorkflow.extraction`` (peptidecentric.py:196-246, the python branch) on one GPU:
        candidates -> scores in HBM -> FDR stage on the tables in HBM -> ``qval <= fdr`` -> the survivors' rows and
        their fragments, copied back as the only transfer of the tables.  Returns ``(precursor_df, fragments_df)`` as
        that branch builds them - the features frame's columns, ``_decoy``, ``proba``, ``qval`` (``_candidate_idx``
        and ``valid`` when fragments competed), ``candidate_idx``; the PSMs in the FDR output order, the fragments in
        candidate / slot order - each with a fresh RangeIndex.  Channel-wise FDR, an FDR manager that is not a
        ``HipFDRManager`` and an attached communicator take the chained calls instead (the reason is logged once).
        Where the handler's own GPU selection runs, the candidate table goes from selection to scoring in HBM as well
        (``select_handover``; ``last_timings["path"]`` is then ``"resident_select"``)."""
        t_0 = time.perf_counter()
        reason = self.resident_refusal()
        if reason is None and self.select_handover():
            return self._extract_selected(dia_data, spectral_library, t_0)
        candidates_df = self.select_candidates(dia_data, spectral_library, apply_cutoff=True)
        if reason is not None:
            if reason not in self._fallbacks_logged:
                self._fallbacks_logged.add(reason)
                self._reporter.log_string(f"Resident extraction not used: {reason}", verbosity="info")
                logger.info("resident extraction not used: %s", reason)
            return self._extract_chained(candidates_df, dia_data, spectral_library, t_0)
        t_1 = time.perf_counter()
        resident = self._candidate_scoring(dia_data, spectral_library).score_resident(candidates_df)
        return self._extract_scored(resident, "resident", t_0, t_1)

    def select_handover(self) -> bool:
        """Whether ``extract`` hands the candidate table from selection to scoring in HBM: the
        handler's own GPU selection runs (no ``selection_handler``) and ``ADH_DEBUG_NO_SELECT_HANDOVER`` is unset."""
        return self._selection_handler is None and not os.environ.get("ADH_DEBUG_NO_SELECT_HANDOVER")

    def _extract_selected(self, dia_data, spectral_library, t_0: float) -> tuple[pd.DataFrame, pd.DataFrame]:
        """``extract`` with the candidate table handed from selection to scoring in HBM: ``select_candidates(...,
        apply_cutoff=True)`` and ``score_resident`` without the frame in between.  Logs what ``select_candidates`` logs."""
        cutoff = self._optimization_manager.score_cutoff
        self._reporter.log_string(
            f"Extracting batch of {len(spectral_library.precursor_df)} precursors", verbosity="progress"
        )
        scorer = self._candidate_scoring(dia_data, spectral_library)  # (stages the run and the library)
        selected = self._candidate_selection(dia_data, spectral_library).select_resident(
            apply_cutoff=True, score_cutoff=cutoff, score_grouped=self._scoring_config.score_grouped,
            reference_channel=self._scoring_config.reference_channel)
        self._reporter.log_string(
            f"Removed {selected.n_selected - selected.n_kept} precursors with score below cutoff "
            f"{cutoff}. {selected.n_kept} precursors remain.",
            verbosity="info",
        )
        t_1 = time.perf_counter()
        return self._extract_scored(scorer.score_resident(selected), "resident_select", t_0, t_1)

    def _extract_scored(self, resident, path: str, t_0: float, t_1: float) -> tuple[pd.DataFrame, pd.DataFrame]:
        """The FDR stage on the tables in HBM and the survivors' frames."""
        fdr_config = self._config["fdr"]
        t_2 = time.perf_counter()
        psm_df = self._fdr_manager.fit_predict_resident(
            resident, competitive=fdr_config["competitive_scoring"],
            version=getattr(self._optimization_manager, "classifier_version", -1))
        too_few = bool(psm_df.attrs.get("too_few_psms", False))
        competed = bool(psm_df.attrs.get("fragment_competition", False))
        t_3 = time.perf_counter()
        psm_df = psm_df[psm_df["qval"].to_numpy() <= fdr_config["fdr"]]
        self._reporter.log_string("Removing fragments below FDR threshold")
        precursor_df, fragments_df = resident.frames(psm_df["table_row"].to_numpy())
        _attach_fdr_columns(precursor_df, psm_df, too_few, competed)
        precursor_df["candidate_idx"] = candidate_hash(precursor_df["precursor_idx"].to_numpy(),
                                                       precursor_df["rank"].to_numpy())
        fragments_df["candidate_idx"] = candidate_hash(fragments_df["precursor_idx"].to_numpy(),
                                                       fragments_df["rank"].to_numpy())
        t_4 = time.perf_counter()
        # wall time of the stages of the last call, in ms (select includes the cutoff)
        self.last_timings = {"path": path, "select_ms": (t_1 - t_0) * 1e3, "score_ms": (t_2 - t_1) * 1e3,
                             "fdr_ms": (t_3 - t_2) * 1e3, "filter_ms": (t_4 - t_3) * 1e3, "total_ms": (t_4 - t_0) * 1e3}
        return precursor_df, fragments_df

    def _extract_chained(self, candidates_df, dia_data, spectral_library, t_0=None) -> tuple[pd.DataFrame, pd.DataFrame]:
        """peptidecentric.py:202-246 as written: the frames go through the host between the stages."""
        fdr_config = self._config["fdr"]
        t_1 = time.perf_counter()
        features_df, fragments_df = self.score_and_quantify_candidates(candidates_df, dia_data, spectral_library)
        t_2 = time.perf_counter()
        precursor_df = self._fdr_manager.fit_predict(
            features_df,
            decoy_strategy="precursor_channel_wise" if fdr_config["channel_wise_fdr"] else "precursor",
            competitive=fdr_config["competitive_scoring"],
            df_fragments=fragments_df,
            version=getattr(self._optimization_manager, "classifier_version", -1),
        )
        t_3 = time.perf_counter()
        precursor_df = precursor_df[precursor_df["qval"] <= fdr_config["fdr"]].copy()
        self._reporter.log_string("Removing fragments below FDR threshold")
        fragments_df["candidate_idx"] = candidate_hash(fragments_df["precursor_idx"].values, fragments_df["rank"].values)
        precursor_df["candidate_idx"] = candidate_hash(precursor_df["precursor_idx"].values, precursor_df["rank"].values)
        fragments_df = fragments_df[fragments_df["candidate_idx"].isin(precursor_df["candidate_idx"])]
        precursor_df, fragments_df = precursor_df.reset_index(drop=True), fragments_df.reset_index(drop=True)
        t_4 = time.perf_counter()
        t_0 = t_1 if t_0 is None else t_0
        self.last_timings = {"path": "chained", "select_ms": (t_1 - t_0) * 1e3, "score_ms": (t_2 - t_1) * 1e3,
                             "fdr_ms": (t_3 - t_2) * 1e3, "filter_ms": (t_4 - t_3) * 1e3, "total_ms": (t_4 - t_0) * 1e3}
        return precursor_df, fragments_df

    # ------------------------------------------------------------------ the optimisation loop
    def _log_fallback(self, reason: str, what: str, logged: set[str]) -> None:
        key = f"{what}: {reason}"
        if key not in logged:
            logged.add(key)
            self._reporter.log_string(f"{what} not used: {reason}", verbosity="info")
            logger.info("%s not used: %s", what.lower(), reason)

    def process_optimization_batch(self, dia_data, optlock) -> pd.DataFrame:
        """The python branch of ``OptimizationHandler._process_batch`` (optimization_handler.py:381-456) for a
        ``HipOptimizationLock``: select on the batch library, score the candidates behind the rows the lock has
        accumulated in HBM, run the FDR stage over all of them there (``fit_predict_resident``: the classifier
        version, seed draw and column order of ``fit_predict(optlock.features_df, ..., df_fragments=
        optlock.fragments_df)``) and ``optlock.update_with_fdr``.  Returns one row per FDR output row - the ids,
        ``decoy``, ``channel``, ``_decoy``, ``proba``, ``qval`` and ``table_row`` - enough for ``update_with_fdr``
        and ``log_precursor_df``; ``filter_for_calibration`` builds ``_filter_dfs``'s frames from it.  Channel-wise
        FDR, an FDR manager that is not a ``HipFDRManager`` and an attached communicator take the chained calls
        instead; the frame returned is then ``fit_predict``'s.  The reason is logged once per lock (the workflow
        creates a handler per step).  The caller logs "=== Extracting elution groups ..." before and the classifier
        version after, as ``_process_batch`` does; this method logs the "=== Extracted ..." line."""
        t_0 = time.perf_counter()
        library = optlock.batch_library
        candidates_df = self.select_candidates(dia_data, library)
        reason = self.resident_refusal()
        if reason is not None:
            self._log_fallback(reason, "Resident optimisation step", getattr(optlock, "fallbacks_logged",
                                                                             self._fallbacks_logged))
            return self._process_optimization_batch_chained(candidates_df, dia_data, optlock, t_0)
        t_1 = time.perf_counter()
        optlock.append_resident(self._candidate_scoring(dia_data, library), candidates_df)
        t_2 = time.perf_counter()
        psm_df = self._fdr_manager.fit_predict_resident(
            optlock.resident, competitive=self._config["fdr"]["competitive_scoring"],
            version=getattr(self._optimization_manager, "classifier_version", -1))
        psm_df.attrs["resident"] = True
        t_3 = time.perf_counter()
        self._reporter.log_string(
            f"=== Extracted {optlock.n_features} precursors and {optlock.n_fragments} fragments ===",
            verbosity="progress")
        optlock.update_with_fdr(psm_df)
        self._optlock = optlock
        self.last_timings = {"path": "resident", "select_ms": (t_1 - t_0) * 1e3, "score_ms": (t_2 - t_1) * 1e3,
                             "fdr_ms": (t_3 - t_2) * 1e3, "total_ms": (time.perf_counter() - t_0) * 1e3}
        return psm_df

    def _process_optimization_batch_chained(self, candidates_df, dia_data, optlock, t_0=None) -> pd.DataFrame:
        """optimization_handler.py:405-451 as written: the lock concatenates host frames, the FDR stage stages them."""
        fdr_config = self._config["fdr"]
        t_1 = time.perf_counter()
        features_df, fragments_df = self.score_and_quantify_candidates(candidates_df, dia_data, optlock.batch_library)
        optlock.update_with_extraction(features_df, fragments_df)
        t_2 = time.perf_counter()
        precursor_df = self._fdr_manager.fit_predict(
            optlock.features_df,
            decoy_strategy="precursor_channel_wise" if fdr_config["channel_wise_fdr"] else "precursor",
            competitive=fdr_config["competitive_scoring"],
            df_fragments=optlock.fragments_df,
            version=getattr(self._optimization_manager, "classifier_version", -1),
        )
        t_3 = time.perf_counter()
        self._reporter.log_string(
            f"=== Extracted {optlock.n_features} precursors and {optlock.n_fragments} fragments ===",
            verbosity="progress")
        optlock.update_with_fdr(precursor_df)
        self._optlock = optlock
        t_0 = t_1 if t_0 is None else t_0
        self.last_timings = {"path": "chained", "select_ms": (t_1 - t_0) * 1e3, "score_ms": (t_2 - t_1) * 1e3,
                             "fdr_ms": (t_3 - t_2) * 1e3, "total_ms": (time.perf_counter() - t_0) * 1e3}
        return precursor_df

    def filter_for_calibration(self, psm_df: pd.DataFrame, config) -> tuple[pd.DataFrame, pd.DataFrame]:
        """``OptimizationHandler._filter_dfs(psm_df, optlock.fragments_df)`` (optimization_handler.py:518-574) for
        the lock of the last ``process_optimization_batch``: the targets at ``qval < 0.01`` with the columns
        ``fit_predict`` gives them, and the best fragments of their precursors for calibration.  After a resident
        step only those precursors' rows and fragments cross PCIe, and both frames come with a fresh RangeIndex;
        after a chained step this is ``_filter_dfs`` itself, and the frames keep the indexes it leaves them."""
        from alphadia_amd.optimization import filter_fragments_for_calibration

        calibration = config["calibration"]
        optlock = self._optlock
        keep = (psm_df["qval"] < 0.01) & (psm_df["decoy"] == 0)
        if not psm_df.attrs.get("resident", False):
            precursor_df = psm_df[keep]
            fragments_df = filter_fragments_for_calibration(optlock.fragments_df, precursor_df["precursor_idx"],
                                                            calibration["min_correlation"], calibration["max_fragments"])
            return precursor_df, fragments_df
        psm_kept = psm_df[keep]
        resident = optlock.resident
        pidx = psm_kept["precursor_idx"].to_numpy()
        fragment_rows = np.flatnonzero(np.isin(resident.metadata["precursor_idx"].to_numpy(), pidx))
        precursor_df, fragments_df = resident.frames(psm_kept["table_row"].to_numpy(), fragments_of=fragment_rows)
        _attach_fdr_columns(precursor_df, psm_kept, bool(psm_df.attrs.get("too_few_psms", False)),
                            bool(psm_df.attrs.get("fragment_competition", False)))
        fragments_df = filter_fragments_for_calibration(fragments_df, pidx, calibration["min_correlation"],
                                                        calibration["max_fragments"])
        self._reporter.log_string(f"fragments_df: keeping {len(fragments_df)} of {optlock.n_fragments}")
        return precursor_df, fragments_df.reset_index(drop=True)

    def quantify_candidates(self, candidates_df, precursor_fdr_df, dia_data, spectral_library,
                            top_k_fragments: int | None = None):
        """extraction_handler.py:488-507: scoring and quantification are one pass here too."""
        del precursor_fdr_df
        _features_df, fragments_df = self.score_and_quantify_candidates(
            candidates_df, dia_data, spectral_library, top_k_fragments
        )
        return None, fragments_df


def _attach_fdr_columns(precursor_df: pd.DataFrame, psm_df: pd.DataFrame, too_few: bool, competed: bool) -> None:
    """The columns perform_fdr adds to the features frame, for the frame of ``psm_df``'s rows in its order."""
    if len(precursor_df) != len(psm_df):
        raise RuntimeError("the FDR stage kept rows the scoring call marked invalid")
    if too_few:  # perform_fdr's answer for too few PSMs (fdr.py:125-137): qval, then proba, no _decoy
        precursor_df["qval"] = 1.0
        precursor_df["proba"] = 1.0
    else:
        precursor_df["_decoy"] = psm_df["_decoy"].to_numpy()
        precursor_df["proba"] = psm_df["proba"].to_numpy()
        precursor_df["qval"] = psm_df["qval"].to_numpy()
        if competed:  # the columns FragmentCompetition leaves behind (fragcomp.py:291-299)
            precursor_df["_candidate_idx"] = candidate_hash(precursor_df["precursor_idx"].to_numpy(),
                                                            precursor_df["rank"].to_numpy())
            precursor_df["valid"] = True


def resident_refusal(config, fdr_manager, comm_attached) -> str | None:
    """The reason the resident extraction does not apply, or None: channel-wise FDR (the device classifier stages
    whole tables, not row subsets), an FDR manager other than ``HipFDRManager``, or a communicator on the context
    (``comm_attached()``; any world size - the tables are then a rank's shard plus a gather)."""
    from alphadia_amd.fdr import HipFDRManager

    if config["fdr"]["channel_wise_fdr"]:
        return "channel-wise FDR needs row subsets in the device classifier's staging"
    if not isinstance(fdr_manager, HipFDRManager):
        return f"the FDR manager is a {type(fdr_manager).__name__}, not a HipFDRManager"
    if comm_attached():
        return "a communicator is attached: the device tables are a rank's shard plus a gather"
    return None


def create_handler(config, optimization_manager, fdr_manager, reporter, column_name_handler,
                   selection_handler=None, device: int | None = None):
    """What ``ExtractionHandler.create_handler`` returns for ``extraction_backend: hip``."""
    backend = config["search"]["extraction_backend"].lower()
    if backend != "hip":
        raise ValueError(
            f"Invalid extraction backend '{backend}' for alphadia_amd. Supported backend: 'hip'"
        )
    reporter.log_string(f"Using {backend} extraction backend", verbosity="info")
    return HipExtractionHandler(
        config, optimization_manager, fdr_manager, reporter, column_name_handler,
        selection_handler=selection_handler, device=device,
    )
