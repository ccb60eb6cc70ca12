"""Multiplex requantification on the HIP backend.

Plug-in counterpart of ``MultiplexingRequantificationHandler.requantify``
(alphadia/workflow/peptidecentric/multiplexing_requantification_handler.py:44-149).  The work is in
:func:`alphadia_amd.scoring.requantify_multiplexed` (candidate expansion over the label channels +
grouped scoring on the GPU).  ``requantify`` reads the workflow's configuration and hands the feature table to the
workflow's own FDR manager; ``requantify_filtered`` is the workflow's whole requantification step (scoring, the
channel-decoy FDR, the q-value filter) and, with a ``HipFDRManager``, leaves the tables in HBM and copies back only the
rows that pass the filter.
"""

from __future__ import annotations

import logging
import time

import pandas as pd

from alphadia_amd.scoring import requantify_multiplexed

logger = logging.getLogger(__name__)


class HipMultiplexingRequantificationHandler:
    """``last_timings`` holds the path (``"resident"`` / ``"chained"``) and the wall ms per stage of the last
    ``requantify_filtered`` call, as ``HipExtractionHandler.last_timings`` does for extraction."""

    def __init__(self, config, calibration_manager, fdr_manager, reporter, column_name_handler,
                 spectral_library, device: int | None = None):
        self._config, self._calibration, self._fdr, self._reporter = config, calibration_manager, fdr_manager, reporter
        self._names, self._library, self._device = column_name_handler, spectral_library, device
        self._fallbacks_logged: set[str] = set()
        self.last_timings: dict = {}

    def _score(self, dia_data, psm_df: pd.DataFrame, resident: bool):
        """Handler :45-140: calibrated library columns, the channel list, candidate expansion and grouped scoring."""
        if "multiplexing" not in self._config:
            raise ValueError("no multiplexing config found")
        mp = self._config["multiplexing"]
        if self._calibration is not None:  # calibrated columns of the unfiltered library (handler :45-50)
            self._calibration.predict(self._library.precursor_df_unfiltered, "precursor")
            predict_staged = getattr(self._calibration, "predict_staged", None)
            if predict_staged is not None:  # (a library that is staged is recalibrated in HBM)
                predict_staged(self._library._fragment_df, "fragment", device=self._device, only_if_staged=True)
            else:
                self._calibration.predict(self._library._fragment_df, "fragment")
        # every channel that occurs anywhere: identified, reference, targets, decoy (handler :60-93)
        channels = sorted({*psm_df["channel"].unique().tolist(), mp["reference_channel"], mp["decoy_channel"],
                           *(int(c) for c in str(mp["target_channels"]).split(","))})
        self._reporter.log_string(f"=== Multiplexing {len(psm_df):,} precursors over channels {channels} ===",
                                  verbosity="progress")
        return requantify_multiplexed(
            dia_data, psm_df, self._library.precursor_df_unfiltered, self._library.fragment_df, channels,
            mp["reference_channel"], self._config["search"]["experimental_xic"],
            dict(rt_column=self._names.get_rt_column(), mobility_column=self._names.get_mobility_column(),
                 precursor_mz_column=self._names.get_precursor_mz_column(),
                 fragment_mz_column=self._names.get_fragment_mz_column()),
            device=self._device, resident=resident,
        )

    def requantify(self, dia_data, psm_df: pd.DataFrame) -> pd.DataFrame:
        features, _ = self._score(dia_data, psm_df, resident=False)
        mp = self._config["multiplexing"]
        return self._fdr.fit_predict(features, decoy_strategy="channel", competitive=mp["competitive_scoring"],
                                     decoy_channel=mp["decoy_channel"])

    def resident_refusal(self) -> str | None:
        """The reason ``requantify_filtered`` takes the chained calls, or None (``extraction_handler.resident_refusal``
        without the channel-wise clause: the parts of the channel strategy are staged on the device)."""
        from alphadia_amd import runtime
        from alphadia_amd.fdr import HipFDRManager

        if not isinstance(self._fdr, HipFDRManager):
            return f"the FDR manager is a {type(self._fdr).__name__}, not a HipFDRManager"
        if getattr(runtime.get_context(self._device), "_comm_attached", False):
            return "a communicator is attached: the device tables are a rank's shard plus a gather"
        return None

    def requantify_filtered(self, dia_data, psm_df: pd.DataFrame) -> pd.DataFrame:
        """``PeptideCentricWorkflow.requantify`` (peptidecentric.py:268-293) on one GPU: the channel copies are scored
        into HBM, the channel-decoy FDR runs on the tables there (``HipFDRManager.fit_predict_resident`` with the
        "channel" strategy), and only the rows at ``qval <= config["fdr"]["fdr"]`` are copied back, in one
        ``take_rows`` copy-out.  Returns what ``requantify()`` followed by that filter returns, with a fresh
        RangeIndex: the features frame's columns, ``_decoy``, ``proba``, ``qval``; ``decoy`` set on the decoy channel;
        a row of the decoy channel once per target channel it survived with.  An FDR manager that is not a
        ``HipFDRManager`` and an attached communicator take the chained calls instead (the reason is logged once)."""
        from alphadia_amd import runtime

        t_0 = time.perf_counter()
        threshold = self._config["fdr"]["fdr"]
        reason = self.resident_refusal()
        if reason is not None:
            if reason not in self._fallbacks_logged:
                self._fallbacks_logged.add(reason)
                self._reporter.log_string(f"Resident requantification not used: {reason}", verbosity="info")
                logger.info("resident requantification not used: %s", reason)
            out = self.requantify(dia_data, psm_df)
            t_1 = time.perf_counter()
            out = out[out["qval"] <= threshold].reset_index(drop=True)
            self.last_timings = {"path": "chained", "score_fdr_ms": (t_1 - t_0) * 1e3,
                                 "filter_ms": (time.perf_counter() - t_1) * 1e3,
                                 "total_ms": (time.perf_counter() - t_0) * 1e3}
            return out
        resident = self._score(dia_data, psm_df, resident=True)
        mp = self._config["multiplexing"]
        runtime.get_context(self._device).synchronize()  # (score_resident copies nothing back: the stage clock waits)
        t_1 = time.perf_counter()
        fdr_df = self._fdr.fit_predict_resident(resident, competitive=mp["competitive_scoring"],
                                                decoy_strategy="channel", decoy_channel=mp["decoy_channel"])
        t_2 = time.perf_counter()
        kept = fdr_df[fdr_df["qval"].to_numpy() <= threshold]
        out, _ = resident.frames(kept["table_row"].to_numpy())
        if len(out) != len(kept):
            raise RuntimeError("the FDR stage kept rows the scoring call marked invalid")
        parts = fdr_df.attrs.get("parts", [])
        if fdr_df.attrs.get("too_few_psms", False):  # perform_fdr's answer for too few PSMs: qval, then proba, no _decoy
            columns = ["qval", "proba"]
        elif parts and parts[0][2]:  # (the host manager's concatenation when its first part had too few PSMs)
            columns = ["qval", "proba", "_decoy"]
        else:
            columns = ["_decoy", "proba", "qval"]
        for c in columns:
            out[c] = kept[c].to_numpy()
        out.loc[out["channel"] == mp["decoy_channel"], "decoy"] = 1  # fdr_manager.py:223
        t_3 = time.perf_counter()
        self.last_timings = {"path": "resident", "score_ms": (t_1 - t_0) * 1e3, "fdr_ms": (t_2 - t_1) * 1e3,
                             "filter_ms": (t_3 - t_2) * 1e3, "total_ms": (t_3 - t_0) * 1e3}
        return out
