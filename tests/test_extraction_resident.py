"""Resident extraction, host side (no GPU): the ctypes declarations of the two entries and the compact
output against the header, the frames ResidentScores builds from a compact copy-out, and HipExtractionHandler.extract's
fallback decision and frame assembly, with stand-ins for the device."""

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import synthetic as syn
from alphadia_amd import _abi
from alphadia_amd.fdr import HipFDRManager
from alphadia_amd.fragcomp import candidate_hash
from alphadia_amd.scoring import (DEFAULT_FEATURE_COLUMNS, FRAGMENT_DF_COLUMNS, ResidentScores, assemble_candidates,
                                  collect_candidates, collect_fragments_compact)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resident_entries_match_the_header():
    """The two entries take the structs themselves (tests/test_abi.py holds every prototype against the header), and
    the compact output has the header's fields."""
    header = open(os.path.join(ROOT, "include", "alphadia_hip.h")).read()
    handle, table, config = C.c_void_p, C.POINTER(_abi.Candidates), C.POINTER(_abi.ScoringConfig)
    assert _abi.PROTOTYPES["adh_score_candidates_resident"] == (C.c_int32, [handle, table, config])
    assert _abi.PROTOTYPES["adh_take_rows"] == (C.c_int32, [handle, C.POINTER(C.c_int64), C.c_int64,
                                                            C.POINTER(_abi.CompactOutput)])
    body = re.search(r"typedef struct adh_compact_output \{(.*?)\} adh_compact_output_t;", header, re.S).group(1)
    fields = re.findall(r"^\s*[\w ]+?\**\s*\**(\w+);", body, re.M)
    assert fields == [f for f, _ in _abi.CompactOutput._fields_]


# ---------------------------------------------------------------------------------------------- frames()
class _FakeTables:
    """Padded tables of n rows and what adh_take_rows returns for a row list (valid rows in list order, their
    leading filled slots)."""

    def __init__(self, n, top_k, seed=0):
        rng = np.random.default_rng(seed)
        self.valid = rng.random(n) < 0.8
        self.features = rng.standard_normal((n, _abi.NUM_FEATURES)).astype(np.float32)
        self.k = rng.integers(0, top_k + 1, n)
        self.slot = {name: rng.integers(1, 200, (n, top_k)).astype(dt) for name, dt in _abi.COMPACT_SLOT_FIELDS}
        self.n, self.top_k = n, top_k
        self.tables_serial = 1
        self.device = 0
        self.calls = []

    def take_rows(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        self.calls.append(rows)
        keep = rows[self.valid[rows]]
        filled = np.arange(self.top_k)[None, :] < self.k[keep][:, None]
        out = {"row": keep.astype(np.uint32), "precursor_idx": self.pidx[keep].astype(np.uint32),
               "rank": self.rank[keep].astype(np.uint8), "features": np.ascontiguousarray(self.features[keep].T)}
        for name, dt in _abi.COMPACT_SLOT_FIELDS:
            out[name] = self.slot[name][keep][filled].astype(dt)
        out["fragment_row"] = np.repeat(keep, filled.sum(axis=1)).astype(np.uint32)
        out["fragment_precursor_idx"] = np.repeat(self.pidx[keep], filled.sum(axis=1)).astype(np.uint32)
        out["fragment_rank"] = np.repeat(self.rank[keep], filled.sum(axis=1)).astype(np.uint8)
        out["top_k"] = self.top_k
        return out


def _resident(top_k=6, seed=0):
    case = syn.make_case(300, 100, config_id=83, per_precursor=2, run=False)
    pdf = case.library.precursor_df.sort_values(by="precursor_idx")
    soa = assemble_candidates(case.candidates_df, pdf, "mz_library")
    tables = _FakeTables(len(soa["order"]), top_k, seed)
    tables.pidx, tables.rank = np.asarray(soa["precursor_idx"]), np.asarray(soa["rank"])
    seq = pdf["sequence"]
    scorer = SimpleNamespace(_ctx=tables, precursors_flat_df=pdf, rt_column="rt_library",
                             mobility_column="mobility_library", precursor_mz_column="mz_library",
                             _sequence_counts=lambda: tuple(seq.str.count(a).values for a in ("K", "R", "P")))
    return ResidentScores(scorer, case.candidates_df, soa, tables.tables_serial), case, scorer, tables


def test_frames_are_the_operator_frames_at_the_listed_rows():
    res, case, scorer, tables = _resident()
    n = res.n_table
    # the operator's frames over every valid row (what HipCandidateScoring.__call__ builds from the compact copy-out)
    full = tables.take_rows(np.arange(n))
    f_all = collect_candidates(case.candidates_df, None, scorer.precursors_flat_df, "rt_library", "mobility_library",
                               "mz_library", row_maps=(res.order, res.prec_row), sequence_counts=scorer._sequence_counts(),
                               compact=full)
    fr_all = collect_fragments_compact(full, scorer.precursors_flat_df, res.prec_row)
    rows = np.random.default_rng(1).permutation(n)[: n // 2]
    f, fr = res.frames(rows)
    # one copy-out, of the listed rows in table order
    assert len(tables.calls) == 2 and np.array_equal(tables.calls[-1], np.sort(rows))
    # features: the valid listed rows in list order; columns, order and dtypes of the operator's frame
    pos = np.searchsorted(full["row"], rows[tables.valid[rows]])
    assert list(f.columns) == list(f_all.columns) and list(f.columns[:46]) == DEFAULT_FEATURE_COLUMNS
    assert len(f) == int(tables.valid[rows].sum()) > 0
    exp = f_all.iloc[pos].reset_index(drop=True)
    for c in f.columns:
        assert f[c].dtype == exp[c].dtype, c
        assert (f[c].to_numpy() == exp[c].to_numpy()).all() or np.array_equal(f[c].to_numpy(), exp[c].to_numpy(), equal_nan=True), c
    # fragments: the listed rows' slots in table-row / slot order
    sel = np.isin(full["fragment_row"], rows)
    exp_fr = fr_all[sel].reset_index(drop=True)
    assert list(fr.columns) == list(fr_all.columns) and list(fr.columns[:14]) == FRAGMENT_DF_COLUMNS
    assert len(fr) == int(sel.sum()) > 0
    for c in fr.columns:
        assert fr[c].dtype == exp_fr[c].dtype and np.array_equal(fr[c].to_numpy(), exp_fr[c].to_numpy()), c
    # no rows: the empty frames with the same columns and dtypes; the column list of the features frame
    f0, fr0 = res.frames(np.zeros(0, np.int64))
    assert len(f0) == len(fr0) == 0
    assert list(f0.dtypes) == list(f_all.dtypes) and list(fr0.dtypes) == list(fr_all.dtypes)
    assert res.feature_columns() == list(f_all.columns)
    # per table row: library columns through the precursor row, sequence counts, candidate columns
    assert np.array_equal(res.table_column("mz_library"), scorer.precursors_flat_df["mz_library"].to_numpy()[res.prec_row])
    assert np.array_equal(res.table_column("n_K"), scorer._sequence_counts()[0][res.prec_row])
    assert np.array_equal(res.table_column("score"), case.candidates_df["score"].to_numpy()[res.order])


def test_frames_refuse_tables_replaced_since():
    from alphadia_amd.runtime import HipBackendError

    res, _, _, tables = _resident()
    tables.tables_serial += 1
    with pytest.raises(HipBackendError):
        res.frames(np.arange(3))


# ---------------------------------------------------------------------------------------------- extract()
def _config(channel_wise=False, fdr=0.01):
    return {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                       "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
            "general": {"thread_count": 1},
            "fdr": {"fdr": fdr, "competitive_scoring": True, "channel_wise_fdr": channel_wise}}


def test_fallback_decision():
    from alphadia_amd.extraction_handler import resident_refusal

    mgr = HipFDRManager(["rt_observed"], object())
    assert resident_refusal(_config(), mgr, lambda: False) is None
    assert "channel-wise" in resident_refusal(_config(channel_wise=True), mgr, lambda: False)
    assert "not a HipFDRManager" in resident_refusal(_config(), SimpleNamespace(fit_predict=None), lambda: False)
    assert "communicator" in resident_refusal(_config(), mgr, lambda: True)
    # the cheap checks decide before anybody looks at a GPU context
    assert "channel-wise" in resident_refusal(_config(channel_wise=True), mgr, lambda: 1 / 0)


class _Manager(HipFDRManager):
    """Stand-in for the device FDR stage: fixed survivors in a fixed order."""

    def __init__(self, psm_df):
        super().__init__(["rt_observed"], object())
        self.psm_df = psm_df

    def fit_predict_resident(self, resident, competitive, version=-1):
        self.got = (resident, competitive, version)
        return self.psm_df


@pytest.mark.parametrize("too_few", [False, True])
def test_extract_assembles_the_python_branch_frames(monkeypatch, too_few):
    from alphadia_amd.extraction_handler import HipExtractionHandler

    res, case, _, tables = _resident(top_k=12)
    valid_rows = np.flatnonzero(tables.valid)
    order = np.random.default_rng(2).permutation(valid_rows)[:40]
    psm = res.metadata.iloc[order].copy()
    psm["_decoy"] = psm["decoy"].to_numpy().astype(np.float64)
    psm["proba"] = np.linspace(0, 1, len(order)).astype(np.float32)
    psm["qval"] = np.r_[np.zeros(30), np.ones(10)]
    psm["table_row"] = order
    psm.attrs["fragment_competition"] = True
    if too_few:
        psm.attrs["too_few_psms"] = True
    mgr = _Manager(psm)
    opt = SimpleNamespace(score_cutoff=0.0, classifier_version=3)
    log = []
    h = HipExtractionHandler(_config(fdr=1.0 if too_few else 0.01), opt, mgr, SimpleNamespace(log_string=lambda m, **k: log.append(m)),
                             None, selection_handler=SimpleNamespace(select_candidates=lambda *a, **k: case.candidates_df))
    monkeypatch.setattr(h, "_comm_attached", lambda: False)
    monkeypatch.setattr(h, "_candidate_scoring", lambda *a, **k: SimpleNamespace(score_resident=lambda c: res))
    pre, frag = h.extract(None, None)
    assert mgr.got[1:] == (True, 3)
    kept = order if too_few else order[:30]
    features, fragments = res.frames(kept)
    assert isinstance(pre.index, pd.RangeIndex) and isinstance(frag.index, pd.RangeIndex)
    tail = ["qval", "proba", "candidate_idx"] if too_few else ["_decoy", "proba", "qval", "_candidate_idx", "valid", "candidate_idx"]
    assert list(pre.columns) == list(features.columns) + tail
    assert np.array_equal(pre["precursor_idx"].to_numpy(), res.metadata["precursor_idx"].to_numpy()[kept])
    key = candidate_hash(pre["precursor_idx"].to_numpy(), pre["rank"].to_numpy())
    assert pre["candidate_idx"].dtype == np.uint64 and np.array_equal(pre["candidate_idx"].to_numpy(), key)
    if not too_few:
        assert pre["proba"].dtype == np.float32 and pre["valid"].all()
        assert np.array_equal(pre["_candidate_idx"].to_numpy(), key)
        assert np.array_equal(pre["qval"].to_numpy(), psm["qval"].to_numpy()[:30])
    else:
        assert (pre["qval"] == 1.0).all() and (pre["proba"] == 1.0).all() and pre["proba"].dtype == np.float64
    # fragments: those of the kept candidates, in table-row order, with their candidate key
    assert list(frag.columns) == list(fragments.columns) + ["candidate_idx"]
    assert np.isin(frag["candidate_idx"].to_numpy(), key).all() and len(frag) == len(fragments) > 0
    assert np.array_equal(frag["candidate_idx"].to_numpy(),
                          candidate_hash(frag["precursor_idx"].to_numpy(), frag["rank"].to_numpy()))
