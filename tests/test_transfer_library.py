"""Host side of the transfer-learning library (alphadia_amd/transfer_library.py): the NumPy restatements against the
goldens of the reference, bit for bit; the dense scatter on a hand-made table; the C-ABI declarations of adh_tl_*;
the reference's own known answer of the MS2 quality control.  No GPU needed."""

from __future__ import annotations

import os

import numpy as np
import pandas as pd
import pytest

import transfer_library_golden as G
from alphadia_amd import _abi
from alphadia_amd import transfer_library as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", G.cases("update"))
def test_host_update_equals_reference_after_every_run(case):
    g = G.load(case)
    cons = None
    for run, exp in zip(g["runs"], g["after"]):
        cons = T.host_update(cons, run, g["meta"]["keep_top"])
        G.assert_libraries_identical(cons, exp)
    if g["post"] is not None:
        with np.errstate(invalid="ignore"):
            T.host_normalize_rt_delta_max(cons)
        T.host_ms2_quality_control(cons)
        G.assert_libraries_identical(cons, g["post"])


@pytest.mark.parametrize("looped", [False, True])
@pytest.mark.parametrize("case", G.cases("qc"))
def test_host_quality_control_equals_reference(case, looped):
    g = G.load(case)
    m = g["meta"]
    lib = T.host_ms2_quality_control(g["lib"], m["cutoff"], m["ratio"], looped=looped)
    G.assert_frames_identical(lib.precursor_df, g["out_precursor"])
    G.assert_frames_identical(lib.fragment_intensity_df, g["out_intensity"])
    assert np.array_equal(lib.fragment_intensity_df.to_numpy().view(np.uint32),
                          g["out_intensity"].to_numpy().view(np.uint32))


@pytest.mark.parametrize("case", G.cases("rt"))
def test_host_rt_normalisation_equals_reference(case):
    g = G.load(case)
    for name, exp in g["out"].items():
        df = g["precursor"].copy()
        if name.endswith("_nan"):
            df.loc[g["meta"]["nan_row"], "rt_observed"] = np.nan
        fn = T.host_normalize_rt_max if name.startswith("max") else T.host_normalize_rt_delta_max
        got = fn(G.Library(df, {})).precursor_df
        G.assert_frames_identical(got[["rt_norm"]], exp)


def test_golden_cases_cover_the_issue():
    counts = set(G.meta("qc_sizes")["masked_counts"])
    s = T.QC_LDS_SLICE
    assert {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, s - 1, s, s + 1}.issubset(counts) and max(counts) >= 600
    g = G.load("qc_sizes")
    prec = g["lib"].precursor_df
    assert (prec["frag_start_idx"] == prec["frag_stop_idx"]).any()  # an empty block
    inten, corr = (f.to_numpy() for f in (g["lib"]._fragment_intensity_df, g["lib"]._fragment_correlation_df))
    at_cutoff = at_threshold = 0
    for a, b in zip(prec["frag_start_idx"], prec["frag_stop_idx"]):
        mask = inten[a:b] > 0
        if mask.sum() < 3:
            continue
        med = np.median(corr[a:b][mask])
        at_cutoff += med == np.float32(0.6)
        at_threshold += (corr[a:b] == np.float32(med * np.float32(0.9))).any()
    assert at_cutoff >= 3 and at_threshold >= 10
    sp = G.load("qc_special")
    si, sc = sp["lib"]._fragment_intensity_df.to_numpy(), sp["lib"]._fragment_correlation_df.to_numpy()
    assert np.isnan(sc[si > 0]).any() and np.isnan(sc[si == 0]).any() and np.isnan(si).any() and (si < 0).any()
    out = sp["out_intensity"].to_numpy()
    assert np.isnan(out).any() and (np.signbit(out) & (out == 0)).any()  # NaN * False and negative * False
    assert sorted(G.meta(c)["keep_top"] for c in G.cases("update") if c.startswith("topk")) == [1, 2, 3, 5]
    seen = set()
    for c in G.cases("update"):
        g = G.load(c)
        runs = [r.precursor_df for r in g["runs"]]
        h = pd.concat(runs)["mod_seq_hash"]
        seen.add((str(h.dtype), str(runs[0]["proba"].dtype)))
        if h.dtype == np.int64:
            assert (h < 0).any()
        else:
            assert (h > np.uint64(1 << 63)).any()
        if c.startswith("topk"):
            per_hash = h.value_counts()  # peptides seen in one run, and in more runs than keep_top (five runs)
            assert (per_hash == 1).any() and (per_hash > min(g["meta"]["keep_top"], 4)).any()
            assert pd.concat(runs)["proba"].isna().any()
            assert pd.concat(runs).duplicated(["mod_seq_hash", "proba", "precursor_idx"]).any()
    assert {("uint64", "float32"), ("int64", "float64"), ("uint64", "float64"), ("int64", "float32")} <= seen


def test_equal_proba_is_broken_by_precursor_idx_not_arrival():
    kept = T.host_top_k(np.array([5, 5, 5], np.uint64), np.array([0.5, 0.5, 0.5]), np.array([3, 9, 2]), 2)
    assert kept.tolist() == [2, 0]
    kept = T.host_top_k(np.array([5, 5, 5, 4], np.int64), np.array([np.nan, 0.5, 0.5, 1.0]), np.array([0, 7, 7, 1]), 3)
    assert kept.tolist() == [3, 1, 2, 0]  # full ties in arrival order, NaN last


def test_host_scatter_dense_on_six_flat_rows():
    charged = ["b_z1", "y_z1", "y_H2O_z2", "b_modloss_z1"]
    psm = pd.DataFrame({"precursor_idx": [10, 11, 12], "sequence": ["PEPK", "AAAAK", "XXK"], "decoy": [0, 1, 0],
                        "mod_seq_hash": np.array([1, 2, 3], np.uint64), "proba": [0.1, 0.2, 0.3]})
    frag = pd.DataFrame({
        "precursor_idx": [10, 10, 12, 12, 11, 10],
        "type": [98, 121, 121, 98, 98, 99],       # b, y, y, b, b (a decoy's), c (no column)
        "loss_type": [0, 0, 18, 98, 0, 0],
        "charge": [1, 1, 2, 1, 1, 1],
        "position": [0, 2, 1, 0, 0, 1],
        "mz": [100.5, 200.5, 300.5, 400.5, 500.5, 600.5],
        "intensity": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0],
        "correlation": [0.1, 0.2, 0.3, 0.4, 0.5, 0.6],
    })
    prec, n_rows, row, col, mz, inten, corr = T.flat_run(psm, frag, charged)
    assert prec["precursor_idx"].tolist() == [10, 12]
    assert prec["frag_start_idx"].tolist() == [0, 3] and prec["frag_stop_idx"].tolist() == [3, 5] and n_rows == 5
    assert row.tolist() == [0, 2, 4, 3] and col.tolist() == [0, 1, 2, 3]
    m_mz, m_in, m_co = T.host_scatter_dense(n_rows, 4, row, col, mz, inten, corr)
    exp = np.zeros((5, 4), np.float32)
    exp[0, 0], exp[2, 1], exp[4, 2], exp[3, 3] = 1.0, 2.0, 3.0, 4.0
    assert m_in.dtype == np.float32 and np.array_equal(m_in, exp)
    assert m_mz[4, 2] == np.float32(300.5) and m_co[3, 3] == np.float32(0.4) and np.count_nonzero(m_mz) == 4
    with pytest.raises(ValueError, match="one cell"):
        T.host_scatter_dense(n_rows, 4, [0, 0], [1, 1], mz[:2], inten[:2], corr[:2])
    with pytest.raises(ValueError, match="beyond its peptide"):
        T.flat_run(psm, frag.assign(position=[0, 3, 1, 0, 0, 1]), charged)


def test_reference_known_answer_use_for_ms2():
    """tests/unit_tests/outputtransform/test_outputaccumulator.py:285-336 of the reference: integer intensities,
    float64 correlations, cutoff 0.6, ratio 0.9."""
    for looped in (False, True):
        prec = pd.DataFrame({"frag_start_idx": [0, 2, 4], "frag_stop_idx": [2, 4, 6], "sequence": ["aa", "bb", "cc"]})
        inten = pd.DataFrame({"intensity_1": [10, 20, 30, 40, 0, 0], "intensity_2": [5, 15, 25, 35, 0, 0]})
        corr = pd.DataFrame({"intensity_1": [0.4, 0.5, 0.8, 0.9, 0.8, 0.9], "intensity_2": [0.3, 0.5, 0.9, 0.7, 0.8, 0.9]})
        lib = G.Library(prec, {"_fragment_intensity_df": inten, "_fragment_correlation_df": corr})
        T.host_ms2_quality_control(lib, 0.6, 0.9, looped=looped)
        np.testing.assert_array_equal(lib.precursor_df["use_for_ms2"].values, [False, True, False])


def test_quality_control_refuses_overlapping_blocks():
    prec = pd.DataFrame({"frag_start_idx": [0, 1], "frag_stop_idx": [2, 3]})
    f = pd.DataFrame(np.ones((3, 2), np.float32))
    with pytest.raises(ValueError, match="overlap"):
        T.host_ms2_quality_control(G.Library(prec, {"_fragment_intensity_df": f, "_fragment_correlation_df": f.copy()}))


def test_tl_abi_declarations_agree():
    """The nine adh_tl_* entries of the prototype table (tests/test_abi.py holds it against the header) and the two
    limits this module and the header share."""
    header = open(os.path.join(ROOT, "include", "alphadia_hip.h")).read()
    assert len([name for name in _abi.PROTOTYPES if name.startswith("adh_tl_")]) == 9
    assert f"#define ADH_TL_QC_SLICE {_abi.TL_QC_SLICE}" in header and T.QC_LDS_SLICE == _abi.TL_QC_SLICE
    assert f"#define ADH_TL_MAX_MATRICES {_abi.TL_MAX_MATRICES}" in header
