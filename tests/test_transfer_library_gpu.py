"""The transfer-learning library on the GPU (alphadia_amd/transfer_library.py, adh_tl_*): the public classes and
functions against the goldens of the reference and against the host restatements.  Every comparison is exact."""

from __future__ import annotations

import logging

import numpy as np
import pandas as pd
import pytest

import transfer_library_golden as G
from alphadia_amd import transfer_library as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", G.cases("update"))
def test_device_update_equals_reference_after_every_run(case):
    g = G.load(case)
    acc = T.HipTransferLearningAccumulator(keep_top=g["meta"]["keep_top"])
    for run, exp in zip(g["runs"], g["after"]):
        acc.update(run)
        G.assert_libraries_identical(acc.consensus_speclibase, exp)
    if g["post"] is not None:
        acc.post_process()
        G.assert_libraries_identical(acc.consensus_speclibase, g["post"])
    acc.close()


@pytest.mark.parametrize("case", G.cases("qc"))
def test_device_quality_control_equals_reference(case):
    g = G.load(case)
    lib = T.ms2_quality_control(g["lib"], g["meta"]["cutoff"], g["meta"]["ratio"])
    G.assert_frames_identical(lib.precursor_df, g["out_precursor"])
    assert np.array_equal(lib.fragment_intensity_df.to_numpy().view(np.uint32),
                          g["out_intensity"].to_numpy().view(np.uint32))
    G.assert_frames_identical(lib.fragment_intensity_df, g["out_intensity"])
    if case == "qc_sizes":  # slice + 1 and 600 masked cells
        assert T.last_timing["qc_large_blocks"] == sum(c > T.QC_LDS_SLICE for c in g["meta"]["masked_counts"])


@pytest.mark.parametrize("case", G.cases("rt"))
def test_device_rt_normalisation_equals_reference(case):
    g = G.load(case)
    for name, exp in g["out"].items():
        df = g["precursor"].copy()
        if name.endswith("_nan"):
            df.loc[g["meta"]["nan_row"], "rt_observed"] = np.nan
        fn = T.normalize_rt_max if name.startswith("max") else T.normalize_rt_delta_max
        got = fn(G.Library(df, {})).precursor_df
        G.assert_frames_identical(got[["rt_norm"]], exp)


@pytest.fixture(scope="module")
def cohort():
    """8 runs x 20 000 peptides, keep_top 3: the runs and the host restatement's consensus after the last one."""
    rng = np.random.default_rng(5)
    runs = [G.cohort_run(rng, r, 20_000) for r in range(8)]
    cons = None
    for run in runs:
        cons = T.host_update(cons, run, 3)
    return runs, cons


def test_cohort_equals_host_restatement(cohort):
    runs, host = cohort
    acc = T.HipTransferLearningAccumulator(keep_top=3)
    for run in runs:
        acc.update(run)
    dev = acc.consensus_speclibase
    assert len(dev.precursor_df) > 40_000
    G.assert_libraries_identical(dev, host)
    acc.post_process()
    post = G.Library(host.precursor_df.copy(), {n: getattr(host, n).copy() for n in host.available_dense_fragment_dfs()})
    with np.errstate(invalid="ignore"):
        T.host_normalize_rt_delta_max(post)
    T.host_ms2_quality_control(post)
    G.assert_libraries_identical(acc.consensus_speclibase, post)
    assert acc.consensus_speclibase.precursor_df["use_for_ms2"].mean() > 0.1
    acc.close()


@pytest.mark.parametrize("n_columns", [3, 4])
def test_quality_control_at_the_wavefront_slice(n_columns):
    """slice - 1, slice and slice + 1 masked cells, a block of 5 000 on the workgroup path, beside small blocks."""
    rng = np.random.default_rng(8)
    s = T.QC_LDS_SLICE
    counts = [s - 1, 5, s, 0, s + 1, 64, 5000, 1, 2 * s]
    inten, corr, start, stop, row = [], [], [], [], 0
    for m in counts:
        rows = -(-m // n_columns) + 2
        i = np.zeros(rows * n_columns, np.float32)
        i[rng.permutation(rows * n_columns)[:m]] = rng.lognormal(8, 1, m).astype(np.float32)
        c = (np.float32(0.125) * rng.integers(0, 9, rows * n_columns)).astype(np.float32)  # ties around the middle
        c[::7] = rng.uniform(0, 1, len(c[::7])).astype(np.float32)
        inten.append(i), corr.append(c), start.append(row), stop.append(row + rows)
        row += rows
    order = rng.permutation(len(counts))

    def lib():
        cols = [f"c{k}" for k in range(n_columns)]
        prec = pd.DataFrame({"frag_start_idx": np.asarray(start)[order], "frag_stop_idx": np.asarray(stop)[order]})
        return G.Library(prec, {
            "_fragment_intensity_df": pd.DataFrame(np.concatenate(inten).reshape(-1, n_columns), columns=cols),
            "_fragment_correlation_df": pd.DataFrame(np.concatenate(corr).reshape(-1, n_columns), columns=cols)})

    got = T.ms2_quality_control(lib(), 0.6, 0.9)
    assert T.last_timing["qc_large_blocks"] == 3
    for looped in (False, True):
        exp = T.host_ms2_quality_control(lib(), 0.6, 0.9, looped=looped)
        G.assert_frames_identical(got.precursor_df, exp.precursor_df)
        G.assert_frames_identical(got.fragment_intensity_df, exp.fragment_intensity_df)
    assert got.precursor_df["use_for_ms2"].any() and not got.precursor_df["use_for_ms2"].all()


@pytest.fixture(scope="module")
def flat_cohort():
    rng = np.random.default_rng(9)
    return [G.flat_tables(G.cohort_run(rng, r, 300, strings=False), rng) for r in range(3)]


def test_add_run_equals_host_scatter_then_update(flat_cohort):
    a, b = T.HipTransferLearningAccumulator(keep_top=2), T.HipTransferLearningAccumulator(keep_top=2)
    host = None
    for psm, frag, expect in flat_cohort:
        a.add_run(psm, frag, G.FRAG_TYPES)
        prec, n_rows, row, col, mz, inten, corr = T.flat_run(psm, frag, G.FRAG_TYPES)
        mats = T.host_scatter_dense(n_rows, len(G.FRAG_TYPES), row, col, mz, inten, corr)
        for m, name in zip(mats, G.DENSE):  # what the scatter builds is what the run held
            assert np.array_equal(m.view(np.uint32), getattr(expect, name).to_numpy().view(np.uint32)), name
        b.update(T._FlatLibrary(prec, G.FRAG_TYPES, mats))
        host = T.host_add_run(host, psm, frag, G.FRAG_TYPES, keep_top=2)
        G.assert_libraries_identical(a.consensus_speclibase, b.consensus_speclibase)
        G.assert_libraries_identical(a.consensus_speclibase, host)
    assert (a.consensus_speclibase.precursor_df["decoy"] == 0).all()
    a.close(), b.close()


def test_reference_calling_sequence_equals_add_run(flat_cohort):
    """``update`` per run from library objects and ``post_process``, as the reference's broadcaster drives it."""
    a, b = T.HipTransferLearningAccumulator(), T.HipTransferLearningAccumulator()
    for psm, frag, _ in flat_cohort:
        a.add_run(psm, frag, G.FRAG_TYPES)
        prec, n_rows, row, col, mz, inten, corr = T.flat_run(psm, frag, G.FRAG_TYPES)
        b.update(T._FlatLibrary(prec, G.FRAG_TYPES, T.host_scatter_dense(n_rows, 4, row, col, mz, inten, corr)))
    a.post_process(), b.post_process()
    G.assert_libraries_identical(a.consensus_speclibase, b.consensus_speclibase)
    assert {"rt_norm", "use_for_ms2"} <= set(a.consensus_speclibase.precursor_df.columns)
    a.close(), b.close()


def test_a_cell_written_twice_raises(flat_cohort):
    psm, frag, _ = flat_cohort[0]
    targets = psm.loc[psm["decoy"] == 0, "precursor_idx"]
    placed = frag[(frag["type"] != ord("c")) & frag["precursor_idx"].isin(targets)]
    twice = pd.concat([frag, placed.iloc[[7]]], ignore_index=True)
    acc = T.HipTransferLearningAccumulator()
    with pytest.raises(ValueError, match="one cell"):
        acc.add_run(psm, twice, G.FRAG_TYPES)
    assert acc.consensus_speclibase is None
    acc.add_run(psm, frag, G.FRAG_TYPES)  # the accumulator is still usable
    assert len(acc.consensus_speclibase.precursor_df) == int((psm["decoy"] == 0).sum())
    acc.close()


def test_post_process_without_rt_calibrated_falls_back_to_max(caplog):
    g = G.load("chain")
    acc = T.HipTransferLearningAccumulator()
    host = None
    for run in g["runs"]:
        run._precursor_df = run.precursor_df.drop(columns=["rt_calibrated"])
        acc.update(run)
        host = T.host_update(host, run, 3)
    with caplog.at_level(logging.WARNING):
        acc.post_process()
    assert any("delta-max normalization will not be performed" in r.getMessage() for r in caplog.records)
    T.host_ms2_quality_control(T.host_normalize_rt_max(host))
    G.assert_libraries_identical(acc.consensus_speclibase, host)
    acc.close()


def test_update_refuses_what_it_cannot_take():
    g = G.load("topk_k1")
    run = g["runs"][0]
    acc = T.HipTransferLearningAccumulator()
    bad = G.Library(run.precursor_df.assign(frag_stop_idx=run.precursor_df["frag_stop_idx"] + 10_000),
                    {n: getattr(run, n) for n in run.available_dense_fragment_dfs()})
    with pytest.raises(Exception, match="outside the run's matrices"):
        acc.update(bad)
    f64 = G.Library(run.precursor_df, {n: getattr(run, n).astype(np.float64) for n in run.available_dense_fragment_dfs()})
    with pytest.raises(TypeError, match="float32"):
        acc.update(f64)
