"""The cross-run fragment quantity matrices on the GPU (alphadia_amd/quant.py, csrc/adh_quant.hip): the accumulated
frames and every filter call equal the reference's goldens exactly; a 60-run cohort of 1.2 M keys against a host
restatement; the folder reader."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import quant_golden as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", G.cases())
def test_accumulate_and_filter_equal_reference(case):
    from alphadia_amd import quant as Q

    runs, psm, frames, calls, meta = G.load(case)
    loader = Q.HipFragmentQuantLoader(psm[psm["decoy"] == 0])
    got = loader.accumulate(iter(runs))
    for q in ("intensity", "correlation"):
        G.assert_frames_identical(got[q], frames[q])
    # the device path keeps the matrices for the filter; a run with a key twice takes the host merges
    assert (Q._resident(got["correlation"], meta["runs"]) is not None) == (case != "dup_key")
    exp_i, exp_q = frames["intensity"], frames["correlation"]
    for group, top_n, min_corr, total, rank, keep in calls:
        fi, fq = Q.filter_frag_df(got["intensity"], got["correlation"], min_correlation=min_corr, top_n=top_n,
                                  group_column=group)
        qd = got["correlation"]
        assert qd["total"].dtype == np.float32 and qd["rank"].dtype == np.float64
        assert np.array_equal(qd["total"].to_numpy().view(np.uint32), total.view(np.uint32))
        np.testing.assert_array_equal(qd["rank"].to_numpy(), rank)
        assert np.array_equal(fq.index.to_numpy(), keep)
        ri, rq = Q.host_filter_frag_df(exp_i, exp_q, min_correlation=min_corr, top_n=top_n, group_column=group)
        G.assert_frames_identical(fi, ri)
        G.assert_frames_identical(fq, rq)


def test_filter_of_an_uploaded_frame_equals_resident():
    from alphadia_amd import quant as Q

    runs, psm, frames, calls, meta = G.load("twelve_runs")
    got = Q.HipFragmentQuantLoader(psm[psm["decoy"] == 0]).accumulate(iter(runs))
    copy_i, copy_q = got["intensity"].copy(), got["correlation"].copy()
    assert Q._resident(copy_q, meta["runs"]) is None
    for group, top_n, min_corr, *_ in calls:
        a = Q.filter_frag_df(got["intensity"], got["correlation"], min_corr, top_n, group)
        b = Q.filter_frag_df(copy_i, copy_q, min_corr, top_n, group)
        for x, y in zip(a, b):
            G.assert_frames_identical(x, y)


def _cohort(n_runs, n_prec=100_000, n_frag=12, present=0.8, seed=0):
    """Synthetic cohort: n_prec precursors with n_frag fragments each, a `present` fraction per run, rows shuffled."""
    rng = np.random.default_rng(seed)
    psm = pd.DataFrame({"precursor_idx": np.arange(n_prec, dtype=np.uint32)})
    psm["pg"] = np.array([f"PG{i // 6}" for i in range(n_prec)], dtype=object)
    psm["mod_seq_hash"] = (np.arange(n_prec, dtype=np.uint64) // np.uint64(3)) * np.uint64(2654435761)
    psm["mod_seq_charge_hash"] = psm["mod_seq_hash"] + np.arange(n_prec, dtype=np.uint64) % np.uint64(3)
    f = np.arange(n_frag)
    runs = []
    for r in range(n_runs):
        p = np.flatnonzero(rng.random(n_prec) < present).astype(np.uint32)
        pp = np.repeat(p, n_frag)
        ff = np.tile(f, len(p))
        order = rng.permutation(len(pp))
        n = len(pp)
        corr = rng.random(n, dtype=np.float32)
        corr[rng.random(n) < 0.01] = np.nan
        runs.append((f"run_{r:03d}", pd.DataFrame({
            "precursor_idx": pp[order], "number": (ff[order] // 2 + 1).astype(np.uint8),
            "type": (98 + 23 * (ff[order] % 2)).astype(np.uint8), "charge": np.ones(n, np.uint8),
            "loss_type": np.where(ff[order] % 4 == 3, 18, 0).astype(np.uint8),
            "intensity": rng.lognormal(10, 1, n).astype(np.float32), "correlation": corr,
        })))
    return psm, runs


def test_sixty_runs_against_host_restatement():
    """60 runs x 100 000 precursors x 12 fragments (1.2 M keys): the union, the matrices and the three filters
    against a NumPy / pandas restatement (sorted union, one searchsorted per run, np.mean and groupby rank)."""
    from alphadia_amd import quant as Q

    psm, runs = _cohort(60)
    got = Q.HipFragmentQuantLoader(psm).accumulate(iter(runs))
    ions = [Q.ion_hash(*(df[c].values for c in ("precursor_idx", *Q.KEY_COLUMNS))) for _, df in runs]
    union = np.unique(np.concatenate(ions))
    assert len(union) == 1_200_000
    qi, qc = got["intensity"], got["correlation"]
    assert np.array_equal(qi["ion"].to_numpy(), union) and qi["precursor_idx"].dtype == np.uint32
    assert np.array_equal(qi["precursor_idx"].to_numpy(), (union & 0xFFFFFFFF).astype(np.uint32))
    for r, (name, df) in enumerate(runs):
        at = np.searchsorted(union, ions[r])
        for q, frame in (("intensity", qi), ("correlation", qc)):
            col = np.zeros(len(union), np.float32)
            col[at] = np.nan_to_num(df[q].to_numpy(), nan=0.0)
            assert np.array_equal(frame[name].to_numpy().view(np.uint32), col.view(np.uint32)), (name, q)
    assert list(qc.columns[-3:]) == Q.METADATA_COLUMNS and qc["pg"].dtype == object
    meta = psm.set_index("precursor_idx").loc[qc["precursor_idx"].to_numpy()]
    assert np.array_equal(qc["pg"].to_numpy(), meta["pg"].to_numpy())
    ref_i, ref_q = qi.copy(), qc.copy()
    for group in ("mod_seq_charge_hash", "mod_seq_hash", "pg"):
        fi, fq = Q.filter_frag_df(qi, qc, min_correlation=0.5, top_n=3, group_column=group)
        ri, rq = Q.host_filter_frag_df(ref_i, ref_q, min_correlation=0.5, top_n=3, group_column=group)
        assert np.array_equal(qc["total"].to_numpy().view(np.uint32), ref_q["total"].to_numpy().view(np.uint32))
        np.testing.assert_array_equal(qc["rank"].to_numpy(), ref_q["rank"].to_numpy())
        assert fi.index.equals(ri.index) and fq.index.equals(rq.index) and len(fq) > 0


def test_accumulate_from_folders(tmp_path):
    from alphadia_amd import quant as Q

    runs, psm, frames, _, _ = G.load("five_runs")
    folders = []
    for name, df in runs:
        d = tmp_path / name
        d.mkdir()
        df.to_parquet(d / "frag.parquet")
        folders.append(str(d))
    missing = tmp_path / "run_without_frag"
    missing.mkdir()
    folders.insert(2, str(missing))
    got = Q.HipFragmentQuantLoader(psm[psm["decoy"] == 0]).accumulate_from_folders(folders)
    for q in ("intensity", "correlation"):
        G.assert_frames_identical(got[q], frames[q])
    assert Q.HipFragmentQuantLoader(psm).accumulate_from_folders([str(missing)]) is None
