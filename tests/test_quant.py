"""Host side of the cross-run fragment quantity matrices (alphadia_amd/quant.py): the host restatement of the
reference's merges against the goldens, the duplicate-key path, the folder reader and the threshold rounding.
No GPU needed."""

from __future__ import annotations

import logging

import numpy as np
import pandas as pd
import pytest

import quant_golden as G
from alphadia_amd import quant as Q


@pytest.mark.parametrize("case", G.cases())
def test_host_accumulate_equals_reference(case):
    runs, psm, frames, _, _ = G.load(case)
    got = Q.host_accumulate(iter(runs), psm[psm["decoy"] == 0])
    for q in ("intensity", "correlation"):
        G.assert_frames_identical(got[q], frames[q])


def test_duplicate_key_case_is_a_cartesian_product():
    runs, psm, frames, _, _ = G.load("dup_key")
    ions = Q.ion_hash(*(runs[1][1][c].values for c in ("precursor_idx", *Q.KEY_COLUMNS)))
    assert len(np.unique(ions)) == len(ions) - 1
    assert len(frames["intensity"]) > len(np.unique(frames["intensity"]["ion"]))


def test_ion_hash_is_int64_for_uint8_columns():
    u8 = lambda *v: np.array(v, dtype=np.uint8)  # noqa: E731
    h = Q.ion_hash(np.array([7, 7, 7], dtype=np.uint32), u8(1, 2, 1), u8(98, 98, 121), u8(1, 1, 2), u8(0, 18, 200))
    assert h.dtype == np.int64 and len(set(h.tolist())) == 3
    assert h[0] == 7 + (1 << 32) + (98 << 40) + (1 << 48)
    assert h[2] < 0  # loss_type >= 128 wraps, as int64 arithmetic does


def test_host_filter_restatement_matches_goldens():
    """total (bit for bit), rank and the kept rows of every golden filter call; the sequential float32 sum over the
    runs that the kernel uses gives the same totals."""
    for case in G.cases():
        if case == "dup_key":
            continue
        runs, psm, frames, calls, meta = G.load(case)
        inten, qual = frames["intensity"], frames["correlation"]
        m = qual[meta["runs"]].to_numpy()
        seq = m[:, 0].copy()
        for r in range(1, m.shape[1]):
            seq += m[:, r]
        seq /= np.float32(m.shape[1])
        for group, top_n, min_corr, total, rank, keep in calls:
            fi, fq = Q.host_filter_frag_df(inten, qual, min_correlation=min_corr, top_n=top_n, group_column=group)
            assert np.array_equal(qual["total"].to_numpy().view(np.uint32), total.view(np.uint32))
            assert np.array_equal(seq.view(np.uint32), total.view(np.uint32))
            np.testing.assert_array_equal(qual["rank"].to_numpy(), rank)
            assert np.array_equal(fq.index.to_numpy(), keep) and fi.index.equals(fq.index)


def test_golden_cases_cover_the_issue():
    seen = {}
    for case in G.cases():
        runs, psm, frames, calls, meta = G.load(case)
        seen[case] = len(runs)
        qual = frames["correlation"]
        if len(runs) > 1:
            present = np.stack([np.isin(frames["intensity"]["ion"], Q.ion_hash(
                *(df[c].values for c in ("precursor_idx", *Q.KEY_COLUMNS)))) for _, df in runs])
            if case != "dup_key":
                assert not present.all()  # ions missing from some runs
        assert any(df["correlation"].isna().any() for _, df in runs) or case == "dup_key"
        assert sum(len(df) for _, df in runs) > sum((df["precursor_idx"].isin(psm["precursor_idx"])).sum()
                                                    for _, df in runs)  # PSMs remove rows
        assert {c[0] for c in calls} == set(Q.METADATA_COLUMNS)
        if case == "five_runs":  # a group with exactly top_n fragments
            assert any((qual.groupby(g).size() == t).any() for g, t, *_ in calls)
    assert {1, 2, 5}.issubset(set(seen.values()))
    _, _, frames, calls, _ = G.load("two_runs")
    assert any((t == np.float32(c[2])).any() for c in calls for t in [c[3]])  # a total equal to min_correlation


def test_threshold_is_rounded_like_numpy_compares():
    t = np.array([0.1, 0.5], dtype=np.float32)
    for thr in (0.1, 0.5, np.float64(0.1), np.float32(0.1), 0):
        assert np.array_equal(t > thr, t.astype(np.float64) > Q._threshold(thr))


def test_frag_reader_skips_missing_and_unreadable(tmp_path, caplog):
    runs, _, _, _, _ = G.load("two_runs")
    folders = []
    for name, df in runs:
        d = tmp_path / name
        d.mkdir()
        df.to_parquet(d / "frag.parquet")
        folders.append(str(d))
    missing = tmp_path / "missing_run"
    missing.mkdir()
    broken = tmp_path / "broken_run"
    broken.mkdir()
    (broken / "frag.parquet").write_bytes(b"not a parquet file")
    with caplog.at_level(logging.WARNING):
        got = list(Q.HipFragmentQuantLoader._frag_df_generator([folders[0], str(missing), str(broken), folders[1]]))
    assert [n for n, _ in got] == [runs[0][0], runs[1][0]]
    for (_, a), (_, b) in zip(got, runs):
        pd.testing.assert_frame_equal(a, b)
    assert any("no frag file found for missing_run" in r.getMessage() for r in caplog.records)
    assert any("Error reading frag file for broken_run" in r.getMessage() for r in caplog.records)
