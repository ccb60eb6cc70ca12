"""One session object reused across inputs of very different sizes (csrc/adh_session.h: DevArray growth, DevBufs
release) gives what a fresh session gives on the same input, bit for bit, and its timers stay sane.  The grouping
and MBR sessions have their reuse tests in test_grouping_gpu.py and test_mbr_library_gpu.py."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = {"quant": (5_000, 40, 9_000), "tl": (2_000, 30, 3_000), "pfdr": (3_000, 50, 4_000)}


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def sane(times):
    return all(np.isfinite(t) and t >= 0.0 for t in times)


# ---- quant: the per-run scratch and the appended rows regrow; build and two filters share the work buffer -----------

N_PSM = 4_000


def quant_run(rng, n_kept):
    """A run of which exactly n_kept rows belong to PSM precursors (precursor_idx < N_PSM), with distinct keys."""
    n = n_kept + n_kept // 4 + 7
    cell = rng.permutation(N_PSM * 40)[:n_kept]  # (precursor, fragment number) pairs, each once
    p = np.concatenate([cell // 40, rng.integers(N_PSM, N_PSM + 500, n - n_kept)]).astype(np.uint32)
    number = np.concatenate([cell % 40 + 1, rng.integers(1, 41, n - n_kept)]).astype(np.uint8)
    order = rng.permutation(n)
    corr = rng.random(n, dtype=np.float32)
    corr[rng.random(n) < 0.02] = np.nan
    cols = [rng.lognormal(8, 1, n).astype(np.float32)[order], corr[order]]
    one = np.ones(n, np.uint8)
    return p[order], number[order], one * 98, one, one * 0, cols


def test_quant_session_reused_across_sizes(ctx):
    rng = np.random.default_rng(11)
    psm = np.arange(N_PSM, dtype=np.uint32)
    runs = [quant_run(rng, k) for k in SIZES["quant"]]
    one = ctx.quant_matrices(2, psm)
    fresh_rows = []
    try:
        for k, run in zip(SIZES["quant"], runs):
            assert one.add_run(*run) == k
            f = ctx.quant_matrices(2, psm)
            try:
                assert f.add_run(*run) == k
                fresh_rows.append(f.rows())
            finally:
                f.close()
        ion, pidx, run_id, cols = one.rows()
        assert same(ion, np.concatenate([r[0] for r in fresh_rows]))
        assert same(pidx, np.concatenate([r[1] for r in fresh_rows]))
        assert np.array_equal(run_id, np.repeat(np.arange(3, dtype=np.uint32), SIZES["quant"]))
        for c in range(2):
            assert same(cols[c], np.concatenate([r[3][c] for r in fresh_rows]))

        n_keys, dup = one.build()
        assert not dup and 9_000 <= n_keys <= sum(SIZES["quant"])
        group_a = (one.keys()[1] // 3).astype(np.int32)
        group_b = (one.keys()[1] % 97).astype(np.int32)
        group_b[::50] = -1
        got_a = one.filter(1, group_a, int(group_a.max()) + 1, 3, 0.7)
        got_b = one.filter(1, group_b, 97, 2, 0.9)
        assert sane(one.time_ms())
        # fresh objects of two sizes take the matrix from the host: all keys, and the keys of a few precursors
        quality = one.matrix(1)
        few = np.flatnonzero(one.keys()[1] < 12)
        assert 0 < len(few) < 400
        for rows, group, n_groups, top_n, thr, exp in ((slice(None), group_a, int(group_a.max()) + 1, 3, 0.7, got_a),
                                                       (slice(None), group_b, 97, 2, 0.9, got_b)):
            f = ctx.quant_matrices(1, psm)
            try:
                f.set_matrix(list(quality[:, rows]))
                got = f.filter(0, group[rows], n_groups, top_n, thr)
                assert sane(f.time_ms())
            finally:
                f.close()
            for x, y in zip(got, exp):
                assert same(x, y)
        f = ctx.quant_matrices(1, psm)
        try:
            f.set_matrix(list(quality[:, few]))
            small = f.filter(0, group_a[few], int(group_a.max()) + 1, 3, 0.7)
        finally:
            f.close()
        # groups of group_a are whole precursors, so the few precursors' rows rank as they do among all keys
        for x, y in zip(small, got_a):
            assert same(x, y[few])
    finally:
        one.close()


# ---- transfer library: the consensus shrinks and grows under one session ---------------------------------------------

TL_COLUMNS, TL_MATRICES, KEEP_TOP = 4, 3, 2


def tl_run(rng, n, pool):
    rows = rng.integers(1, 4, n)
    stop = np.cumsum(rows).astype(np.int64)
    start = stop - rows
    proba = rng.random(n)
    proba[rng.random(n) < 0.05] = np.nan
    mats = [rng.random((int(stop[-1]), TL_COLUMNS), dtype=np.float32) for _ in range(TL_MATRICES)]
    return dict(hash=rng.integers(0, pool, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15), proba=proba,
                pidx=rng.integers(0, 1 << 40, n).astype(np.int64), start=start, stop=stop, mats=mats)


def tl_concat(a, b):
    if a is None:
        return b
    r0 = a["mats"][0].shape[0]
    return dict(hash=np.concatenate([a["hash"], b["hash"]]), proba=np.concatenate([a["proba"], b["proba"]]),
                pidx=np.concatenate([a["pidx"], b["pidx"]]), start=np.concatenate([a["start"], b["start"] + r0]),
                stop=np.concatenate([a["stop"], b["stop"] + r0]),
                mats=[np.vstack([x, y]) for x, y in zip(a["mats"], b["mats"])])


def tl_update(s, run):
    kept, start, stop = s.update(KEEP_TOP, run["hash"], run["proba"], run["pidx"], run["start"], run["stop"],
                                 run["mats"][0].shape[0], run["mats"])
    return kept, start, stop, [s.matrix(m) for m in range(TL_MATRICES)]


def test_transfer_library_session_reused_across_sizes(ctx):
    rng = np.random.default_rng(12)
    one = ctx.transfer_library(TL_COLUMNS, TL_MATRICES)
    consensus = None
    try:
        for n in SIZES["tl"]:
            run = tl_run(rng, n, pool=max(n // 3, 8))  # about three candidates per peptide, two are kept
            kept, start, stop, mats = tl_update(one, run)
            assert sane(one.time_ms())
            # a fresh session takes the consensus so far and the run as one run: the same rows in the same order
            both = tl_concat(consensus, run)
            fresh = ctx.transfer_library(TL_COLUMNS, TL_MATRICES)
            try:
                f_kept, f_start, f_stop, f_mats = tl_update(fresh, both)
            finally:
                fresh.close()
            assert 0 < len(kept) < len(both["hash"])
            assert same(kept, f_kept) and same(start, f_start) and same(stop, f_stop)
            for x, y in zip(mats, f_mats):
                assert same(x, y)
            consensus = dict(hash=both["hash"][kept], proba=both["proba"][kept], pidx=both["pidx"][kept], start=start,
                             stop=stop, mats=mats)
    finally:
        one.close()


# ---- protein FDR: the buffers of the last features call are released and allocated anew ------------------------------


def pfdr_table(rng, n):
    pg = rng.integers(-1, max(n // 6, 3), n).astype(np.int32)
    return (pg, (rng.random(n) < 0.3).astype(np.uint8), rng.integers(0, 1 << 40, n).astype(np.int64),
            rng.integers(0, 200, n).astype(np.int32), rng.integers(0, 6, n).astype(np.int32), rng.random(n))


def test_protein_fdr_session_reused_across_sizes(ctx):
    rng = np.random.default_rng(13)
    one = ctx.protein_fdr()
    try:
        for n in SIZES["pfdr"]:
            table = pfdr_table(rng, n)
            got = one.features(*table, with_row_group=True)
            value = rng.random(one.n_groups)
            rows = one.gather(value)
            assert sane(one.time_ms())
            fresh = ctx.protein_fdr()
            try:
                exp = fresh.features(*table, with_row_group=True)
                exp_rows = fresh.gather(value)
            finally:
                fresh.close()
            for x, y in zip(got, exp):
                assert same(x, y)
            assert same(rows, exp_rows)
    finally:
        one.close()


def test_protein_fdr_epoch_time_adds_up(ctx):
    rng = np.random.default_rng(14)
    n = 300  # two batches of the classifier
    s = ctx.protein_fdr()
    try:
        s.fit_begin(rng.standard_normal((n, s.N_FEATURES)), rng.integers(0, 2, n).astype(np.uint8),
                    rng.standard_normal(s.N_PARAMS) * 0.1)
        assert s.time_ms()[1] == 0.0
        step = np.full(2, 1e-3)
        s.epoch(rng.permutation(n).astype(np.int32), step)
        first = s.time_ms()[1]
        s.epoch(rng.permutation(n).astype(np.int32), step)
        second = s.time_ms()[1]
        assert sane(s.time_ms()) and first > 0.0 and second >= first
        s.predict(rng.standard_normal((7, s.N_FEATURES)))
        assert sane(s.time_ms()) and s.time_ms()[1] == second
    finally:
        s.close()
