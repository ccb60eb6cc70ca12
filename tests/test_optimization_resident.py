"""Resident optimisation steps, host side (no GPU): HipOptimizationLock's batch plan, elution-group order and batch
library, the accumulated tables' growth rule and relayout arithmetic against the table layout of the library, and the
fallback of HipExtractionHandler.process_optimization_batch to the chained calls."""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from alphadia_amd.optimization import (HipOptimizationLock, append_geometry, filter_fragments_for_calibration,
                                       relayout_rows, remove_unused_fragments)


def _library(eg):
    n = len(eg)
    lengths = np.arange(n) % 4 + 1
    stop = np.cumsum(lengths)
    pre = pd.DataFrame({"precursor_idx": np.arange(n), "elution_group_idx": np.asarray(eg),
                        "flat_frag_start_idx": (stop - lengths).astype(np.int64), "flat_frag_stop_idx": stop.astype(np.int64)})
    frag = pd.DataFrame({"mz_library": np.arange(int(stop[-1]), dtype=np.float32) + 100.0})
    return SimpleNamespace(_precursor_df=pre, _fragment_df=frag)


CONFIG = {"calibration": {"optimization_lock_target": 10, "batch_size": 2}}
EG = [12, 12, 3, 8, 8, 1, 9, 2, 7, 0, 4, 6, 11, 5, 10, 13, 14, 15, 16, 17]


def test_lock_batch_plan_and_order_follow_the_reference_rule():
    lock = HipOptimizationLock(_library(EG), CONFIG)
    # the reference's rule: unique elution groups in order of appearance, shuffled by default_rng(772)
    assert lock._elution_group_order.tolist() == [7, 2, 17, 4, 14, 5, 13, 11, 6, 8, 16, 1, 3, 10, 12, 15, 9, 0]
    assert lock.batch_plan == [(0, 2), (2, 6), (6, 14), (14, 18)]
    assert HipOptimizationLock._get_batch_plan(1000, 100) == [(0, 100), (100, 300), (300, 700), (700, 1000)]
    assert HipOptimizationLock._get_batch_plan(5, 10) == [(0, 5)]
    assert (lock.start_idx, lock.stop_idx) == (0, 2) and lock.batches_remaining()
    assert sorted(lock.batch_library.precursor_df["elution_group_idx"].unique()) == [2, 7]
    lock.update_with_fdr(pd.DataFrame({"qval": [0.001] * 3, "decoy": [0] * 3}))
    assert not lock.has_target_num_precursors
    lock.update()
    assert (lock.batch_idx, lock.start_idx, lock.stop_idx) == (1, 2, 6)
    # target reached with 20 of 10 wanted: the smallest step whose stop covers 6 * 10 / 20 = 3 groups
    lock.update_with_fdr(pd.DataFrame({"qval": [0.001] * 20, "decoy": [0] * 20}))
    assert lock.has_target_num_precursors
    lock.update()
    assert (lock.batch_idx, lock.start_idx, lock.stop_idx) == (1, 0, 6)
    assert lock.n_features == 0 and lock.n_fragments == 0


def test_batch_library_renumbers_the_fragments():
    lib = _library(EG)
    pre = lib._precursor_df[lib._precursor_df["elution_group_idx"].isin([8, 2])]
    got_pre, (got_frag,) = remove_unused_fragments(pre, (lib._fragment_df,))
    # precursors 3, 4 (slices [6, 10), [10, 11)) and 7 (slice [16, 20)) keep their order and index
    assert got_pre.index.tolist() == [3, 4, 7]
    assert got_pre["flat_frag_start_idx"].tolist() == [0, 4, 5]
    assert got_pre["flat_frag_stop_idx"].tolist() == [4, 5, 9]
    assert got_pre["flat_frag_start_idx"].dtype == np.int64
    assert got_frag["mz_library"].tolist() == [106, 107, 108, 109, 110, 116, 117, 118, 119]
    assert got_frag.index.tolist() == list(range(9))


def test_append_geometry_grows_geometrically():
    # a doubling batch plan of 100 candidates per group: the rows moved by relayouts stay below twice the total
    cap = top_k = live = moved = 0
    for n, w in [(100, 6), (200, 6), (400, 12), (800, 12), (1600, 9), (3200, 12)]:
        new_cap, new_w, relayout = append_geometry(live, cap, top_k, n, w)
        assert new_cap >= live + n and new_w == max(top_k, w)
        if relayout:
            moved += live
        cap, top_k, live = new_cap, new_w, live + n
    assert moved < 2 * live
    assert append_geometry(0, 5000, 12, 10, 3) == (10, 3, False)  # (an empty table takes the batch's layout)
    assert append_geometry(10, 20, 12, 10, 3) == (20, 12, False)
    assert append_geometry(10, 20, 12, 11, 3) == (40, 12, True)
    assert append_geometry(10, 20, 6, 5, 7) == (20, 7, True)


def _pack(rows, cap, top_k, seed):
    """A packed table buffer as runtime.table_layout lays it out, rows [0, rows) filled, and its fields."""
    from alphadia_amd import runtime

    fields, total, _ = runtime.table_layout(cap, top_k)
    buf = np.zeros(total, np.uint8)
    rng = np.random.default_rng(seed)
    for f in fields:
        width = f["row_elems"]
        nbytes = rows * width * f["elem_bytes"]
        buf[f["offset"]: f["offset"] + nbytes] = rng.integers(1, 255, nbytes, dtype=np.uint8)
    return buf, fields


def _field(buf, f, rows):
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[f["elem_bytes"]]
    return buf[f["offset"]: f["offset"] + rows * f["row_elems"] * f["elem_bytes"]].view(dt)


def test_relayout_arithmetic_matches_the_table_layout():
    """Appending B (3 rows, 7 slots) behind A (5 rows, 4 slots, capacity 5) moves A into a layout of capacity 10 and
    width 7: every field of the result holds A's rows, then B's, as one layout of 8 rows of width 7 would."""
    a, fa = _pack(5, 5, 4, seed=1)
    b, fb = _pack(3, 3, 7, seed=2)
    cap, width, relayout = append_geometry(5, 5, 4, 3, 7)
    assert (cap, width, relayout) == (10, 7, True)
    out, fo = _pack(0, cap, width, seed=3)
    for f_a, f_b, f_o in zip(fa, fb, fo, strict=True):
        assert f_a["name"] == f_b["name"] == f_o["name"]
        per_row = f_o["row_elems"] != width or f_a["row_elems"] == f_b["row_elems"]
        dst = _field(out, f_o, cap)
        wa, wb, wo = f_a["row_elems"], f_b["row_elems"], f_o["row_elems"]
        relayout_rows(_field(a, f_a, 5), wa, dst, wo, 5, 0)
        relayout_rows(_field(b, f_b, 3), wb, dst, wo, 3, 5)
        got = dst[: 8 * wo].reshape(8, wo)
        exp_a = _field(a, f_a, 5).reshape(5, wa)
        exp_b = _field(b, f_b, 3).reshape(3, wb)
        assert np.array_equal(got[:5, :wa], exp_a) and np.array_equal(got[5:, :wb], exp_b), f_o["name"]
        if not per_row:
            assert (got[:5, wa:] == 0).all() and (got[5:, wb:] == 0).all(), f_o["name"]
        # the fields stay inside their own region of the new layout
        assert f_o["offset"] + cap * wo * f_o["elem_bytes"] <= (fo[fo.index(f_o) + 1]["offset"] if f_o is not fo[-1] else len(out))


def test_filter_fragments_for_calibration_is_filter_dfs():
    rng = np.random.default_rng(4)
    frag = pd.DataFrame({"precursor_idx": rng.integers(0, 30, 400), "mass_error": rng.normal(0, 150, 400),
                         "correlation": np.round(rng.random(400), 2)})
    got = filter_fragments_for_calibration(frag, [1, 2, 3, 5, 8, 13, 21], 0.5, 20)
    sel = frag[frag["precursor_idx"].isin([1, 2, 3, 5, 8, 13, 21]) & (frag["mass_error"].abs() <= 200)]
    sel = sel.sort_values(by=["correlation", "precursor_idx"], ascending=False)
    assert got.equals(sel.head(min(int((sel["correlation"] > 0.5).sum()), 20)))
    assert len(got) == 20


class _FakeFdr:
    def __init__(self):
        self.calls = []

    def fit_predict(self, features_df, decoy_strategy, competitive, df_fragments=None, version=-1):
        self.calls.append((len(features_df), decoy_strategy, len(df_fragments)))
        out = features_df.copy()
        out["qval"] = 0.001
        return out


def _handler(fdr_manager, channel_wise=False):
    from alphadia_amd.extraction_handler import HipExtractionHandler

    config = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                         "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
              "general": {"thread_count": 4},
              "fdr": {"fdr": 0.01, "competitive_scoring": True, "channel_wise_fdr": channel_wise},
              "calibration": {"min_correlation": 0.5, "max_fragments": 5}}
    log = []
    reporter = SimpleNamespace(log_string=lambda msg, **k: log.append(msg))
    selection = SimpleNamespace(select_candidates=lambda dia, lib, apply_cutoff=False: pd.DataFrame({"x": [1]}))
    names = SimpleNamespace()
    h = HipExtractionHandler(config, SimpleNamespace(classifier_version=-1), fdr_manager, reporter, names,
                             selection_handler=selection, device=0)
    h.log = log
    return h, config


@pytest.mark.parametrize("channel_wise", [True, False])
def test_optimization_step_falls_back_to_the_chained_calls(channel_wise):
    """Channel-wise FDR, or an FDR manager that is not a HipFDRManager, take the chained calls (logged once): the
    lock then holds host frames as the reference's does."""
    fdr = _FakeFdr()
    h, config = _handler(fdr, channel_wise=channel_wise)
    lock = HipOptimizationLock(_library(EG), CONFIG)

    def score(cands, dia, lib):
        pidx = lib.precursor_df["precursor_idx"].to_numpy()
        feats = pd.DataFrame({"precursor_idx": pidx, "rank": 0, "decoy": 0,
                              "elution_group_idx": lib.precursor_df["elution_group_idx"].to_numpy()})
        frags = pd.DataFrame({"precursor_idx": np.repeat(pidx, 2), "mass_error": 1.0,
                              "correlation": np.linspace(0.4, 0.9, 2 * len(pidx))})
        return feats, frags

    h.score_and_quantify_candidates = score
    psm = h.process_optimization_batch(None, lock)
    lock.update()
    psm = h.process_optimization_batch(None, lock)
    reasons = [m for m in h.log if m.startswith("Resident optimisation step not used")]
    assert len(reasons) == 1
    assert ("channel-wise" in reasons[0]) == channel_wise and ("_FakeFdr" in reasons[0]) == (not channel_wise)
    n2, n6 = 2, int(lock._library._precursor_df["elution_group_idx"].isin(lock._elution_group_order[:6]).sum())
    assert [c[0] for c in fdr.calls] == [
        int(lock._library._precursor_df["elution_group_idx"].isin(lock._elution_group_order[:2]).sum()), n6]
    assert fdr.calls[0][1] == ("precursor_channel_wise" if channel_wise else "precursor")
    assert lock.n_features == len(psm) == n6 and lock.n_fragments == 2 * n6 and n2 == 2
    assert lock.total_elution_groups == 6
    pre, frag = h.filter_for_calibration(psm, config)
    assert len(pre) == len(psm) and len(frag) == 5
    assert frag["correlation"].is_monotonic_decreasing


def test_fallback_reason_is_logged_once_per_lock():
    """The workflow creates an extraction handler per optimisation step: the fallback reason is logged once for the
    lock, not once per handler."""
    lock = HipOptimizationLock(_library(EG), CONFIG)
    logs = []
    for _ in range(2):
        h, _config = _handler(_FakeFdr())

        def score(cands, dia, lib):
            pidx = lib.precursor_df["precursor_idx"].to_numpy()
            return (pd.DataFrame({"precursor_idx": pidx, "rank": 0, "decoy": 0,
                                  "elution_group_idx": lib.precursor_df["elution_group_idx"].to_numpy()}),
                    pd.DataFrame({"precursor_idx": pidx, "mass_error": 1.0, "correlation": 0.9}))

        h.score_and_quantify_candidates = score
        h.process_optimization_batch(None, lock)
        lock.update()
        logs += h.log
    assert sum(m.startswith("Resident optimisation step not used") for m in logs) == 1
    assert not any(m.startswith("=== Extracting elution groups") for m in logs)
