"""The device flatten (alphadia_amd/csrc/adh_flatten.hip) against ``flatten.host_flatten_library``, bit for bit: the
hand cases of tests/test_flatten.py, blocks and groups around every size at which a kernel takes another path, a
seeded random library, every route forced, the page-locked upload in more than one piece, and the records staged on
a context against ``stage_fragments_columns`` of the returned frame."""

from __future__ import annotations

import functools
import os
import re

import numpy as np
import pytest

import flatten_cases as fc
import synthetic as syn
from alphadia_amd import flatten as fl
from alphadia_amd import runtime
from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring, assemble_candidates, fragment_columns
from test_abi import ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "include", "alphadia_hip_flatten.h")) as _f:
    BOUNDS = {k: int(v) for k, v in re.findall(r"#define (ADFL_\w+) (\d+)", _f.read())}
CARD_WAVE = BOUNDS["ADFL_CARD_WAVE_MAX_MEMBERS"]
SELECT_WAVE = BOUNDS["ADFL_SELECT_WAVE_MAX_CELLS"]


def bits(column) -> np.ndarray:
    a = np.ascontiguousarray(column)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def device(case, context=None):
    flat = fl.HipFlattenLibrary(case.top_k, case.min_intensity, device=0)(case, context)
    return flat._precursor_df, flat._fragment_df


def assert_parity(case, context=None) -> dict:
    """Device frames == restatement frames in every bit; returns the call's ``last_timing``."""
    want_pre, want_frag = case.host()
    pre, frag = device(case, context)
    timing = dict(fl.last_timing)
    assert list(frag.columns) == list(want_frag.columns) == list(fl.FRAGMENT_COLUMNS)
    assert len(frag) == len(want_frag) == timing["n_fragments"]
    for c in frag.columns:
        assert frag[c].dtype == want_frag[c].dtype, c
        assert np.array_equal(bits(frag[c].to_numpy()), bits(want_frag[c].to_numpy())), c
    assert list(pre.columns) == list(want_pre.columns) and pre.index.equals(want_pre.index)
    for c in pre.columns:
        assert pre[c].dtype == want_pre[c].dtype and np.array_equal(pre[c].to_numpy(), want_pre[c].to_numpy()), c
    routes = timing["routes"]
    sizes = np.unique(case.precursor_df.assign(decoy=case.precursor_df.get("decoy", 0)).groupby(
        ["decoy", "elution_group_idx"]).size().to_numpy(), return_counts=True) if len(pre) else ((), ())
    if "ADFL_DEBUG_ROUTE" not in os.environ:  # the routes that ran are those the bounds name
        cells = ((case.precursor_df["frag_stop_idx"] - case.precursor_df["frag_start_idx"]) * case.fragment_mz_df.shape[1])
        assert routes["select_wave"] == int((cells <= SELECT_WAVE).sum()) and routes["select_block"] == int((cells > SELECT_WAVE).sum())
        assert routes["card_wave"] == sum(int(c) for s, c in zip(*sizes) if s <= CARD_WAVE)
        assert routes["card_block"] == sum(int(c) for s, c in zip(*sizes) if s > CARD_WAVE)
    assert timing["h2d_bytes"] >= 8 * case.fragment_mz_df.size * (len(pre) > 0)
    assert timing["d2h_bytes"] == (14 * len(frag) + 8 * len(pre) + 64) * (len(pre) > 0)
    return timing


HAND = {
    "two_charge_states": fc.two_charge_states, "target_and_decoy": fc.target_and_decoy,
    "unequal_row_counts": fc.unequal_row_counts, "one_ulp_apart": fc.one_ulp_apart,
    "at_the_threshold": fc.at_the_threshold, "ties_at_rank_k": fc.ties_at_rank_k,
    "descending_starts": fc.descending_starts, "empty_library": fc.empty_library,
    **{f"four_cells_top_{k}": functools.partial(fc.four_cells, k) for k in (1, 2, 4, 5)},
    **{f"nan_top_{k}": functools.partial(fc.nan_intensity, k) for k in (1, 2, 3, 4)},
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(name):
    assert_parity(HAND[name]())


@pytest.mark.parametrize("make", [fc.overlapping, lambda: fc.group_of(256), lambda: fc.four_cells(0)],
                         ids=["overlap", "group_of_256", "top_k_0"])
def test_refused_inputs_raise_on_both_sides(make):
    with pytest.raises(ValueError) as host:
        make().host()
    with pytest.raises(ValueError) as dev:
        device(make())
    assert str(host.value).split("flatten: ")[1] == str(dev.value).split("flatten: ")[1]


def shape_of(cells: int) -> tuple:
    """``(rows, column names)`` of a block of exactly ``cells`` cells, with as few columns as the row limit allows."""
    n_cols = next(c for c in range(1, fl.MAX_COLUMNS + 1) if cells % c == 0 and cells // c <= fl.MAX_ROWS)
    return cells // n_cols, fc.COLS32[:n_cols]


@pytest.mark.parametrize("rows, cols", [(63, ["y_z1"]), (64, ["y_z1"]), (65, ["y_z1"]), (16, fc.COLS4),
                                        (255, ["b_z1"]), (255, fc.COLS4), (255, fc.COLS32),
                                        shape_of(SELECT_WAVE - 1), shape_of(SELECT_WAVE), shape_of(SELECT_WAVE + 1)],
                         ids=lambda v: str(v) if isinstance(v, int) else f"x{len(v)}")
def test_block_sizes(rows, cols):
    for top_k in (12, rows * len(cols)):
        timing = assert_parity(fc.one_block(rows, cols, top_k=top_k))
        assert timing["routes"]["select_block"] == (rows * len(cols) > SELECT_WAVE)


@pytest.mark.parametrize("m", [1, 2, 3, CARD_WAVE - 1, CARD_WAVE, CARD_WAVE + 1, 64, 65, 255])
def test_group_sizes(m):
    timing = assert_parity(fc.group_of(m, rows=2))
    assert timing["routes"]["card_block"] == int(m > CARD_WAVE)  # (every other group is a single precursor)
    case = fc.group_of(m, cols=fc.COLS8, rows=3)  # ... and with m/z that differ in some cells
    mz = case.fragment_mz_df.to_numpy()
    mz[np.random.default_rng(m).random(mz.shape) < 0.4] += np.float32(1.0)
    assert_parity(case)


@pytest.mark.parametrize("where", [0, 2, 4])
def test_a_precursor_with_nothing_kept(where):
    case = fc.nothing_kept_at(where)
    assert case.precursor_df["frag_stop_idx"].iloc[-1] == len(case.fragment_mz_df)  # the last block ends the matrix
    assert_parity(case)
    pre, _ = device(case)
    assert pre["flat_frag_start_idx"].iloc[where] == pre["flat_frag_stop_idx"].iloc[where]


@functools.lru_cache(maxsize=None)
def random_case(n_cols: int):
    return fc.random_library(n_prec=3000, cols=fc.COLS4 if n_cols == 4 else fc.COLS8, seed=5 + n_cols)


@pytest.mark.parametrize("n_cols", [4, 8])
def test_random_library(n_cols):
    timing = assert_parity(random_case(n_cols))
    assert timing["routes"]["select_wave"] > 0 and (n_cols == 4 or timing["routes"]["select_block"] > 0)
    assert timing["kernel_ms"] > 0


def test_every_route_gives_the_same_bits(monkeypatch):
    """A library whose groups (up to 40 precursors) and blocks (up to 480 cells) take both routes by default is sent
    down each route that can take it: ADFL_DEBUG_ROUTE=block, ADFL_DEBUG_ROUTE=wave."""
    case = fc.random_library(n_prec=500, cols=fc.COLS8, seed=77, max_rows=60, max_group=40)
    default = assert_parity(case)["routes"]
    assert min(default.values()) > 0
    monkeypatch.setenv("ADFL_DEBUG_ROUTE", "block")
    forced = assert_parity(case)["routes"]
    assert forced["card_wave"] == forced["select_wave"] == 0
    assert forced["card_block"] == default["card_wave"] + default["card_block"] and forced["select_block"] == 500
    monkeypatch.setenv("ADFL_DEBUG_ROUTE", "wave")
    forced = assert_parity(case)["routes"]
    assert forced["card_block"] == 0 and forced["card_wave"] == default["card_wave"] + default["card_block"]
    assert (forced["select_wave"], forced["select_block"]) == (default["select_wave"], default["select_block"])
    monkeypatch.setenv("ADFL_DEBUG_ROUTE", "neither")
    with pytest.raises(ValueError, match="ADFL_DEBUG_ROUTE"):
        device(case)


def test_the_upload_in_several_pieces(monkeypatch):
    """The matrices go through the page-locked lanes in pieces of 4 MB: with one lane and no lower limit, a matrix of
    more than one piece."""
    monkeypatch.setenv("ADH_UPLOAD_MIN_MB", "0")
    monkeypatch.setenv("ADH_UPLOAD_LANES", "1")
    case = fc.random_library(n_prec=24000, cols=fc.COLS4, seed=9, max_rows=28, max_group=2)
    assert case.fragment_mz_df.to_numpy().nbytes > 4 << 20
    assert_parity(case)


# ---- staging on a context ------------------------------------------------------------------------------------------

def nine(frag) -> tuple:
    return (frag["mz"].values, frag["mz"].values, *(frag[c].values for c in fl.FRAGMENT_COLUMNS[1:]))


def test_the_staged_records_are_those_of_the_returned_frame():
    one, two = runtime.Context(0), runtime.Context(0)
    try:
        for case in (random_case(4), fc.descending_starts(), fc.empty_library()):
            assert_parity(case, context=one)
            assert fl.last_timing["staged"]
            _, frag = device(case, context=one)
            assert not one.stage_fragments(*nine(frag))  # the context knows the frame: nothing is staged again
            two.stage_fragments_columns(*nine(frag))
            for mirror in (False, True):
                got, want = one.staged_fragment_records(host_mirror=mirror), two.staged_fragment_records(host_mirror=mirror)
                assert got.shape == want.shape == (len(frag),) and got.tobytes() == want.tobytes()
            assert np.array_equal(bits(got["mz_library"]), bits(frag["mz"].to_numpy())) and not got["pad"].any()
    finally:
        one.close()
        two.close()


def test_a_refused_input_leaves_the_staged_library():
    ctx = runtime.Context(0)
    try:
        _, frag = device(fc.two_charge_states(), context=ctx)
        before = [ctx.staged_fragment_records(host_mirror=m).tobytes() for m in (False, True)]
        assert len(before[0]) == 16 * 32
        for make in (fc.overlapping, lambda: fc.group_of(256)):
            with pytest.raises(ValueError):
                device(make(), context=ctx)
            assert [ctx.staged_fragment_records(host_mirror=m).tobytes() for m in (False, True)] == before
            assert not ctx.stage_fragments(*nine(frag))
    finally:
        ctx.close()


def test_scoring_through_the_flatten_staged_library():
    """One small synthetic scoring input: the tables scored over the library the flatten left staged equal those over
    the same frame staged the classic way."""
    case = syn.make_case(n_precursors=60, n_cycles=40, config_id=901, per_precursor=2, n_ms2=8, ms1_peaks=200,
                         ms2_peaks=100, mz_lo=400, mz_hi=480, frag_mz_lo=200, frag_mz_hi=350, ms1_mz_range=(395, 500),
                         ms2_mz_range=(195, 355), planted_fraction=0.5, threads=1)
    old = case.library.fragment_df
    # the flat synthetic library as a dense one of a single y_z1 column: one dense row per fragment
    pre = case.library.precursor_df.rename(columns={"flat_frag_start_idx": "frag_start_idx", "flat_frag_stop_idx": "frag_stop_idx"})
    dense = fc.Dense(pre[["frag_start_idx", "frag_stop_idx"]].to_numpy(), pre["elution_group_idx"].to_numpy(),
                     old["mz_library"].to_numpy(), old["intensity"].to_numpy(), cols=["y_z1"], top_k=8, min_intensity=0.2)
    dense.precursor_df = pre
    ctx = runtime.get_context(0)
    flat = fl.init_flat_columns(fl.HipFlattenLibrary(8, 0.2, device=0)(dense, ctx))
    assert 0 < len(flat.fragment_df) < len(old)
    assert not ctx.stage_fragments(*fragment_columns(flat.fragment_df, "mz_library"))
    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15))

    def score():
        scorer = HipCandidateScoring(dia_data=case.dia, precursors_flat=flat.precursor_df, fragments_flat=flat.fragment_df,
                                     rt_column="rt_library", mobility_column="mobility_library",
                                     precursor_mz_column="mz_library", fragment_mz_column="mz_library", config=cfg, device=0)
        return scorer.score_soa(assemble_candidates(case.candidates_df, scorer.precursors_flat_df, "mz_library"))

    through_flatten = score()
    ctx.stage_fragments(*fragment_columns(flat.fragment_df, "mz_library"), force=True)
    classic = score()
    assert through_flatten.valid.sum() > 0 and np.array_equal(through_flatten.valid, classic.valid)
    assert through_flatten.features.tobytes() == classic.features.tobytes()
