"""The count and pack launches of the compacted copy-out (adh_pack_count_kernel, adh_pack_rows_kernel: one workgroup per
256 rows of a chunk, each summing the totals of the workgroups in front of it) at the edges of their workgroups, on
both wires - the dense block (ADH_SPARSE_SLOTS=0) and the sparse-slot one (=1) - and the chunk boundaries of the tables
they serve (adh_chunk_cuts, no GPU).

A chunk of exactly L rows: the first chunk of a table is ADH_CHUNK / ADH_FIRST_CHUNK_DIV rows long (ADH_CHUNK and
ADH_CHUNK_MIN are both at least 1024, so neither makes a chunk of 1 or 255 rows by itself); the table is the first
2 x ADH_CHUNK rows of the case, which ADH_CHUNK then cuts in two."""

import numpy as np
import pytest

import helpers as H
import synthetic as syn
from alphadia_amd.scoring import CandidateScoringConfig, assemble_candidates, fragment_columns, pack_assembled

TABLES = list(H.OUT_NAMES) + ["stat_matched_peaks", "fragment_lib_slot"]
WG = 256  # rows per workgroup of both launches
_CHUNK_ENV = ("ADH_CHUNK", "ADH_CHUNK_PARTS", "ADH_CHUNK_MIN", "ADH_FIRST_CHUNK_DIV", "ADH_LAST_CHUNK_DIV")
_STATE: dict = {}  # the case, and per (rows, skipped range, copies) the reference tables: computed once, never changed


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def _case(ctx):
    if "case" not in _STATE:
        case = syn.make_case(2500, 400, config_id=2, per_precursor=3, threads=8, seed=22)
        cfg = CandidateScoringConfig()
        cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                        experimental_xic=True, top_k_fragments=12))
        soa = assemble_candidates(case.candidates_df, case.library.precursor_df, "mz_library")
        _STATE["case"] = (case, cfg.to_jitclass(), soa)
    case, cfg, soa = _STATE["case"]
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)
    return cfg, soa


def _table(soa, rows, skipped=None, copies=1):
    """the first `rows` candidates of the case, `copies` times over; every 13th row and the rows of `skipped` (a range)
    carry ADH_FLAG_SKIP"""
    n = len(soa["precursor_idx"])
    assert rows <= n
    idx = np.tile(np.arange(rows), copies)
    t = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v)
         for k, v in soa.items()}
    t["flags"][::13] |= 1
    if skipped is not None:
        t["flags"][skipped[0]:skipped[1]] |= 1
    return t


def _reference(ctx, monkeypatch, soa, cfg, rows, skipped=None, copies=1):
    key = (rows, skipped, copies)
    if key not in _STATE:
        with monkeypatch.context() as mp:
            for name in _CHUNK_ENV:
                mp.delenv(name, raising=False)
            mp.setenv("ADH_DEBUG_COPY_ALL", "1")
            ref = ctx.score_host(pack_assembled(_table(soa, rows, skipped, copies)), cfg, with_stats=True)
            ref = {k: np.array(v, copy=True) for k, v in ref.items()}
        for v in ref.values():
            v.flags.writeable = False
        assert (ref["precursor_idx"][::13] == 0).all() and ref["valid"].any() and ref["fragment_lib_slot"].any()
        _STATE[key] = ref
    return _STATE[key]


def _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows, skipped=None, copies=1, expect_sparse=True):
    from alphadia_amd import runtime

    m = pack_assembled(_table(soa, rows, skipped, copies))
    monkeypatch.setenv("ADH_COMPACT_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_SPARSE_SLOTS_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_REBUILD_MIN_THREADS", "0")
    monkeypatch.setenv("ADH_HOST_THREADS", "16")
    n = len(ref["valid"])
    slots = int((ref["fragment_lib_slot"] > 0).sum())
    moved = {}
    for wire in ("0", "1"):
        monkeypatch.setenv("ADH_SPARSE_SLOTS", wire)
        ctx.d2h_bytes(reset=True)
        got = ctx.score_host(m, cfg, with_stats=True)
        moved[wire] = ctx.d2h_bytes(reset=True)
        for k in TABLES:
            assert got[k].tobytes() == ref[k].tobytes(), (k, wire)
    # the packed blocks did travel (not the padded tables), and the sparse wire is the shorter one where it applies
    assert moved["0"] < n * (1 + 46 * 4 + 12 * 22) and moved["0"] >= n * (1 + 46 * 4) + slots * 22
    if expect_sparse and slots:
        assert moved["1"] < moved["0"]
    return runtime.chunk_cuts(n, packed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1, WG - 1, WG, WG + 1, 2 * WG + 1])
def test_chunks_at_the_workgroup_edges(ctx, monkeypatch, length):
    """A first chunk of 1, 255, 256, 257 and 513 rows - one row, one row short of a workgroup, exactly one, one row in
    a second, one row in a third - followed by chunks that start at that row: off the 64-row anchor grid for all but
    256.  Every table equals the copy of every table, on both wires."""
    cfg, soa = _case(ctx)
    div = -(-1024 // length)
    chunk = length * div
    rows = 2 * chunk
    ref = _reference(ctx, monkeypatch, soa, cfg, rows)
    monkeypatch.setenv("ADH_CHUNK", str(chunk))
    monkeypatch.setenv("ADH_FIRST_CHUNK_DIV", str(div))
    cuts = _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows)
    assert cuts[:3] == [0, length, length + chunk] and cuts[-1] == rows


@pytest.mark.gpu
def test_chunk_that_starts_off_the_anchor_grid(ctx, monkeypatch):
    """Chunks that start at rows 750, 2250, ... of 7500 - none a multiple of 64 - and end inside a workgroup."""
    cfg, soa = _case(ctx)
    rows = len(soa["precursor_idx"])
    ref = _reference(ctx, monkeypatch, soa, cfg, rows)
    monkeypatch.setenv("ADH_CHUNK", "1500")
    cuts = _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows)
    assert len(cuts) >= 6 and all(c % 64 for c in cuts[1:-1]) and all((b - a) % WG for a, b in zip(cuts, cuts[1:]))


@pytest.mark.gpu
def test_chunk_whose_rows_are_all_skipped(ctx, monkeypatch):
    """The second chunk (rows 750 - 2250) holds skipped rows only: no filled slot, S = 0, an empty block between two
    full ones."""
    cfg, soa = _case(ctx)
    rows = len(soa["precursor_idx"])
    skipped = (750, 2250)
    ref = _reference(ctx, monkeypatch, soa, cfg, rows, skipped)
    assert not ref["fragment_lib_slot"][750:2250].any() and ref["fragment_lib_slot"][:750].any()
    monkeypatch.setenv("ADH_CHUNK", "1500")
    cuts = _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows, skipped)
    assert cuts[1:3] == [750, 2250]


@pytest.mark.gpu
def test_rows_with_every_slot_filled(ctx, monkeypatch):
    """top_k 12 and 12 kept fragments: the case has rows that fill all 12 slots (and rows of every other count), so a
    workgroup's slot loop runs to the last slot."""
    cfg, soa = _case(ctx)
    rows = len(soa["precursor_idx"])
    ref = _reference(ctx, monkeypatch, soa, cfg, rows)
    assert ref["fragment_lib_slot"].shape[1] == 12
    filled = (ref["fragment_lib_slot"] > 0).sum(axis=1)
    assert (filled == 12).sum() > 100 and len(np.unique(filled)) >= 10
    monkeypatch.setenv("ADH_CHUNK", "2048")
    _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows)


@pytest.mark.gpu
def test_chunk_without_room_for_the_flags(ctx, monkeypatch):
    """ADH_DEBUG_SPARSE_BIG_FROM=3: chunks hold slot values that leave no room for the flags (the 0x4000 fallback), so
    their sparse-wire blocks carry the dense columns behind the header."""
    cfg, soa = _case(ctx)
    rows = len(soa["precursor_idx"])
    ref = _reference(ctx, monkeypatch, soa, cfg, rows)
    assert (ref["fragment_lib_slot"] >= 3).any()
    monkeypatch.setenv("ADH_DEBUG_SPARSE_BIG_FROM", "3")
    monkeypatch.setenv("ADH_CHUNK", "1777")
    _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows, expect_sparse=False)


@pytest.mark.gpu
def test_more_workgroups_than_threads_in_a_chunk(ctx, monkeypatch):
    """A chunk of 67 500 rows is 264 workgroups: a workgroup's 256 threads take more than one pass over the totals of
    the workgroups in front of it."""
    cfg, soa = _case(ctx)
    rows, copies = len(soa["precursor_idx"]), 9
    ref = _reference(ctx, monkeypatch, soa, cfg, rows, None, copies)
    monkeypatch.setenv("ADH_CHUNK", str(10 * rows * copies))
    cuts = _both_wires_equal(ctx, monkeypatch, soa, cfg, ref, rows, None, copies)
    assert cuts == [0, rows * copies] and -(-rows * copies // WG) > WG


# n below 2 M rows, packed: the cuts of the commit before the two-launch pack chain (printed by that build)
_PARENT_CUTS = {
    7_500: [0, 7500],
    375_000: [0, 37500, 112500, 187500, 262500, 337500, 365625, 375000],
    1_000_000: [0, 100000, 300000, 500000, 700000, 900000, 975000, 1000000],
    1_999_999: [0, 200000, 600000, 1000000, 1400000, 1800000, 1950000, 1999999],
}


def test_chunk_cuts_of_packed_tables(monkeypatch):
    """adh_chunk_cuts for packed tables, no GPU: from 0 to n and strictly increasing, no chunk below ADH_CHUNK_MIN's
    default (40 960 rows) but the short last one the packed mode splits off - a quarter of a chunk - and none above
    the bound of the 32-bit slot offsets; below 2 M rows exactly the cuts of the parent commit."""
    from alphadia_amd import runtime

    for name in _CHUNK_ENV:
        monkeypatch.delenv(name, raising=False)
    fits_32 = 0xFFFFFFFF // 12 - 1
    for n in (2_000_000, 3_000_000, 3_000_001, 10_000_000):
        cuts = runtime.chunk_cuts(n, max_rows=fits_32, packed=True)
        assert cuts[0] == 0 and cuts[-1] == n and all(b > a for a, b in zip(cuts, cuts[1:])), n
        lengths = [b - a for a, b in zip(cuts, cuts[1:])]
        assert min(lengths) >= 40_960 and max(lengths) <= min(fits_32, 524_288), (n, lengths)
    for n, expected in _PARENT_CUTS.items():
        assert runtime.chunk_cuts(n, max_rows=fits_32, packed=True) == expected, n
