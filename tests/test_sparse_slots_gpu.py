"""GPU tests of the sparse-slot wire of the compacted copy-out (adh_score_candidates): fragment_intensity and
fragment_correlation of the filled slots leave the device as streams of their non-zero words, flagged in the top two
bits of the slot words and anchored at every row whose number in the table is a multiple of 64; the host team writes the same padded tables.  On by itself for
tables of 1 000 000 rows and more (ADH_SPARSE_SLOTS_MIN_ROWS lowers the threshold here)."""

import numpy as np
import pytest

import helpers as H
import synthetic as syn
from alphadia_amd.scoring import CandidateScoringConfig, assemble_candidates, fragment_columns, pack_assembled

pytestmark = pytest.mark.gpu

TABLES = list(H.OUT_NAMES) + ["stat_matched_peaks", "fragment_lib_slot"]
WIRE_ROW = 1 + 46 * 4  # valid + features: still copied row range by row range
ANCHOR_ROWS = 64
_CASES: dict = {}  # (k_fragments, top_k) -> (case, cfg, reference tables): computed once, never changed


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def _cfg(**kw):
    cfg = CandidateScoringConfig()
    cfg.update(dict(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                         experimental_xic=True), **kw))
    return cfg.to_jitclass()


def _stage(ctx, case):
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)


def _soa(case, pool=None):
    soa = assemble_candidates(case.candidates_df, case.library.precursor_df, "mz_library", pool=pool)
    soa["flags"] = soa["flags"].copy()
    soa["flags"][::13] |= 1  # ADH_FLAG_SKIP: such rows stay zero everywhere
    return soa


def _same(a: dict, b: dict, names=TABLES):
    for k in names:
        assert a[k].tobytes() == b[k].tobytes(), k


def _a16(x: int) -> int:
    return (x + 15) // 16 * 16


def _block_bytes(rows: int, slots: int) -> int:
    """the dense packed block (PadBlock)"""
    return _a16((rows + 1) * 4) + _a16(slots * 2) + 5 * _a16(slots * 4)


def _sparse_block_bytes(rows: int, slots: int, nz_i: int, nz_c: int) -> int:
    """header, offsets, anchors, slot words, three dense float columns, the two streams - of a chunk that starts at
    row 0 of the table (an anchor for every row whose number in the table is a multiple of 64)"""
    anchors = (rows + ANCHOR_ROWS - 1) // ANCHOR_ROWS * 8
    return (16 + _a16((rows + 1) * 4) + _a16(anchors) + _a16(slots * 2) + 3 * _a16(slots * 4)
            + _a16(nz_i * 4) + _a16(nz_c * 4))


def _counts(ref):
    """filled slots and the non-zero words of both streams among them, from padded tables"""
    filled = ref["fragment_lib_slot"] > 0
    bits_i = np.ascontiguousarray(ref["fragment_intensity"]).view(np.uint32)[filled]
    bits_c = np.ascontiguousarray(ref["fragment_correlation"]).view(np.uint32)[filled]
    return int(filled.sum()), int((bits_i != 0).sum()), int((bits_c != 0).sum())


def _reference(ctx, monkeypatch, k_fragments=12, top_k=12):
    """The case of every test here and its tables as the copy of every table gives them (ADH_DEBUG_COPY_ALL)."""
    key = (k_fragments, top_k)
    if key not in _CASES:
        kw = {} if k_fragments == 12 else dict(k_fragments=k_fragments)
        case = syn.make_case(2500, 400, config_id=2, per_precursor=3, threads=8, seed=22, **kw)
        cfg = _cfg(top_k_fragments=top_k)
        _stage(ctx, case)
        with monkeypatch.context() as mp:
            mp.setenv("ADH_DEBUG_COPY_ALL", "1")
            mp.setenv("ADH_CHUNK", "1500")
            ref = ctx.score_host(pack_assembled(_soa(case)), cfg, with_stats=True)
            ref = {k: np.array(v, copy=True) for k, v in ref.items()}
        for v in ref.values():
            v.flags.writeable = False
        n = len(ref["valid"])
        assert ref["valid"].sum() > n // 4 and (ref["precursor_idx"][::13] == 0).all()
        # both streams really are sparse on this case: otherwise the tests below prove nothing
        slots, nz_i, nz_c = _counts(ref)
        print(f"case {key}: {n} rows, {slots} filled slots, zero share intensity {1 - nz_i / slots:.3f}, "
              f"correlation {1 - nz_c / slots:.3f}")
        assert 1 - nz_i / slots > 0.3 and 1 - nz_c / slots > 0.3
        assert nz_i > 0 and nz_c > 0
        _CASES[key] = (case, cfg, ref)
    case, cfg, ref = _CASES[key]
    _stage(ctx, case)
    return case, cfg, ref


def _policy_on(monkeypatch):
    monkeypatch.setenv("ADH_COMPACT_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_SPARSE_SLOTS_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_REBUILD_MIN_THREADS", "0")


@pytest.mark.parametrize("k_fragments,top_k", [(12, 12), ((17, 40), 9999)])
def test_sparse_slots_tables_are_byte_identical(ctx, monkeypatch, k_fragments, top_k):
    """Both thresholds lowered, several chunks whose lengths are no multiples of the anchor stride or of 16, skipped
    rows, 1 / 3 / 16 host threads, the usual width and a transfer-library width: every table equals the one of copying
    every table; so do the page-locked buffers of reuse_buffers=True after they were filled with 0xA5.  Every call
    moves fewer bytes than dense packed blocks could."""
    case, cfg, ref = _reference(ctx, monkeypatch, k_fragments, top_k)
    n = len(ref["valid"])
    if top_k != 12:
        assert ref["fragment_mz_library"].shape[1] > 12
    slots, _, _ = _counts(ref)
    _policy_on(monkeypatch)
    soa = _soa(case)
    pinned = pack_assembled(_soa(case, pool=ctx.pinned))
    for threads, chunk in (("1", "1500"), ("3", "1777"), ("16", "2048")):
        monkeypatch.setenv("ADH_HOST_THREADS", threads)
        monkeypatch.setenv("ADH_CHUNK", chunk)
        # the compacted copy-out's policy needs 12 threads: below that, its forced switch
        with monkeypatch.context() as mp:
            if int(threads) < 12:
                mp.setenv("ADH_COMPACT_COPY_OUT", "1")
            got = ctx.score_host(pack_assembled(soa), cfg, with_stats=True)
            _same(got, ref)
            prev = ctx.score_host(pinned, cfg, reuse_buffers=True)
            for v in prev.values():
                v.view(np.uint8)[...] = 0xA5
            ctx.d2h_bytes(reset=True)
            got = ctx.score_host(pinned, cfg, reuse_buffers=True)
            moved = ctx.d2h_bytes(reset=True)
            assert got["valid"].ctypes.data == prev["valid"].ctypes.data  # (the same buffers)
            _same(got, ref, [k for k in TABLES if k in got])
            assert moved < n * (WIRE_ROW + 4) + slots * 22  # (what dense blocks hold without their alignment)


def test_sparse_slots_bytes_on_the_link(ctx, monkeypatch):
    """One chunk: the bytes on the link are valid + features per row and the sparse block - header, offsets, anchors,
    slot words, three dense float columns and 4 bytes per non-zero intensity / correlation word, each column 16-byte
    aligned - strictly fewer than the dense block.  ADH_SPARSE_SLOTS=0, and the threshold at its default, restore
    the dense block byte for byte; ADH_SPARSE_SLOTS=1 turns the format on below the threshold."""
    case, cfg, ref = _reference(ctx, monkeypatch)
    n = len(ref["valid"])
    assert ref["fragment_mz_library"].shape[1] == 12
    slots, nz_i, nz_c = _counts(ref)
    m = pack_assembled(_soa(case))
    names = None
    monkeypatch.setenv("ADH_HOST_THREADS", "16")
    monkeypatch.setenv("ADH_CHUNK", str(10 * n))
    _policy_on(monkeypatch)
    dense = n * WIRE_ROW + _block_bytes(n, slots)
    sparse = n * WIRE_ROW + _sparse_block_bytes(n, slots, nz_i, nz_c)
    print(f"{n} rows, {slots} slots, {nz_i} + {nz_c} non-zero words: dense {dense} bytes, sparse {sparse}")
    assert sparse < dense

    def moved():
        nonlocal names
        ctx.d2h_bytes(reset=True)
        got = ctx.score_host(m, cfg, reuse_buffers=True)
        b = ctx.d2h_bytes(reset=True)
        names = names or [k for k in TABLES if k in got]
        _same(got, ref, names)
        return b

    assert moved() == sparse
    monkeypatch.setenv("ADH_SPARSE_SLOTS", "0")
    assert moved() == dense
    monkeypatch.delenv("ADH_SPARSE_SLOTS")
    monkeypatch.delenv("ADH_SPARSE_SLOTS_MIN_ROWS")  # (the default threshold: 1 000 000 rows)
    assert moved() == dense
    monkeypatch.setenv("ADH_SPARSE_SLOTS", "1")
    assert moved() == sparse
    # the format belongs to the compacted copy-out: without that, the padded wire
    monkeypatch.setenv("ADH_COMPACT_COPY_OUT", "0")
    assert moved() == n * (WIRE_ROW + 12 * 22)


def test_sparse_slots_chunk_without_room_for_flags(ctx, monkeypatch):
    """A chunk that holds a slot value with no room for the two flag bits (0x4000 and more; the developer switch
    ADH_DEBUG_SPARSE_BIG_FROM lowers the bound so that this case has such values) travels as the dense block behind
    the header, and says so in it: the dense block's bytes plus the 16 of the header, the same tables."""
    case, cfg, ref = _reference(ctx, monkeypatch)
    n = len(ref["valid"])
    slots, _, _ = _counts(ref)
    assert (ref["fragment_lib_slot"] >= 3).any()
    m = pack_assembled(_soa(case))
    monkeypatch.setenv("ADH_HOST_THREADS", "16")
    monkeypatch.setenv("ADH_CHUNK", str(10 * n))
    monkeypatch.setenv("ADH_DEBUG_SPARSE_BIG_FROM", "3")
    _policy_on(monkeypatch)
    ctx.d2h_bytes(reset=True)
    got = ctx.score_host(m, cfg, reuse_buffers=True)
    assert ctx.d2h_bytes(reset=True) == n * WIRE_ROW + 16 + _block_bytes(n, slots)
    _same(got, ref, [k for k in TABLES if k in got])
    monkeypatch.setenv("ADH_CHUNK", "1777")
    got = ctx.score_host(m, cfg, with_stats=True)
    _same(got, ref)
