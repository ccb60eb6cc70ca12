"""GPU tests of the compacted copy-out of the padded path (adh_score_candidates): the filled fragment slots of the six
wire fragment columns leave in one packed block per chunk, and the host team writes the padded rows and the library /
id columns in one pass.  It is on by default for large tables (ADH_COMPACT_MIN_ROWS lowers the threshold here)."""

import numpy as np
import pytest

import helpers as H
import synthetic as syn
from alphadia_amd.scoring import CandidateScoringConfig, assemble_candidates, fragment_columns, pack_assembled

pytestmark = pytest.mark.gpu

TABLES = list(H.OUT_NAMES) + ["stat_matched_peaks", "fragment_lib_slot"]
WIRE_ROW = 1 + 46 * 4  # valid + features: still copied row range by row range


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


def _block_bytes(rows: int, slots: int) -> int:
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    return a16((rows + 1) * 4) + a16(slots * 2) + 5 * a16(slots * 4)


@pytest.mark.parametrize("k_fragments,top_k", [(12, 12), ((17, 40), 9999)])
def test_compact_copy_out_is_byte_identical(ctx, monkeypatch, k_fragments, top_k):
    """Policy on (the row threshold lowered), several chunks, skipped rows, 1 / 3 / 16 host threads, the usual width
    and a transfer-library width: every table equals the one of copying every table (ADH_DEBUG_COPY_ALL); so do the
    page-locked buffers of reuse_buffers=True after they were filled with garbage."""
    case = syn.make_case(2500, 400, config_id=2, per_precursor=3, threads=8, seed=21, k_fragments=k_fragments)
    cfg = _cfg(top_k_fragments=top_k)
    _stage(ctx, case)
    soa = _soa(case)
    n = len(soa["precursor_idx"])
    monkeypatch.setenv("ADH_DEBUG_COPY_ALL", "1")
    monkeypatch.setenv("ADH_CHUNK", "1500")
    ref = ctx.score_host(pack_assembled(soa), cfg, with_stats=True)
    ref = {k: np.array(v, copy=True) for k, v in ref.items()}
    monkeypatch.delenv("ADH_DEBUG_COPY_ALL")
    assert ref["valid"].sum() > n // 4 and (ref["precursor_idx"][::13] == 0).all()
    if top_k != 12:
        assert ref["fragment_mz_library"].shape[1] > 12
    monkeypatch.setenv("ADH_COMPACT_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_REBUILD_MIN_THREADS", "0")
    pinned = pack_assembled(_soa(case, pool=ctx.pinned))
    for threads, chunk in (("1", "1500"), ("3", "1777"), ("16", "2048")):
        monkeypatch.setenv("ADH_HOST_THREADS", threads)
        monkeypatch.setenv("ADH_CHUNK", chunk)
        # the policy needs 12 threads: below that, the forced switch
        with monkeypatch.context() as mp:
            if int(threads) < 12:
                mp.setenv("ADH_COMPACT_COPY_OUT", "1")
            got = ctx.score_host(pack_assembled(soa), cfg, with_stats=True)
            _same(got, ref)
            # production form: page-locked buffers (the previous call's content overwritten with garbage first), no
            # host table for the slots
            prev = ctx.score_host(pinned, cfg, reuse_buffers=True)
            for v in prev.values():
                v.view(np.uint8)[...] = 0xA5
            got = ctx.score_host(pinned, cfg, reuse_buffers=True)
            assert got["valid"].ctypes.data == prev["valid"].ctypes.data  # (the same buffers)
            _same(got, ref, [k for k in TABLES if k in got])


def test_compact_copy_out_bytes_on_the_link(ctx, monkeypatch):
    """One chunk: the bytes on the link are valid + features per row and the packed block (offsets, slot column and
    five float columns of the filled slots, each 16-byte aligned).  ADH_COMPACT_COPY_OUT=0 restores the padded wire
    (449 bytes per row at top_k 12); the policy leaves small tables on it."""
    case = syn.make_case(2500, 400, config_id=2, per_precursor=3, threads=8, seed=22)
    cfg = _cfg(top_k_fragments=12)
    _stage(ctx, case)
    soa = _soa(case)
    n = len(soa["precursor_idx"])
    m = pack_assembled(soa)
    monkeypatch.setenv("ADH_REBUILD_MIN_THREADS", "0")
    monkeypatch.setenv("ADH_HOST_THREADS", "16")
    monkeypatch.setenv("ADH_CHUNK", str(10 * n))
    ref = ctx.score_host(m, cfg, with_stats=True)
    ref = {k: np.array(v, copy=True) for k, v in ref.items()}
    assert ref["fragment_mz_library"].shape[1] == 12
    slots = int((ref["fragment_lib_slot"] > 0).sum())
    padded = n * (WIRE_ROW + 12 * 22)
    ctx.d2h_bytes(reset=True)
    ctx.score_host(m, cfg, reuse_buffers=True)
    assert ctx.d2h_bytes(reset=True) == padded  # (below ADH_COMPACT_MIN_ROWS: today's path)
    monkeypatch.setenv("ADH_COMPACT_MIN_ROWS", "1000")
    got = ctx.score_host(m, cfg, reuse_buffers=True)
    assert ctx.d2h_bytes(reset=True) == n * WIRE_ROW + _block_bytes(n, slots)
    _same(got, ref, [k for k in TABLES if k in got])
    monkeypatch.setenv("ADH_COMPACT_COPY_OUT", "0")
    got = ctx.score_host(m, cfg, reuse_buffers=True)
    assert ctx.d2h_bytes(reset=True) == padded
    _same(got, ref, [k for k in TABLES if k in got])
    # several chunks: the same columns, within a block's alignment slack per chunk
    monkeypatch.delenv("ADH_COMPACT_COPY_OUT")
    monkeypatch.setenv("ADH_CHUNK", "1500")
    got = ctx.score_host(m, cfg, reuse_buffers=True)
    b = ctx.d2h_bytes(reset=True)
    lo = n * (WIRE_ROW + 4) + slots * 22
    assert lo <= b <= lo + 16 * 7 * (n // 1000 + 2)
    _same(got, ref, [k for k in TABLES if k in got])
