"""GPU tests of the hand-off of landed blocks to the host team (BlockHandoff in adh_copyout.hip): the compacted
copy-out of adh_score_candidates and the operator's adh_score_candidates_compact give a block to their team when its
copy ends - a thread of the team waits on the copy's event, the enqueue thread only appends events.  Many small
chunks and a team of several threads make the threads meet at the hand-off; every table is compared byte for byte
with the one of copying every table (ADH_DEBUG_COPY_ALL), as in test_compact_copyout_gpu.py.

Consecutive calls score DIFFERENT inputs (two sets of skipped rows, each with its own reference): the library's
page-locked staging blocks then hold another call's bytes when a block is handed over, so a block published before
its copy has landed shows as a difference instead of reading stale but equal data."""

import ctypes as C
import threading

import numpy as np
import pytest

import helpers as H
import synthetic as syn
from alphadia_amd import _abi, runtime
from alphadia_amd.scoring import CandidateScoringConfig, assemble_candidates, fragment_columns, pack_assembled

pytestmark = pytest.mark.gpu

TABLES = list(H.OUT_NAMES) + ["stat_matched_peaks", "fragment_lib_slot"]
CHUNK = 2800          # 72 000 candidates: 27 chunks
STRIDES = (13, 3)     # every 13th / every 3rd row skipped: the packed blocks of the two inputs differ in every chunk
CALL_TIMEOUT = 120.0  # seconds a call may take before the test calls it a hang (a call takes a few ms)
SLOT_COLUMNS = ("fragment_mz_library", "fragment_mz_observed", "fragment_height", "fragment_intensity",
                "fragment_mass_error", "fragment_correlation", "fragment_number", "fragment_type")


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


@pytest.fixture(scope="module")
def case():
    # 24 000 precursors x 3 candidates = 72 000 rows: host_threads_for gives a thread per 16 384 rows, so a team of
    # four exists (tables below 65 536 rows run with one or two threads whatever ADH_HOST_THREADS says)
    return syn.make_case(24000, 400, config_id=2, per_precursor=3, threads=8, seed=31)


def _cfg(**kw):
    cfg = CandidateScoringConfig()
    cfg.update(dict(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                         experimental_xic=True, top_k_fragments=12), **kw))
    return cfg.to_jitclass()


def _stage(ctx, case):
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)


def _soa(case, stride, pool=None):
    soa = assemble_candidates(case.candidates_df, case.library.precursor_df, "mz_library", pool=pool)
    soa["flags"] = soa["flags"].copy()
    soa["flags"][::stride] |= 1  # ADH_FLAG_SKIP: such rows stay zero everywhere
    return soa


def _same(a: dict, b: dict, names=TABLES):
    for k in names:
        assert a[k].tobytes() == b[k].tobytes(), k


def _reference(ctx, monkeypatch, soa, cfg):
    """Every table copied back as the kernels wrote it."""
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_COPY_ALL", "1")
        mp.setenv("ADH_CHUNK", str(CHUNK))
        ref = ctx.score_host(pack_assembled(soa), cfg, with_stats=True)
        return {k: np.array(v, copy=True) for k, v in ref.items()}


def _inputs(ctx, case, monkeypatch, cfg):
    """The two inputs with their references; their packed blocks differ."""
    soas = [_soa(case, s) for s in STRIDES]
    refs = [_reference(ctx, monkeypatch, soa, cfg) for soa in soas]
    n = len(soas[0]["precursor_idx"])
    assert n >= 65536 and -(-n // CHUNK) >= 24
    for ref, s in zip(refs, STRIDES):
        assert ref["valid"].sum() > n // 4 and (ref["precursor_idx"][::s] == 0).all()
    assert refs[0]["fragment_lib_slot"].tobytes() != refs[1]["fragment_lib_slot"].tobytes()
    return soas, refs, n


def _in_time(fn):
    """Run fn on a thread; a call that does not return within CALL_TIMEOUT fails the test instead of hanging it."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001  (handed to the calling thread)
            box["error"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(CALL_TIMEOUT)
    assert not t.is_alive(), f"the call did not return within {CALL_TIMEOUT:.0f} s"
    if "error" in box:
        raise box["error"]
    return box["value"]


def _check_operator(got: dict, ref: dict):
    rows = np.flatnonzero(ref["valid"])
    filled = ref["fragment_lib_slot"][rows] > 0
    assert np.array_equal(got["row"], rows)
    assert got["precursor_idx"].tobytes() == ref["precursor_idx"][rows].tobytes()
    assert got["rank"].tobytes() == ref["rank"][rows].tobytes()
    assert np.ascontiguousarray(got["features"].T).tobytes() == ref["features"][rows].tobytes()
    assert np.array_equal(got["fragment_row"], np.repeat(rows, filled.sum(axis=1)))
    for name in SLOT_COLUMNS:
        assert got[name].tobytes() == ref[name][rows][filled].tobytes(), name


def test_many_small_chunks_reach_the_team_byte_identical(ctx, case, monkeypatch):
    """At least 24 chunks, ADH_HOST_THREADS 1 / 3 / 16, page-locked buffers filled with garbage, calls in a row on one
    handle that alternate between the two inputs: every table equals the one of copying every table."""
    cfg = _cfg()
    _stage(ctx, case)
    soas, refs, n = _inputs(ctx, case, monkeypatch, cfg)
    slots = [int((ref["fragment_lib_slot"] > 0).sum()) for ref in refs]
    monkeypatch.setenv("ADH_COMPACT_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_REBUILD_MIN_THREADS", "0")
    monkeypatch.setenv("ADH_CHUNK", str(CHUNK))
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("ADH_HOST_THREADS", threads)
        team = runtime.host_threads(n)[0]
        assert team == min(int(threads), n // 16384), team
        if threads != "1":
            assert team > 1  # (more than one thread takes part in the hand-off)
        with monkeypatch.context() as mp:
            if int(threads) < 12:  # the policy needs 12 threads: below that, the forced switch
                mp.setenv("ADH_COMPACT_COPY_OUT", "1")
            prev = None
            for call in range(4):
                which = call % 2
                got = _in_time(lambda: ctx.score_host(pack_assembled(soas[which]), cfg, with_stats=True))
                _same(got, refs[which])
                # production form: page-locked candidate columns and output buffers, the latter holding garbage
                pinned = pack_assembled(_soa(case, STRIDES[which], pool=ctx.pinned))
                if prev is not None:
                    for v in prev.values():
                        v.view(np.uint8)[...] = 0xA5
                ctx.d2h_bytes(reset=True)
                got = _in_time(lambda: ctx.score_host(pinned, cfg, reuse_buffers=True))
                # (the packed wire: valid + features + an offset per row, 22 bytes per filled slot, alignment slack)
                assert n * 189 + slots[which] * 22 <= ctx.d2h_bytes(reset=True) < n * (185 + 12 * 22)
                if prev is not None:
                    assert got["valid"].ctypes.data == prev["valid"].ctypes.data  # (the same buffers)
                _same(got, refs[which], [k for k in TABLES if k in got])
                prev = got


def test_operator_blocks_reach_the_team(ctx, case, monkeypatch):
    """The same through adh_score_candidates_compact: its rows are the padded call's valid rows, its features theirs,
    its slots the filled slots in row order - at 1, 3 and 16 threads, calls in a row that alternate between the two
    inputs, into arrays that hold garbage."""
    cfg = _cfg()
    _stage(ctx, case)
    soas, refs, n = _inputs(ctx, case, monkeypatch, cfg)
    monkeypatch.setenv("ADH_CHUNK", str(CHUNK))
    keep: dict = {}
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("ADH_HOST_THREADS", threads)
        if threads != "1":
            assert runtime.host_threads(n)[0] > 1
        for call in range(4):
            for arrays in keep.values():
                for v in arrays.values():
                    v.view(np.uint8)[...] = 0xA5
            got = _in_time(lambda: ctx.score_host_compact(pack_assembled(soas[call % 2]), cfg, buffers=keep))
            _check_operator(got, refs[call % 2])


@pytest.mark.parametrize("entry", ["padded", "operator"])
def test_error_in_a_late_chunk_returns_and_leaves_the_handle_usable(ctx, case, monkeypatch, entry):
    """A candidate of a late chunk with frame limits outside the run: the plan kernel reports it, the call raises the
    documented error (team and watcher end, no hang), and the next valid call on the handle - of the OTHER input - is
    byte-identical to its reference."""
    cfg = _cfg()
    _stage(ctx, case)
    soas, refs, n = _inputs(ctx, case, monkeypatch, cfg)
    monkeypatch.setenv("ADH_COMPACT_MIN_ROWS", "1000")
    monkeypatch.setenv("ADH_REBUILD_MIN_THREADS", "0")
    monkeypatch.setenv("ADH_HOST_THREADS", "16")
    monkeypatch.setenv("ADH_CHUNK", str(CHUNK))
    if entry == "padded":
        call = lambda s: ctx.score_host(pack_assembled(s), cfg, with_stats=True)  # noqa: E731
    else:
        call = lambda s: ctx.score_host_compact(pack_assembled(s), cfg)  # noqa: E731
    for which in (0, 1, 0):
        bad = dict(soas[which])
        bad["frame_stop"] = bad["frame_stop"].copy()
        late = n - CHUNK - 7  # (a row of the last chunks that is not skipped)
        while bad["flags"][late] & 1:
            late += 1
        bad["frame_stop"][late] = case.dia.n_spectra + case.dia.cycle_len * 5
        with pytest.raises(runtime.HipBackendError, match="frame limits"):
            _in_time(lambda: call(bad))
        got = _in_time(lambda: call(soas[1 - which]))
        if entry == "padded":
            _same(got, refs[1 - which])
        else:
            _check_operator(got, refs[1 - which])


def test_operator_rejects_a_width_its_count_byte_cannot_hold(ctx, case):
    """adh_score_candidates_compact sends a row's number of filled slots as one byte: top_k above 255 is refused
    before anything runs."""
    _stage(ctx, case)
    cands = pack_assembled(_soa(case, STRIDES[0]))
    out = _abi.CompactOutput()
    out.rows_capacity, out.slots_capacity, out.top_k = 16, 16, 256
    pcfg = _abi.pack_config(_cfg())
    rc = runtime.lib.adh_score_candidates_compact(ctx._h, cands.ref(), C.byref(pcfg), C.byref(out))
    assert rc == -1  # ADH_ERR_INVALID_ARGUMENT
    assert b"top_k above 255" in runtime.lib.adh_last_error()
