"""No legal AlphaRaw scoring input is refused for the size of its tile: the generic kernel class (36) is launched in
groups by each candidate's OWN LDS layout, and a candidate whose own layout exceeds the LDS of a CU goes through the
spill instantiation (its [K][O][F] planes in the scratch slab).  HIP against the oracle and against itself on the
inputs of tests/test_generic_oversize.py; ``Context.generic_launch_stats`` proves which path ran.
Run with ``-m gpu`` on an MI355X."""

import numpy as np
import pytest

import box_sweep as bs
import test_generic_oversize as go
from alphadia_amd import runtime
from alphadia_amd.runtime import HipBackendError
from alphadia_amd.scoring import pack_assembled
from test_gpu_parity import PPM_ABS_TOL_ORACLE, REL_TOL, compare
from test_kernel_classes_gpu import _compact_equals_padded, _rows, _same, _staged, score_batches

pytestmark = pytest.mark.gpu

config_of = bs.config_of


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


def _score(ctx, soa, cfg, idx=None):
    m = pack_assembled(soa if idx is None else _rows(soa, idx))
    return {k: np.array(v, copy=True) for k, v in ctx.score_host(m, cfg.to_jitclass(), with_stats=True).items()}


def _take(tab: dict, idx) -> dict:
    return {k: v[idx] for k, v in tab.items()}


def _stats_equal(got: dict, want: dict, times: int = 1):
    assert np.array_equal(got["candidates"], want["candidates"] * times), (got, want)
    assert np.array_equal(got["lds_bytes"], want["lds_bytes"]), (got, want)


def _against_oracle(got, exp, cfg):
    # experimental_xic = False: the K x K contraction runs on MFMA in another summation order than the oracle's
    corr_abs = 0.0 if cfg.experimental_xic else 2e-6
    compare(got, exp, PPM_ABS_TOL_ORACLE, rel_tol=REL_TOL, corr_abs=corr_abs)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    assert not any(compare.last_masked["rescued"].values()), compare.last_masked["rescued"]  # no knife-edge mask needed


@pytest.mark.parametrize("name", go.CONFIG_NAMES)
def test_the_ragged_sweep_in_one_call(ctx, oracle_lib, monkeypatch, name):
    """Input A: refused before this for the product of its maxima (232 992 bytes), while no candidate needs more than
    141 392.  One call equals the per-batch calls bit for bit and the oracle, by default and with every candidate in
    the generic class; nothing spills."""
    case, soa, spec = go.ragged_sweep()
    cfg = config_of(name)
    exp = go.oracle_tables(oracle_lib, "A", name)
    _staged(ctx, case)
    for no_fast in (False, True):
        with monkeypatch.context() as mp:
            if no_fast:
                mp.setenv("ADH_DEBUG_NO_FAST", "1")
            per_batch = score_batches(ctx, soa, spec["batch"].values, cfg)
            ctx.plan_class_counts(reset=True)
            ctx.generic_launch_stats(reset=True)
            got = _score(ctx, soa, cfg)
            counts = ctx.plan_class_counts(reset=True)
            stats = ctx.generic_launch_stats(reset=True)
        _same(got, per_batch, f"one call, no_fast={no_fast}")
        _against_oracle(got, exp, cfg)
        want, _ = go.expected_stats(case, soa, cfg, no_fast=no_fast)
        _stats_equal(stats, want)
        assert stats["candidates"][go.GROUP_SPILL] == 0 and stats["candidates"].sum() == counts[bs.CLASS_GENERIC]
        assert np.array_equal(counts, bs.histogram(bs.classes_of(case, soa, cfg, no_fast=no_fast)))
        if no_fast:
            assert counts[bs.CLASS_GENERIC] == len(spec) == 1386
        assert ctx.generic_launch_stats()["candidates"].sum() == 0


@pytest.mark.parametrize("name", go.CONFIG_NAMES)
def test_the_oversize_sweep(ctx, oracle_lib, name):
    """Input B: 117 candidates whose own layout exceeds the LDS of a CU take the spill path, the 18 just under it an
    LDS group; all match the oracle, and a row's bits do not depend on what it is scored with."""
    case, soa, spec = go.oversize_sweep()
    cfg = config_of(name)
    exp = go.oracle_tables(oracle_lib, "B", name)
    _staged(ctx, case)
    ctx.plan_class_counts(reset=True)
    ctx.generic_launch_stats(reset=True)
    got = _score(ctx, soa, cfg)
    counts = ctx.plan_class_counts(reset=True)
    stats = ctx.generic_launch_stats(reset=True)
    _against_oracle(got, exp, cfg)
    assert got["valid"].astype(bool).all()
    want, group = go.expected_stats(case, soa, cfg)
    _stats_equal(stats, want)
    assert np.array_equal(counts, bs.histogram(bs.classes_of(case, soa, cfg)))
    spilled = np.flatnonzero(group == go.GROUP_SPILL)
    # (a two-observation row of 200 fragments is generic under every configuration: all 117 are in the spill group)
    assert len(spilled) == 117 == stats["candidates"][go.GROUP_SPILL]
    t = bs.shape_table(case, soa, cfg)
    under = np.flatnonzero((t["k_cap"].values == 200) & (t["O"].values == 2) & np.isin(t["F"].values, (22, 23)))
    assert len(under) == 18 and (group[under] == go.GROUP_LARGE).all()
    # the 117 alone, the rest alone
    rest = np.flatnonzero(group != go.GROUP_SPILL)
    alone = _score(ctx, soa, cfg, spilled)
    s_alone = ctx.generic_launch_stats(reset=True)
    assert s_alone["candidates"].tolist() == [0, 0, 117] and s_alone["lds_bytes"][go.GROUP_SPILL] == want["lds_bytes"][go.GROUP_SPILL]
    others = _score(ctx, soa, cfg, rest)
    s_rest = ctx.generic_launch_stats(reset=True)
    assert s_rest["candidates"][go.GROUP_SPILL] == 0 and s_rest["candidates"].sum() == want["candidates"].sum() - 117
    for part, idx in ((alone, spilled), (others, rest)):
        _same(part, _take(got, idx), "rows scored apart")


@pytest.mark.parametrize("name", ["all_fragments", "no_xic_all_fragments"])
def test_spill_instantiation_equals_the_lds_one(ctx, monkeypatch, name):
    """ADH_DEBUG_GENERIC_SPILL=1 with ADH_DEBUG_NO_FAST=1 on input A: every candidate runs the spill instantiation,
    and the tables are bit-equal to the LDS instantiation's at every shape of the sweep (the same candidates under
    ADH_DEBUG_NO_FAST alone) and, on the rows the default run sends to the generic class, to the default run."""
    case, soa, spec = go.ragged_sweep()
    cfg = config_of(name)
    _staged(ctx, case)
    default = _score(ctx, soa, cfg)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_NO_FAST", "1")
        lds = _score(ctx, soa, cfg)
        mp.setenv("ADH_DEBUG_GENERIC_SPILL", "1")
        ctx.plan_class_counts(reset=True)
        ctx.generic_launch_stats(reset=True)
        spill = _score(ctx, soa, cfg)
        counts = ctx.plan_class_counts(reset=True)
        stats = ctx.generic_launch_stats(reset=True)
    assert stats["candidates"].tolist() == [0, 0, 1386] and counts[bs.CLASS_GENERIC] == 1386 == counts.sum()
    want, _ = go.expected_stats(case, soa, cfg, spill_all=True, no_fast=True)
    _stats_equal(stats, want)
    _same(spill, lds, "spill against LDS instantiation")
    generic = np.flatnonzero(bs.classes_of(case, soa, cfg) == bs.CLASS_GENERIC)
    assert len(generic) >= 100
    _same(_take(spill, generic), _take(default, generic), "spill against the default run")
    if not cfg.experimental_xic:
        assert len(generic) == 1386


def test_oversize_sweep_in_chunks(ctx, monkeypatch):
    """Input B tiled past three chunks (ADH_CHUNK=256; the library's floor is 1024 rows a chunk): every copy equals
    the single call, and the launch statistics are the per-copy ones times the copies."""
    case, soa, spec = go.oversize_sweep()
    cfg = config_of("all_fragments")
    _staged(ctx, case)
    got = _score(ctx, soa, cfg)
    ctx.plan_class_counts(reset=True)
    ctx.generic_launch_stats(reset=True)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_CHUNK", "256")
        chunked, chunks, copies = score_batches(ctx, soa, np.zeros(len(spec), np.int64), cfg, tile_to=3 * 1024 + 1)
        counts = ctx.plan_class_counts(reset=True)
        stats = ctx.generic_launch_stats(reset=True)
    assert min(chunks) >= 3 and copies == [3], (chunks, copies)
    _same(chunked, got, "ADH_CHUNK=256")
    want, _ = go.expected_stats(case, soa, cfg)
    _stats_equal(stats, want, times=3)
    assert stats["candidates"][go.GROUP_SPILL] == 3 * 117
    assert np.array_equal(counts, 3 * bs.histogram(bs.classes_of(case, soa, cfg)))


def test_compact_and_resident_entry_points_on_the_oversize_sweep(ctx):
    case, soa, spec = go.oversize_sweep()
    cfg = config_of("all_fragments")
    _staged(ctx, case)
    m = pack_assembled(soa)
    tab = {k: np.array(v, copy=True) for k, v in ctx.score_host(m, cfg.to_jitclass(), with_stats=True).items()}
    want, _ = go.expected_stats(case, soa, cfg)
    hist = bs.histogram(bs.classes_of(case, soa, cfg))
    ctx.plan_class_counts(reset=True)
    ctx.generic_launch_stats(reset=True)
    comp = ctx.score_host_compact(m, cfg.to_jitclass())
    assert np.array_equal(ctx.plan_class_counts(reset=True), hist)
    _stats_equal(ctx.generic_launch_stats(reset=True), want)
    slots = _compact_equals_padded(comp, tab)
    ctx.score_resident(m, cfg.to_jitclass())
    assert np.array_equal(ctx.plan_class_counts(reset=True), hist)
    _stats_equal(ctx.generic_launch_stats(reset=True), want)
    _compact_equals_padded(ctx.take_rows(np.arange(len(spec))), tab)
    assert slots.max() >= 150 and len(slots) == 1386


def test_the_bound_that_is_left(ctx, oracle_lib):
    """The spill layout still grows with K * O (32 bytes a pair, 73 a fragment): one candidate whose library slice is
    one fragment past the bound is refused before anything is launched or counted, the one on the bound is scored."""
    case, soa, spec = go.ragged_sweep()
    cfg = config_of("all_fragments")
    row = int(np.flatnonzero((spec["O"].values == 2) & (spec["F"].values == 8) & (spec["position"].values == 1))[0])
    k_max = go.spill_k_max(2, 8, 3)
    start = int(soa["frag_start_idx"][row])
    assert start + k_max + 1 <= len(case.library.fragment_df) and k_max > 1000
    _staged(ctx, case)

    def one(k):
        s = _rows(soa, np.array([row]))
        s["frag_stop_idx"] = (s["frag_start_idx"].astype(np.int64) + k).astype(s["frag_stop_idx"].dtype)
        return s

    ctx.plan_class_counts(reset=True)
    ctx.generic_launch_stats(reset=True)
    with pytest.raises(HipBackendError, match=rf"spill path of the generic kernel \(K={k_max + 1} O=2\): exceeds the bound of {go.LDS_LIMIT} bytes"):
        ctx.score_host(pack_assembled(one(k_max + 1)), cfg.to_jitclass())
    assert ctx.plan_class_counts().sum() == 0 and ctx.generic_launch_stats()["candidates"].sum() == 0
    assert ctx.generic_launch_stats()["lds_bytes"].sum() == 0

    inside = one(k_max)
    got = {k: np.array(v, copy=True) for k, v in ctx.score_host(pack_assembled(inside), cfg.to_jitclass(), with_stats=True).items()}
    stats = ctx.generic_launch_stats(reset=True)
    assert stats["candidates"].tolist() == [0, 0, 1]
    assert stats["lds_bytes"][go.GROUP_SPILL] == go.layout_bytes(k_max, 2, 8, 3, spill=True) > go.LDS_LIMIT - 200
    from alphadia_amd.scoring import fragment_columns
    exp = oracle_lib.score(case.dia, fragment_columns(case.library.fragment_df, "mz_library"), pack_assembled(inside),
                           cfg.to_jitclass(), n_threads=1, with_stats=True)
    assert exp["valid"].astype(bool).all()
    _against_oracle(got, exp, cfg)
