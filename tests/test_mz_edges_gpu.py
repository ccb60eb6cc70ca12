"""GPU: the four implementations of m/z window matching on the designed-edge runs of tests/mz_edges.py - peaks on the
float32 bounds of the tolerance windows, on the edges of the transposed run's bins, on powers of two, on the ends of
the run, equal m/z, intensities at the cuts of the running mean; TOF bins on the bounds and on the lookup buckets.

* the dense tile of the gather kernels against the reference's ``get_dense`` (tests/golden/get_dense_mz_edges.npz),
  bit for bit, with the membership decoded per designed peak;
* every scoring kernel class with a matching loop or a window plumbing of its own against the oracle (which
  tests/test_mz_edges.py pins to the reference on the same runs) and against each other;
* candidate selection, on both run layouts, against the oracle's - on runs of its own (``selection_case``,
  ``selection_case_timstof``) with peaks on and one step outside the bounds of every window, not on the queries above.

Run with ``-m gpu`` on an MI355X."""

import numpy as np
import pytest

import box_sweep as bs
import helpers as H
import mz_edges as E
import test_generic_oversize as go
from alphadia_amd import runtime
from alphadia_amd.runtime import HipBackendError
from alphadia_amd.scoring import fragment_columns, pack_assembled
from test_gpu_parity import PPM_ABS_TOL_ORACLE, compare
from test_mz_edges import ALPHARAW_RUNS, built

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(H.golden_path("get_dense_mz_edges.npz"))


# ---------------------------------------------------------------------------------------------- dense tile
SLAB_PEAKS, BLOCK_CYCLES, BLOCKS_PER_GROUP = 100, 8, 8  # (ADH_SUB = 8 blocks a group, adh_device.h: slabs are whole groups)


@pytest.mark.parametrize("run,slabs", [(r, "one_slab") for r in ALPHARAW_RUNS] + [("main", "several_slabs")])
def test_hip_dense_tile_matches_reference_on_edges(ctx, golden, monkeypatch, run, slabs):
    """The standard of test_hip_dense_tile_matches_reference_alpharaw on every designed case: observation list and both
    planes bit for bit; the run of 136 cycles also in blocks of 8 cycles, one slab per group of 64 (the runs of 8 cycles
    are one group however they are staged).  The one non-ascending query list is refused: the kernels sort by m/z,
    get_dense walks the list as given, and no caller of the gather passes an unsorted list."""
    dia, cases = built(run)
    with monkeypatch.context() as mp:
        if slabs == "several_slabs":
            # three groups of blocks, each with more peaks than a slab may hold together with its neighbour: three slabs
            # (the library exports no slab count; this is the guard of test_run_staged_in_slabs_scores_identically)
            per_group = BLOCK_CYCLES * BLOCKS_PER_GROUP * dia.cycle_len
            groups = [(int(dia.peak_start_idx_list[a]), int(dia.peak_stop_idx_list[min(a + per_group, dia.n_spectra) - 1]))
                      for a in range(0, dia.n_spectra, per_group)]
            assert len(groups) == 3 and all(b - a > SLAB_PEAKS for a, b in groups), groups
            mp.setenv("ADH_STAGE_SLAB_PEAKS", str(SLAB_PEAKS))
            mp.setenv("ADH_BLOCK_CYCLES", str(BLOCK_CYCLES))
        ctx.stage_run(dia, force=True)
    wrong, hits = [], 0
    for c in cases:
        fl = c.frame_limits
        if not c.ascending:
            with pytest.raises(HipBackendError, match=r"\(-1\): mz_query must ascend"):
                ctx.debug_get_dense(fl[0, 0], fl[0, 1], c.mz_query, c.tol, c.quad[0, 0], c.quad[0, 1])
            continue
        e = golden[f"{run}_{c.name}_dense"]
        dense, obs = ctx.debug_get_dense(fl[0, 0], fl[0, 1], c.mz_query, c.tol, c.quad[0, 0], c.quad[0, 1])
        assert np.array_equal(obs, golden[f"{run}_{c.name}_pidx"]), c.name
        assert dense.shape == e.shape[:3] + (1,) + e.shape[4:], (c.name, dense.shape, e.shape)
        if c.expected is not None and not np.array_equal(dense[0, :, 0, 0, :], c.expected):
            wrong.append(E.describe_difference(c, dense[0, :, 0, 0, :]))
            continue
        assert np.array_equal(e[:, :, :, 0, :], e[:, :, :, 1, :]), c.name  # the reference writes the same value to both scan slots
        if not np.array_equal(dense[0, :, :, 0, :], e[0, :, :, 0, :]):
            wrong.append(f"case {c.name}: intensity plane differs from the reference")
        elif not np.array_equal(dense[1, :, :, 0, :], e[1, :, :, 0, :]):
            at = tuple(np.argwhere(dense[1, :, :, 0, :] != e[1, :, :, 0, :])[0])
            wrong.append(f"case {c.name}: m/z plane differs at (query, observation, cycle) {at}: "
                         f"{dense[1, :, :, 0, :][at]!r} != {e[1, :, :, 0, :][at]!r}")
        hits += int((e[0] > 0).sum())
    ctx.stage_run(dia, force=True)  # (leave the handle with the default staging)
    assert not wrong, "\n".join(wrong)
    assert hits > 50


@pytest.mark.parametrize("layout", ["tiled", "ADH_IM_TILED=0"])
def test_hip_dense_tile_matches_reference_on_timstof_edges(ctx, golden, monkeypatch, layout):
    """The same for the ion-mobility run (test_hip_dense_tile_matches_reference_timstof): TOF bins on the bounds and
    one float64 step beside them, bounds on the lookup buckets' edges, with the tile layout and without."""
    dia, cases = built("tims")
    with monkeypatch.context() as mp:
        if layout != "tiled":
            mp.setenv("ADH_IM_TILED", "0")
        ctx.stage_run(dia, force=True)
    wrong, hits = [], 0
    for c in cases:
        fl, sl = c.frame_limits, c.scan_limits
        e = golden[f"tims_{c.name}_dense"]
        dense, obs = ctx.debug_get_dense(fl[0, 0], fl[0, 1], c.mz_query, c.tol, c.quad[0, 0], c.quad[0, 1],
                                         scan_start=sl[0, 0], scan_stop=sl[0, 1])
        assert np.array_equal(obs, golden[f"tims_{c.name}_pidx"]) and dense.shape == e.shape, c.name
        if not np.array_equal(dense[0], c.expected):
            wrong.append(E.describe_difference(c, dense[0]))
        elif not np.array_equal(dense, e):
            wrong.append(f"case {c.name}: differs from the reference")
        hits += int((e[0] > 0).sum())
    ctx.stage_run(dia, force=True)
    assert not wrong, "\n".join(wrong)
    assert hits > 50


# ---------------------------------------------------------------------------------------------- scoring, AlphaRaw
def _score(ctx, soa, cfg):
    ctx.plan_class_counts(reset=True)
    ctx.generic_launch_stats(reset=True)
    got = ctx.score_host(pack_assembled(soa), cfg.to_jitclass(), with_stats=True)
    got = {k: np.array(v, copy=True) for k, v in got.items()}
    return got, ctx.plan_class_counts(reset=True), ctx.generic_launch_stats(reset=True)


def _against_oracle(got, exp, what):
    compare(got, exp, PPM_ABS_TOL_ORACLE)
    assert not any(compare.last_masked["rescued"].values()), (what, compare.last_masked["rescued"])  # no mask may rescue a row here
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"]), what
    v = exp["valid"].astype(bool)
    for t in ("fragment_intensity", "fragment_mz_observed"):
        same = (got[t][v] == exp[t][v]) | (np.isnan(got[t][v]) & np.isnan(exp[t][v]))
        assert same.all(), (what, t, np.argwhere(~same)[:5].tolist())


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.fixture(scope="module")
def edge_scoring(oracle_lib):
    """The edge queries as libraries of at most 12 fragments a precursor and of 17 ... 64, with the oracle's tables."""
    dia, cases = built("main")
    out = {}
    for name, kw, updates in (("narrow", dict(at_most=12, at_least=4), dict(top_k_fragments=12)),
                              ("wide", dict(at_most=24, at_least=17, every_query=True), dict(top_k_fragments=9999))):
        case = E.scoring_case(dia, cases, **kw)
        cfg = bs.config_of("isotopes4")  # the handler's settings with all four isotope windows
        cfg.update(updates)
        soa = H.soa_for(case, cfg)
        exp, _ = H.oracle_score(oracle_lib, case, cfg, soa=soa, n_threads=4, with_stats=True)
        assert exp["valid"].astype(bool).all() and exp["stat_matched_peaks"].min() > 0
        out[name] = (case, cfg, soa, exp)
    return out


def test_scoring_kernels_on_edges_up_to_12_fragments(ctx, edge_scoring, monkeypatch):
    """The fused kernel (bit patterns: win_bits / task_run) and the register kernels behind the gather kernel
    (floats: bins_of / gather_task) on the same rows, at the handler's 15 ppm (the cases designed at another tolerance
    are ordinary windows here: test_scoring_kernels_on_edges_at_other_tolerances): each equals the oracle with stat_matched_peaks exact and the
    fragment intensities and observed m/z bit for bit, and they equal each other bit for bit."""
    case, cfg, soa, exp = edge_scoring["narrow"]
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)
    fused, counts, _ = _score(ctx, soa, cfg)
    assert np.array_equal(counts, bs.histogram(bs.classes_of(case, soa, cfg)))
    assert counts[:14].sum() == len(soa["precursor_idx"]) and counts[bs.CLASS_FUSED1:bs.CLASS_FUSED2].sum() > 0 and counts[bs.CLASS_FUSED2:14].sum() > 0
    _against_oracle(fused, exp, "fused")
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_NO_FUSED", "1")
        two, counts, _ = _score(ctx, soa, cfg)
    assert np.array_equal(counts, bs.histogram(bs.classes_of(case, soa, cfg, no_fused=True)))
    assert counts[bs.CLASS_FAST2:bs.CLASS_WIDE2].sum() == len(soa["precursor_idx"]) and counts[bs.CLASS_FAST1:bs.CLASS_WIDE2].sum() > 0
    _against_oracle(two, exp, "register kernels")
    _same(two, fused, "register kernels against the fused kernel")
    # blocks of 8 cycles, one slab per group of 64: the box (60, 72) crosses a group
    with monkeypatch.context() as mp:
        mp.setenv("ADH_STAGE_SLAB_PEAKS", "100")
        mp.setenv("ADH_BLOCK_CYCLES", "8")
        ctx.stage_run(case.dia, force=True)
        _same(_score(ctx, soa, cfg)[0], fused, "fused kernel, three groups of blocks")
        mp.setenv("ADH_DEBUG_NO_FUSED", "1")
        _same(_score(ctx, soa, cfg)[0], fused, "register kernels, three groups of blocks")
    ctx.stage_run(case.dia, force=True)


@pytest.mark.parametrize("tol", [5.0, 60.0, 200.0])
def test_scoring_kernels_on_edges_at_other_tolerances(ctx, oracle_lib, monkeypatch, tol):
    """The scoring legs above run at the handler's 15 ppm, where the cases designed at 5, 60 and 200 ppm are ordinary
    windows.  Here the fragment tolerance is the case's own: the window inside one bin, the cell that continues over
    three bins (``first_bin`` / ``b > w.b_lo``) and the windows three deep reach the fused kernel and the register
    kernels with their edges - against the oracle, bit-equal to each other."""
    dia, cases = built("main")
    case = E.scoring_case(dia, cases, lists=[E.tolerance_lists(cases)[tol]])
    cfg = bs.config_of("isotopes4")
    cfg.update(dict(fragment_mz_tolerance=tol))
    soa = H.soa_for(case, cfg)
    exp, _ = H.oracle_score(oracle_lib, case, cfg, soa=soa, n_threads=4, with_stats=True)
    assert exp["valid"].astype(bool).all() and exp["stat_matched_peaks"].min() > 0
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)
    fused, counts, _ = _score(ctx, soa, cfg)
    assert counts[:14].sum() == len(soa["precursor_idx"])
    _against_oracle(fused, exp, f"fused, {tol} ppm")
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_NO_FUSED", "1")
        two, counts, _ = _score(ctx, soa, cfg)
    assert counts[bs.CLASS_FAST2:bs.CLASS_WIDE2].sum() == len(soa["precursor_idx"])
    _against_oracle(two, exp, f"register kernels, {tol} ppm")
    _same(two, fused, f"register kernels against the fused kernel, {tol} ppm")


def test_scoring_kernels_on_edges_past_16_fragments(ctx, edge_scoring, monkeypatch):
    """17 ... 64 kept fragments (top_k_fragments = 9999): the wide register kernels, the generic kernel in their place
    (ADH_DEBUG_NO_WIDE) and its spill form (ADH_DEBUG_GENERIC_SPILL) - each against the oracle, all bit-equal."""
    case, cfg, soa, exp = edge_scoring["wide"]
    n = len(soa["precursor_idx"])
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)
    wide, counts, _ = _score(ctx, soa, cfg)
    assert np.array_equal(counts, bs.histogram(bs.classes_of(case, soa, cfg)))
    assert counts[bs.CLASS_WIDE2:bs.CLASS_GENERIC].sum() == n
    assert counts[bs.CLASS_WIDE2:bs.CLASS_MID2].sum() > 0 and counts[bs.CLASS_MID2:bs.CLASS_GENERIC].sum() > 0  # 64 and 32 lanes
    _against_oracle(wide, exp, "wide")
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_NO_WIDE", "1")
        generic, counts, stats = _score(ctx, soa, cfg)
        assert counts[bs.CLASS_GENERIC] == n == counts.sum() and stats["candidates"][go.GROUP_SPILL] == 0
        mp.setenv("ADH_DEBUG_GENERIC_SPILL", "1")
        spill, counts, stats = _score(ctx, soa, cfg)
        assert counts[bs.CLASS_GENERIC] == n and stats["candidates"].tolist() == [0, 0, n]
    _against_oracle(generic, exp, "generic")
    _against_oracle(spill, exp, "generic, spill form")
    _same(generic, wide, "generic against the wide kernels")
    _same(spill, generic, "spill form against the LDS form")


# ---------------------------------------------------------------------------------------------- scoring, ion mobility
def test_ion_mobility_scoring_kernels_on_edges(ctx, oracle_lib, monkeypatch):
    """The TOF search of the ion-mobility kernels (adh_index_im.hip over the lookup table) under the edge queries as a
    library: the four-candidates-a-wavefront kernel and the two-observation tile route by default, the dynamic route
    (ADH_DEBUG_IM_DYNAMIC_LAYOUT) and its spill form (ADH_DEBUG_IM_SPILL) - against the oracle, all bit-equal."""
    import box_sweep_im as bi
    import box_sweep_im_oversize as bo

    dia, cases = built("tims")
    case = E.scoring_case_timstof(dia, cases)
    cfg = bi.config_of("defaults")
    soa = H.soa_for(case, cfg)
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    exp = oracle_lib.score_timstof(dia, cols, pack_assembled(soa), cfg.to_jitclass(), n_threads=4, with_stats=True)
    assert exp["valid"].astype(bool).all() and exp["stat_matched_peaks"].min() > 0
    table = bi.shape_table(case, soa, cfg)
    one_batch = np.zeros(len(table), dtype=np.int64)
    assert set(bi.routes_of(table, one_batch, cfg).tolist()) == {(bi.CLASS_SMALL, "small", "fused4"), (bi.CLASS_TWO, "common2", "tile4")}
    assert set(bi.routes_of(table, one_batch, cfg, {"ADH_DEBUG_IM_DYNAMIC_LAYOUT": "1"}).tolist()) == {(bi.CLASS_SMALL, "dynamic", "one"), (bi.CLASS_TWO, "dynamic", "one")}
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*cols, force=True)

    def score():
        ctx.plan_class_counts(reset=True)
        ctx.im_launch_stats(reset=True)
        got = {k: np.array(v, copy=True) for k, v in ctx.score_host(pack_assembled(soa), cfg.to_jitclass(), with_stats=True).items()}
        return got, ctx.plan_class_counts(reset=True), ctx.im_launch_stats(reset=True)

    def against_oracle(got, what):
        _against_oracle(got, exp, what)
        assert np.array_equal(np.isnan(got["features"]), np.isnan(exp["features"])), what

    default, counts, stats = score()
    assert np.array_equal(counts, bi.histogram(bi.classes_of(table))) and stats["candidates"].sum() == 0  # (no dynamic launch)
    against_oracle(default, "default routes")
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_IM_DYNAMIC_LAYOUT", "1")
        dynamic, _, stats = score()
        assert stats["candidates"].sum() == len(table) and stats["candidates"][bo.GROUP_SPILL] == 0
        mp.setenv("ADH_DEBUG_IM_SPILL", "1")
        spill, _, stats = score()
        assert stats["candidates"].tolist() == [0, 0, len(table)]
    against_oracle(dynamic, "dynamic route")
    _same(dynamic, default, "dynamic route against the default routes")
    _same(spill, default, "spill form against the default routes")
    with monkeypatch.context() as mp:  # without the tile layout of the staged run the gather walks the TOF bin ranges
        mp.setenv("ADH_IM_TILED", "0")
        ctx.stage_run(dia, force=True)
        _same(score()[0], default, "ADH_IM_TILED=0 against the default staging")
    ctx.stage_run(dia, force=True)


# ---------------------------------------------------------------------------------------------- candidate selection
def test_selection_on_edges(ctx, oracle_lib):
    """adh_select.hip's intensity-only copy of the matching loop: peaks on lo and hi of every fragment and isotope
    window and, ten times as strong, one ulp outside.  The candidate table equals the oracle's under the rules of
    tests/test_selection_limits_gpu.py; tests/test_mz_edges.py shows that one peak on the wrong side moves the score
    by three orders of magnitude more than that comparison allows."""
    import selection_limits as SL
    from test_mz_edges import select_on_edges

    def device(dia, cols, pm, cfg, kern):
        ctx.stage_run(dia, force=True)
        ctx.stage_fragments(*cols, force=True)
        return SL.copy_table(ctx.select_candidates(pm, cfg, kern))

    got, case = select_on_edges(device)
    exp, _ = select_on_edges(lambda dia, cols, pm, cfg, kern: oracle_lib.select(dia, cols, pm, cfg, kern, n_threads=4))
    assert (np.asarray(exp["score"]).reshape(E.SELECT_PRECURSORS, 3)[:, 0] > 0).all()
    SL.assert_tables_equal(got, exp, "m/z edges")


def test_selection_on_timstof_edges(ctx, oracle_lib):
    """Selection's ion-mobility gather is a consumer of its own of the TOF search (adh_index_im.hip): TOF bins on lo and
    one float64 step below hi of every fragment and isotope window and, ten times as strong, one step below lo and on
    hi (exclusive); one lo on an edge of the lookup buckets.  The candidate table equals the oracle's
    ``select_timstof`` under the rules of tests/test_selection_limits_gpu.py."""
    import selection_limits as SL
    from test_mz_edges import select_on_timstof_edges

    def device(dia, cols, pm, cfg, kern):
        ctx.stage_run(dia, force=True)
        ctx.stage_fragments(*cols, force=True)
        return SL.copy_table(ctx.select_candidates(pm, cfg, kern))

    got, case = select_on_timstof_edges(device)
    exp, _ = select_on_timstof_edges(lambda dia, cols, pm, cfg, kern: oracle_lib.select_timstof(dia, cols, pm, cfg, kern, n_threads=4))
    assert (np.asarray(exp["score"]).reshape(len(E.TS_PRECURSORS), 3)[:, 0] > 0).all()
    SL.assert_tables_equal(got, exp, "m/z edges, ion mobility")
