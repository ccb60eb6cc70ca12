"""No timsTOF scoring input is refused for the product of a call's maxima, or for a single candidate's tile below the
spill bound: the dynamic route of the ion-mobility feature kernel is launched in groups by each candidate's OWN LDS
layout, and a candidate whose own layout exceeds the LDS of a CU goes through the spill instantiation (its work and
profile regions in the scratch slab).  HIP against the oracle and against itself on the inputs of
tests/box_sweep_im_oversize.py; ``Context.im_launch_stats`` proves which path ran.  Run with ``-m gpu`` on an MI355X."""

import numpy as np
import pytest

import box_sweep_im as bi
import box_sweep_im_oversize as bo
import helpers as H
from alphadia_amd import runtime
from alphadia_amd.runtime import HipBackendError
from alphadia_amd.scoring import fragment_columns, pack_assembled
from test_gpu_parity import PPM_ABS_TOL_ORACLE, REL_TOL, compare
from test_kernel_classes_gpu import _compact_equals_padded, _same, _staged, score_batches

pytestmark = pytest.mark.gpu

RESCUED_CAP = 0   # rows a knife-edge mask of compare() may take out of a comparison that would have failed


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


def _score(ctx, soa, cfg, idx=None):
    m = pack_assembled(soa if idx is None else bo.rows_of(soa, idx))
    return {k: np.array(v, copy=True) for k, v in ctx.score_host(m, cfg.to_jitclass(), with_stats=True).items()}


def _take(tab: dict, idx) -> dict:
    return {k: v[idx] for k, v in tab.items()}


def _stats_equal(got: dict, want: dict, times: int = 1):
    assert np.array_equal(got["candidates"], want["candidates"] * times), (got, want)
    assert np.array_equal(got["lds_bytes"], want["lds_bytes"]), (got, want)


def _against_oracle(got, exp, cfg):
    # experimental_xic = False: the K x K contraction runs on MFMA in another summation order than the oracle's;
    # correlations near zero get the absolute floor of test_kernel_classes_im_gpu
    corr_abs = 0.0 if cfg.experimental_xic else 2e-6
    assert np.array_equal(got["valid"].astype(bool), exp["valid"].astype(bool))
    compare(got, exp, PPM_ABS_TOL_ORACLE, rel_tol=REL_TOL, corr_abs=corr_abs)
    rescued = dict(compare.last_masked["rescued"])
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    v = exp["valid"].astype(bool)
    assert np.array_equal(np.isnan(got["features"][v]), np.isnan(exp["features"][v]))
    assert not any(n > RESCUED_CAP for n in rescued.values()), rescued   # no knife-edge mask needed


def _histogram(case, soa, cfg):
    return bi.histogram(bi.classes_of(bi.shape_table(case, soa, cfg)))


@pytest.mark.parametrize("name", bo.CONFIG_NAMES)
def test_the_ragged_rows_in_one_call(ctx, oracle_lib, name):
    """Input A: refused before this for the product of its maxima, while no candidate needs more than the LDS of a CU.
    One call equals the per-batch calls bit for bit and the oracle; nothing spills."""
    case, soa, spec = bo.ragged()
    cfg = bo.config_of(name, "A")
    exp = bo.oracle_tables(oracle_lib, "A", name)
    _staged(ctx, case)
    per_batch = score_batches(ctx, soa, spec["batch"].values, cfg)
    ctx.plan_class_counts(reset=True)
    ctx.im_launch_stats(reset=True)
    got = _score(ctx, soa, cfg)
    counts = ctx.plan_class_counts(reset=True)
    stats = ctx.im_launch_stats(reset=True)
    _same(got, per_batch, "one call")
    _against_oracle(got, exp, cfg)
    want, _ = bo.expected_stats(case, soa, cfg)
    _stats_equal(stats, want)
    assert stats["candidates"][bo.GROUP_SPILL] == 0 and stats["candidates"][bo.GROUP_LARGE] >= 60
    assert np.array_equal(counts, _histogram(case, soa, cfg))
    assert ctx.im_launch_stats()["candidates"].sum() == 0


@pytest.mark.parametrize("name", bo.CONFIG_NAMES)
@pytest.mark.parametrize("which", ["B", "C"])
def test_the_oversize_inputs(ctx, oracle_lib, which, name):
    """Inputs B and C: the candidates whose own layout exceeds the LDS of a CU take the spill path, the others an LDS
    group; all match the oracle, and a row's bits do not depend on what it is scored with."""
    case, soa, spec = bo.input_of(which)
    cfg = bo.config_of(name, which)
    exp = bo.oracle_tables(oracle_lib, which, name)
    _staged(ctx, case)
    ctx.plan_class_counts(reset=True)
    ctx.im_launch_stats(reset=True)
    got = _score(ctx, soa, cfg)
    counts = ctx.plan_class_counts(reset=True)
    stats = ctx.im_launch_stats(reset=True)
    _against_oracle(got, exp, cfg)
    want, group = bo.expected_stats(case, soa, cfg)
    _stats_equal(stats, want)
    assert np.array_equal(counts, _histogram(case, soa, cfg))
    t = bi.shape_table(case, soa, cfg)
    over = bo.own_layouts(t, 3) > bo.LDS_LIMIT
    spilled = np.flatnonzero(group == bo.GROUP_SPILL)
    assert np.array_equal(spilled, np.flatnonzero(over)) and len(spilled) == stats["candidates"][bo.GROUP_SPILL] >= 5
    assert got["valid"].astype(bool)[spilled].sum() >= (60 if which == "B" else 5)
    # the rows over the limit alone, the rest alone
    rest = np.flatnonzero(~over)
    alone = _score(ctx, soa, cfg, spilled)
    s_alone = ctx.im_launch_stats(reset=True)
    assert s_alone["candidates"].tolist() == [0, 0, len(spilled)]
    assert s_alone["lds_bytes"][bo.GROUP_SPILL] == want["lds_bytes"][bo.GROUP_SPILL]
    others = _score(ctx, soa, cfg, rest)
    s_rest = ctx.im_launch_stats(reset=True)
    assert s_rest["candidates"][bo.GROUP_SPILL] == 0
    _stats_equal(s_rest, bo.expected_stats(case, bo.rows_of(soa, rest), cfg)[0])
    for part, idx in ((alone, spilled), (others, rest)):
        _same(part, _take(got, idx), "rows scored apart")


def test_spill_instantiation_equals_the_lds_one_on_the_base_sweep(ctx, monkeypatch):
    """ADH_DEBUG_IM_DYNAMIC_LAYOUT=1 with ADH_DEBUG_IM_SPILL=1 on the base sweep of tests/box_sweep_im.py: every
    candidate runs the spill instantiation, and the tables are bit-equal to the default path's on every row."""
    case = bi.sweep_case("base")
    cfg = bi.config_of("defaults")
    soa = H.soa_for(case, cfg)
    batch = bi.spec_rows("base")["batch"].values
    _staged(ctx, case)
    default = score_batches(ctx, soa, batch, cfg)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_IM_DYNAMIC_LAYOUT", "1")
        mp.setenv("ADH_DEBUG_IM_SPILL", "1")
        ctx.im_launch_stats(reset=True)
        spill = score_batches(ctx, soa, batch, cfg)
        stats = ctx.im_launch_stats(reset=True)
    assert stats["candidates"].tolist() == [0, 0, len(batch)] and default["valid"].sum() >= 500
    t = bi.shape_table(case, soa, cfg)
    assert stats["lds_bytes"][bo.GROUP_SPILL] == bo.own_layouts(t, 3, spill=True).max()
    _same(spill, default, "spill instantiation against the default path")


@pytest.mark.parametrize("name", ["all_fragments", "no_xic_all_fragments"])
def test_spill_instantiation_equals_the_lds_one_on_the_ragged_rows(ctx, monkeypatch, name):
    """The same on input A (up to 200 kept fragments): bit-equal to the default path, which takes the LDS groups."""
    case, soa, spec = bo.ragged()
    cfg = bo.config_of(name, "A")
    _staged(ctx, case)
    default = _score(ctx, soa, cfg)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_IM_DYNAMIC_LAYOUT", "1")
        lds = _score(ctx, soa, cfg)
        mp.setenv("ADH_DEBUG_IM_SPILL", "1")
        ctx.im_launch_stats(reset=True)
        spill = _score(ctx, soa, cfg)
        stats = ctx.im_launch_stats(reset=True)
        want, _ = bo.expected_stats(case, soa, cfg, env={"ADH_DEBUG_IM_DYNAMIC_LAYOUT": "1", "ADH_DEBUG_IM_SPILL": "1"})
    assert stats["candidates"].tolist() == [0, 0, len(spec)]
    _stats_equal(stats, want)
    _same(lds, default, "dynamic layout against the default path")
    _same(spill, default, "spill against the LDS instantiation")


def test_oversize_by_fragments_in_chunks(ctx, monkeypatch):
    """Input B tiled past three chunks (ADH_CHUNK=256; the library's floor is 1024 rows a chunk): every copy equals the
    single call, and the launch statistics are the per-copy ones times the copies."""
    case, soa, spec = bo.oversize_by_fragments()
    cfg = bo.config_of("all_fragments", "B")
    _staged(ctx, case)
    got = _score(ctx, soa, cfg)
    ctx.plan_class_counts(reset=True)
    ctx.im_launch_stats(reset=True)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_CHUNK", "256")
        chunked, _, copies = score_batches(ctx, soa, np.zeros(len(spec), np.int64), cfg, tile_to=3 * 1024 + 1)
        counts = ctx.plan_class_counts(reset=True)
        stats = ctx.im_launch_stats(reset=True)
        cuts = runtime.chunk_cuts(len(spec) * copies[0], ion_mobility=True)
    assert len(cuts) - 1 >= 3 and copies[0] * len(spec) >= 3 * 1024 + 1
    _same(chunked, got, "ADH_CHUNK=256")
    # a chunk is a plan of its own (its maxima choose the routes of its classes): the expectation is summed over the chunks
    rows = np.tile(np.arange(len(spec)), copies[0])
    cand, lds = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        want, _ = bo.expected_stats(case, bo.rows_of(soa, rows[a:b]), cfg)
        cand += want["candidates"]
        lds = np.maximum(lds, want["lds_bytes"])
    per_copy, group = bo.expected_stats(case, soa, cfg)
    assert np.array_equal(cand, per_copy["candidates"] * copies[0]) and np.array_equal(lds, per_copy["lds_bytes"])
    _stats_equal(stats, per_copy, times=copies[0])
    assert stats["candidates"][bo.GROUP_SPILL] == copies[0] * int((group == bo.GROUP_SPILL).sum())
    assert np.array_equal(counts, copies[0] * _histogram(case, soa, cfg))


def test_other_entry_points_on_oversize_by_fragments(ctx, oracle_lib):
    """``score_host_compact``, ``score_resident`` + ``take_rows`` and the operator on input B: the padded tables' valid
    rows and filled slots, rows of 150 and more filled slots among them; the padded table itself against the oracle
    (rows with all 200 slots filled).  Input B as drawn fills 61 ... 116 slots of a
    200-fragment slice (116 the most on an MI355X): a 15 ppm window is narrower than a TOF bin of the run, and about
    half the windows hold none.  This test therefore takes B with every library fragment ON a TOF bin - the same
    boxes, slices and routes."""
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS, HipCandidateScoring

    case, soa, spec = bo.oversize_by_fragments(on_bins=True)
    cfg = bo.config_of("all_fragments", "B")
    _staged(ctx, case)
    m = pack_assembled(soa)
    tab = {k: np.array(v, copy=True) for k, v in ctx.score_host(m, cfg.to_jitclass(), with_stats=True).items()}
    exp = oracle_lib.score_timstof(case.dia, fragment_columns(case.library.fragment_df, "mz_library"), m, cfg.to_jitclass(),
                                   n_threads=8, with_stats=True)
    _against_oracle(tab, exp, cfg)
    want, _ = bo.expected_stats(case, soa, cfg)
    hist = _histogram(case, soa, cfg)
    ctx.plan_class_counts(reset=True)
    ctx.im_launch_stats(reset=True)
    comp = ctx.score_host_compact(m, cfg.to_jitclass())
    assert np.array_equal(ctx.plan_class_counts(reset=True), hist)
    _stats_equal(ctx.im_launch_stats(reset=True), want)
    slots = _compact_equals_padded(comp, tab)
    ctx.score_resident(m, cfg.to_jitclass())
    assert np.array_equal(ctx.plan_class_counts(reset=True), hist)
    _stats_equal(ctx.im_launch_stats(reset=True), want)
    _compact_equals_padded(ctx.take_rows(np.arange(len(spec))), tab)
    assert slots.max() >= 150 and (slots >= 150).sum() >= 60

    scorer = HipCandidateScoring(
        dia_data=case.dia, precursors_flat=case.library.precursor_df, fragments_flat=case.library.fragment_df,
        rt_column="rt_library", mobility_column="mobility_library", precursor_mz_column="mz_library",
        fragment_mz_column="mz_library", config=cfg, device=0)
    fdf, frdf = scorer(case.candidates_df)
    keep = np.flatnonzero(tab["valid"].astype(bool))
    order = np.argsort(fdf["precursor_idx"].values, kind="stable")
    assert np.array_equal(fdf["precursor_idx"].values[order], tab["precursor_idx"][keep])
    assert np.array_equal(fdf[DEFAULT_FEATURE_COLUMNS].to_numpy()[order], tab["features"][keep], equal_nan=True)
    per_precursor = frdf.groupby("precursor_idx").size()
    assert np.array_equal(per_precursor.index.values, tab["precursor_idx"][keep])
    assert np.array_equal(per_precursor.values, slots) and len(frdf) == slots.sum()
    ctx.stage_run(case.dia, force=True)  # (the operator staged its own copies: leave the handle as the other tests expect it)


@pytest.mark.parametrize("O,S,F", [(2, 40, 32), (6, 48, 36)])
def test_the_bound_that_is_left(ctx, oracle_lib, O, S, F):
    """The spill layout still grows with K * O (221 bytes a fragment at two observations): one candidate whose library
    slice is one fragment past the bound is refused before anything is launched or counted, the one on the bound is
    scored; so are K = 300 at two observations in 40 x 32 and K = 200 at six in 48 x 36."""
    case, soa, spec, row = bo.bound_case(O, S, F)
    cfg = bo.config_of("all_fragments", "B")
    k_max = bo.spill_k_max(O, S, F, 3)
    k_asked = {2: 300, 6: 200}[O]
    start = int(soa["frag_start_idx"][row])
    assert start + k_max + 1 <= len(case.library.fragment_df) and k_max >= k_asked
    _staged(ctx, case)

    def one(k):
        s = bo.rows_of(soa, np.array([row]))
        s["frag_stop_idx"] = (s["frag_start_idx"].astype(np.int64) + k).astype(s["frag_stop_idx"].dtype)
        return s

    ctx.plan_class_counts(reset=True)
    ctx.im_launch_stats(reset=True)
    message = (rf"spill path of the ion-mobility feature kernel \(K={k_max + 1} O={O} S={S} F={F}\): "
               rf"exceeds the bound of {bo.LDS_LIMIT} bytes")
    with pytest.raises(HipBackendError, match=message):
        ctx.score_host(pack_assembled(one(k_max + 1)), cfg.to_jitclass())
    assert ctx.plan_class_counts().sum() == 0 and ctx.im_launch_stats()["candidates"].sum() == 0
    assert ctx.im_launch_stats()["lds_bytes"].sum() == 0

    for k in (k_max, k_asked):
        inside = one(k)
        got = {n: np.array(v, copy=True) for n, v in ctx.score_host(pack_assembled(inside), cfg.to_jitclass(), with_stats=True).items()}
        stats = ctx.im_launch_stats(reset=True)
        assert stats["candidates"].tolist() == [0, 0, 1]
        assert stats["lds_bytes"][bo.GROUP_SPILL] == bo.layout_bytes(k, O, S, F, 3, spill=True)
        exp = oracle_lib.score_timstof(case.dia, fragment_columns(case.library.fragment_df, "mz_library"), pack_assembled(inside),
                                       cfg.to_jitclass(), n_threads=1, with_stats=True)
        assert exp["valid"].astype(bool).all()
        _against_oracle(got, exp, cfg)
    assert bo.layout_bytes(k_max, O, S, F, 3, spill=True) > bo.LDS_LIMIT - 400
