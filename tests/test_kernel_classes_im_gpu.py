"""The ion-mobility scoring kernels at their scan and cycle limits: HIP against the oracle on the shape sweep of
tests/box_sweep_im.py (boxes of 2 ... 36 cycles x 2 ... 48 scans at every edge of a run that ends inside a cycle, centres
on the first / middle / last cycle and scan, one to six observations, one and two MS1 rows, slices of 1 ... 40
fragments, batches whose maxima sit below, at and past the limits of the fixed layouts, and candidates whose events
are written cell by cell onto every rung of the gather's overflow ladder).

Per configuration: the routing (``Context.plan_class_counts``) equals the restated class rule exactly, the default
path equals the oracle with no row behind a knife-edge mask, and scoring in several chunks changes nothing.  On the
default configuration every other way to the same numbers (one-kernel path, one candidate per wavefront, dynamic layout,
all tiles materialised, certain batches, the tile layouts of the staged run) is bit-equal to the default, and the
candidates that took the materialised tiles (ADH_DEBUG_IM_DROP_DENSE) are the ones designed to.  Run with ``-m gpu`` on
an MI355X."""

import time

import numpy as np
import pytest

import box_sweep_im as bi
import helpers as H
from alphadia_amd import runtime
from alphadia_amd.scoring import assemble_candidates, fragment_columns, pack_assembled
from test_gpu_parity import PPM_ABS_TOL_GOLDEN, PPM_ABS_TOL_ORACLE, REL_TOL, compare
from test_kernel_classes_gpu import _rows, _same, score_batches

pytestmark = pytest.mark.gpu

RESCUED_CAP = 0   # rows a knife-edge mask of compare() may take out of a comparison that would have failed


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


@pytest.fixture(scope="module")
def sweeps():
    """The three runs of the sweep with their assembled candidate tables, batches and specifications: built once, never
    written to."""
    out = {}
    for run in bi.RUNS:
        case = bi.sweep_case(run)
        soa = H.soa_for(case, bi.config_of("defaults"))
        spec = bi.spec_rows(run)
        assert np.array_equal(soa["precursor_idx"], np.arange(len(spec)))  # (table order = sweep order)
        out[run] = (case, soa, spec)
    return out


_oracle_cache, _default_cache = {}, {}


def oracle_tables(oracle_lib, sweeps, run, name):
    if (run, name) not in _oracle_cache:
        case, soa, _ = sweeps[run]
        _oracle_cache[(run, name)] = oracle_lib.score_timstof(
            case.dia, fragment_columns(case.library.fragment_df, "mz_library"), pack_assembled(soa),
            bi.config_of(name).to_jitclass(), n_threads=8, with_stats=True)
    return _oracle_cache[(run, name)]


def _staged(ctx, case):
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)


def default_tables(ctx, sweeps, run):
    """The default path of the default configuration (no switch set), scored once per run."""
    if run not in _default_cache:
        case, soa, spec = sweeps[run]
        _staged(ctx, case)
        _default_cache[run] = score_batches(ctx, soa, spec["batch"].values, bi.config_of("defaults"))
    return _default_cache[run]


def _name_rows(rows, spec, table, classes):
    return [dict(row=int(r), S=int(table["S"][r]), F=int(table["F"][r]), O=int(table["O"][r]), batch=str(spec["batch"][r]),
                 density=str(spec["density"][r]), kernel_class=int(classes[r])) for r in rows]


def _rescued_rows(got, exp, corr_abs):
    """Rows of the valid table a knife-edge mask of compare() took out of a comparison that would have failed."""
    bad = []
    for r in np.flatnonzero(exp["valid"].astype(bool)):
        compare({k: a[r:r + 1] for k, a in got.items()}, {k: a[r:r + 1] for k, a in exp.items()}, PPM_ABS_TOL_ORACLE, corr_abs=corr_abs)
        if any(compare.last_masked["rescued"].values()):
            bad.append(int(r))
    return bad


def _against_the_oracle(got, exp, corr_abs, spec, table, classes):
    compare(got, exp, PPM_ABS_TOL_ORACLE, rel_tol=REL_TOL, corr_abs=corr_abs)
    rescued = dict(compare.last_masked["rescued"])
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    v = exp["valid"].astype(bool)
    assert np.array_equal(np.isnan(got["features"][v]), np.isnan(exp["features"][v]))
    if any(n > RESCUED_CAP for n in rescued.values()):
        pytest.fail(f"knife-edge masks rescued {rescued}: {_name_rows(_rescued_rows(got, exp, corr_abs), spec, table, classes)}")


@pytest.mark.parametrize("name", list(bi.CONFIGS))
def test_every_route_matches_the_oracle(ctx, oracle_lib, sweeps, monkeypatch, name, capsys):
    t0 = time.perf_counter()
    cfg = bi.config_of(name)
    # experimental_xic = False: the K x K contraction runs on MFMA in another summation order than the oracle's;
    # correlations near zero get the absolute floor of test_timstof_randomized
    corr_abs = 0.0 if cfg.experimental_xic else 2e-6
    for run in bi.RUNS:
        case, soa, spec = sweeps[run]
        batch = spec["batch"].values
        exp = oracle_tables(oracle_lib, sweeps, run, name)
        table = bi.shape_table(case, soa, cfg)
        classes = bi.classes_of(table)
        _staged(ctx, case)
        # routing: the plan's counts are the restated rule's
        ctx.plan_class_counts(reset=True)
        got = score_batches(ctx, soa, batch, cfg)
        counts = ctx.plan_class_counts(reset=True)
        with capsys.disabled():
            print(f"\n[ion-mobility classes] {name} / {run}: {len(batch)} candidates, {int(exp['valid'].sum())} valid, classes "
                  f"{ {int(c): int(n) for c, n in enumerate(counts) if n} }")
        assert np.array_equal(counts, bi.histogram(classes)), (run, counts.tolist())
        assert ctx.plan_class_counts().sum() == 0
        if run == "base":
            assert set(bi.routes_of(table, batch, cfg).tolist()) == bi.REACHES[name]
        # values: the default path against the oracle; no row may need a knife-edge mask
        _against_the_oracle(got, exp, corr_abs, spec, table, classes)
        if run != "base":
            continue
        # several chunks (ADH_CHUNK=256; the library's floor is 1024 rows a chunk, so every batch is scored in as many
        # copies as make three chunks at least; a chunk is a launch of its own, with maxima of its own)
        with monkeypatch.context() as mp:
            mp.setenv("ADH_CHUNK", "256")
            chunked, _, copies = score_batches(ctx, soa, batch, cfg, tile_to=3 * 1024 + 1)
            chunk_counts = ctx.plan_class_counts(reset=True)
            for b, c in zip(np.unique(batch), copies):
                assert len(runtime.chunk_cuts(int((batch == b).sum()) * c, ion_mobility=True)) - 1 >= 3, b
        per_batch = [bi.histogram(classes[batch == b]) * c for b, c in zip(np.unique(batch), copies)]
        assert np.array_equal(chunk_counts, np.sum(per_batch, axis=0))
        _same(chunked, got, "ADH_CHUNK=256")
    with capsys.disabled():
        print(f"[ion-mobility classes] {name}: {time.perf_counter() - t0:.2f} s")


# (switch, value, read when the run is staged)
WAYS = [("ADH_DEBUG_IM_NO_SPLIT", "1", False), ("ADH_DEBUG_IM_TILE1", "1", False), ("ADH_DEBUG_IM_NO_FUSE4", "1", False),
        ("ADH_DEBUG_IM_TILE1_TWO", "1", False), ("ADH_DEBUG_IM_NO_SPLIT2", "1", False), ("ADH_DEBUG_IM_DYNAMIC_LAYOUT", "1", False),
        ("ADH_DEBUG_IM", "8", False), ("ADH_DEBUG_IM", "14", False), ("ADH_IM_TILED", "0", True),
        ("ADH_IM_TILE_SHIFTS", "2,3", True), ("ADH_IM_TILE_FRAMES", "0", True)]


@pytest.mark.parametrize("switch,value,at_staging", WAYS, ids=[f"{s}={v}" for s, v, _ in WAYS])
def test_every_way_to_the_same_numbers_is_bit_equal(ctx, sweeps, monkeypatch, switch, value, at_staging):
    """On the whole sweep - every batch, every density row, all three cycles - and not on a mid-sized random case."""
    cfg = bi.config_of("defaults")
    for run in bi.RUNS:
        base = default_tables(ctx, sweeps, run)
        case, soa, spec = sweeps[run]
        with monkeypatch.context() as mp:
            mp.setenv(switch, value)
            _staged(ctx, case)   # (the tile layout switches are read here; the others at the launch)
            other = score_batches(ctx, soa, spec["batch"].values, cfg)
        _same(other, base, f"{switch}={value} / {run}")
        assert base["valid"].sum() >= 50
    if at_staging:
        ctx.stage_run(sweeps["base"][0].dia, force=True)  # (leave the handle with the default layout)


def test_the_rows_that_take_the_materialised_tiles_are_the_designed_ones(ctx, sweeps, monkeypatch, capsys):
    """ADH_DEBUG_IM_DROP_DENSE=1 drops a candidate where the gather would have materialised its tiles: the rows valid by
    default and invalid then are the ones that took the dense path."""
    cfg = bi.config_of("defaults")
    case, soa, spec = sweeps["base"]
    batch, density = spec["batch"].values, spec["density"].values
    base = default_tables(ctx, sweeps, "base")
    _staged(ctx, case)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_IM_DROP_DENSE", "1")
        dropped = score_batches(ctx, soa, batch, cfg)
    valid = base["valid"].astype(bool)
    dense = valid & ~dropped["valid"].astype(bool)
    assert not (dropped["valid"].astype(bool) & ~valid).any()
    by_design = np.isin(density, bi.DENSE_BY_DESIGN)
    fits_by_design = (density != "") & ~by_design
    table = bi.shape_table(case, soa, cfg)
    routes = bi.routes_of(table, batch, cfg)
    with capsys.disabled():
        print(f"\n[ion-mobility dense rows] by design {int(by_design.sum())}, in fact {int(dense.sum())} of {int(valid.sum())} valid rows "
              f"(planted rows among them: {int((dense & (density == '')).sum())}); per density "
              f"{ {d: (int((dense & (density == d)).sum()), int((density == d).sum())) for d in bi.DENSITIES} }")
    assert valid[density != ""].all()
    assert dense[by_design].all(), np.flatnonzero(by_design & ~dense).tolist()
    assert not dense[fits_by_design].any(), np.flatnonzero(fits_by_design & dense).tolist()
    # the mixed launches: sparse candidates four to a wavefront, the dense ones on the side list of the same grid
    for b, route in (("a", (bi.CLASS_SMALL, "small", "fused4")), ("a", (bi.CLASS_TWO, "common2", "tile4")),
                     ("b1", (bi.CLASS_ONE, "common", "fused4")), ("b1", (bi.CLASS_TWO, "common2", "tile4"))):
        launch = (batch == b) & np.array([r == route for r in routes])
        assert (launch & dense).sum() >= 4 and (launch & valid & ~dense).sum() >= 16, (b, route, int((launch & dense).sum()))
    # every other row: the same bits
    keep = ~dense
    for k in base:
        assert np.array_equal(base[k][keep], dropped[k][keep], equal_nan=True), k


def test_rows_over_the_pair_capacity_take_the_materialised_tiles(ctx, oracle_lib, sweeps, monkeypatch, capsys):
    """The run "fine" under the wide tolerance, staged without the tile layout (ADH_IM_TILED=0: the gather counts
    (window, TOF bin) pairs; with the layout it counts (window, tile) pairs where those fit): the rows designed over
    ADH_IM_PAIR_CAP take the materialised tiles, the rows designed under it do not, in launches that hold both; the
    tables equal the oracle and, bit for bit, those of the default staging."""
    cfg = bi.config_of("wide_tolerance")
    case, soa, spec = sweeps["fine"]
    batch, density = spec["batch"].values, spec["density"].values
    _staged(ctx, case)
    with_layout = score_batches(ctx, soa, batch, cfg)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_IM_TILED", "0")
        _staged(ctx, case)
        got = score_batches(ctx, soa, batch, cfg)
        mp.setenv("ADH_DEBUG_IM_DROP_DENSE", "1")
        dropped = score_batches(ctx, soa, batch, cfg)
    ctx.stage_run(case.dia, force=True)  # (leave the handle with the default layout)
    _same(got, with_layout, "ADH_IM_TILED=0 / fine")
    exp = oracle_tables(oracle_lib, sweeps, "fine", "wide_tolerance")
    table = bi.shape_table(case, soa, cfg)
    _against_the_oracle(got, exp, 0.0, spec, table, bi.classes_of(table))
    valid = got["valid"].astype(bool)
    dense = valid & ~dropped["valid"].astype(bool)
    over = density == "pairs_over"
    with capsys.disabled():
        print(f"\n[ion-mobility pair capacity] over by design {int(over.sum())}, dense in fact {int(dense.sum())} of {int(valid.sum())} valid rows")
    assert valid.all() and dense[over].all() and not dense[~over].any(), np.flatnonzero(dense != over).tolist()
    routes = bi.routes_of(table, batch, cfg)
    for route in bi._SPLIT:
        launch = np.array([r == route for r in routes])
        assert (launch & dense).sum() >= 4 and (launch & ~dense).sum() >= 4, route
    for k in got:
        assert np.array_equal(got[k][~dense], dropped[k][~dense], equal_nan=True), k


@pytest.mark.parametrize("b", ["a", "b1"])
def test_more_materialised_tiles_than_blocks_that_take_them(ctx, sweeps, monkeypatch, b):
    """A split launch hands its materialised tiles to at most 1024 blocks of its grid, which take them in turn.  With
    every tile materialised (ADH_DEBUG_IM=8) and a batch in so many copies that each of its classes holds more than 1024
    rows, every copy equals the default path of the batch bit for bit."""
    cfg = bi.config_of("defaults")
    case, soa, spec = sweeps["base"]
    base = default_tables(ctx, sweeps, "base")
    idx = np.flatnonzero(spec["batch"].values == b)
    classes = bi.classes_of(bi.shape_table(case, soa, cfg))[idx]
    fewest = min(int((classes == c).sum()) for c in (bi.CLASS_ONE, bi.CLASS_TWO, bi.CLASS_SMALL) if (classes == c).any())
    copies = -(-1025 // fewest)
    _staged(ctx, case)
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_IM", "8")
        ctx.plan_class_counts(reset=True)
        got, _, reps = score_batches(ctx, _rows(soa, idx), spec["batch"].values[idx], cfg, tile_to=copies * len(idx))
        counts = ctx.plan_class_counts(reset=True)
    assert reps == [copies] and len(runtime.chunk_cuts(copies * len(idx), ion_mobility=True)) == 2  # (one chunk, one launch per class)
    assert min(int(n) for n in counts if n) > 1024
    for k in got:
        assert np.array_equal(got[k], base[k][idx], equal_nan=True), k


def test_fixture_rows_match_the_reference(ctx, oracle_lib):
    """tests/golden/scoring_boxes_timstof.npz: the thinned sweep against the reference's values, at the bar of
    test_timstof_golden_inputs."""
    from test_oracle_golden import _tims_golden

    z, dia, fragment_df, precursor_df, cand, cfg = _tims_golden("scoring_boxes_timstof.npz")
    soa = assemble_candidates(cand, precursor_df, "mz_library")
    ctx.stage_run(dia, force=True)
    ctx.stage_fragments(*fragment_columns(fragment_df, "mz_library"), force=True)
    got = ctx.score_host(pack_assembled(soa), cfg.to_jitclass(), with_stats=True)
    got = {k: np.array(v, copy=True) for k, v in got.items()}
    exp = oracle_lib.score_timstof(dia, fragment_columns(fragment_df, "mz_library"), pack_assembled(soa), cfg.to_jitclass(),
                                   with_stats=True)
    compare(got, exp, PPM_ABS_TOL_ORACLE)
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    golden = {n: z["out_" + n] for n in H.OUT_NAMES}
    compare(got, golden, PPM_ABS_TOL_GOLDEN, rel_tol=REL_TOL, corr_abs=1e-3)
    assert got["valid"].sum() >= 100
