"""Every kernel class of candidate scoring at its cycle and fragment limits: HIP against the oracle on the shape sweep
of tests/box_sweep.py (boxes of 2 ... 36 cycles, centre on the first / middle / last cycle, boxes at both ends of a
run that ends inside a cycle, one and two observations, library slices of 1 ... 200 fragments).

Per configuration: the routing (``Context.plan_class_counts``) equals the restated class rule exactly, the default
path equals the oracle, the two-kernel path (ADH_DEBUG_NO_FUSED) and the generic kernel in place of the wide ones
(ADH_DEBUG_NO_WIDE) are bit-equal to it, the generic kernel alone (ADH_DEBUG_NO_FAST) equals the oracle, no row needs
a knife-edge mask, and scoring in several chunks changes nothing.  Run with ``-m gpu`` on an MI355X."""

import time

import numpy as np
import pytest

import box_sweep as bs
import helpers as H
from alphadia_amd import _abi, runtime
from alphadia_amd.scoring import fragment_columns, pack_assembled
from test_full_size_gpu import RESCUED_BOUND
from test_gpu_parity import PPM_ABS_TOL_ORACLE, REL_TOL, compare

pytestmark = pytest.mark.gpu

CONFIGS, REACHES, config_of = bs.CONFIGS, bs.REACHES, bs.config_of


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


@pytest.fixture(scope="module")
def sweeps():
    """Both variants of the sweep with their assembled candidate tables and batches: built once, never written to."""
    out = {}
    for ragged in (False, True):
        case = bs.sweep_case(ragged)
        soa = H.soa_for(case, config_of("defaults"))
        batch = bs.spec_rows(ragged)["batch"].values
        assert np.array_equal(soa["precursor_idx"], np.arange(len(batch)))  # (table order = sweep order)
        out[ragged] = (case, soa, batch)
    return out


_oracle_cache = {}


def oracle_tables(oracle_lib, sweeps, name):
    if name not in _oracle_cache:
        case, soa, _ = sweeps[CONFIGS[name][0]]
        _oracle_cache[name] = H.oracle_score(oracle_lib, case, config_of(name), soa=soa, n_threads=4, with_stats=True)[0]
    return _oracle_cache[name]


def _rows(soa: dict, idx) -> dict:
    n = len(soa["precursor_idx"])
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in soa.items()}


def _staged(ctx, case):
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)


def score_batches(ctx, soa, batch, cfg, tile_to=0):
    """The sweep through the public entry point, one call per batch (box_sweep.NL_LONG), merged into tables of the
    widest call in sweep order.  ``tile_to``: every batch is repeated until it has that many rows (ADH_CHUNK has a
    floor of 1024 rows: several chunks need several thousand rows); the copies must equal each other bit for bit and
    the first one is returned, together with the number of chunks and of copies of every call."""
    n = len(batch)
    parts, chunks, copies = [], [], []
    for b in np.unique(batch):
        idx = np.flatnonzero(batch == b)
        reps = max(1, -(-tile_to // len(idx)))
        got = ctx.score_host(pack_assembled(_rows(soa, np.tile(idx, reps))), cfg.to_jitclass(), with_stats=True)
        got = {k: np.array(v, copy=True) for k, v in got.items()}
        for k, v in got.items():
            for r in range(1, reps):
                assert np.array_equal(v[r * len(idx):(r + 1) * len(idx)], v[:len(idx)], equal_nan=True), (k, r)
        parts.append((idx, {k: v[:len(idx)] for k, v in got.items()}))
        chunks.append(len(runtime.chunk_cuts(len(idx) * reps)) - 1)
        copies.append(reps)
    merged = {}
    for k in parts[0][1]:
        first = parts[0][1][k]
        width = max(p[k].shape[1] if p[k].ndim == 2 else 0 for _, p in parts)
        merged[k] = np.zeros((n, width) if first.ndim == 2 else (n,), dtype=first.dtype)
        for idx, p in parts:
            if first.ndim == 2:
                merged[k][idx, : p[k].shape[1]] = p[k]
            else:
                merged[k][idx] = p[k]
    return (merged, chunks, copies) if tile_to else merged


def _same(a: dict, b: dict, what: str):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _name_rows(rows, classes, table):
    return [dict(row=int(r), kernel_class=int(classes[r]), F=int(table["F"][r]), O=int(table["O"][r]), k_cap=int(table["k_cap"][r]))
            for r in rows]


def _rescued_rows(got, exp, corr_abs):
    """Rows of the valid table a knife-edge mask of compare() took out of a comparison that would have failed."""
    v = exp["valid"].astype(bool)
    rows = np.flatnonzero(v)
    bad = set()
    for r in rows:
        one = {k: a[r:r + 1] for k, a in got.items()}, {k: a[r:r + 1] for k, a in exp.items()}
        compare(*one, PPM_ABS_TOL_ORACLE, corr_abs=corr_abs)
        if any(compare.last_masked["rescued"].values()):
            bad.add(int(r))
    return sorted(bad)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_class_matches_the_oracle(ctx, oracle_lib, sweeps, monkeypatch, name, capsys):
    t0 = time.perf_counter()
    case, soa, batch = sweeps[CONFIGS[name][0]]
    cfg = config_of(name)
    # experimental_xic = False: the K x K contraction runs on MFMA in another summation order than the oracle's;
    # correlations near zero get the absolute floor of test_randomized_shapes_and_settings
    corr_abs = 0.0 if cfg.experimental_xic else 2e-6
    exp = oracle_tables(oracle_lib, sweeps, name)
    table = bs.shape_table(case, soa, cfg)
    classes = bs.classes_of(case, soa, cfg)
    want = bs.histogram(classes)
    _staged(ctx, case)

    # routing: the plan's counts are the restated rule's, and every class of this configuration ran
    ctx.plan_class_counts(reset=True)
    got = score_batches(ctx, soa, batch, cfg)
    counts = ctx.plan_class_counts(reset=True)
    with capsys.disabled():
        print(f"\n[kernel classes] {name}: {len(batch)} candidates, {int(exp['valid'].sum())} valid, class histogram {counts.tolist()}")
    assert np.array_equal(counts, want), (counts.tolist(), want.tolist())
    assert set(np.flatnonzero(counts)) == REACHES[name], sorted(set(np.flatnonzero(counts)) ^ REACHES[name])
    assert ctx.plan_class_counts().sum() == 0

    # the default path against the oracle; no row may need a knife-edge mask
    compare(got, exp, PPM_ABS_TOL_ORACLE, rel_tol=REL_TOL, corr_abs=corr_abs)
    masked = compare.last_masked
    assert np.array_equal(got["stat_matched_peaks"], exp["stat_matched_peaks"])
    if any(n > RESCUED_BOUND * masked["rows"] for n in masked["rescued"].values()):
        pytest.fail(f"knife-edge masks rescued {masked['rescued']}: {_name_rows(_rescued_rows(got, exp, corr_abs), classes, table)}")

    # kernel families: the two-kernel path (for both observation counts, for two only) and the generic kernel in place
    # of the wide ones are bit-equal to the default path
    for switch in ("ADH_DEBUG_NO_FUSED", "ADH_DEBUG_NO_FUSED2", "ADH_DEBUG_NO_WIDE"):
        with monkeypatch.context() as mp:
            mp.setenv(switch, "1")
            other = score_batches(ctx, soa, batch, cfg)
            other_counts = ctx.plan_class_counts(reset=True)
        key = {"ADH_DEBUG_NO_FUSED": "no_fused", "ADH_DEBUG_NO_FUSED2": "no_fused2", "ADH_DEBUG_NO_WIDE": "no_wide"}[switch]
        assert np.array_equal(other_counts, bs.histogram(bs.classes_of(case, soa, cfg, **{key: True}))), switch
        _same(other, got, switch)
    # ... and the generic kernel alone equals the oracle
    with monkeypatch.context() as mp:
        mp.setenv("ADH_DEBUG_NO_FAST", "1")
        generic = score_batches(ctx, soa, batch, cfg)
        generic_counts = ctx.plan_class_counts(reset=True)
    assert generic_counts[bs.CLASS_GENERIC] == len(batch) == generic_counts.sum()
    compare(generic, exp, PPM_ABS_TOL_ORACLE, rel_tol=REL_TOL, corr_abs=corr_abs)
    assert np.array_equal(generic["stat_matched_peaks"], exp["stat_matched_peaks"])
    v = exp["valid"].astype(bool)
    worst = max(float(H.rel_err(generic[k][v], got[k][v]).max()) for k in
                ("features", "fragment_mz_observed", "fragment_height", "fragment_intensity", "fragment_correlation"))

    # several chunks (ADH_CHUNK=256; the library's floor is 1024 rows a chunk, so every batch is scored in as many
    # copies as make three chunks at least): the same counts per copy, the same tables
    with monkeypatch.context() as mp:
        mp.setenv("ADH_CHUNK", "256")
        chunked, chunks, copies = score_batches(ctx, soa, batch, cfg, tile_to=3 * 1024 + 1)
        chunk_counts = ctx.plan_class_counts(reset=True)
    assert min(chunks) >= 3, chunks
    per_batch = [bs.histogram(classes[batch == b]) * c for b, c in zip(np.unique(batch), copies)]
    assert np.array_equal(chunk_counts, np.sum(per_batch, axis=0))
    _same(chunked, got, "ADH_CHUNK=256")
    with capsys.disabled():
        print(f"[kernel classes] {name}: generic kernel vs default path, worst relative difference {worst:.3g}; "
              f"{time.perf_counter() - t0:.2f} s")


def _compact_equals_padded(comp: dict, tab: dict):
    keep = np.flatnonzero(tab["valid"].astype(bool))
    assert comp["row"].dtype == np.uint32 and np.array_equal(comp["row"], keep)
    assert np.array_equal(comp["precursor_idx"], tab["precursor_idx"][keep])
    assert np.array_equal(comp["rank"], tab["rank"][keep])
    assert comp["features"].shape == (_abi.NUM_FEATURES, len(keep))
    assert comp["features"].tobytes() == np.ascontiguousarray(tab["features"][keep].T).tobytes()
    filled = tab["fragment_mz_library"][keep] > 0  # (output.py:89-97)
    assert np.array_equal(comp["fragment_row"], np.repeat(keep, filled.sum(axis=1)))
    for field, dt in _abi.COMPACT_SLOT_FIELDS:
        if field != "fragment_row":
            assert comp[field].dtype == dt and comp[field].tobytes() == tab[field][keep][filled].tobytes(), field
    return filled.sum(axis=1)


@pytest.mark.parametrize("name", ["defaults", "all_fragments"])
def test_compact_and_resident_entry_points_equal_the_padded_tables(ctx, sweeps, name):
    """``adh_score_candidates_compact`` and ``adh_score_candidates_resident`` + ``adh_take_rows`` of all rows on the
    sweep: byte for byte the valid rows and filled slots of the padded tables - rows of 62 ... 64 and of 65 and more
    filled slots included."""
    case, soa, batch = sweeps[CONFIGS[name][0]]
    cfg = config_of(name)
    _staged(ctx, case)
    seen = []
    for b in np.unique(batch):
        idx = np.flatnonzero(batch == b)
        m = pack_assembled(_rows(soa, idx))
        tab = {k: np.array(v, copy=True) for k, v in ctx.score_host(m, cfg.to_jitclass(), with_stats=True).items()}
        ctx.plan_class_counts(reset=True)
        comp = ctx.score_host_compact(m, cfg.to_jitclass())
        counts_compact = ctx.plan_class_counts(reset=True)
        seen.append(_compact_equals_padded(comp, tab))
        ctx.score_resident(m, cfg.to_jitclass())
        counts_resident = ctx.plan_class_counts(reset=True)
        _compact_equals_padded(ctx.take_rows(np.arange(len(idx))), tab)
        want = bs.histogram(bs.classes_of(case, _rows(soa, idx), cfg))
        assert np.array_equal(counts_compact, want) and np.array_equal(counts_resident, want)
    slots = np.concatenate(seen)
    if name == "all_fragments":
        assert {62, 63, 64}.issubset(set(slots.tolist())) and (slots >= 65).sum() >= 10 and slots.max() >= 150
    else:
        assert slots.max() == 12
