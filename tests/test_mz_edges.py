"""CPU: m/z window matching at tolerance, bin, exponent and run-range edges (tests/mz_edges.py).  The reference's
``get_dense`` on the designed runs (tests/golden/get_dense_mz_edges.npz) takes exactly the peaks the builder says it
must, and the oracle equals the reference bit for bit on both planes - which is what makes the GPU leg
(tests/test_mz_edges_gpu.py) meaningful."""

import numpy as np
import pytest

import helpers as H
import mz_edges as E

ALPHARAW_RUNS = list(E.RUNS)
TIMS_COLS = ["cycle", "dia_precursor_cycle", "rt_values", "mobility_values", "mz_values", "tof_indptr", "push_indices", "intensity_values"]


@pytest.fixture(scope="module")
def golden():
    return np.load(H.golden_path("get_dense_mz_edges.npz"))


_BUILT = {}


def built(run):
    """The builder's run and cases, made once per process (the GPU tests share them)."""
    if run not in _BUILT:
        _BUILT[run] = E.build_timstof(0) if run == "tims" else E.build_alpharaw(0, run)
    return _BUILT[run]


def reference_plane(z, run, case):
    """The intensity plane of the reference's output in the layout of ``case.expected``."""
    e = z[f"{run}_{case.name}_dense"]
    return e[0] if run == "tims" else e[0, :, 0, 0, :]


@pytest.mark.parametrize("run", ALPHARAW_RUNS + ["tims"])
def test_builder_draws_the_committed_runs(golden, run):
    """The fixture holds the runs and queries the builder makes today: a change of the builder without a new fixture
    (or the other way round) shows here."""
    dia, cases = built(run)
    if run == "tims":
        for c in TIMS_COLS:
            got = getattr(dia, c)
            assert got.dtype == golden["tims_" + c].dtype and np.array_equal(got, golden["tims_" + c]), c
    else:
        for key, got in (("dia_cycle", dia.cycle), ("dia_rt_values", dia.rt_values), ("dia_peak_start", dia.peak_start_idx_list),
                         ("dia_peak_stop", dia.peak_stop_idx_list), ("dia_mz", dia.mz_values), ("dia_intensity", dia.intensity_values)):
            assert got.dtype == golden[f"{run}_{key}"].dtype and np.array_equal(got, golden[f"{run}_{key}"]), key
    assert [c.name for c in cases] == golden[f"{run}_cases"].tolist()
    for c in cases:
        q = f"{run}_{c.name}_"
        assert np.array_equal(c.mz_query, golden[q + "mz"]) and c.tol == golden[q + "tol"] and np.array_equal(c.quad, golden[q + "quad"])
        assert np.array_equal(c.frame_limits, golden[q + "frame_limits"])
        if run == "tims":
            assert np.array_equal(c.scan_limits, golden[q + "scan_limits"])


@pytest.mark.parametrize("run", ALPHARAW_RUNS + ["tims"])
def test_reference_takes_the_peaks_the_builder_states(golden, run):
    """Per case: the membership decoded from the reference's intensity plane is the builder's expectation (which comes
    from the builder's own restatement of the loop, not from the reference's output)."""
    _, cases = built(run)
    wrong = []
    for c in cases:
        if c.expected is None:
            continue
        plane = reference_plane(golden, run, c)
        assert plane.shape == c.expected.shape, c.name
        if not np.array_equal(plane, c.expected):
            wrong.append(E.describe_difference(c, plane))
    assert not wrong, "\n".join(wrong)


def test_edge_families_are_all_there(capsys):
    """What the fixture is for, in numbers: cases and designed peaks inside / outside a window per edge family."""
    cases = [c for run in ALPHARAW_RUNS for c in built(run)[1]]
    counts = E.family_counts(cases)
    counts.update(E.family_counts(built("tims")[1]))
    with capsys.disabled():
        for fam in sorted(counts):
            n, i, o = counts[fam]
            print(f"\n  m/z edges {fam}: {n} cases, {i} designed peaks inside / {o} outside", end="")
        print()
    assert sorted(counts) == ["E1", "E2", "E3", "E4", "E5", "E6", "E7", "E8", "T"]
    for fam, (n, i, o) in counts.items():
        assert n >= 2 and i >= 4 and (o >= 4 or fam == "E7"), (fam, n, i, o)
    names = {c.name for c in cases}
    for must in ("E2_non_ascending_ms2", "E3_three_bins_one_cell_ms2", "E4_hi_is_512_ms1", "E5_lo_is_mz_min_ms2", "E5_one_bin_all_ms2",
                 "E5_wide_mz_max_inside_ms1", "E7_intensities_ms2", "E8_cycles_5_7_ms1"):
        assert must in names, must
    # the cells of E7 really reach both branches of the running mean and the intensity cut
    e7 = next(c for c in cases if c.name == "E7_intensities_ms2")
    v = np.asarray(e7.intensity, dtype=np.float32)
    assert (v == 0).any() and ((v > 0) & (v < 1e-38)).any() and ((v > 1e-26) & (v < 1e-20)).any() and (v == 2.0 ** 24).any()


@pytest.mark.parametrize("run", ALPHARAW_RUNS)
def test_oracle_get_dense_matches_reference_on_edges(oracle_lib, golden, run):
    """The standard of test_get_dense_matches_reference: observation list and both planes bit for bit, every case
    (the non-ascending query list included: the oracle restates the loop, which never steps back)."""
    dia, cases = built(run)
    wrong = []
    for c in cases:
        q = f"{run}_{c.name}_"
        fl = c.frame_limits
        dense, pidx = oracle_lib.get_dense(dia, fl[0, 0], fl[0, 1], c.mz_query, c.tol, c.quad[0, 0], c.quad[0, 1], True)
        e = golden[q + "dense"]
        assert dense.shape == e.shape and np.array_equal(pidx, golden[q + "pidx"]), c.name
        if not np.array_equal(dense[0], e[0]):
            wrong.append(E.describe_difference(c, dense[0, :, 0, 0, :]) or f"case {c.name}: intensity plane differs")
        elif not np.array_equal(dense[1], e[1]):
            at = tuple(np.argwhere(dense[1] != e[1])[0])
            wrong.append(f"case {c.name}: m/z plane differs at {at}: {dense[1][at]!r} != {e[1][at]!r}")
    assert not wrong, "\n".join(wrong)


def test_oracle_get_dense_timstof_matches_reference_on_edges(oracle_lib, golden):
    dia, cases = built("tims")
    wrong = []
    for c in cases:
        q = f"tims_{c.name}_"
        fl, sl = c.frame_limits, c.scan_limits
        dense, pidx = oracle_lib.get_dense_timstof(dia, fl[0, 0], fl[0, 1], sl[0, 0], sl[0, 1], c.mz_query, c.tol, c.quad[0, 0], c.quad[0, 1])
        e = golden[q + "dense"]
        assert dense.shape == e.shape and np.array_equal(pidx, golden[q + "pidx"]), c.name
        if not np.array_equal(dense[0], e[0]):
            wrong.append(E.describe_difference(c, dense[0]) or f"case {c.name}: intensity plane differs")
        elif not np.array_equal(dense[1], e[1]):
            wrong.append(f"case {c.name}: m/z plane differs")
    assert not wrong, "\n".join(wrong)


def test_predicate_is_sensitive_to_one_ulp():
    """The builder's checks are not vacuous: moving one bound of the restated loop by one ulp changes what it takes
    from a designed spectrum, for lo and for hi."""
    dia, cases = built("main")
    c = next(x for x in cases if x.name == "E1_bounds_ms2")
    lo, hi = E.bounds(c.mz_query, c.tol)
    sp = int(c.frame_limits[0, 0]) // dia.cycle_len * dia.cycle_len + E.MS2_ROW
    a, b = dia.peak_start_idx_list[sp], dia.peak_stop_idx_list[sp]
    mz = dia.mz_values[a:b]
    base = E.take(mz, lo, hi)[0]
    assert base[1] - base[0] == 4
    assert E.take(mz, [E.up(lo[0])], hi)[0][1] - E.take(mz, [E.up(lo[0])], hi)[0][0] == 3
    assert E.take(mz, [E.down(lo[0])], hi)[0][1] - E.take(mz, [E.down(lo[0])], hi)[0][0] == 5
    assert E.take(mz, lo, [E.down(hi[0])])[0][1] - base[0] == 3 and E.take(mz, lo, [E.up(hi[0])])[0][1] - base[0] == 5


def select_on_edges(select, flip=False):
    """Candidate selection on the selection run of the builder: ``select(dia, fragment columns, packed precursors,
    config, kernel)`` is the oracle's or the device's; returns the table and what produced it."""
    import selection_limits as SL
    import test_selection as TS
    from alphadia_amd.scoring import fragment_columns
    from alphadia_amd.selection import gaussian_kernel

    case = E.selection_case(0, flip)
    cfg = SL.config(rt_tolerance=30.0, candidate_count=3, min_size_rt=3)
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    pm = TS._pack(case.library.precursor_df)
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    return select(case.dia, cols, pm, cfg, kern), case


def test_selection_score_moves_when_one_edge_peak_changes_sides(oracle_lib):
    """The selection leg is sensitive: every precursor of the selection run gets its candidate on its apex, and with the
    one peak below lo of one fragment window standing on lo instead, the oracle's top-1 score of that precursor - and of
    no other - changes by far more than the 1e-6 relative of the suite's comparison for selection."""
    tables = []
    for flip in (False, True):
        exp, case = select_on_edges(lambda dia, cols, pm, cfg, kern: oracle_lib.select(dia, cols, pm, cfg, kern, n_threads=4), flip)
        top = {k: np.asarray(v).reshape(E.SELECT_PRECURSORS, 3)[:, 0] for k, v in exp.items()}
        assert (top["score"] > 0).all() and np.array_equal(top["frame_center"], case.apex_cycle * case.dia.cycle_len)
        tables.append(top["score"].astype(np.float64))
    rel = np.abs(tables[1] - tables[0]) / tables[0]
    assert rel[0] > 1e-3 and (rel[1:] == 0).all(), rel


def select_on_timstof_edges(select, flip=False):
    """``select_on_edges`` for the ion-mobility selection run."""
    import selection_limits as SL
    import test_selection as TS
    from alphadia_amd.scoring import fragment_columns

    case = E.selection_case_timstof(0, flip)
    cfg = SL.config(candidate_count=3, top_k_precursors=3,
                    **dict(SL.IM_CFG, precursor_mz_tolerance=E.TS_PRECURSOR_TOL, fragment_mz_tolerance=E.TS_FRAGMENT_TOL))
    kern = SL.im_kernel(case.dia, cfg)
    pdf = case.library.precursor_df
    assert SL.tims_tiles(case.dia, pdf, cfg, kern.shape)[4].all()
    return select(case.dia, fragment_columns(case.library.fragment_df, "mz_library"), TS._pack(pdf), cfg, kern), case


def test_timstof_selection_score_moves_when_one_edge_bin_changes_sides(oracle_lib):
    """The same for the ion-mobility run: every precursor's candidate sits on its apex frame and scan, and with the
    events one float64 step below lo of one fragment window counted into the bin on lo, the top-1 score of that
    precursor alone moves by far more than the 1e-6 relative of the comparison."""
    tables = []
    for flip in (False, True):
        exp, case = select_on_timstof_edges(lambda dia, cols, pm, cfg, kern: oracle_lib.select_timstof(dia, cols, pm, cfg, kern, n_threads=4), flip)
        top = {k: np.asarray(v).reshape(len(E.TS_PRECURSORS), 3)[:, 0] for k, v in exp.items()}
        assert (top["score"] > 0).all()
        assert np.array_equal(top["frame_center"], [1 + c * case.dia.cycle_len for _, c, _ in E.TS_PRECURSORS])
        assert np.array_equal(top["scan_center"], [s for _, _, s in E.TS_PRECURSORS])
        tables.append(top["score"].astype(np.float64))
    rel = np.abs(tables[1] - tables[0]) / tables[0]
    assert rel[0] > 1e-3 and (rel[1:] == 0).all(), rel
