"""Protein inference on the GPU (alphadia_amd/grouping.py, csrc/adh_grouping.hip): every golden call equals the
reference's frame exactly; many small components, a component whose set sizes live in global memory and a seeded
cohort of both classes against the host restatement; repeated runs of one table; the stage times and the input
checks of the C ABI.  Every comparison is equality."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import grouping_golden as G

pytestmark = pytest.mark.gpu

MODES = [dict(group=True), dict(group=False, return_parsimony_groups=True)]


def _same_as_host(df: pd.DataFrame, **kwargs) -> pd.DataFrame:
    from alphadia_amd import grouping as PG

    exp = PG.host_perform_grouping(df.copy(), **kwargs)
    got = PG.perform_grouping(df.copy(), **kwargs)
    G.assert_frames_identical(got, exp)
    return got


@pytest.mark.parametrize("case,k", G.call_ids())
def test_perform_grouping_equals_reference(case, k):
    from alphadia_amd import grouping as PG

    G.check_call(PG.perform_grouping, case, k)
    if case == "chain":  # one path of 3 000 nodes: hooking with pointer jumping, not neighbour propagation
        assert PG.last_timing["components"] == 1 and PG.last_timing["large_components"] == 1
        assert PG.last_timing["label_rounds"] <= 36


@pytest.mark.parametrize("mode", MODES, ids=["heuristic", "parsimony_groups"])
def test_many_small_components(mode):
    """20 000 components of one to three ids: one wavefront each, four per block, the last block partly filled."""
    from alphadia_amd import grouping as PG

    rng = np.random.default_rng(5)
    n_comp = 20_001
    rows = []
    for c in range(n_comp):
        ids = [f"S{c:05d}_{j}" for j in rng.permutation(int(rng.integers(1, 4)))]
        if len(ids) > 1:
            rows.append(";".join(ids))
        for name in ids:
            rows.extend([name] * int(rng.integers(0 if len(ids) > 1 else 1, 3)))
    df = pd.DataFrame({"precursor_idx": rng.permutation(len(rows)), "proteins": np.array(rows, dtype=object),
                       "decoy": np.zeros(len(rows), dtype=np.int64)})
    _same_as_host(df, **mode)
    assert PG.last_timing["components"] == n_comp and PG.last_timing["large_components"] == 0


def test_component_with_set_sizes_in_global_memory():
    """9 000 ids in one component: more than the workgroup kernel keeps in LDS."""
    from alphadia_amd import grouping as PG

    df = G.giant_component(9000, seed=2)
    _same_as_host(df, group=False, return_parsimony_groups=True)
    assert PG.last_timing["components"] == 1 and PG.last_timing["large_components"] == 1


@pytest.fixture(scope="module")
def cohort():
    """20 000 ids per class, 120 000 precursors, 30 % shared, and the host restatement's result per mode."""
    from alphadia_amd import grouping as PG

    df = G.cohort(20_000, 120_000, seed=7)
    return df, [PG.host_perform_grouping(df.copy(), **mode) for mode in MODES]


@pytest.mark.parametrize("m", [0, 1], ids=["heuristic", "parsimony_groups"])
def test_cohort_of_both_classes(cohort, m):
    from alphadia_amd import grouping as PG

    df, expected = cohort
    got = PG.perform_grouping(df.copy(), **MODES[m])
    G.assert_frames_identical(got, expected[m])
    assert set(df["decoy"]) == {0, 1} and df["precursor_idx"].nunique() == 120_000
    assert PG.last_timing["ids"] > 30_000 and PG.last_timing["large_components"] > 0
    # the stage times are readable and non-negative
    times = [PG.last_timing[k] for k in ("label_ms", "cover_ms", "filter_ms")]
    assert all(isinstance(t, float) and t >= 0.0 for t in times) and times[0] > 0.0 and times[1] > 0.0
    assert (times[2] > 0.0) == MODES[m]["group"]


def test_three_runs_of_one_table_get_the_same_groups(cohort):
    """The rows repeated three times under the same precursor_idx: every copy gets the groups of the single table."""
    from alphadia_amd import grouping as PG

    df, expected = cohort
    three = pd.concat([df.assign(run=np.int32(r)) for r in range(3)], ignore_index=True)
    got = PG.perform_grouping(three, **MODES[0])
    assert len(got) == 3 * len(df) and list(got.columns) == list(expected[0].columns)
    for r in range(3):
        part = got[got["run"] == r].reset_index(drop=True)
        for c in ("precursor_idx", "proteins", "decoy", "pg_master", "pg"):
            assert np.array_equal(part[c].to_numpy(), expected[0][c].to_numpy()), (r, c)


def test_malformed_input_is_refused_before_any_launch():
    from alphadia_amd import runtime

    pg = runtime.get_context().protein_groups()
    ep, ei, w = np.array([0, 1, 1], np.int32), np.array([0, 0, 1], np.int32), np.array([2, 1], np.int32)
    master, emptied = pg.solve(ep, ei, w, 2)
    assert master.tolist() == [0, 0] and emptied.tolist() == [-1, 0]
    for bad in ((np.array([0, 1, 2], np.int32), ei, w, 2), (ep, np.array([0, 0, 2], np.int32), w, 2),
                (ep, np.array([0, -1, 1], np.int32), w, 2), (ep, ei, np.array([2, -1], np.int32), 2),
                (np.array([0, 0, 0, 0, 0], np.int32), np.array([0, 0, 0, 0, 0], np.int32), w, 2),
                (ep[:0], ei[:0], w, 2)):
        with pytest.raises(runtime.HipBackendError, match=r"adh_pg_solve failed \(-1\)"):
            pg.solve(*bad)
    master, emptied = pg.solve(ep, ei, w, 2)  # the object is still usable
    assert master.tolist() == [0, 0]
    with pytest.raises(runtime.HipBackendError, match=r"adh_pg_filter failed \(-1\)"):
        pg.filter(np.array([0, 5], np.int32), np.array([0, 1], np.int32), 2)
    off, ids = pg.filter(np.array([1, 0], np.int32), np.array([1, 0], np.int32), 2)
    assert off.tolist() == [0, 1, 2] and ids.tolist() == [0, 0]
    assert all(t >= 0.0 for t in pg.time_ms())
    pg.close()
