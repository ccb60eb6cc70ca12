"""The match-between-runs library on the GPU (alphadia_amd/mbr_library.py, adh_mbr_*): the public classes against the
goldens of the reference and against the host restatements.  Every comparison is exact: the median is a selection plus
at most one add and halve, everything else is integer."""

from __future__ import annotations

import numpy as np
import pytest

import mbr_library_golden as G
from alphadia_amd import mbr_library as M

pytestmark = pytest.mark.gpu


def _builder(meta, **kw):
    if meta["keep_decoys"]:
        kw.update(decoy_generator=G.standin_decoy_generator, rehash=G.standin_rehash)
    return M.HipMbrLibraryBuilder(fdr=meta["fdr"], keep_decoys=meta["keep_decoys"], **kw)


@pytest.mark.parametrize("gather", ["device", "host"])
@pytest.mark.parametrize("case", G.cases("forward"))
def test_device_build_equals_reference(case, gather):
    g = G.load(case)
    before = g["library"]._precursor_df.copy()
    builder = _builder(g["meta"], gather=gather)
    if g["raises"]:
        with pytest.raises(ValueError) as e:
            builder(g["psm"], g["library"])
        assert type(e.value).__name__ == g["raises"]
    else:
        got = builder(g["psm"], g["library"])
        G.assert_libraries_identical(got, g["out"])
        G.assert_frames_identical(g["library"]._precursor_df, before)  # base_library is not modified
        assert M.last_timing["n_passed"] == g["meta"]["n_passed"] and M.last_timing["n_kept"] > 0
        assert M.last_timing["h2d_bytes"] > 0 and M.last_timing["d2h_bytes"] > 0
    builder.close()


@pytest.mark.parametrize("case", G.cases("index"))
def test_device_index_builder_equals_reference(case):
    g = G.load(case)
    keys = [g[k] for k in ("target_keys", "target_fallback_keys", "fallback_lookup_keys", "specific_lookup_keys")]
    if g["raises"]:
        with pytest.raises(ValueError) as e:
            M.HipIndexBuilder(*keys)
        assert type(e.value).__name__ == g["raises"]
        return
    b = M.HipIndexBuilder(*keys)
    for name, got in (("fallback", b._fallback_indices), ("mask", b._specific_index_mask), ("specific", b._specific_indices)):
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    applied = b.apply(g["fallback_values"], g["specific_values"])
    assert applied.dtype == g["applied"].dtype and np.array_equal(applied, g["applied"])
    words = np.array([f"w{k}" for k in range(len(g["fallback_values"]))], dtype=object)
    other = np.array([f"s{k}" for k in range(len(g["specific_values"]))], dtype=object)
    assert [x[0] == "s" for x in b.apply(words, other)] == list(g["mask"])


def test_device_index_builder_refuses_a_missing_fallback_key():
    with pytest.raises(ValueError, match="fallback key"):
        M.HipIndexBuilder(np.array([1, 2]), np.array([10, 11]), np.array([10]), np.array([1]))


def _sweep(seed, n_groups, mean_rows, n_columns):
    rng = np.random.default_rng(seed)
    rows = rng.poisson(mean_rows / 0.6, n_groups) * (rng.random(n_groups) < 0.6)  # four groups in ten are never seen
    return G.cohort(rng, n_groups, rows, n_columns=n_columns, max_block=12)


def test_seeded_sweep_equals_host_and_a_smaller_repeat_call_reads_no_stale_rows():
    """About 5 000 library precursors and 30 000 PSM rows (several tiles of the sort, several blocks of the scans),
    then a smaller input with other dtypes and an odd column count on the same handle: the parked tables and matrices
    of the first call are longer than the second call's."""
    psm, lib = _sweep(7, 2500, 12, 8)
    assert 4500 < len(lib._precursor_df) < 5500 and 28_000 < len(psm) < 32_000
    builder = M.HipMbrLibraryBuilder()
    got = builder(psm, lib)
    first = dict(M.last_timing)
    G.assert_libraries_identical(got, M.host_build_mbr_library(psm, lib))
    assert 2000 < first["n_kept"] < 4000
    rng = np.random.default_rng(8)
    psm2, lib2 = G.cohort(rng, 90, rng.poisson(6, 90), n_columns=3, rt_dtype=np.float64, group_dtype=np.int64,
                          library_group_dtype=np.uint32)
    got = builder(psm2, lib2)
    assert 0 < M.last_timing["n_kept"] < first["n_kept"] // 10
    G.assert_libraries_identical(got, M.host_build_mbr_library(psm2, lib2))
    G.assert_libraries_identical(builder(psm, lib), M.host_build_mbr_library(psm, lib))  # and back up again
    builder.close()


def test_device_tables_equal_host_aggregate():
    """The two aggregate tables and the passed groups as the device leaves them, not only what reaches the library."""
    from alphadia_amd import runtime

    psm_df, _ = _sweep(9, 300, 10, 4)
    psm = M._psm_parts(psm_df, False)
    exp = M.host_aggregate(psm, 0.01, False)
    s = runtime.get_context().mbr_library()
    n_passed, n_group, n_hash, n_groups = s.aggregate(psm["qval"], psm["decoy"], psm["eg"], psm["hash"], psm["rt"],
                                                      psm["pg_notnull"], 0.01, False)
    assert (n_passed, n_group, n_hash, n_groups) == (exp["n_passed"], len(exp["by_group"][0]), len(exp["by_hash"][0]),
                                                     len(exp["groups"]))
    for which, name in ((0, "by_group"), (1, "by_hash")):
        keys, med, first = s.table(which)
        assert keys.dtype == exp[name][0].dtype and np.array_equal(keys, exp[name][0])
        assert med.dtype == exp[name][1].dtype and np.array_equal(med.view(np.uint32), exp[name][1].view(np.uint32))
        assert np.array_equal(first, exp[name][2])
    assert np.array_equal(s.groups(), exp["groups"])
    s.close()


def test_notnull_objects_equals_pandas():
    from alphadia_amd import runtime
    import pandas as pd

    pg = np.array(["a", None, "b;c", np.nan, float("nan"), pd.NA, 3, "", None], dtype=object)
    got = runtime.notnull_objects(pg)
    assert got.dtype == np.bool_ and np.array_equal(got, pd.notna(pg))
    assert np.array_equal(runtime.notnull_objects(pg[:0]), np.zeros(0, bool))
    assert np.array_equal(runtime.notnull_objects(pg[::2]), pd.notna(pg[::2]))  # not contiguous: pandas
