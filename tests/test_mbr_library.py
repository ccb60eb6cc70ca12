"""Host side of the match-between-runs library (alphadia_amd/mbr_library.py): the NumPy restatements against the goldens
of the reference, bit for bit; the C-ABI declarations of adh_mbr_*; argument validation.  No GPU needed."""

from __future__ import annotations

import os
import re

import numpy as np
import pandas as pd
import pytest

import mbr_library_golden as G
from alphadia_amd import _abi
from alphadia_amd import mbr_library as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _builder_args(meta):
    kw = dict(fdr=meta["fdr"], keep_decoys=meta["keep_decoys"])
    if meta["keep_decoys"]:
        kw.update(decoy_generator=G.standin_decoy_generator, rehash=G.standin_rehash)
    return kw


@pytest.mark.parametrize("case", G.cases("forward"))
def test_host_build_equals_reference(case):
    g = G.load(case)
    before = g["library"]._precursor_df.copy()
    if g["raises"]:
        with pytest.raises(ValueError) as e:
            M.host_build_mbr_library(g["psm"], g["library"], **_builder_args(g["meta"]))
        assert type(e.value).__name__ == g["raises"]
        return
    got = M.host_build_mbr_library(g["psm"], g["library"], **_builder_args(g["meta"]))
    G.assert_libraries_identical(got, g["out"])
    G.assert_frames_identical(g["library"]._precursor_df, before)  # base_library is not modified
    assert got.fragment_mz_df is got._fragment_mz_df
    assert M.last_timing["host_total_s"] > 0


@pytest.mark.parametrize("case", G.cases("index"))
def test_host_index_builder_equals_reference(case):
    g = G.load(case)
    keys = [g[k] for k in ("target_keys", "target_fallback_keys", "fallback_lookup_keys", "specific_lookup_keys")]
    if g["raises"]:
        with pytest.raises(ValueError) as e:
            M.host_index_builder(*keys)
        assert type(e.value).__name__ == g["raises"]
        return
    b = M.host_index_builder(*keys)
    for name, got in (("fallback", b._fallback_indices), ("mask", b._specific_index_mask), ("specific", b._specific_indices)):
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    applied = b.apply(g["fallback_values"], g["specific_values"])
    assert applied.dtype == g["applied"].dtype and np.array_equal(applied, g["applied"])
    words = np.array([f"w{k}" for k in range(len(g["fallback_values"]))], dtype=object)
    other = np.array([f"s{k}" for k in range(len(g["specific_values"]))], dtype=object)
    taken = b.apply(words, other)  # object arrays
    assert taken.dtype == object and all(isinstance(x, str) for x in taken)
    assert [x[0] == "s" for x in taken] == list(g["mask"])


def test_golden_cases_cover_the_issue():
    sizes = set(G.meta("tiles_f32")["group_sizes"])
    assert {1, 2, 3, 64, 65} <= sizes and max(sizes) >= 1100
    assert G.meta("tiles_f32")["n_passed"] > 4352  # more than a radix-sort block takes
    g = G.load("tiles_f32")
    psm, lib, out = g["psm"], g["library"]._precursor_df, g["out"]._precursor_df
    assert psm["rt_observed"].dtype == np.float32 and G.load("f64_signed")["psm"]["rt_observed"].dtype == np.float64
    assert psm["elution_group_idx"].dtype == np.uint32 and lib["elution_group_idx"].dtype == np.int64
    assert G.load("f64_signed")["psm"]["mod_seq_charge_hash"].dtype == np.int64
    assert (psm["mod_seq_charge_hash"].to_numpy() >= np.uint64(1 << 63)).any()
    assert (psm["qval"] == 0.01).any() and psm["qval"].isna().any()
    passed = psm[psm["qval"] <= 0.01]
    by_group = passed.groupby("elution_group_idx")["rt_observed"]
    assert (by_group.apply(lambda r: r.isna().all())).any()  # a whole group of NaN
    assert (by_group.apply(lambda r: r.isna().any() and not r.isna().all())).any()
    assert (by_group.apply(lambda r: r.dropna().duplicated().any())).any()  # tied RTs
    assert passed.groupby("elution_group_idx")["pg"].apply(lambda s: s.iloc[0] is None).any()
    assert not isinstance(lib.index, pd.RangeIndex) and not lib["frag_start_idx"].is_monotonic_increasing
    assert ((lib["frag_stop_idx"] - lib["frag_start_idx"]) == 0).any()
    decoy_only = passed.groupby("mod_seq_charge_hash")["decoy"].min() == 1
    assert lib["mod_seq_charge_hash"].isin(decoy_only[decoy_only].index).any()
    absent = ~out["mod_seq_charge_hash"].isin(passed["mod_seq_charge_hash"])
    assert absent.any() and out["rt"][absent].notna().any()  # the fallback path
    assert out["rt"].isna().any()
    assert G.meta("none_pass")["raises"] == "ValueError" and G.meta("index_duplicate")["raises"] == "ValueError"
    assert len(G.load("index_empty_specific")["specific_lookup_keys"]) == 0


def test_median_of_two_is_the_float64_mean_rounded_once():
    rt = np.array([1.1, 2.3, 7.0], dtype=np.float32)
    keys, med, first, _, _ = M.host_aggregate_key(np.array([4, 4, 9]), rt, np.array([False, True, True]), np.arange(3))
    assert med.dtype == np.float32 and list(keys) == [4, 9] and list(first) == [1, 2]
    assert med[0] == np.float32((float(rt[0]) + float(rt[1])) / 2) and med[1] == rt[2]


def test_missing_elution_group_is_a_value_error():
    with pytest.raises(ValueError, match="fallback key"):
        M.host_index_builder(np.array([1, 2]), np.array([10, 11]), np.array([10]), np.array([1]))


def test_argument_validation():
    g = G.load("keep_decoys")
    with pytest.raises(ValueError, match="decoy_generator"):
        M.HipMbrLibraryBuilder(keep_decoys=True)
    with pytest.raises(ValueError, match="decoy_generator"):
        M.host_build_mbr_library(g["psm"], g["library"], keep_decoys=True)
    with pytest.raises(ValueError, match="gather"):
        M.HipMbrLibraryBuilder(gather="nowhere")
    with pytest.raises(ValueError, match="lacks"):
        M.host_build_mbr_library(g["psm"].drop(columns=["pg"]), g["library"])
    lib = g["library"]
    with pytest.raises(ValueError, match="lacks"):
        M.host_build_mbr_library(g["psm"], G.Library(lib._precursor_df.drop(columns=["frag_stop_idx"]),
                                                     {n: getattr(lib, n) for n in G.DENSE}))
    with pytest.raises(TypeError, match="float32"):
        M.host_build_mbr_library(g["psm"], G.Library(lib._precursor_df, {G.DENSE[0]: lib._fragment_mz_df.astype(np.float64)}))
    with pytest.raises(TypeError, match="uint64"):
        M.host_lookup(np.array([1], np.uint64), np.array([1], np.int64))


def test_mbr_abi_declarations_agree():
    """Every adh_mbr_* entry of the prototype table (tests/test_abi.py holds it against the header) is defined in
    adh_mbr_library.hip, which adh_api.hip includes (checked without loading the library)."""
    decl = [name for name in _abi.PROTOTYPES if name.startswith("adh_mbr_")]
    assert len(decl) == 11
    csrc = open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_mbr_library.hip")).read()
    assert all(re.search(rf"\bint {name}\(", csrc) for name in decl)
    assert '#include "adh_mbr_library.hip"' in open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_api.hip")).read()
