"""Label-free quantification on the device (alphadia_amd.lfq.direct_lfq, alphadia_amd/csrc/adh_lfq.hip) against the
NumPy restatement ``host_direct_lfq`` - to which alone it is pinned; ``directlfq`` is not at hand.

Exact: the kept groups, their order and the zero pattern.  Non-zero cells: ``|log2 got - log2 want| <= 1e-9``.  Each
log2 is within an ulp (< 2^-47 at these magnitudes), a total shift is a chain of at most 50 medians of differences
plus weighted means, the scale a sum of at most 2 * 10^4 terms: about 1e-11 together.  The bound leaves two orders of
margin and sits seven orders below what a wrong merge moves with the 0.05 log2 noise of the data.  The condition on
the inputs (lfq_cases.margins_hold: every merge's best variance clear of the runner-up) is no tolerance; seeds are
picked for it and no case is skipped.

Shapes: 1, 2, 5 and 65 runs (65: past one wavefront's lanes); groups of 1, 2, 3, 16, 17, 65 and 300 ions in one
frame whose rows are not sorted by group (16 | 17: wavefront | workgroup route; 65 and 300: the linear path at
q = 50, everything above 4 at q = 4); min_nonan 1 and 3; sample normalisation on and off.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

import lfq_cases as cases
from alphadia_amd import lfq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9
WORST = {"max_abs_log2_difference": 0.0, "cells": 0, "cases": 0}


def assert_same(got, want, exact: bool = False):
    assert list(got.columns) == list(want.columns)
    assert got.dtypes.equals(want.dtypes)
    assert list(got.iloc[:, 0]) == list(want.iloc[:, 0])  # kept groups and their order
    a, b = got.iloc[:, 1:].to_numpy(), want.iloc[:, 1:].to_numpy()
    if exact:
        assert a.tobytes() == b.tobytes()
        return
    assert np.array_equal(a == 0, b == 0)
    assert np.isfinite(a).all()
    nz = b != 0
    err = float(np.abs(np.log2(a[nz]) - np.log2(b[nz])).max()) if nz.any() else 0.0
    print(f"max |log2 got - log2 want| = {err:.3e} over {int(nz.sum())} cells")
    WORST["max_abs_log2_difference"] = max(WORST["max_abs_log2_difference"], err)
    WORST["cells"] += int(nz.sum())
    WORST["cases"] += 1
    assert err <= BOUND


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("min_nonan", [1, 3])
@pytest.mark.parametrize("q", [4, 50])
@pytest.mark.parametrize("R", [1, 2, 5, 65])
def test_device_equals_the_restatement(R, q, min_nonan, normalize):
    df, want = cases.corner_case(R, q, min_nonan, normalize)
    got = lfq.direct_lfq(df, "pg", min_nonan=min_nonan, num_samples_quadratic=q, normalize=normalize)
    if min_nonan == 1:  # the corner groups are reported: no common run, one common run, a zero row between two ions
        assert len(want) >= len(cases.GROUP_SIZES) + (R >= 2) + (R >= 3) + 1
    assert_same(got, want)


def test_integer_group_keys_keep_their_dtype():
    vals, grp = cases.cohort_values((3, 1, 5), 5, seed=7)
    df = cases.frame(vals, (grp.astype(np.uint64) + np.uint64(2**63)), level="mod_seq_charge_hash")
    trace = []
    want = lfq.host_direct_lfq(df, "mod_seq_charge_hash", 1, 50, True, trace=trace)
    assert cases.margins_hold(trace) and want["mod_seq_charge_hash"].dtype == np.uint64
    assert_same(lfq.direct_lfq(df, "mod_seq_charge_hash", min_nonan=1), want)


def test_scratch_route_and_repeated_calls_give_the_same_bits(monkeypatch):
    df, want = cases.corner_case(5, 50, 1, True)
    first = lfq.direct_lfq(df, "pg", min_nonan=1, num_samples_quadratic=50, normalize=True)
    again = lfq.direct_lfq(df, "pg", min_nonan=1, num_samples_quadratic=50, normalize=True)
    assert_same(again, first, exact=True)
    monkeypatch.setenv("ADH_DEBUG_LFQ_ROUTE", "scratch")  # every group from a global slab instead of LDS
    slab = lfq.direct_lfq(df, "pg", min_nonan=1, num_samples_quadratic=50, normalize=True)
    assert_same(slab, first, exact=True)
    assert_same(slab, want)


def test_resident_frame_equals_uploaded_frame():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from bench_quant import cohort
    finally:
        sys.path.pop(0)
    from alphadia_amd import quant as Q

    psm, runs = cohort(5, n_prec=240, n_frag=7, seed=4)
    acc = Q.HipFragmentQuantLoader(psm).accumulate(iter(runs))
    for level in ("mod_seq_charge_hash", "pg"):
        fi, _ = Q.filter_frag_df(acc["intensity"], acc["correlation"], min_correlation=0.5, top_n=3, group_column=level)
        assert lfq._filtered(fi, lfq.run_columns(fi)) is not None and 0 < len(fi) < len(acc["intensity"])
        resident = lfq.direct_lfq(fi, level, min_nonan=2)
        copy = fi.copy()
        assert lfq._filtered(copy, lfq.run_columns(copy)) is None
        uploaded = lfq.direct_lfq(copy, level, min_nonan=2)
        assert len(resident) > 10
        assert_same(uploaded, resident, exact=True)
    trace = []
    want = lfq.host_direct_lfq(fi, "pg", 2, 50, True, trace=trace)
    assert cases.margins_hold(trace)
    assert_same(resident, want)


def test_parity_record():
    """Writes the largest difference the cases above saw where ADH_LFQ_PARITY_OUT names a file (the record under
    profiles/ comes from such a run)."""
    assert WORST["max_abs_log2_difference"] <= BOUND
    out = os.environ.get("ADH_LFQ_PARITY_OUT")
    if out and WORST["cases"]:
        with open(out, "w") as f:
            json.dump(dict(bound=BOUND, reference="alphadia_amd.lfq.host_direct_lfq (this repository's restatement)",
                           **WORST), f, indent=1)
