"""Synthetic intensity frames for the label-free quantification tests (tests/test_lfq.py, tests/test_lfq_gpu.py):
``precursor_idx, ion, <runs...>, pg, mod_seq_hash, mod_seq_charge_hash`` as ``quant.filter_frag_df`` hands them on,
with the corner rows the contract names, and the condition on the inputs that lets a float64 device be compared
with the NumPy restatement - every merge step's best variance is clear of the runner-up."""

from __future__ import annotations

import functools

import numpy as np
import pandas as pd

from alphadia_amd import lfq

GROUP_SIZES = (1, 2, 3, 16, 17, 65, 300)
NOISE = 0.05  # log2 noise of one ion in one run


def frame(values, groups, level: str = "pg") -> pd.DataFrame:
    """An intensity frame over ``values[n][R]`` (float32) whose ``level`` column holds ``groups``."""
    values = np.asarray(values, dtype=np.float32)
    n, R = values.shape
    df = pd.DataFrame({"precursor_idx": np.arange(n, dtype=np.uint32), "ion": np.arange(n, dtype=np.int64) * 7})
    for r in range(R):
        df[f"run_{r:03d}"] = values[:, r]
    for c in ("pg", "mod_seq_hash", "mod_seq_charge_hash"):
        df[c] = np.arange(n, dtype=np.uint64)
    df[level] = groups
    return df


def cohort_values(sizes, R: int, seed: int, missing: float = 0.25):
    """Intensities of groups of ``sizes`` ions over ``R`` runs: a group profile, an ion offset, a run effect and
    NOISE in log2, ``missing`` of the cells zero.  Returns ``(values, group of every row)``."""
    rng = np.random.default_rng(seed)
    run_effect = rng.normal(0, 0.5, R)
    vals, grp = [], []
    for g, n in enumerate(sizes):
        x = 15 + rng.normal(0, 1, R)[None, :] + rng.normal(0, 2, n)[:, None] + run_effect[None, :] + rng.normal(0, NOISE, (n, R))
        v = np.exp2(x)
        v[rng.random((n, R)) < missing] = 0.0
        vals.append(v)
        grp += [g] * n
    return np.concatenate(vals).astype(np.float32), np.array(grp)


def corner_frame(R: int, seed: int) -> pd.DataFrame:
    """Every group size of GROUP_SIZES plus the corner groups, rows shuffled so that no group is contiguous:
    a pair of ions without a common run (R >= 2), a pair with exactly one (R >= 3), an all-zero row inside a group,
    a group of zeros only, and an empty run (R >= 5)."""
    vals, grp = cohort_values(GROUP_SIZES, R, seed)
    rng = np.random.default_rng(seed + 1000)
    extra, eg = [], []
    g = len(GROUP_SIZES)
    base = np.exp2(15 + rng.normal(0, 1, (8, R))).astype(np.float32)
    if R >= 2:  # no common run: the +inf stop
        a, b = base[0].copy(), base[1].copy()
        a[1::2], b[0::2] = 0, 0
        extra += [a, b]
        eg += [g, g]
        g += 1
    if R >= 3:  # one common run: variance exactly 0
        a, b = base[2].copy(), base[3].copy()
        a[2:], b[0] = 0, 0
        extra += [a, b]
        eg += [g, g]
        g += 1
    extra += [base[4], np.zeros(R, np.float32), base[5]]  # an all-zero row between two ions
    eg += [g, g, g]
    g += 1
    extra += [np.zeros(R, np.float32), np.zeros(R, np.float32)]  # a group without any value
    eg += [g, g]
    vals = np.concatenate([vals, np.array(extra, dtype=np.float32)])
    grp = np.concatenate([grp, np.array(eg)])
    if R >= 5:
        vals[:, 3] = 0  # an empty run
    order = rng.permutation(len(grp))
    names = np.array([f"PG{x:03d}" for x in grp], dtype=object)
    return frame(vals[order], names[order])


def margins_hold(trace) -> bool:
    """Every merge: runner_up - best > 1e-6 * runner_up, or both exactly 0 (single overlaps); a step without a
    finite runner-up has no competitor."""
    for best, runner in trace:
        if not np.isfinite(runner) or (best == 0.0 and runner == 0.0):
            continue
        if not runner - best > 1e-6 * runner:
            return False
    return True


@functools.lru_cache(maxsize=None)
def corner_case(R: int, q: int, min_nonan: int, normalize: bool):
    """``(frame, host result)`` of the corner frame for the first seed whose merges are all clear."""
    for seed in range(20):
        df = corner_frame(R, 100 * R + seed)
        trace = []
        want = lfq.host_direct_lfq(df, "pg", min_nonan, q, normalize, trace=trace)
        if margins_hold(trace):
            return df, want
    raise AssertionError("no seed with clear merge margins")
