"""Loading of tests/golden/grouping.npz (written by tests/golden/make_golden_grouping.py) for the protein inference
tests, and the seeded synthetic cohorts the GPU tests and the benchmark share."""

from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouping.npz")

_Z = None


def _z():
    global _Z
    if _Z is None:
        _Z = dict(np.load(PATH))
    return _Z


def cases() -> list[str]:
    return sorted({k.split("/")[0] for k in _z()})


def _column(z, key):
    if key in z:
        return z[key]
    codes, names = z[key + ".codes"], z[key + ".names"]
    out = np.empty(len(codes), dtype=object)
    out[:] = np.nan
    ok = codes >= 0
    out[ok] = names.astype(object)[codes[ok]]
    return out


def meta(case: str) -> dict:
    return json.loads(bytes(_z()[f"{case}/meta"]).decode())


def table(case: str) -> pd.DataFrame:
    """The input table of a case, fresh (the calls change the id column in place)."""
    z = _z()
    return pd.DataFrame({c: _column(z, f"{case}/in/{c}") for c in meta(case)["columns"]})


def calls(case: str):
    """Per call ``(kwargs, expected frame, id column)`` - the frame as the reference returned it."""
    z, m = _z(), meta(case)
    out = []
    for k, ((column, decoy, group, parsimony), res) in enumerate(zip(m["calls"], m["results"])):
        exp = table(case)
        for c in (column, "pg_master", "pg"):
            exp[c] = _column(z, f"{case}/out{k}/{c}")
        exp = exp[res["columns"]].astype({c: t for c, t in zip(res["columns"], res["dtypes"]) if t != "object"})
        assert res["index_is_range"]
        out.append((dict(genes_or_proteins=column, decoy_column=decoy, group=group, return_parsimony_groups=parsimony),
                    exp, column))
    return out


def call_ids() -> list[tuple[str, int]]:
    return [(c, k) for c in cases() for k in range(len(meta(c)["calls"]))]


def assert_frames_identical(got: pd.DataFrame, exp: pd.DataFrame) -> None:
    """Columns, column order, dtypes, the RangeIndex and every value: strings equal, NaN exactly where expected."""
    assert list(got.columns) == list(exp.columns)
    assert [str(t) for t in got.dtypes] == [str(t) for t in exp.dtypes], (list(got.dtypes), list(exp.dtypes))
    assert isinstance(got.index, pd.RangeIndex) and got.index.equals(pd.RangeIndex(len(exp)))
    for c in exp.columns:
        a, b = got[c].to_numpy(), exp[c].to_numpy()
        if a.dtype == object:
            na, nb = pd.isna(a), pd.isna(b)
            assert np.array_equal(na, nb), c
            assert all(type(x) is str for x in a[~na]), c
            assert np.array_equal(a[~na], b[~nb]), c
        elif a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c
        else:
            assert np.array_equal(a, b), c


def check_call(fn, case: str, k: int) -> None:
    """One golden call through ``fn``: the returned frame and the id column left on the caller's frame."""
    kwargs, exp, column = calls(case)[k]
    df = table(case)
    before = df.copy()
    got = fn(df, **kwargs)
    assert_frames_identical(got, exp)
    assert df[column].dtype == object and np.array_equal(df[column].to_numpy(), before[column].astype(str).to_numpy())
    for c in before.columns:
        if c != column:
            assert df[c].equals(before[c]), c


def cohort(n_ids: int, n_precursors: int, seed: int = 0, shared: float = 0.3, window: int = 40, decoys: bool = True,
           rows_per_precursor: int = 1) -> pd.DataFrame:
    """A seeded synthetic precursor table: ``n_ids`` protein ids per class, ``n_precursors`` unique precursors, a
    ``shared`` fraction of them carried by two to four ids that lie within ``window`` of each other (protein
    families), decoys as reversed twins.  ``rows_per_precursor`` repeats the table (several runs)."""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, n_ids, n_precursors)
    k = np.where(rng.random(n_precursors) < shared, rng.integers(2, 5, n_precursors), 1)
    decoy = (rng.random(n_precursors) < 0.5).astype(np.int64) if decoys else np.zeros(n_precursors, dtype=np.int64)
    name = np.array([f"P{i:06d}" for i in rng.permutation(n_ids)], dtype=object)
    rname = np.array(["REV_" + s for s in name], dtype=object)
    offs = rng.integers(-window, window + 1, (n_precursors, 3))
    ids = []
    for r in range(n_precursors):
        m = [int(first[r])]
        for j in range(int(k[r]) - 1):
            m.append(int((first[r] + offs[r, j]) % n_ids))
        table_ = rname if decoy[r] else name
        ids.append(";".join(table_[m]))
    df = pd.DataFrame({"precursor_idx": rng.permutation(n_precursors).astype(np.int64),
                       "proteins": np.array(ids, dtype=object), "decoy": decoy,
                       "run": np.zeros(n_precursors, dtype=np.int32)})
    if rows_per_precursor > 1:
        df = pd.concat([df.assign(run=np.int32(r)) for r in range(rows_per_precursor)], ignore_index=True)
    return df


def giant_component(n_ids: int, seed: int = 0) -> pd.DataFrame:
    """One component of ``n_ids`` ids: every id shares a precursor with a random earlier id (a random tree, shallow
    and bushy) and has 0 - 3 precursors of its own."""
    rng = np.random.default_rng(seed)
    name = np.array([f"G{i:06d}" for i in rng.permutation(n_ids)], dtype=object)
    rows = []
    own = rng.integers(0, 4, n_ids)
    for i in range(n_ids):
        if i:
            rows.append(f"{name[i]};{name[int(rng.integers(0, i))]}")
        rows.extend([name[i]] * int(own[i]))
    return pd.DataFrame({"precursor_idx": np.arange(len(rows), dtype=np.int64), "proteins": np.array(rows, dtype=object),
                         "decoy": np.zeros(len(rows), dtype=np.int64)})
