"""Golden vectors of protein inference, produced by RUNNING THE REFERENCE's ``perform_grouping``
(alphadia/outputtransform/grouping.py:100-194) in the build container:

    python tests/golden/make_golden_grouping.py

TEST INFRASTRUCTURE, same rules as make_golden.py: the reference is imported from /root/reference (this module needs
only NumPy and pandas; ref_shim puts the reference on the path), fed tables built here, and inputs + outputs are
stored in ``tests/golden/grouping.npz`` - arrays only, every string column as int32 codes (-1: NaN) into a
fixed-width Unicode name table.

Per case ``<c>``:

    <c>/in/<column>                  the input table (string columns as <column>.codes / <column>.names)
    <c>/out<k>/<column>.codes/.names the id column as the call left it on the caller's frame, pg_master and pg
    <c>/meta                         JSON: input columns, the calls (id column, decoy column, group,
                                     return_parsimony_groups) and per call the result's columns, dtypes and whether
                                     its index is a RangeIndex
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402

ref_shim.install()

from alphadia.outputtransform.grouping import perform_grouping  # noqa: E402

# (group, return_parsimony_groups)
ALL_MODES = [(False, False), (True, False), (False, True)]


def _table(rows, column="proteins", **extra):
    """rows: (precursor_idx, id string, decoy)."""
    df = pd.DataFrame({"precursor_idx": np.array([r[0] for r in rows], dtype=np.int64),
                       column: np.array([r[1] for r in rows], dtype=object),
                       "decoy": np.array([r[2] for r in rows], dtype=np.int64)})
    df["score"] = np.arange(len(df), dtype=np.float32) * np.float32(0.5)  # a column of the caller's
    for k, v in extra.items():
        df[k] = v
    return df


def textbook():
    ids = ["A", "A", "B",                      # distinct
           "C", "C;D", "D",                    # differentiable
           "E;F", "E;F",                       # indistinguishable
           "G", "G;H",                         # subset
           "I", "I;J", "J;K", "K",             # subsumable
           "O;P", "O;Q", "P", "Q",             # shared only
           "R;S", "S;T", "T;R"]                # circular
    return _table([(100 + i, s, 0) for i, s in enumerate(ids)])


def ties():
    """Equal set sizes where the id that appeared first is the later one in string order."""
    ids = ["Zeta;Alpha", "Y", "B", "Y;B", "m2;m1", "m1;m2;m0", "m0;m2"]
    return _table([(i, s, 0) for i, s in enumerate(ids)])


def later_rows():
    """Later rows of a precursor_idx carry another id string; rows are not in precursor order."""
    rows = [(7, "A", 0), (3, "B;C", 0), (7, "B;C", 0), (5, "C", 0), (3, "A", 0), (9, "A;B", 0), (5, "Q", 0),
            (9, "Q", 0), (1, "C;B", 0), (7, "Q;R", 0)]
    return _table(rows)


def odd_strings():
    ids = ["A;A", "A;", "", "B;;B", np.nan, "nan;A", np.nan, "B"]
    return _table([(i, s, 0) for i, s in enumerate(ids)])


def decoys():
    """One table, several decoy columns: all 0, all 1, mixed, and a third value that leaves rows without a group."""
    ids = ["T1", "T1;T2", "T2", "T2;T3", "D1", "D1;D2", "D2", "T1;D1", "T3;D2", "T1;T3", "D2;D1", "T3"]
    n = len(ids)
    mixed = np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1], dtype=np.int64)
    third = np.array([0, 0, 2, 0, 1, 1, 2, 1, 0, 2, 1, 1], dtype=np.int64)
    df = _table([(10 * i, s, 0) for i, s in enumerate(ids)], all1=np.ones(n, dtype=np.int64), mixed=mixed, third=third)
    return pd.concat([df, df.iloc[[2, 6, 9]]], ignore_index=True)  # (second rows of three precursors)


def target_only_master():
    """T1 is a master among the targets only and appears in decoy rows."""
    rows = [(0, "T1", 0), (1, "T1", 0), (2, "T1;X", 0), (3, "T1;D1", 1), (4, "D1", 1), (5, "D1", 1), (6, "X;D1", 1)]
    return _table(rows)


def code_points():
    ids = ["P9", "P10", "P9;P10;a;B;P100", "a", "B", "P100", "b;B", "b"]
    return _table([(i, s, 0) for i, s in enumerate(ids)])


def shared_string():
    rows = [(i, "M1;M2", 0) for i in range(50)] + [(50, "M2", 0), (51, "M2;M3", 0), (52, "M3", 0)]
    rows += [(60 + i, "M3;M1", 1) for i in range(40)]
    return _table(rows)


def genes():
    ids = ["GA", "GA;GB", "GB", "GC;GB", "GC"]
    df = _table([(i, s, i % 2) for i, s in enumerate(ids)], column="genes")
    df["proteins"] = np.array(["PX"] * len(ids), dtype=object)
    return df


def random_small():
    """300 ids, 900 precursors, both classes, 30 % shared."""
    rng = np.random.default_rng(11)
    rows = []
    for i in range(900):
        decoy = int(rng.random() < 0.4)
        k = 1 if rng.random() > 0.3 else int(rng.integers(2, 5))
        first = int(rng.integers(0, 300))
        members = {first, *(int(x) % 300 for x in first + rng.integers(-6, 7, k - 1))}
        order = rng.permutation(sorted(members))
        rows.append((i, ";".join(f"{'D' if decoy else 'T'}{m:03d}" for m in order), decoy))
    df = _table(rows)
    return pd.concat([df, df.sample(200, random_state=3)], ignore_index=True)


def _chain_rows(decoy: int, first_idx: int):
    """1 500 ids in a path: row k holds ids k and k + 1, names permuted so that first appearance is not name order,
    and 0 - 4 rows of its own per id.  One component, diameter 3 000, ties throughout."""
    rng = np.random.default_rng(21)
    n = 1500
    name = [f"C{j:04d}" for j in rng.permutation(n)]
    rows = []
    for k in range(n):
        if k + 1 < n:
            pair = (name[k], name[k + 1]) if k % 3 else (name[k + 1], name[k])
            rows.append((first_idx + len(rows), ";".join(pair), decoy))
        for _ in range(int(rng.integers(0, 5))):
            rows.append((first_idx + len(rows), name[k], decoy))
    return rows


def _hub_rows(decoy: int, first_idx: int):
    """One id shares a row with each of 3 000 private ids, which have 0 - 2 rows of their own."""
    rng = np.random.default_rng(22)
    rows = []
    for k in range(3000):
        p = f"H{k:04d}"
        rows.append((first_idx + len(rows), f"HUB;{p}" if k % 2 else f"{p};HUB", decoy))
        for _ in range(int(rng.integers(0, 3))):
            rows.append((first_idx + len(rows), p, decoy))
    return rows


def chain():
    return _table(_chain_rows(0, 0))


def hub():
    return _table(_hub_rows(0, 0))


def wide():
    """One row with 200 ids, half of which have a row of their own."""
    rng = np.random.default_rng(23)
    names = [f"W{j:03d}" for j in rng.permutation(200)]
    rows = [(0, ";".join(names), 0)]
    rows += [(1 + j, names[j], 0) for j in range(0, 200, 2)]
    return _table(rows)


def two_class():
    rows = _chain_rows(0, 0)
    return _table(rows + _hub_rows(1, len(rows)))


def _calls(modes, column="proteins", decoy="decoy"):
    return [(column, decoy, g, p) for g, p in modes]


CASES = {
    "textbook": (textbook, _calls(ALL_MODES)),
    "ties": (ties, _calls(ALL_MODES)),
    "later_rows": (later_rows, _calls(ALL_MODES)),
    "odd_strings": (odd_strings, _calls(ALL_MODES)),
    "decoys": (decoys, [c for d in ("decoy", "all1", "mixed", "third") for c in _calls(ALL_MODES, decoy=d)]),
    "target_only_master": (target_only_master, _calls(ALL_MODES)),
    "code_points": (code_points, _calls(ALL_MODES)),
    "shared_string": (shared_string, _calls(ALL_MODES)),
    "genes": (genes, _calls(ALL_MODES, column="genes")),
    "random_small": (random_small, _calls(ALL_MODES)),
    "chain": (chain, _calls([(False, True), (True, False)])),
    "hub": (hub, _calls([(False, True), (True, False)])),
    "wide": (wide, _calls([(False, True), (True, False)])),
    "two_class": (two_class, _calls([(True, False), (False, True)])),
}


def _put(out, key, values):
    """A column: numeric as it is, strings as codes into a name table (-1: a missing value)."""
    v = np.asarray(values)
    if v.dtype != object:
        out[key] = v
        return
    missing = np.array([not isinstance(x, str) for x in v], dtype=bool)
    assert all(isinstance(x, float) and np.isnan(x) for x in v[missing])
    names, codes = np.unique(v[~missing].astype(str), return_inverse=True) if (~missing).any() else (np.zeros(0, "U1"), [])
    full = np.full(len(v), -1, dtype=np.int32)
    full[~missing] = codes
    out[key + ".codes"] = full
    out[key + ".names"] = names if len(names) else np.zeros(0, dtype="U1")


def run_case(name, spec, out, summary):
    make, calls = spec
    table = make()
    for c in table.columns:
        _put(out, f"{name}/in/{c}", table[c].to_numpy())
    meta = dict(columns=list(table.columns), calls=[list(c) for c in calls], results=[])
    for k, (column, decoy, group, parsimony) in enumerate(calls):
        df = table.copy()
        res = perform_grouping(df, genes_or_proteins=column, decoy_column=decoy, group=group,
                               return_parsimony_groups=parsimony)
        assert list(res.columns) == [*table.columns, "pg_master", "pg"]
        for c in table.columns:  # the call changes nothing on the caller's frame but the id column
            if c != column:
                assert res[c].equals(table[c]) and df[c].equals(table[c]), (name, c)
        assert res[column].equals(df[column])
        for c in (column, "pg_master", "pg"):
            _put(out, f"{name}/out{k}/{c}", res[c].to_numpy())
        meta["results"].append(dict(columns=list(res.columns), dtypes=[str(t) for t in res.dtypes],
                                    index_is_range=bool(res.index.equals(pd.RangeIndex(len(res))))))
    out[f"{name}/meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    summary[name] = (len(table), len(calls))


def main():
    out: dict[str, np.ndarray] = {}
    summary = {}
    for name, spec in CASES.items():
        run_case(name, spec, out, summary)
    path = os.path.join(OUT_DIR, "grouping.npz")
    np.savez_compressed(path, **out)
    print(path, summary, f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
