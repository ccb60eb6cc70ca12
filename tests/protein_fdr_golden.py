"""Loading of tests/golden/protein_fdr.npz (written by tests/golden/make_golden_protein_fdr.py) for the protein-group
FDR tests, the checks the CPU and the GPU tests share, and the seeded synthetic cohort of the GPU tests and the
benchmark."""

from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "protein_fdr.npz")
CASES = ["tiny", "ragged_f32", "ragged_f64", "even", "separable"]
ERRORS = ["one_group", "one_class"]

_Z = None


def z():
    global _Z
    if _Z is None:
        _Z = dict(np.load(PATH))
    return _Z


def _column(key):
    if key in z():
        return z()[key]
    codes, names = z()[key + ".codes"], z()[key + ".names"]
    out = np.empty(len(codes), dtype=object)
    out[:] = np.nan
    ok = codes >= 0
    out[ok] = names.astype(object)[codes[ok]]
    return out


def meta(case: str) -> dict:
    return json.loads(bytes(z()[f"{case}/meta"]).decode())


def table(case: str) -> pd.DataFrame:
    """The input table of a case, fresh."""
    m = meta(case)
    df = pd.DataFrame({c: _column(f"{case}/in/{c}") for c in m["columns"]})
    return df.astype({c: t for c, t in zip(m["columns"], m["dtypes"]) if t != "object"})


def value(case: str, key: str) -> np.ndarray:
    return z()[f"{case}/{key}"]


def tol(case: str) -> float:
    return float(z()[f"{case}/tol"])


def feature_groups(case: str):
    """``(pg names, decoy, X)`` of the reference's group feature frame."""
    return _column(f"{case}/feat/pg"), value(case, "feat/decoy"), value(case, "feat/X")


def expected_frame(case: str) -> pd.DataFrame:
    """The frame the reference returned: the input's rows out/row_id under the index out/index, and pg_qval."""
    m = meta(case)
    exp = table(case).iloc[value(case, "out/row_id")]
    exp.index = pd.Index(value(case, "out/index"))
    exp["pg_qval"] = value(case, "out/pg_qval")
    assert list(exp.columns) == m["out_columns"] and [str(t) for t in exp.dtypes] == m["out_dtypes"]
    return exp


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint8)


def assert_frames_identical(got: pd.DataFrame, exp: pd.DataFrame) -> None:
    """Columns, their order and dtypes, the (repeated) index, strings equal, NaN exactly where expected, every float
    bit for bit."""
    assert list(got.columns) == list(exp.columns)
    assert [str(t) for t in got.dtypes] == [str(t) for t in exp.dtypes], (list(got.dtypes), list(exp.dtypes))
    assert got.index.dtype == exp.index.dtype and np.array_equal(got.index.to_numpy(), exp.index.to_numpy())
    for c in exp.columns:
        a, b = got[c].to_numpy(), exp[c].to_numpy()
        if a.dtype == object:
            na, nb = pd.isna(a), pd.isna(b)
            assert np.array_equal(na, nb), c
            assert np.array_equal(a[~na], b[~nb]), c
        elif a.dtype.kind == "f":
            assert np.array_equal(np.isnan(a), np.isnan(b)), c
            assert np.array_equal(bits(a), bits(b)), c
        else:
            assert np.array_equal(a, b), c


def assert_features_equal_golden(case: str, group_pg, group_decoy, x, pg_names) -> None:
    """The group order and the feature matrix, bit for bit."""
    names, decoy, gx = feature_groups(case)
    assert np.array_equal(np.asarray(pg_names, dtype=object)[group_pg], names)
    assert np.array_equal(np.asarray(group_decoy).astype(np.int64), decoy)
    assert x.dtype == np.float64 and x.shape == gx.shape
    for k in range(gx.shape[1]):
        assert np.array_equal(bits(x[:, k]), bits(gx[:, k])), f"feature column {k}"


def assert_training_within_tol(case: str, proba, n_iter, curve, *, label="") -> None:
    """n_iter equal; loss curve and probabilities within the case's stored tol, relative.  Prints the figures."""
    t = tol(case)
    gp, gc = value(case, "mlp/proba"), value(case, "mlp/loss_curve")
    print(f"{label}{case}: n_iter {n_iter} (golden {int(value(case, 'mlp/n_iter'))}), tol {t:.3e}")
    assert n_iter == int(value(case, "mlp/n_iter")) and len(curve) == len(gc)
    dp = float(np.max(np.abs(proba - gp) / gp))
    dc = float(np.max(np.abs(curve - gc) / gc))
    print(f"{label}{case}: max rel deviation proba {dp:.3e}, loss {dc:.3e}")
    assert dc <= t, (dc, t)
    assert dp <= t, (dp, t)


def assert_last_fit_equals_golden(case: str, last_fit: dict, *, label="") -> None:
    """Everything ``protein_fdr.last_fit`` holds after a call on the case's table."""
    assert_features_equal_golden(case, last_fit["group_pg"], last_fit["group_decoy"], last_fit["features"],
                                 last_fit["pg_names"])
    assert np.array_equal(last_fit["idx_train"], value(case, "split/train"))
    assert np.array_equal(last_fit["idx_test"], value(case, "split/test"))
    assert np.array_equal(bits(last_fit["mean"]), bits(value(case, "scaler/mean")))
    assert np.array_equal(bits(last_fit["scale"]), bits(value(case, "scaler/scale")))
    assert np.array_equal(bits(last_fit["x_scaled"]), bits(value(case, "mlp/x_all")))
    assert_training_within_tol(case, last_fit["proba"], last_fit["n_iter"], last_fit["loss_curve"], label=label)


def cohort(n_groups_per_class: int, rows_per_group: float = 10.0, n_runs: int = 6, seed: int = 0,
           dtype=np.float32) -> pd.DataFrame:
    """A seeded synthetic cohort: ``n_groups_per_class`` target and as many decoy protein groups with a geometric
    number of rows around ``rows_per_group``, precursors shared between the runs, scores that separate the classes
    only partly, 1 % of the rows without a pg, the rows shuffled."""
    rng = np.random.default_rng(seed)
    g = 2 * n_groups_per_class
    size = rng.geometric(1.0 / rows_per_group, g)
    group = np.repeat(np.arange(g), size)
    n = len(group)
    decoy = (group >= n_groups_per_class).astype(np.int64)
    quality = rng.beta(2, 2, g)[group]
    proba = np.where(decoy == 1, rng.beta(4, 2, n), rng.beta(1 + quality, 3 + 6 * quality, n))
    first = np.concatenate([[0], np.cumsum(size)[:-1]])[group]
    prec = first + rng.integers(0, np.maximum(1, size[group] // 3 + 1))
    names = np.array([f"PG{i:07d}" for i in range(n_groups_per_class)] +
                     [f"REV_PG{i:07d}" for i in range(n_groups_per_class)], dtype=object)
    runs = np.array([f"run_{r:02d}" for r in range(n_runs)], dtype=object)
    seqs = np.array([f"PEP{i:08d}" for i in range(n // 2 + 1)], dtype=object)
    df = pd.DataFrame({"pg": names[group], "decoy": decoy, "precursor_idx": prec.astype(np.int64),
                       "sequence": seqs[prec // 2], "run": runs[rng.integers(0, n_runs, n)],
                       "proba": np.clip(proba, 1e-6, 1 - 1e-6).astype(dtype)})
    df.loc[rng.random(n) < 0.01, "pg"] = np.nan
    return df.iloc[rng.permutation(n)].reset_index(drop=True)
