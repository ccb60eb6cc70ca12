"""Golden vectors of the protein-group FDR, produced by RUNNING THE REFERENCE's ``perform_protein_fdr``
(alphadia/outputtransform/protein_fdr.py:15-112, with sklearn's MLPClassifier and StandardScaler) in the build
container:

    python tests/golden/make_golden_protein_fdr.py

TEST INFRASTRUCTURE, same rules as make_golden.py: the reference is imported through ref_shim, fed tables built here,
and inputs + captured intermediates + outputs are stored in ``tests/golden/protein_fdr.npz`` - arrays only, every
string column as int32 codes (-1: NaN) into a fixed-width Unicode name table.

Per case ``<c>``:

    <c>/in/<column>          the input table (string columns as <column>.codes / <column>.names); ``row_id`` numbers
                             the rows, so that out/row_id tells where every returned row came from
    <c>/feat/pg.codes/.names, <c>/feat/decoy, <c>/feat/X
                             the group feature frame in the reference's group order, X [groups, 7] float64 in the
                             order of the reference's feature_columns
    <c>/feat/mean_is_f32     whether mean / best / worst score came out as float32 (they do for a float32 proba)
    <c>/scaler/mean, scale   StandardScaler.mean_ / scale_
    <c>/split/train, test    the indices of train_test_split
    <c>/mlp/x_train, y_train the scaled training matrix and labels the classifier was fitted on
    <c>/mlp/x_all            the scaled matrix of all groups
    <c>/mlp/n_iter, loss_curve, proba
    <c>/out/row_id, index, pg_qval
                             the returned frame: source row, index value and pg_qval of every returned row
    <c>/assoc_spread, tol, min_gap, min_edge
                             the measured numbers the tolerances rest on (see below)
    <c>/meta                 JSON: columns and dtypes of the input and of the returned frame, the seed used

plus ``errors/<name>/in/...`` for the two tables on which the call must raise.

Tolerance.  For every case the NumPy restatement of the classifier (alphadia_amd/protein_fdr.py:host_fit_predict) runs
twice: with BLAS products, and with every contraction summed in reversed order through einsum without BLAS.
``assoc_spread`` is the larger of the two runs' maximum relative deviation from sklearn's probabilities and
``tol = 64 * max(assoc_spread, 2**-52)``: a device training differs from sklearn in the same things the two
restatements differ in (the association of the contractions, <= 2 ulp in exp / log).  The recipe asserts, and draws
the next seed if an assertion fails, that (a) neighbouring distinct probabilities of opposite class differ by more
than ``4 * tol`` relative (so the order behind the q-values cannot flip within tol) and (b) at every epoch
``|loss - (best - 1e-4)| > 1e-9`` (so no stop decision sits on an edge).
"""

from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_shim  # noqa: E402

ref_shim.install()

from alphadia.exceptions import TooFewProteinsError  # noqa: E402
from alphadia.outputtransform import protein_fdr as ref  # noqa: E402

from alphadia_amd import protein_fdr as PF  # noqa: E402

RUNS = [f"run_{r}" for r in range(6)]
EDGE_SIZES = [1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1100]


def cohort(seed: int, n_target: int, n_decoy: int, dtype, sizes=(), mean_rows: float = 6.0, separation: float = 1.0,
           shared_names: int = 0, nan_rows: int = 0, big_idx: bool = False) -> pd.DataFrame:
    """A seeded table of ``n_target`` + ``n_decoy`` protein groups.  ``sizes`` fixes the row count of the first
    groups (alternating classes), the others hold 1 + Poisson rows.  Inside a group precursors, sequences and runs
    repeat.  ``shared_names`` decoy groups carry the pg string of a target group; ``nan_rows`` rows have no pg."""
    rng = np.random.default_rng(seed)
    groups = [(f"PG{g:04d}", 0) for g in range(n_target)] + [(f"REV_PG{g:04d}", 1) for g in range(n_decoy)]
    for k in range(shared_names):
        groups[n_target + k] = (groups[3 * k + 1][0], 1)
    order = rng.permutation(len(groups))
    fixed = {int(order[k]): int(s) for k, s in enumerate(sizes)}
    rows = []
    next_idx = 1000
    for g, (name, decoy) in enumerate(groups):
        n = fixed.get(g, 1 + int(rng.poisson(mean_rows - 1)))
        quality = rng.beta(2, 2)  # of the group: a good target group has low scores throughout
        n_prec = max(1, int(np.ceil(n / rng.integers(1, 5))))
        prec = next_idx + rng.integers(0, n_prec, n)
        next_idx += n_prec
        if decoy:
            p = rng.beta(2 + 2 * separation, 2, n)
        else:
            p = rng.beta(1 + quality, 1 + (2 + 6 * quality) * separation, n)
        for i in range(n):
            rows.append((name, decoy, int(prec[i]), f"PEP{int(prec[i]) // 2:06d}", RUNS[int(rng.integers(0, 6))],
                         float(p[i])))
    df = pd.DataFrame({"pg": np.array([r[0] for r in rows], dtype=object),
                       "decoy": np.array([r[1] for r in rows], dtype=np.int64),
                       "precursor_idx": np.array([r[2] for r in rows], dtype=np.int64),
                       "sequence": np.array([r[3] for r in rows], dtype=object),
                       "run": np.array([r[4] for r in rows], dtype=object),
                       "proba": np.clip(np.array([r[5] for r in rows]), 1e-6, 1 - 1e-6).astype(dtype)})
    if big_idx:
        df.loc[df["precursor_idx"] % 7 == 0, "precursor_idx"] += (1 << 32) + 5
    if nan_rows:
        extra = df.sample(nan_rows, random_state=seed).copy()
        extra["pg"] = np.nan
        df = pd.concat([df, extra], ignore_index=True)
    df = df.sample(frac=1.0, random_state=seed + 1).reset_index(drop=True)  # a shuffled row order
    df["genes"] = df["pg"]
    df["proteins"] = df["pg"]
    df["row_id"] = np.arange(len(df), dtype=np.int64)
    return df


CASES = {
    "tiny": dict(n_target=22, n_decoy=18, dtype=np.float32, mean_rows=4.0),
    "ragged_f32": dict(n_target=150, n_decoy=130, dtype=np.float32, sizes=EDGE_SIZES, shared_names=5, nan_rows=17,
                       big_idx=True),
    "ragged_f64": dict(n_target=150, n_decoy=130, dtype=np.float64, sizes=EDGE_SIZES, shared_names=5, nan_rows=17,
                       big_idx=True),
    "even": dict(n_target=260, n_decoy=240, dtype=np.float32, mean_rows=3.0),
    "separable": dict(n_target=270, n_decoy=250, dtype=np.float32, mean_rows=3.0, separation=12.0),
}


def _put(out, key, values):
    v = np.asarray(values)
    if v.dtype != object:
        out[key] = v
        return
    missing = np.array([not isinstance(x, str) for x in v], dtype=bool)
    names, codes = np.unique(v[~missing].astype(str), return_inverse=True) if (~missing).any() else (np.zeros(0, "U1"), [])
    full = np.full(len(v), -1, dtype=np.int32)
    full[~missing] = codes
    out[key + ".codes"] = full
    out[key + ".names"] = names if len(names) else np.zeros(0, dtype="U1")


def dot_reversed(a, b):
    """The matrix product with every contraction summed from its last term to its first, without BLAS."""
    return np.einsum("ik,kj->ij", a[:, ::-1], b[::-1, :], optimize=False)


class Capture:
    """Runs the reference with its collaborators wrapped so that the intermediates can be stored."""

    def __init__(self):
        self.seen = {}

    def __enter__(self):
        seen = self.seen
        self.saved = (ref.train_test_split_, ref.StandardScaler, ref.MLPClassifier, ref.fdr.get_q_values)
        split, scaler_cls, mlp_cls, q_values = self.saved

        def split_(x, y, **kw):
            res = split(x, y, **kw)
            seen["x"], seen["y"], seen["train"], seen["test"] = x, y, res[4], res[5]
            return res

        class Scaler(scaler_cls):
            def fit_transform(self, x, y=None, **kw):
                seen["scaler"] = self
                return super().fit_transform(x, y, **kw)

        class Mlp(mlp_cls):
            def fit(self, x, y):
                seen["mlp"], seen["x_train"], seen["y_train"] = self, np.array(x), np.array(y)
                return super().fit(x, y)

            def predict_proba(self, x):
                seen["x_all"] = np.array(x)
                return super().predict_proba(x)

        def q_values_(df, **kw):
            seen["features"] = df.copy()
            return q_values(df, **kw)

        ref.train_test_split_, ref.StandardScaler, ref.MLPClassifier, ref.fdr.get_q_values = split_, Scaler, Mlp, q_values_
        return self

    def __exit__(self, *exc):
        ref.train_test_split_, ref.StandardScaler, ref.MLPClassifier, ref.fdr.get_q_values = self.saved


def try_case(name: str, spec: dict, seed: int):
    table = cohort(seed=seed, **spec)
    with Capture() as cap, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ref.perform_protein_fdr(table.copy(), None)
    s = cap.seen
    feats = s["features"]
    proba = feats["proba"].to_numpy()
    mlp = s["mlp"]
    curve = np.asarray(mlp.loss_curve_, dtype=np.float64)

    # the measured spread of the restatement under two associations of its contractions
    spread = 0.0
    for dot in (np.matmul, dot_reversed):
        p, n_iter, c = PF.host_fit_predict(s["x_train"], s["y_train"], s["x_all"], dot=dot)
        if n_iter != mlp.n_iter_:
            return None, f"restatement stopped after {n_iter} epochs, sklearn after {mlp.n_iter_}"
        spread = max(spread, float(np.max(np.abs(p - proba) / proba)))
    tol = 64 * max(spread, 2.0**-52)

    # (a) no two neighbouring probabilities of opposite class within 4 tol
    order = np.argsort(proba, kind="stable")
    ps, ds = proba[order], feats["decoy"].to_numpy()[order]
    cross = (ds[1:] != ds[:-1]) & (ps[1:] != ps[:-1])
    gap = float(np.min((ps[1:] - ps[:-1])[cross] / ps[1:][cross])) if cross.any() else np.inf
    if not gap > 4 * tol:
        return None, f"opposite-class probabilities {gap:.3g} apart, 4 tol = {4 * tol:.3g}"
    # (b) no stop decision on an edge
    best = np.minimum.accumulate(np.concatenate([[np.inf], curve[:-1]]))
    edge = float(np.min(np.abs(curve - (best - 1e-4))))
    if not edge > 1e-9:
        return None, f"a stop decision {edge:.3g} from its edge"
    return dict(table=table, res=res, seen=s, proba=proba, curve=curve, spread=spread, tol=tol, gap=gap, edge=edge,
                seed=seed), ""


def run_case(name, spec, out, summary):
    for seed in range(100, 120):
        got, why = try_case(name, spec, seed)
        if got is not None:
            break
        print(f"{name}: seed {seed} re-drawn ({why})")
    else:
        raise SystemExit(f"{name}: no seed passed the assertions")
    table, res, s = got["table"], got["res"], got["seen"]
    feats, mlp = s["features"], s["mlp"]
    # the frame q-values were computed on is the feature frame with proba; its order is the groups' order
    assert list(feats.columns[:4]) == ["pg", "genes", "proteins", "decoy"]
    x = feats[PF.FEATURE_COLUMNS].to_numpy()
    assert x.dtype == np.float64 and np.array_equal(x, s["x"])
    for c in table.columns:
        _put(out, f"{name}/in/{c}", table[c].to_numpy())
    _put(out, f"{name}/feat/pg", feats["pg"].to_numpy())
    out[f"{name}/feat/decoy"] = feats["decoy"].to_numpy().astype(np.int64)
    out[f"{name}/feat/X"] = x
    out[f"{name}/feat/mean_is_f32"] = np.array(all(feats[c].dtype == np.float32
                                                   for c in ("mean_score", "best_score", "worst_score")))
    out[f"{name}/scaler/mean"] = np.asarray(s["scaler"].mean_, dtype=np.float64)
    out[f"{name}/scaler/scale"] = np.asarray(s["scaler"].scale_, dtype=np.float64)
    out[f"{name}/split/train"] = np.asarray(s["train"], dtype=np.int64)
    out[f"{name}/split/test"] = np.asarray(s["test"], dtype=np.int64)
    out[f"{name}/mlp/x_train"] = np.ascontiguousarray(s["x_train"], dtype=np.float64)
    out[f"{name}/mlp/y_train"] = np.asarray(s["y_train"]).astype(np.uint8)
    out[f"{name}/mlp/x_all"] = np.ascontiguousarray(s["x_all"], dtype=np.float64)
    out[f"{name}/mlp/n_iter"] = np.array(mlp.n_iter_, dtype=np.int64)
    out[f"{name}/mlp/loss_curve"] = got["curve"]
    out[f"{name}/mlp/proba"] = got["proba"]
    # the returned frame: every column but pg_qval is the input's row, in the order out/row_id gives
    assert list(res.columns) == [*table.columns, "pg_qval"] and res["pg_qval"].dtype == np.float64
    rid = res["row_id"].to_numpy()
    for c in table.columns:
        assert res[c].dtype == table[c].dtype and res[c].reset_index(drop=True).equals(
            table[c].iloc[rid].reset_index(drop=True)), (name, c)
    out[f"{name}/out/row_id"] = rid
    out[f"{name}/out/index"] = np.asarray(res.index, dtype=np.int64)
    out[f"{name}/out/pg_qval"] = res["pg_qval"].to_numpy()
    out[f"{name}/assoc_spread"] = np.array(got["spread"])
    out[f"{name}/tol"] = np.array(got["tol"])
    out[f"{name}/min_gap"] = np.array(got["gap"])
    out[f"{name}/min_edge"] = np.array(got["edge"])
    meta = dict(columns=list(table.columns), dtypes=[str(t) for t in table.dtypes], out_columns=list(res.columns),
                out_dtypes=[str(t) for t in res.dtypes], seed=got["seed"])
    out[f"{name}/meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    summary[name] = dict(rows=len(table), groups=len(feats), n_iter=int(mlp.n_iter_), spread=got["spread"],
                         tol=got["tol"], gap=got["gap"], edge=got["edge"], seed=got["seed"])


def error_cases(out, summary):
    one_group = cohort(seed=7, n_target=1, n_decoy=0, dtype=np.float32)
    try:
        ref.perform_protein_fdr(one_group.copy(), None)
    except TooFewProteinsError:
        pass
    else:
        raise SystemExit("one_group: the reference did not raise TooFewProteinsError")
    one_class = cohort(seed=8, n_target=30, n_decoy=0, dtype=np.float32)
    for name, table in (("one_group", one_group), ("one_class", one_class)):
        for c in table.columns:
            _put(out, f"errors/{name}/in/{c}", table[c].to_numpy())
        meta = dict(columns=list(table.columns), dtypes=[str(t) for t in table.dtypes])
        out[f"errors/{name}/meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        summary[name] = dict(rows=len(table))


def main():
    out: dict[str, np.ndarray] = {}
    summary = {}
    for name, spec in CASES.items():
        run_case(name, spec, out, summary)
    assert summary["tiny"]["n_iter"] == 200 and summary["separable"]["n_iter"] < 200, summary
    assert summary["even"]["groups"] == 500
    error_cases(out, summary)
    path = os.path.join(OUT_DIR, "protein_fdr.npz")
    np.savez_compressed(path, **out)
    for k, v in summary.items():
        print(k, v)
    print(path, f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
