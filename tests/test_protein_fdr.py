"""Host side of the protein-group FDR (alphadia_amd/protein_fdr.py): the NumPy restatement against the reference's
goldens, the pairwise sum against NumPy's, the error cases and the C-ABI declarations of adh_pfdr_*.  No GPU needed."""

from __future__ import annotations

import ast
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import protein_fdr_golden as G
from alphadia_amd import _abi
from alphadia_amd import protein_fdr as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", G.CASES)
def test_host_perform_protein_fdr_equals_reference(case):
    df = G.table(case)
    before = df.copy()
    got = PF.host_perform_protein_fdr(df, None)
    G.assert_last_fit_equals_golden(case, PF.last_fit)
    exp = G.expected_frame(case)
    G.assert_frames_identical(got, exp)
    assert got["pg_qval"].dtype == np.float64 and list(got.columns)[-1] == "pg_qval"
    assert np.array_equal(got["pg_qval"].isna().to_numpy(), got["pg"].isna().to_numpy())
    n_target = int((before["decoy"] == 0).sum())
    assert np.array_equal(got.index.to_numpy(), np.concatenate([np.arange(n_target), np.arange(len(before) - n_target)]))
    pd.testing.assert_frame_equal(df, before)  # the caller's frame is left alone
    assert PF.last_timing["groups"] == len(G.value(case, "feat/decoy")) and PF.last_timing["epochs"] == PF.last_fit["n_iter"]


def test_golden_cases_cover_the_issue():
    for case in G.CASES:
        # the recipe's assertions: (a) opposite-class neighbours further apart than 4 tol, (b) no stop on an edge
        assert G.tol(case) == 64 * max(float(G.value(case, "assoc_spread")), 2.0**-52)
        assert float(G.value(case, "min_gap")) > 4 * G.tol(case) and float(G.value(case, "min_edge")) > 1e-9
    n_train = {c: len(G.value(c, "split/train")) for c in G.CASES}
    assert n_train["tiny"] < 200 and int(G.value("tiny", "mlp/n_iter")) == 200
    assert 250 <= len(G.value("ragged_f32", "feat/decoy")) <= 300 and n_train["ragged_f32"] % 200 != 0
    assert len(G.value("even", "feat/decoy")) == 500 and n_train["even"] == 400
    assert 500 <= len(G.value("separable", "feat/decoy")) <= 550 and int(G.value("separable", "mlp/n_iter")) < 200
    assert G.table("ragged_f32")["proba"].dtype == np.float32 and G.table("ragged_f64")["proba"].dtype == np.float64
    assert bool(G.value("ragged_f32", "feat/mean_is_f32")) and not bool(G.value("ragged_f64", "feat/mean_is_f32"))
    for case in ("ragged_f32", "ragged_f64"):
        df = G.table(case)
        names, decoy, x = G.feature_groups(case)
        sizes = set(x[:, 0].astype(int).tolist())
        assert {1, 7, 8, 9, 127, 128, 129, 255, 256, 257} <= sizes and max(sizes) >= 1100
        assert (x[:, 3] < x[:, 0]).any() and (x[:, 2] < x[:, 3]).any() and (x[:, 4] < x[:, 0]).any()  # repeats
        assert (df["precursor_idx"] > 2**32).any() and df["pg"].isna().sum() > 0
        assert len(set(names[decoy == 0]) & set(names[decoy == 1])) >= 1  # a pg in both classes
        pg = df["pg"].dropna().to_numpy()
        assert not np.array_equal(pg, np.sort(pg))  # shuffled rows
    assert os.path.getsize(G.PATH) < 600_000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pairwise_sum_is_numpys(dtype):
    rng = np.random.default_rng(5)
    for n in [*range(1, 301), 1100, 4099, 8191, 8192, 8193, 16385, 70_001, 262_145]:
        a = (rng.random(n) * 10 ** rng.uniform(-3, 3)).astype(dtype)
        got, exp = PF.pairwise_sum(a), np.add.reduce(a)
        assert type(got) is dtype and got == exp, (n, got, exp)


def test_standard_scaler_constant_column_and_layout():
    x = np.random.default_rng(1).random((50, 7))
    x[:, 2] = 3.0
    mean, scale = PF.standard_scaler(x)
    assert scale[2] == 1.0 and mean[2] == 3.0
    assert np.allclose(mean, x.mean(axis=0), rtol=1e-15) and np.allclose(scale[:2], x[:, :2].std(axis=0), rtol=1e-14)


def test_initial_parameters_and_step_sizes():
    p = PF.initial_parameters(np.random.RandomState(0))
    assert p.shape == (PF.N_PARAMS,) and PF.N_PARAMS == 901
    rs = np.random.RandomState(0)
    b1, b2 = np.sqrt(6.0 / 107), np.sqrt(6.0 / 101)
    w1 = rs.uniform(-b1, b1, (7, 100))
    i1 = rs.uniform(-b1, b1, 100)
    w2 = rs.uniform(-b2, b2, (100, 1))
    i2 = rs.uniform(-b2, b2, 1)
    assert np.array_equal(p, np.concatenate([w1.ravel(), i1, w2.ravel(), i2]))
    lr = PF.learning_rates(3, 2)
    assert lr.tolist() == [1e-3 * np.sqrt(1 - 0.999**t) / (1 - 0.9**t) for t in (4, 5)]


def test_stopping_rule():
    rule = PF.StoppingRule()
    assert not rule.stop(1.0)
    for k in range(10):
        assert not rule.stop(1.0 - 5e-5)  # within tol of the best: no improvement
    assert rule.stop(1.0 - 5e-5)  # the eleventh in a row
    rule = PF.StoppingRule()
    rule.stop(1.0)
    for k in range(10):
        assert not rule.stop(1.0)
    assert not rule.stop(0.5) and rule.stalled == 0


def _small(**changes):
    df = G.table("tiny")
    for c, (rows, v) in changes.items():
        df.loc[rows, c] = v
    return df


def test_value_errors():
    grouped = np.flatnonzero(G.table("tiny")["pg"].notna().to_numpy())
    with pytest.raises(ValueError, match="finite"):
        PF.host_perform_protein_fdr(_small(proba=(grouped[3], np.nan)))
    with pytest.raises(ValueError, match="finite"):
        PF.host_perform_protein_fdr(_small(proba=(grouped[5], np.inf)))
    with pytest.raises(ValueError, match="decoy must be 0 or 1"):
        PF.host_perform_protein_fdr(_small(decoy=(grouped[2], 2)))
    df = G.table("errors/one_class")
    assert set(df["decoy"]) == {0} and df["pg"].nunique() > 5
    with pytest.raises(ValueError, match="0 decoy protein groups") as e:
        PF.host_perform_protein_fdr(df)
    assert not isinstance(e.value, PF.TooFewProteinsError)
    df = df.assign(decoy=1)
    with pytest.raises(ValueError, match="0 target"):
        PF.host_perform_protein_fdr(df)
    # the same values in rows of no group harm nobody
    df = G.table("tiny")
    df.loc[len(df)] = df.loc[0]
    df.loc[len(df) - 1, ["pg", "proba", "decoy"]] = [np.nan, np.nan, 1]
    out = PF.host_perform_protein_fdr(df)
    assert len(out) == len(df) and np.isnan(out["pg_qval"].to_numpy()[-1])


def test_too_few_proteins():
    df = G.table("errors/one_group")
    assert df["pg"].nunique() == 1
    with pytest.raises(PF.TooFewProteinsError, match="train set will be empty"):
        PF.host_perform_protein_fdr(df)
    with pytest.raises(PF.TooFewProteinsError, match="no row"):
        PF.host_perform_protein_fdr(G.table("tiny").assign(pg=np.nan))


def test_build_precursor_table_chain(monkeypatch):
    """The chain around the FDR with both device stages replaced by their host comparators."""
    from alphadia_amd import grouping as PG

    seen = []

    def inference(psm_df, inference_strategy, group_level, device=None):
        seen.append((inference_strategy, group_level, device))
        return PG.host_perform_grouping(psm_df, genes_or_proteins=group_level, group=True)

    monkeypatch.setattr(PG, "apply_protein_inference", inference)
    monkeypatch.setattr(PF, "perform_protein_fdr", lambda df, figure_path=None, device=None: PF.host_perform_protein_fdr(df))
    df = G.table("even").drop(columns=["pg"])
    full = PF.host_perform_protein_fdr(PG.host_perform_grouping(df.copy(), genes_or_proteins="proteins", group=True))
    for fdr, keep in ((0.5, True), (0.5, False), (2.0, True)):
        got = PF.build_precursor_table(df.copy(), "heuristic", "proteins", fdr, keep, device=1)
        exp = full[full["pg_qval"] <= fdr]
        exp = exp if keep else exp[exp["decoy"] == 0]
        G.assert_frames_identical(got, exp)
        assert len(got) > 0 and (keep or set(got["decoy"]) == {0})
    assert seen == [("heuristic", "proteins", 1)] * 3


def test_pfdr_abi_declarations_agree():
    """Every adh_pfdr_* entry of the prototype table (tests/test_abi.py holds it against the header) is called by the
    wrapper class and defined in adh_protein_fdr.hip, which adh_api.hip includes (checked without loading the library)."""
    decl = [name for name in _abi.PROTOTYPES if name.startswith("adh_pfdr_")]
    assert len(decl) == 9
    src = open(os.path.join(ROOT, "alphadia_amd", "runtime.py")).read()
    wrapper = src[src.index("class DeviceProteinFdr"):]
    assert set(decl) == set(re.findall(r"lib\.(adh_pfdr_[a-z_]+)\(", wrapper))
    source = open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_protein_fdr.hip")).read()
    assert set(decl) == set(re.findall(r"^int (adh_pfdr_[a-z_]+)\(", source, re.M))
    assert '#include "adh_protein_fdr.hip"' in open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_api.hip")).read()


def test_the_product_does_not_import_sklearn():
    tree = ast.parse(open(PF.__file__).read())
    modules = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    modules += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert modules and not [m for m in modules if m.split(".")[0] in ("sklearn", "scipy")]


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference checkout is not on this machine")
def test_regenerating_the_golden_reproduces_the_committed_file(tmp_path):
    recipe = os.path.join(ROOT, "tests", "golden", "make_golden_protein_fdr.py")
    p = subprocess.run([sys.executable, recipe, "--out", str(tmp_path)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    fresh, golden = np.load(tmp_path / "protein_fdr.npz"), np.load(G.PATH)
    assert sorted(fresh.files) == sorted(golden.files)
    for key in golden.files:
        assert fresh[key].dtype == golden[key].dtype and fresh[key].shape == golden[key].shape, key
        case, _, what = key.partition("/")
        if what in ("assoc_spread", "tol", "min_gap", "min_edge"):
            continue  # measured with this machine's BLAS
        if what in ("mlp/proba", "mlp/loss_curve"):  # sklearn's products go through BLAS too
            assert np.max(np.abs(fresh[key] - golden[key]) / golden[key]) <= G.tol(case), key
        else:
            assert np.array_equal(G.bits(fresh[key]), G.bits(golden[key])), key
