"""Host side of protein inference (alphadia_amd/grouping.py): the host restatement against the reference's goldens,
the string plumbing on hand-made inputs, the error cases, and the dispatch of apply_protein_inference.
No GPU needed."""

from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import grouping_golden as G
from alphadia_amd import grouping as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("case,k", G.call_ids())
def test_host_perform_grouping_equals_reference(case, k):
    G.check_call(PG.host_perform_grouping, case, k)


def _frame(ids, decoy=None):
    n = len(ids)
    return pd.DataFrame({"precursor_idx": np.arange(n), "proteins": ids,
                         "decoy": np.zeros(n, dtype=np.int64) if decoy is None else decoy})


def test_unknown_column_raises():
    df = _frame(["A"])
    df["peptides"] = df["proteins"]
    with pytest.raises(ValueError, match="genes.*proteins"):
        PG.host_perform_grouping(df, genes_or_proteins="peptides")


@pytest.mark.parametrize("decoy", [[], [0, 2, 0], [1, 2, 2], [2, 3]])
def test_a_class_without_rows_raises(decoy):
    df = _frame(["A", "A;B", "B"][: len(decoy)], np.array(decoy, dtype=np.int64))
    with pytest.raises(ValueError):
        PG.host_perform_grouping(df)


def test_first_appearance_codes_edges_weights_and_ranks():
    strings = np.array(["b;a", "a", "b;a", "c;c;b", "", "a;", "b;a", "zz"], dtype=object)
    cls = np.array([0, 0, 0, 0, 0, 0, 1, -1], dtype=np.int8)
    g = PG.build_graph(strings, cls)
    # patterns in order of first appearance; rows 0 and 2 share one, the decoy row with the same string does not
    assert g.row_pattern.tolist() == [0, 1, 0, 2, 3, 4, 5, -1]
    assert g.weight.tolist() == [2, 1, 1, 1, 1, 1] and g.weight.dtype == np.int32
    assert g.pattern_class.tolist() == [0, 0, 0, 0, 0, 1]
    # ids by first appearance, scanning rows in order and each string left to right; the classes have their own ids
    assert g.names.tolist() == ["b", "a", "c", "", "b", "a"]
    assert g.id_class.tolist() == [0, 0, 0, 0, 1, 1]
    edges = list(zip(g.edge_pattern.tolist(), g.edge_id.tolist()))
    assert edges == [(0, 0), (0, 1), (1, 1), (2, 2), (2, 0), (3, 3), (4, 1), (4, 3), (5, 4), (5, 5)]
    assert len(set(edges)) == len(edges) and g.edge_id.dtype == np.int32
    # ranks: the place of the id's string among the distinct strings as Python sorts them, shared by both classes
    order = sorted(set(g.names.tolist()))
    assert g.n_strings == len(order) == 4
    assert g.id_rank.tolist() == [order.index(s) for s in g.names.tolist()]
    assert g.id_string[0] == g.id_string[4] and g.id_string[1] == g.id_string[5]


def test_ranks_follow_code_points():
    names = ["P9", "P10", "a", "B", "b", "P100", "Ä", ""]
    g = PG.build_graph(np.array([";".join(names)], dtype=object), np.zeros(1, dtype=np.int8))
    assert [g.names[i] for i in np.argsort(g.id_rank)] == sorted(names)


def test_host_cover_ties_sizes_and_emptied():
    # ids: Y (rows 0, 2), B (rows 1, 2), then X only inside Y's shared row
    g = PG.build_graph(np.array(["Y", "B", "Y;B;X", "B"], dtype=object), np.zeros(4, dtype=np.int8))
    master, emptied = PG.host_cover(g)
    assert g.names.tolist() == ["Y", "B", "X"]
    assert g.names[master].tolist() == ["Y", "B", "B"]  # B holds 3 rows: it goes first and takes the shared one
    assert emptied.tolist() == [-1, -1, 1]
    g = PG.build_graph(np.array(["Y", "B", "Y;B;X"], dtype=object), np.zeros(3, dtype=np.int8))
    master, emptied = PG.host_cover(g)
    assert g.names[master].tolist() == ["Y", "B", "Y"]  # a tie: the id that appeared first
    assert emptied.tolist() == [-1, -1, 0]
    off, ids = PG.host_filter(g, master)
    assert off.tolist() == [0, 1, 2, 4] and g.names[ids].tolist() == ["Y", "B", "B", "Y"]


def test_apply_protein_inference_dispatch(monkeypatch):
    seen = []

    def plugged(psm_df, genes_or_proteins="proteins", decoy_column="decoy", group=True, return_parsimony_groups=False,
                device=None):
        seen.append((genes_or_proteins, group, return_parsimony_groups, device))
        return PG.host_perform_grouping(psm_df, genes_or_proteins, decoy_column, group, return_parsimony_groups)

    monkeypatch.setattr(PG, "perform_grouping", plugged)
    kwargs, exp_heuristic, _ = G.calls("genes")[1]
    _, exp_parsimony, _ = G.calls("genes")[0]
    assert kwargs["group"] and not G.calls("genes")[0][0]["group"]
    G.assert_frames_identical(PG.apply_protein_inference(G.table("genes"), "heuristic", "genes", device=3), exp_heuristic)
    G.assert_frames_identical(PG.apply_protein_inference(G.table("genes"), "maximum_parsimony", "genes"), exp_parsimony)
    assert seen == [("genes", True, False, 3), ("genes", False, False, None)]
    df = G.table("genes")
    out = PG.apply_protein_inference(df, "library", "genes")
    assert out is df and list(out.columns)[-2:] == ["pg", "pg_master"] and len(seen) == 2
    assert out["pg"].equals(df["genes"]) and out["pg_master"].equals(df["genes"])
    with pytest.raises(ValueError, match="Unknown inference strategy"):
        PG.apply_protein_inference(G.table("genes"), "parsimony", "genes")


def _graph_of(case, k=0):
    kwargs, exp, column = G.calls(case)[k]
    df = G.table(case)
    uniq = df[~df.duplicated(subset=["precursor_idx"], keep="first")]
    cls = PG.decoy_classes(uniq[kwargs["decoy_column"]])
    return PG.build_graph(uniq[column].astype(str).to_numpy(dtype=object), cls), exp


def test_golden_cases_cover_the_issue():
    # a tie decided against name order: the master of a shared row is the later of its ids in string order
    _, exp, _ = G.calls("ties")[0]
    assert exp["proteins"][0] == "Zeta;Alpha" and exp["pg_master"][0] == "Zeta"
    # a component above 1 024 ids (the chain is one component of 1 500)
    g, _ = _graph_of("chain")
    assert len(g.names) == 1500 and len(g.edge_id) - len(g.weight) == 1499  # a tree over all ids and patterns
    master, _ = PG.host_cover(g)
    assert len(np.unique(master)) > 500
    # an id with more than 1 024 patterns
    g, _ = _graph_of("hub")
    assert np.bincount(g.edge_id).max() == 3000 and len(g.names) == 3001
    # a pattern with 200 ids
    g, _ = _graph_of("wide")
    assert np.bincount(g.edge_pattern).max() == 200
    # a master among the targets only inside a decoy row's pg
    kwargs, exp, _ = G.calls("target_only_master")[1]
    assert kwargs["group"]
    decoy = exp[exp["decoy"] == 1]
    assert "T1" not in set(decoy["pg_master"]) and "T1" in set(exp.loc[exp["decoy"] == 0, "pg_master"])
    assert (decoy["pg"] == "D1;T1").any()
    # a NaN row (a third decoy value), and NaN ids that became the string "nan"
    third = [e for kw, e, _ in G.calls("decoys") if kw["decoy_column"] == "third"]
    assert len(third) == 3 and all(e["pg"].isna().any() and e["pg_master"].isna().sum() == e["pg"].isna().sum() for e in third)
    _, exp, _ = G.calls("odd_strings")[0]
    assert (exp["proteins"] == "nan").sum() == 2 and (exp["pg_master"] == "").any()
    # both classes in one structural table, parsimony groups with members, every mode on the small cases
    kwargs, exp, _ = G.calls("two_class")[0]
    assert kwargs["group"] and set(exp["decoy"]) == {0, 1}
    assert any(";" in s for s in G.calls("chain")[0][1]["pg"])
    assert {(kw["group"], kw["return_parsimony_groups"]) for kw, _, _ in G.calls("textbook")} == {
        (False, False), (True, False), (False, True)}
    assert G.calls("genes")[0][0]["genes_or_proteins"] == "genes"
    assert os.path.getsize(G.PATH) < 1_000_000


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference checkout is not on this machine")
def test_regenerating_the_golden_reproduces_the_committed_file(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_grouping.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    fresh, golden = np.load(tmp_path / "grouping.npz"), np.load(G.PATH)
    assert sorted(fresh.files) == sorted(golden.files)
    for key in golden.files:
        assert fresh[key].dtype == golden[key].dtype and np.array_equal(fresh[key], golden[key]), key
