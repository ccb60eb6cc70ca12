"""Protein inference on the GPU: the greedy set cover of ``perform_grouping`` per connected component.

Drop-ins for ``perform_grouping`` (alphadia/outputtransform/grouping.py:100-194) and ``apply_protein_inference``
(outputtransform/utils.py:243-295).  The reference keeps one set of precursors per protein id and loops: take the id
with the largest set (the first that appeared on a tie), make it the master of those precursors, subtract them from
every other set - quadratic in the number of ids.  The cover on one connected component of the id - precursor graph
never sees another component, so here the graph goes to HBM, its components are labelled, and every component gets
its own cover (alphadia_amd/csrc/adh_grouping.hip).

Strings stay on the host.  Precursors with the same id string in the same decoy class always get the same result,
so the device works on the distinct (class, id string) *patterns* weighted by their number of unique precursors, and
on id codes that number the ids in their order of first appearance (the two decoy classes with disjoint codes: they
are just more components).  The output strings are built once per pattern.

``host_perform_grouping`` restates the same semantics in Python / NumPy with a lazy max-heap, O(edges log ids).  It is
the comparator of the tests and the benchmark, not a fallback: ``perform_grouping`` needs the GPU.
"""

from __future__ import annotations

import heapq
import logging
import time
from dataclasses import dataclass, field

import numpy as np
import pandas as pd

logger = logging.getLogger()

# seconds / milliseconds of the stages of the last call (the benchmark reads them)
last_timing: dict[str, float] = {}


@dataclass
class IdGraph:
    """The id - pattern graph of the unique rows of a precursor table."""

    row_pattern: np.ndarray      # [unique rows] pattern of the row, -1: the row belongs to no cover
    weight: np.ndarray           # [patterns] int32: unique precursors of the pattern
    edge_pattern: np.ndarray     # [edges] int32, deduplicated (pattern, id) pairs, pattern-major
    edge_id: np.ndarray          # [edges] int32
    names: np.ndarray            # [ids] object: the id's string
    id_class: np.ndarray         # [ids] int8: the decoy class of the id's cover
    id_string: np.ndarray        # [ids] int32: code of the id's string over both classes ...
    id_rank: np.ndarray          # [ids] int32: ... and its place among the distinct strings as Python sorts str
    n_strings: int = 0
    pattern_class: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int8))


def decoy_classes(decoy: pd.Series) -> np.ndarray:
    """The cover every unique row belongs to: all 0 if the column holds one distinct value; otherwise 0 for
    ``decoy == 0``, 1 for ``decoy == 1`` and -1 (no cover, NaN in the result) for anything else.  A class without
    rows raises ``ValueError``, as the reference does when it unpacks an empty cover."""
    if len(decoy.unique()) == 1:
        return np.zeros(len(decoy), dtype=np.int8)
    d = decoy.to_numpy()
    cls = np.where(d == 0, 0, np.where(d == 1, 1, -1)).astype(np.int8)
    for c, what in ((0, "target"), (1, "decoy")):
        if not (cls == c).any():
            raise ValueError(f"protein grouping: the table holds no {what} precursors (decoy == {c})")
    return cls


def build_graph(strings: np.ndarray, cls: np.ndarray) -> IdGraph:
    """Patterns, first-appearance id codes, the deduplicated edge list, weights and ranks of the unique rows'
    id ``strings`` (object array of ``str``) and their classes (``decoy_classes``)."""
    keep = cls >= 0
    scode, suniq = pd.factorize(strings[keep])  # codes in order of first appearance
    n_s = max(len(suniq), 1)
    pcode, pkeys = pd.factorize(cls[keep].astype(np.int64) * n_s + scode)  # ... and so are the patterns
    row_pattern = np.full(len(strings), -1, dtype=np.int64)
    row_pattern[keep] = pcode
    weight = np.bincount(pcode, minlength=len(pkeys)).astype(np.int32)
    codes: tuple[dict[str, int], dict[str, int]] = ({}, {})
    names: list[str] = []
    id_class: list[int] = []
    ep: list[int] = []
    ei: list[int] = []
    pattern_class = np.empty(len(pkeys), dtype=np.int8)
    for p, key in enumerate(pkeys.tolist()):
        c, s = divmod(key, n_s)
        pattern_class[p] = c
        of = codes[c]
        for name in dict.fromkeys(suniq[s].split(";")):  # a repeated id counts once; "" is an id like any other
            i = of.get(name)
            if i is None:
                i = of[name] = len(names)
                names.append(name)
                id_class.append(c)
            ep.append(p)
            ei.append(i)
    names_a = np.empty(len(names), dtype=object)
    names_a[:] = names
    distinct, inverse = np.unique(names_a, return_inverse=True) if len(names) else (names_a, np.zeros(0, np.int64))
    rank = inverse.astype(np.int32).reshape(-1)
    return IdGraph(row_pattern, weight, np.asarray(ep, dtype=np.int32), np.asarray(ei, dtype=np.int32), names_a,
                   np.asarray(id_class, dtype=np.int8), rank, rank.copy(), len(distinct), pattern_class)


def _csr(keys: np.ndarray, values: np.ndarray, n: int):
    order = np.argsort(keys, kind="stable")
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys, minlength=n), out=off[1:])
    return off, values[order]


def host_cover(g: IdGraph) -> tuple[np.ndarray, np.ndarray]:
    """The greedy cover on the host: ``(pattern_master, id_emptied_by)`` as ``adh_pg_solve`` returns them.  A max-heap
    of (set size, first appearance) with stale entries dropped when they surface."""
    n_ids, n_pat = len(g.names), len(g.weight)
    ioff, iadj = _csr(g.edge_id, g.edge_pattern, n_ids)
    poff, padj = _csr(g.edge_pattern, g.edge_id, n_pat)
    ioff, iadj, poff, padj, w = ioff.tolist(), iadj.tolist(), poff.tolist(), padj.tolist(), g.weight.tolist()
    size = [sum(w[p] for p in iadj[ioff[i]:ioff[i + 1]]) for i in range(n_ids)]
    master = [-1] * n_pat
    emptied = [-1] * n_ids
    heap = [(-s, i) for i, s in enumerate(size)]
    heapq.heapify(heap)
    while heap:
        s, m = heapq.heappop(heap)
        if -s != size[m]:
            continue  # (stale: the id's set shrank after this entry was pushed)
        if s == 0:
            break
        touched = []
        for p in iadj[ioff[m]:ioff[m + 1]]:
            if master[p] >= 0:
                continue
            master[p] = m
            for j in padj[poff[p]:poff[p + 1]]:
                size[j] -= w[p]
                if j != m:
                    touched.append(j)
        for j in set(touched):
            if size[j] == 0:
                emptied[j] = m
            else:
                heapq.heappush(heap, (-size[j], j))
    return np.asarray(master, dtype=np.int32), np.asarray(emptied, dtype=np.int32)


def host_filter(g: IdGraph, master: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The heuristic filter on the host: ``(offsets, ids)`` as ``adh_pg_filter`` returns them."""
    allowed = np.zeros(max(g.n_strings, 1), dtype=bool)
    allowed[g.id_string[np.unique(master[master >= 0])]] = True
    keep = allowed[g.id_string[g.edge_id]]
    ep, ei = g.edge_pattern[keep], g.edge_id[keep]
    order = np.lexsort((g.id_rank[ei], ep))
    off = np.zeros(len(g.weight) + 1, dtype=np.int32)
    np.cumsum(np.bincount(ep, minlength=len(g.weight)), out=off[1:])
    return off, ei[order]


def _host_solver(g: IdGraph, group: bool):
    master, emptied = host_cover(g)
    return master, emptied, host_filter(g, master) if group else None


def _device_solver(device):
    def solve(g: IdGraph, group: bool):
        from alphadia_amd import runtime

        pg = runtime.get_context(device).protein_groups()
        try:
            master, emptied = pg.solve(g.edge_pattern, g.edge_id, g.weight, len(g.names))
            csr = pg.filter(g.id_string, g.id_rank, g.n_strings) if group else None
            label_ms, cover_ms, filter_ms = pg.time_ms()
            n_comp, n_large, rounds = pg.stats()
            last_timing.update(label_ms=label_ms, cover_ms=cover_ms, filter_ms=filter_ms, components=n_comp,
                               large_components=n_large, label_rounds=rounds)
        finally:
            pg.close()
        return master, emptied, csr

    return solve


def pattern_strings(g: IdGraph, master: np.ndarray, emptied: np.ndarray, csr, return_parsimony_groups: bool):
    """``(pg_master, pg)`` of every pattern as object arrays."""
    names = g.names
    pg_master = names[master]
    if csr is not None:  # the heuristic: the pattern's own ids that are a master somewhere, sorted as str sorts
        off, ids = csr
        kept = names[ids].tolist()
        off = off.tolist()
        pg = np.empty(len(master), dtype=object)
        pg[:] = [";".join(kept[off[p]:off[p + 1]]) for p in range(len(master))]
        return pg_master, pg
    if not return_parsimony_groups:
        return pg_master, pg_master.copy()
    members: dict[int, list[str]] = {}
    for i in np.flatnonzero(emptied >= 0).tolist():  # ascending id code: the order of first appearance
        members.setdefault(int(emptied[i]), []).append(names[i])
    group_of = {m: ";".join([names[m], *members.get(m, [])]) for m in np.unique(master).tolist()}
    pg = np.empty(len(master), dtype=object)
    pg[:] = [group_of[m] for m in master.tolist()]
    return pg_master, pg


def _perform_grouping(psm_df, genes_or_proteins, decoy_column, group, return_parsimony_groups, solver):
    if genes_or_proteins not in ["genes", "proteins"]:
        raise ValueError("Selected column must be 'genes' or 'proteins'")
    last_timing.clear()
    t0 = time.perf_counter()
    unique_mask = ~psm_df.duplicated(subset=["precursor_idx"], keep="first")
    psm_df[genes_or_proteins] = psm_df[genes_or_proteins].astype(str)  # (on the caller's frame, as the reference does)
    unique = psm_df.loc[unique_mask, ["precursor_idx", genes_or_proteins, decoy_column]]
    cls = decoy_classes(unique[decoy_column])
    g = build_graph(unique[genes_or_proteins].to_numpy(dtype=object), cls)
    t1 = time.perf_counter()
    master, emptied, csr = solver(g, group)
    t2 = time.perf_counter()
    if (master < 0).any():
        raise ValueError("Not all precursors were found in the output of the grouping function.")
    pg_master, pg = pattern_strings(g, master, emptied, csr, return_parsimony_groups)
    rows = g.row_pattern >= 0
    at = g.row_pattern[rows]
    result = pd.DataFrame({"precursor_idx": unique["precursor_idx"].to_numpy()[rows], "pg_master": pg_master[at],
                           "pg": pg[at]})
    out = psm_df.merge(result, on="precursor_idx", how="left")
    t3 = time.perf_counter()
    last_timing.update(prepare_s=t1 - t0, solve_s=t2 - t1, build_s=t3 - t2, patterns=len(g.weight), ids=len(g.names),
                       edges=len(g.edge_id))
    return out


def perform_grouping(psm_df: pd.DataFrame, genes_or_proteins: str = "proteins", decoy_column: str = "decoy",
                     group: bool = True, return_parsimony_groups: bool = False, device: int | None = None):
    """``perform_grouping`` with the set cover and the heuristic filter on the GPU.

    Parameters
    ----------
    psm_df : pd.DataFrame
        Precursor table with ``precursor_idx``, the id column and the decoy column.  The id column is turned into
        ``str`` in place, as the reference does.
    genes_or_proteins : str
        ``"proteins"`` or ``"genes"``: the column of ``;``-separated ids.
    decoy_column : str
        One distinct value: one cover over all rows; otherwise one over ``== 0`` and one over ``== 1``.
    group : bool
        The heuristic: ``pg`` becomes the row's own ids that are a master in either cover.
    return_parsimony_groups : bool
        With ``group=False``: ``pg`` lists, after the master, the ids whose last precursor it took.
    device : int | None
        GPU ordinal (default: the process's, ``runtime.default_device``).

    Returns the table left-merged with ``pg_master`` and ``pg`` of the first row of every ``precursor_idx``.
    """
    return _perform_grouping(psm_df, genes_or_proteins, decoy_column, group, return_parsimony_groups,
                             _device_solver(device))


def host_perform_grouping(psm_df: pd.DataFrame, genes_or_proteins: str = "proteins", decoy_column: str = "decoy",
                          group: bool = True, return_parsimony_groups: bool = False):
    """``perform_grouping`` restated on the host (``host_cover``, ``host_filter``), for comparison."""
    return _perform_grouping(psm_df, genes_or_proteins, decoy_column, group, return_parsimony_groups, _host_solver)


def apply_protein_inference(psm_df: pd.DataFrame, inference_strategy: str, group_level: str, device: int | None = None):
    """``apply_protein_inference`` (outputtransform/utils.py:243-295): ``library`` copies the column,
    ``maximum_parsimony`` is the cover alone, ``heuristic`` the cover with the filter."""
    if inference_strategy == "library":
        logger.info("Inference strategy: library. Using library grouping for protein inference")
        psm_df["pg"] = psm_df[group_level]
        psm_df["pg_master"] = psm_df[group_level]
    elif inference_strategy == "maximum_parsimony":
        logger.info("Inference strategy: maximum_parsimony. Using maximum parsimony for protein inference")
        psm_df = perform_grouping(psm_df, genes_or_proteins=group_level, group=False, device=device)
    elif inference_strategy == "heuristic":
        logger.info("Inference strategy: heuristic. Using maximum parsimony with grouping for protein inference")
        psm_df = perform_grouping(psm_df, genes_or_proteins=group_level, group=True, device=device)
    else:
        raise ValueError(f"Unknown inference strategy: {inference_strategy}. Valid options are "
                         "['library', 'maximum_parsimony', 'heuristic']")
    return psm_df
