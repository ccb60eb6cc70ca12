"""The dense library flattened on the GPU: fragment cardinality, intensity threshold with top-k, flat fragment rows.

``HipFlattenLibrary`` is the drop-in for the reference's ``FlattenLibrary`` (alphadia/libtransform/flatten.py:15-53, the
middle step of ``DecoyGenerator -> FlattenLibrary -> InitFlatColumns``, search_step.py:365-383) and
``init_flat_columns`` for ``InitFlatColumns.forward`` (flatten.py:67-108).  alphabase is not at hand, so nothing here is
pinned to that package:

    ``host_flatten_library`` restates ``alphabase.peptide.fragment.calc_fragment_cardinality`` +
    ``SpecLibFlat.parse_base_library`` once in NumPy, with the corner decisions written out below;
    ``HipFlattenLibrary`` runs the same rules on the device (alphadia_amd/csrc/adh_flatten.hip) and is pinned to this
    repository's restatement only, bit for bit; the restatement is pinned to hand-computed answers and invariants
    (tests/test_flatten.py).

Where a deployment finds a difference, the restatement changes and the device follows.  The restatement is the
comparator of the tests and of tools/bench_flatten.py, not a fallback: without the library this module does not import.

The rules
---------
Input: ``precursor_df`` with ``frag_start_idx``, ``frag_stop_idx``, ``elution_group_idx`` and optionally ``decoy``; two
float32 matrices ``[n_dense_rows, n_cols]`` (m/z and intensity) with equal column names, ``n_cols`` <= 32.  A column
name is ``{letter}[_{loss}]_z{charge}``: ``type`` is the letter's code point, ``loss_type`` 0 / 17 (``NH3``) / 18
(``H2O``) / 98 (``modloss``), ``a b c`` count from the N-terminus and ``x y z`` from the C-terminus; anything else is
a ``ValueError`` naming the column.

* A block ``[start, stop)`` has 0 .. 255 rows and lies inside the matrices.  Blocks of different precursors are
  disjoint: on the blocks ordered by (start, row count) every block starts at or behind its predecessor's stop, else
  ``ValueError``.  (Ordered so, an empty block stands before a filled one of the same start; an empty block whose
  start lies strictly inside another block is refused like any overlap.)  Dense rows that no block owns are dropped.
* The group of a precursor: the precursors with its ``elution_group_idx`` (an integer in [0, 2^56)) and, when
  ``decoy`` exists, its ``decoy`` value.  Groups need not be contiguous.  More than 255 in a group: ``ValueError``
  (the cardinality is a uint8).
* cardinality of cell (p, i, c): 1 + the other precursors q of the group with ``abs(mz_q[i, c] - mz_p[i, c]) <
  0.00001``, the difference in float32, the comparison in float64; a NaN difference (NaN, or two equal infinities) does
  not count.  A group whose members differ in row count leaves all its cells at 1.
* A cell is kept iff ``intensity > min_fragment_intensity`` (strict) and it is among the ``top_k`` cells of its block
  by (intensity descending, flat index descending) - what ``np.argsort(intensity, kind="stable")[-top_k:]`` selects.
  NaN is never kept and ranks below every number; ``-0.0`` ties with ``+0.0``.  ``top_k`` is at least 1.
* Fragment rows: the kept cells by dense flat index ``r * n_cols + c``; ``mz``, ``intensity`` float32; ``type``,
  ``loss_type``, ``charge``, ``number``, ``position``, ``cardinality`` uint8 (the dtypes of ``fragments_flat_schema``,
  validation/schemas.py:35-48); ``position`` = i, ``number`` = i + 1 for the N-terminal series and n - i for the
  C-terminal ones.
* Precursor rows: the input frame in its own order with its own index, ``flat_frag_start_idx`` /
  ``flat_frag_stop_idx`` uint32 from the exclusive scan of the kept counts over the blocks in (start, row count)
  order; nothing kept: start == stop; 2^32 rows or more: ``ValueError``.
"""

from __future__ import annotations

import re
import time

import numpy as np
import pandas as pd

from alphadia_amd import runtime
from alphadia_amd.optimization import BatchLibrary

MAX_COLUMNS = 32
MAX_ROWS = 255
MAX_GROUP = 255
LOSS_TYPES = {None: 0, "NH3": 17, "H2O": 18, "modloss": 98}
N_TERMINAL, C_TERMINAL = "abc", "xyz"
FRAGMENT_COLUMNS = ("mz", "intensity", "type", "loss_type", "charge", "number", "position", "cardinality")

last_timing: dict = {}

_COLUMN = re.compile(r"([a-z])(?:_([A-Za-z0-9]+))?_z([0-9]+)")


def parse_columns(names) -> np.ndarray:
    """``codes[4, n_cols]`` uint8 of the dense frames' column names: type, loss_type, charge, counts-from-the-N-terminus."""
    names = list(names)
    if not 1 <= len(names) <= MAX_COLUMNS:
        raise ValueError(f"flatten: 1 to {MAX_COLUMNS} fragment columns, not {len(names)}")
    codes = np.zeros((4, len(names)), dtype=np.uint8)
    for j, name in enumerate(names):
        m = _COLUMN.fullmatch(name) if isinstance(name, str) else None
        if (m is None or m.group(1) not in N_TERMINAL + C_TERMINAL or m.group(2) not in LOSS_TYPES
                or not 1 <= int(m.group(3)) <= 255):
            raise ValueError(f"flatten: fragment column {name!r} is not {{letter}}[_{{loss}}]_z{{charge}}")
        codes[:, j] = ord(m.group(1)), LOSS_TYPES[m.group(2)], int(m.group(3)), m.group(1) in N_TERMINAL
    return codes


def _parts(input):  # noqa: A002
    """``(precursor_df, mz[R, C] float32, intensity[R, C] float32, column codes)`` of a dense library object."""
    pre = getattr(input, "_precursor_df", None)
    pre = input.precursor_df if pre is None else pre
    frames = []
    for name in ("fragment_mz_df", "fragment_intensity_df"):
        f = getattr(input, "_" + name, None)
        frames.append(getattr(input, name) if f is None else f)
    mz_df, int_df = frames
    if list(mz_df.columns) != list(int_df.columns) or mz_df.shape != int_df.shape:
        raise ValueError("flatten: fragment_mz_df and fragment_intensity_df differ in shape or columns")
    codes = parse_columns(mz_df.columns)
    mats = []
    for name, f in (("fragment_mz_df", mz_df), ("fragment_intensity_df", int_df)):
        m = f.to_numpy()
        if m.dtype != np.float32:
            raise TypeError(f"flatten: {name} must be float32, not {m.dtype}")
        mats.append(np.ascontiguousarray(m))
    return pre, mats[0], mats[1], codes


def _precursor_columns(pre: pd.DataFrame, n_rows: int):
    """The four precursor columns as the device takes them, with the checks that need no matrix."""
    missing = [c for c in ("frag_start_idx", "frag_stop_idx", "elution_group_idx") if c not in pre.columns]
    if missing:
        raise ValueError(f"flatten: precursor_df lacks {missing}")
    eg = pre["elution_group_idx"].to_numpy()
    if eg.dtype.kind not in "iu":
        raise ValueError("flatten: elution_group_idx must be an integer column")
    if len(eg) and (int(eg.min()) < 0 or int(eg.max()) >= 1 << 56):
        raise ValueError("flatten: elution_group_idx outside [0, 2^56)")
    start = pre["frag_start_idx"].to_numpy().astype(np.int64)
    stop = pre["frag_stop_idx"].to_numpy().astype(np.int64)
    n = stop - start
    bad = np.flatnonzero((start < 0) | (n < 0) | (stop > n_rows))
    if len(bad):
        raise ValueError(f"flatten: the fragment rows of precursor {int(bad[0])} lie outside the library's matrices")
    bad = np.flatnonzero(n > MAX_ROWS)
    if len(bad):
        raise ValueError(f"flatten: precursor {int(bad[0])} has {int(n[bad[0]])} fragment rows (0 .. {MAX_ROWS} are supported)")
    decoy = pre["decoy"].to_numpy().astype(np.uint8) if "decoy" in pre.columns else None
    return start, stop, eg.astype(np.int64), decoy


def _check_top_k(top_k) -> int:
    if int(top_k) != top_k or int(top_k) < 1:
        raise ValueError(f"flatten: top_k_fragments must be an integer of at least 1, not {top_k!r}")
    return int(top_k)


def _ranges(first: np.ndarray, length: np.ndarray) -> np.ndarray:
    """``concatenate([arange(f, f + l) for f, l in zip(first, length)])``."""
    ends = np.cumsum(length)
    return np.repeat(first - (ends - length), length) + np.arange(int(ends[-1]) if len(ends) else 0, dtype=np.int64)


def order_key(intensity: np.ndarray) -> np.ndarray:
    """uint32 whose order is the ranking's: NaN below every number, ``-0.0`` with ``+0.0``."""
    x = np.ascontiguousarray(intensity, dtype=np.float32) + np.float32(0.0)  # (-0.0 + 0.0 is +0.0)
    u = x.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(x)] = 0
    return key


# ---- the restatement ---------------------------------------------------------------------------------------------

def host_cardinality(start, stop, elution_group, decoy, mz: np.ndarray) -> np.ndarray:
    """uint8 ``[n_dense_rows, n_cols]``: the cardinality of every owned cell (1 in rows nobody owns)."""
    n_prec = len(start)
    card = np.ones(mz.shape, dtype=np.int64)
    if n_prec == 0:
        return card.astype(np.uint8)
    rows = stop - start
    keys = np.stack([decoy if decoy is not None else np.zeros(n_prec, np.uint8), elution_group], axis=1)
    _, gid, size = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    gid = gid.reshape(-1)
    if size.max() > MAX_GROUP:
        p = int(np.flatnonzero(size[gid] > MAX_GROUP)[0])
        raise ValueError(f"flatten: the elution group of precursor {p} has more than {MAX_GROUP} precursors "
                         "(the cardinality is a uint8)")
    by_group = np.argsort(gid, kind="stable")           # members of a group side by side, in row order
    first = np.cumsum(size) - size                      # where every group begins in by_group
    lo, hi = np.full(len(size), np.iinfo(np.int64).max), np.full(len(size), -1)
    np.minimum.at(lo, gid, rows)
    np.maximum.at(hi, gid, rows)
    uniform = lo == hi
    slot = np.arange(n_prec) - first[gid[by_group]]     # a member's place in its group
    g_of = gid[by_group]
    for shift in range(1, int(size.max())):             # every ordered pair (p, q != p) of a group exactly once
        take = uniform[g_of] & (size[g_of] > shift) & (rows[by_group] > 0)
        if not take.any():
            continue
        p = by_group[take]
        q = by_group[first[g_of[take]] + (slot[take] + shift) % size[g_of[take]]]
        rp, rq = _ranges(start[p], rows[p]), _ranges(start[q], rows[p])
        d = np.abs(mz[rq] - mz[rp])                     # float32
        with np.errstate(invalid="ignore"):
            card[rp] += d.astype(np.float64) < 0.00001  # (NaN: False)
    return card.astype(np.uint8)


def host_flatten_library(precursor_df: pd.DataFrame, fragment_mz: np.ndarray, fragment_intensity: np.ndarray, columns,
                         top_k_fragments: int = 12, min_fragment_intensity: float = 0.01):
    """The NumPy restatement of the rules in the module docstring: ``(precursor_df, fragment_df)``."""
    codes = parse_columns(columns)
    mz = np.ascontiguousarray(fragment_mz, dtype=np.float32)
    inten = np.ascontiguousarray(fragment_intensity, dtype=np.float32)
    if mz.ndim != 2 or mz.shape != inten.shape or mz.shape[1] != codes.shape[1]:
        raise ValueError("flatten: two matrices of one shape, one column per name")
    top_k = _check_top_k(top_k_fragments)
    min_int = np.float32(min_fragment_intensity)
    C = mz.shape[1]
    start, stop, eg, decoy = _precursor_columns(precursor_df, mz.shape[0])
    n_prec = len(start)
    rows = stop - start
    order = np.lexsort((rows, start))
    if n_prec > 1:
        bad = np.flatnonzero(start[order][1:] < stop[order][:-1])
        if len(bad):
            raise ValueError(f"flatten: the fragment rows of precursors {int(order[bad[0]])} and "
                             f"{int(order[bad[0] + 1])} overlap")
    card = host_cardinality(start, stop, eg, decoy, mz)

    kept_count = np.zeros(n_prec, dtype=np.int64)       # per position of the block order
    parts = {name: [] for name in FRAGMENT_COLUMNS}
    mz_f, int_f, card_f = mz.reshape(-1), inten.reshape(-1), card.reshape(-1)
    STEP = 65536
    for j0 in range(0, n_prec, STEP):
        p = order[j0:j0 + STEP]
        cells = rows[p] * C
        if cells.sum() == 0:
            continue
        seg = np.repeat(np.arange(len(p), dtype=np.int64), cells)   # the block of every cell, in block order
        flat = _ranges(start[p] * C, cells)                          # its dense flat index
        seg_end = np.cumsum(cells)[seg]
        x = int_f[flat]
        # ascending by (block, key), ties in flat order: np.argsort(kind="stable") per block
        by = np.argsort(seg << 32 | order_key(x).astype(np.int64), kind="stable")
        from_top = np.empty(len(by), dtype=np.int64)
        from_top[by] = seg_end[by] - 1 - np.arange(len(by))
        with np.errstate(invalid="ignore"):
            k = (from_top < top_k) & (x > min_int)
        kept_count[j0:j0 + len(p)] = np.bincount(seg[k], minlength=len(p))
        f, s = flat[k], seg[k]
        i, col = f // C - start[p][s], f % C
        parts["mz"].append(mz_f[f])
        parts["intensity"].append(x[k])
        parts["type"].append(codes[0][col])
        parts["loss_type"].append(codes[1][col])
        parts["charge"].append(codes[2][col])
        parts["number"].append(np.where(codes[3][col] != 0, i + 1, rows[p][s] - i).astype(np.uint8))
        parts["position"].append(i.astype(np.uint8))
        parts["cardinality"].append(card_f[f])
    total = int(kept_count.sum())
    if total >= 0xFFFFFFFF:
        raise ValueError("flatten: the flat library would have 2^32 rows or more")
    dtypes = dict(mz=np.float32, intensity=np.float32)
    frag = pd.DataFrame({name: (np.concatenate(v) if v else np.empty(0)).astype(dtypes.get(name, np.uint8))
                         for name, v in parts.items()})
    flat_start = np.empty(n_prec, dtype=np.uint32)
    flat_stop = np.empty(n_prec, dtype=np.uint32)
    ends = np.cumsum(kept_count)
    flat_start[order] = ends - kept_count
    flat_stop[order] = ends
    pre = precursor_df.copy()
    pre["flat_frag_start_idx"] = flat_start
    pre["flat_frag_stop_idx"] = flat_stop
    return pre, frag


# ---- the device path ---------------------------------------------------------------------------------------------

class HipFlattenLibrary:
    """Drop-in for ``FlattenLibrary``: ``forward(input)`` returns ``flat_factory()`` with ``_precursor_df`` /
    ``_fragment_df`` set (alphabase's ``SpecLibFlat`` in a deployment; by default a two-frame object like
    ``optimization.BatchLibrary``).  ``input``: any object with ``precursor_df`` / ``_precursor_df`` and the two dense
    frames ``fragment_mz_df`` / ``fragment_intensity_df`` (a ``ConsensusLibrary`` included: its frames are fetched to
    the host as usual).  With ``context`` the ``LibRec`` records are left staged there, and the context is told that
    they equal the returned frame's columns: the next ``stage_fragments`` of that frame skips."""

    def __init__(self, top_k_fragments: int = 12, min_fragment_intensity: float = 0.01, device: int | None = None,
                 flat_factory=None) -> None:
        self.top_k_fragments = top_k_fragments
        self.min_fragment_intensity = min_fragment_intensity
        self.device = device
        self.flat_factory = flat_factory

    def validate(self, input) -> bool:  # noqa: A002
        has_pre = hasattr(input, "_precursor_df") or hasattr(input, "precursor_df")
        return has_pre and all(hasattr(input, "_" + n) or hasattr(input, n)
                               for n in ("fragment_mz_df", "fragment_intensity_df"))

    def __call__(self, input, context=None):  # noqa: A002
        if not self.validate(input):
            raise ValueError("HipFlattenLibrary: the input has no precursor_df or no dense fragment frames")
        return self.forward(input, context)

    def forward(self, input, context=None):  # noqa: A002
        t0 = time.perf_counter()
        pre, mz, inten, codes = _parts(input)
        top_k = _check_top_k(self.top_k_fragments)
        start, stop, eg, decoy = _precursor_columns(pre, mz.shape[0])
        t1 = time.perf_counter()
        ctx = context if context is not None else runtime.get_context(self.device)
        out = ctx.flatten_library(start, stop, eg, decoy, mz, inten, codes, top_k, self.min_fragment_intensity,
                                  stage=context is not None)
        t2 = time.perf_counter()
        frag = pd.DataFrame({name: out[name] for name in FRAGMENT_COLUMNS}, copy=False)
        pre = pre.copy()
        pre["flat_frag_start_idx"] = out["flat_frag_start_idx"]
        pre["flat_frag_stop_idx"] = out["flat_frag_stop_idx"]
        if context is not None:
            # (the frame's m/z column is both mz_library and mz of the staged records, under either name)
            mz_col = frag["mz"].values
            ctx.adopt_fragment_columns(mz_col, mz_col, *(frag[name].values for name in FRAGMENT_COLUMNS[1:]))
        flat = self.flat_factory() if self.flat_factory is not None else BatchLibrary(None, None)
        flat._precursor_df = pre
        flat._fragment_df = frag
        t3 = time.perf_counter()
        last_timing.clear()
        last_timing.update(prepare_s=t1 - t0, device_s=t2 - t1, frames_s=t3 - t2, total_s=t3 - t0,
                           kernel_ms=out["kernel_ms"], h2d_bytes=out["h2d_bytes"], d2h_bytes=out["d2h_bytes"],
                           routes=dict(out["routes"]), n_precursors=len(pre), n_fragments=len(frag),
                           staged=context is not None)
        return flat


def init_flat_columns(lib):
    """``InitFlatColumns.forward`` (flatten.py:67-108): the first matching column of each frame becomes ``mz_library`` /
    ``rt_library`` / ``mobility_library``; without a mobility column ``mobility_library`` is 0 (float32, the dtype of
    ``precursors_flat_schema``).  The frames are renamed in place; ``lib`` is returned."""
    precursor_columns = {
        "mz_library": ["mz_library", "mz", "precursor_mz"],
        "rt_library": ["rt_library", "rt", "rt_norm", "rt_pred", "rt_norm_pred", "irt"],
        "mobility_library": ["mobility_library", "mobility", "mobility_pred"],
    }
    fragment_columns = {"mz_library": ["mz_library", "mz", "predicted_mz"]}
    pre = getattr(lib, "_precursor_df", None)
    pre = lib.precursor_df if pre is None else pre
    frag = getattr(lib, "_fragment_df", None)
    frag = lib.fragment_df if frag is None else frag
    for mapping, df in ((precursor_columns, pre), (fragment_columns, frag)):
        for key, candidates in mapping.items():
            for name in candidates:
                if name in df.columns:
                    df.rename(columns={name: key}, inplace=True)
                    break
    if "mobility_library" not in pre.columns:
        pre["mobility_library"] = np.float32(0)
    return lib
