"""The match-between-runs library of the output stage on the GPU: group medians, lookup, fragment drop.

Drop-in for ``MbrLibraryBuilder`` and ``IndexBuilder`` (alphadia/libtransform/mbr.py), the last step of
``SearchPlanOutput._build_mbr_library``.  The reference filters the combined precursor table at 1 % FDR, aggregates the
survivors twice with a pandas group-by (median ``rt_observed``, first ``pg``), cuts the base library down to the
elution groups that passed with ``isin`` and ``remove_unused_fragments``, and joins the aggregates back with two
``reindex`` calls.  Here

* ``adh_mbr_aggregate`` compacts the rows with ``qval <= fdr``, orders them by (key, RT) for each of the two keys with
  stable radix passes and reads every segment's median from the ordered values: the middle value, or the mean of the
  two middle values in float64 rounded to the column's dtype, as pandas' group median does; NaN RTs are skipped, an
  all-NaN group is NaN, ``-0.0`` counts as ``+0.0``.  The first non-null ``pg`` of a group comes back as a row of the
  PSM table; the strings stay on the host;
* ``adh_mbr_filter`` finds the library precursors of the passed elution groups by binary search, keeps them in
  library row order and drops the dense fragment rows of all others: the kept blocks in the order of their old
  ``frag_start_idx``, renumbered by an exclusive scan of their lengths (the bookkeeping and kernels of the
  transfer-learning library), one gather per dense matrix;
* ``adh_mbr_assign`` looks every kept precursor up in the two aggregate tables: its own hash when it was identified,
  its elution group otherwise.

alphabase is not imported.  The result is a ``ConsensusLibrary``: ``precursor_df`` / ``_precursor_df``, the dense
frames under alphabase's names and ``available_dense_fragment_dfs()``.  ``base_library`` is not modified.

``host_build_mbr_library`` and ``host_index_builder`` restate the same semantics in NumPy; they are the comparators of
the tests and the benchmark, not fallbacks: the public classes need the GPU.

Pinned to these restatements only (alphabase's source is not at hand): ``remove_unused_fragments`` - the kept blocks
in the order of their old ``frag_start_idx``, one block per precursor, renumbered by a running sum; the precursor
frame keeps its row order and its index, the dense frames get a RangeIndex - and everything about decoys.

Where the reference misbehaves: a kept precursor whose elution group is in neither aggregate table gets
``NaN.astype(int64)`` as its index there; here that is a ``ValueError``.  It cannot happen through ``forward`` without a
decoy generator that invents elution groups.  No kept precursor at all (no PSM passes) is a ``ValueError`` in both.
"""

from __future__ import annotations

import time

import numpy as np
import pandas as pd

from alphadia_amd import _abi
from alphadia_amd.transfer_library import ConsensusLibrary, host_drop_unused

PSM_COLUMNS = ("qval", "elution_group_idx", "mod_seq_charge_hash", "rt_observed", "pg")
LIBRARY_COLUMNS = ("elution_group_idx", "mod_seq_charge_hash", "frag_start_idx", "frag_stop_idx")

# seconds / milliseconds / bytes of the stages of the last call (the benchmark reads them)
last_timing: dict[str, float] = {}


# --------------------------------------------------------------------------------------------
# the inputs
# --------------------------------------------------------------------------------------------
def _psm_parts(psm_df: pd.DataFrame, keep_decoys: bool, notnull=pd.notna) -> dict:
    need = PSM_COLUMNS if keep_decoys else (*PSM_COLUMNS, "decoy")
    missing = [c for c in need if c not in psm_df.columns]
    if missing:
        raise ValueError(f"MBR library: psm_df lacks {missing}")
    pg = psm_df["pg"].to_numpy()
    decoy = psm_df["decoy"].to_numpy() if "decoy" in psm_df.columns else np.zeros(len(psm_df), np.uint8)
    return dict(qval=psm_df["qval"].to_numpy(), decoy=decoy, eg=psm_df["elution_group_idx"].to_numpy(),
                hash=psm_df["mod_seq_charge_hash"].to_numpy(), rt=psm_df["rt_observed"].to_numpy(), pg=pg,
                pg_notnull=notnull(pg))


def _library_parts(base_library):
    """``(precursor_df, names, columns, matrices)`` of a library object, checked."""
    df = getattr(base_library, "_precursor_df", None)
    if df is None:
        df = base_library.precursor_df
    missing = [c for c in LIBRARY_COLUMNS if c not in df.columns]
    if missing:
        raise ValueError(f"MBR library: precursor_df lacks {missing}")
    names = list(base_library.available_dense_fragment_dfs())
    if not 1 <= len(names) <= _abi.TL_MAX_MATRICES:
        raise ValueError(f"MBR library: 1 to {_abi.TL_MAX_MATRICES} dense fragment frames, not {len(names)}")
    frames = [getattr(base_library, n) for n in names]
    columns = list(frames[0].columns)
    mats = []
    for n, f in zip(names, frames):
        if list(f.columns) != columns or f.shape != frames[0].shape:
            raise ValueError(f"MBR library: {n} differs from {names[0]} in shape or columns")
        m = f.to_numpy()
        if m.dtype != np.float32:
            raise TypeError(f"MBR library: {n} must be float32, not {m.dtype}")
        mats.append(np.ascontiguousarray(m))
    return df, names, columns, mats


def _kept_library(df, kept, start, stop, names, columns, frames=None, fetch=None) -> ConsensusLibrary:
    out = df.iloc[kept].copy()
    out["frag_start_idx"] = start.astype(df["frag_start_idx"].dtype)
    out["frag_stop_idx"] = stop.astype(df["frag_stop_idx"].dtype)
    return ConsensusLibrary(out, names, columns, frames, fetch)


def _decoys(lib, keep_decoys: bool, decoy_generator, rehash):
    if not keep_decoys:
        return lib
    lib = decoy_generator(lib)
    lib._precursor_df = rehash(lib._precursor_df)
    return lib


def _write_columns(lib, rt, pg_row, pg) -> None:
    if len(rt) == 0:  # (the reference: the maximum of no index)
        raise ValueError("MBR library: no library precursor lies in an elution group that passed")
    pg_values = np.empty(len(pg_row), dtype=object)  # (None where a group has no pg)
    has = pg_row >= 0
    pg_values[has] = np.asarray(pg, dtype=object)[pg_row[has]]
    df = lib._precursor_df
    df["rt"] = rt
    df["genes"] = pg_values
    df["proteins"] = pg_values


def _check_builder(keep_decoys, decoy_generator, rehash):
    if keep_decoys and (decoy_generator is None or rehash is None):
        raise ValueError("MBR library: keep_decoys=True needs the reference's DecoyGenerator and hash_precursor_df as "
                         "decoy_generator and rehash (alphabase is not imported here)")


# --------------------------------------------------------------------------------------------
# host restatements
# --------------------------------------------------------------------------------------------
def _ordered_keys(a, what: str = "key") -> np.ndarray:
    """An integer column as uint64 whose order is the column's: signed values with their sign bit flipped."""
    a = np.asarray(a)
    if a.dtype.kind == "u":
        return a.astype(np.uint64)
    if a.dtype.kind == "i":
        return a.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    raise TypeError(f"{what}: an integer column, not {a.dtype}")


def _key_pair(targets, lookup, what: str):
    """Targets and lookup keys in one order-preserving uint64 form (pandas compares the values, not the bits)."""
    t, k = np.asarray(targets), np.asarray(lookup)
    if len(k) == 0:
        k = k.astype(t.dtype if t.dtype.kind in "iu" else np.int64)
    if len(t) == 0:
        t = t.astype(k.dtype)
    if t.dtype.kind not in "iu" or k.dtype.kind not in "iu":
        raise TypeError(f"{what}: integer key columns, not {t.dtype} and {k.dtype}")
    if (t.dtype == np.uint64) != (k.dtype == np.uint64):
        raise TypeError(f"{what}: uint64 keys on one side and {t.dtype if k.dtype == np.uint64 else k.dtype} on the other")
    if t.dtype == np.uint64:
        return t.astype(np.uint64), k.astype(np.uint64)
    return _ordered_keys(t.astype(np.int64)), _ordered_keys(k.astype(np.int64))


def host_lookup(targets, lookup, what: str = "lookup") -> np.ndarray:
    """The position of every target in ``lookup`` (-1: absent); a key twice in ``lookup`` raises ``ValueError`` as
    pandas' ``reindex`` does."""
    t, k = _key_pair(targets, lookup, what)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    if (ks[1:] == ks[:-1]).any():
        raise ValueError("cannot reindex on an axis with duplicate labels")
    at = np.searchsorted(ks, t)
    hit = at < len(ks)
    hit[hit] = ks[at[hit]] == t[hit]
    out = np.full(len(t), -1, np.int64)
    out[hit] = order[at[hit]]
    return out


class _IndexBuilderBase:
    """``IndexBuilder`` (libtransform/mbr.py): ``apply`` is the reference's host take, object arrays included."""

    _lookup = None  # (targets, lookup, what) -> positions or -1

    def __init__(self, target_keys, target_fallback_keys, fallback_lookup_keys, specific_lookup_keys) -> None:
        fallback = self._lookup(target_fallback_keys, fallback_lookup_keys, "fallback keys")
        if (fallback < 0).any():
            raise ValueError(f"IndexBuilder: {int((fallback < 0).sum())} targets have a fallback key that is not in the "
                             "fallback lookup table")
        self._fallback_indices = fallback
        if len(specific_lookup_keys) > 0:
            specific = self._lookup(target_keys, specific_lookup_keys, "specific keys")
            self._specific_index_mask = specific >= 0
            self._specific_indices = np.where(self._specific_index_mask, specific, 0).astype(np.int64)
        else:
            self._specific_index_mask = np.zeros(len(target_keys), dtype=bool)
            self._specific_indices = np.zeros(len(target_keys), dtype=np.int64)

    def apply(self, fallback_values: np.ndarray, specific_values: np.ndarray) -> np.ndarray:
        assert len(fallback_values) > self._fallback_indices.max()
        result = fallback_values[self._fallback_indices]
        if self._specific_index_mask.any():
            chosen = self._specific_indices[self._specific_index_mask]
            assert len(specific_values) > chosen.max()
            result[self._specific_index_mask] = specific_values[chosen]
        return result


class host_index_builder(_IndexBuilderBase):
    """``IndexBuilder`` in NumPy.  A fallback key that is not in its lookup table raises ``ValueError`` (the reference
    turns NaN into an int64 there); a lookup key that occurs twice raises ``ValueError`` as pandas does."""

    _lookup = staticmethod(host_lookup)


def _rt_sort_values(rt):
    with np.errstate(invalid="ignore"):
        return rt + rt.dtype.type(0)  # -0.0 -> +0.0


def host_aggregate_key(key, rt, pg_notnull, sel):
    """``groupby(key).agg(median rt, first pg)`` over the rows ``sel``: ``(distinct keys ascending, median, the row of
    the first non-null pg or -1, segment starts, rows in (key, rt) order)``."""
    k, r = key[sel], _rt_sort_values(rt[sel])
    order = np.lexsort((r, k))  # NaN last inside its group
    ks, rs, rows = k[order], r[order], sel[order]
    head = np.ones(len(ks), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    starts = np.flatnonzero(head)
    if len(starts) == 0:
        return ks[:0], rs[:0], np.zeros(0, np.int64), starts, rows
    count = np.diff(np.append(starts, len(ks)))
    m = count - np.add.reduceat(np.isnan(rs).astype(np.int64), starts)
    has = m > 0
    lo, hi = starts + np.maximum(m - 1, 0) // 2, starts + m // 2
    a, b = rs[lo].astype(np.float64), rs[np.minimum(hi, len(rs) - 1)].astype(np.float64)
    med = np.where(has, np.where(m % 2 == 1, a, (a + b) / 2.0), np.nan).astype(rt.dtype)
    big = np.iinfo(np.int64).max
    first = np.minimum.reduceat(np.where(pg_notnull[rows], rows, big), starts)
    return ks[starts], med, np.where(first == big, -1, first), starts, rows


def host_aggregate(psm: dict, fdr: float, keep_decoys: bool) -> dict:
    """The PSM side: the two aggregate tables and the elution groups that passed (ascending)."""
    with np.errstate(invalid="ignore"):
        sel = np.flatnonzero(psm["qval"] <= fdr)
    by_group = host_aggregate_key(psm["eg"], psm["rt"], psm["pg_notnull"], sel)
    by_hash = host_aggregate_key(psm["hash"], psm["rt"], psm["pg_notnull"], sel)
    groups = by_group[0]
    if not keep_decoys and len(groups):
        starts, rows = by_group[3], by_group[4]
        groups = groups[np.maximum.reduceat((np.asarray(psm["decoy"])[rows] == 0).astype(np.int8), starts) > 0]
    return dict(by_group=by_group[:3], by_hash=by_hash[:3], groups=groups, n_passed=len(sel))


def host_filter(eg, start, stop, matrices, groups):
    """The library side: ``(kept rows, new start, new stop, gathered matrices)``."""
    kept = np.flatnonzero(np.isin(eg, groups))
    new_start, new_stop, mats = host_drop_unused(np.asarray(start)[kept], np.asarray(stop)[kept], matrices)
    return kept, new_start, new_stop, mats


def host_build_mbr_library(psm_df: pd.DataFrame, base_library, fdr: float = 0.01, keep_decoys: bool = False,
                           decoy_generator=None, rehash=None) -> ConsensusLibrary:
    """``MbrLibraryBuilder.forward`` in NumPy."""
    _check_builder(keep_decoys, decoy_generator, rehash)
    t0 = time.perf_counter()
    psm = _psm_parts(psm_df, keep_decoys)
    df, names, columns, mats = _library_parts(base_library)
    agg = host_aggregate(psm, fdr, keep_decoys)
    t1 = time.perf_counter()
    kept, start, stop, mats = host_filter(df["elution_group_idx"].to_numpy(), df["frag_start_idx"].to_numpy(),
                                          df["frag_stop_idx"].to_numpy(), mats, agg["groups"])
    frames = {n: pd.DataFrame(m, columns=columns) for n, m in zip(names, mats)}
    lib = _kept_library(df, kept, start, stop, names, columns, frames)
    t2 = time.perf_counter()
    lib = _decoys(lib, keep_decoys, decoy_generator, rehash)
    t3 = time.perf_counter()
    out = lib._precursor_df
    builder = host_index_builder(out["mod_seq_charge_hash"].to_numpy(), out["elution_group_idx"].to_numpy(),
                                 agg["by_group"][0], agg["by_hash"][0])
    rt = builder.apply(agg["by_group"][1], agg["by_hash"][1]) if len(out) else agg["by_group"][1][:0]
    row = builder.apply(agg["by_group"][2], agg["by_hash"][2]) if len(out) else np.zeros(0, np.int64)
    _write_columns(lib, rt, row, psm["pg"])
    t4 = time.perf_counter()
    last_timing.update(host_aggregate_s=t1 - t0, host_filter_s=t2 - t1, host_decoys_s=t3 - t2, host_assign_s=t4 - t3,
                       host_total_s=t4 - t0)
    return lib


# --------------------------------------------------------------------------------------------
# the device path
# --------------------------------------------------------------------------------------------
def _context(device):
    from alphadia_amd import runtime

    return runtime.get_context(device)


class HipIndexBuilder(_IndexBuilderBase):
    """``IndexBuilder`` with the indices computed on the device (``adh_mbr_index``: the lookup keys sorted with their
    positions, a binary search per target); ``apply`` is the reference's host take and works for object arrays.

    A lookup key that occurs twice raises ``ValueError`` as pandas' ``reindex`` does.  A fallback key that is not in
    its lookup table raises ``ValueError``, where the reference turns NaN into an int64 and indexes with it."""

    def __init__(self, target_keys, target_fallback_keys, fallback_lookup_keys, specific_lookup_keys,
                 device: int | None = None) -> None:
        session = _context(device).mbr_library()

        def lookup(targets, keys, what):
            t, k = _key_pair(targets, keys, what)
            index, duplicate = session.index(t, k)
            if duplicate:
                raise ValueError("cannot reindex on an axis with duplicate labels")
            return index

        self._lookup = lookup
        try:
            super().__init__(target_keys, target_fallback_keys, fallback_lookup_keys, specific_lookup_keys)
        finally:
            del self._lookup
            session.close()


class HipMbrLibraryBuilder:
    """``MbrLibraryBuilder`` on the GPU.  ``forward(psm_df, base_library)`` takes the combined precursor table
    (``qval``, ``decoy``, ``elution_group_idx``, ``mod_seq_charge_hash``, ``rt_observed``, ``pg``) and a library object
    (``_precursor_df`` / ``precursor_df`` with ``elution_group_idx``, ``mod_seq_charge_hash``, ``frag_start_idx``,
    ``frag_stop_idx``; float32 dense frames) and returns the MBR library with ``rt``, ``genes`` and ``proteins``
    written; ``base_library`` is not modified.

    With ``keep_decoys=True`` the caller supplies the reference's ``DecoyGenerator(decoy_type="diann")`` and
    ``hash_precursor_df`` as ``decoy_generator`` and ``rehash``; they run on the host between the filter and the
    assignment, and a ``ValueError`` says so when they are missing.

    ``gather``: "device" uploads the dense matrices and gathers the kept rows in HBM; "host" takes only the row map
    from the device and gathers with NumPy (tools/bench_mbr_library.py measures both).

    Raises ``ValueError`` when no library precursor is kept (the reference: the maximum of an empty index) and when a
    kept precursor's elution group is in neither aggregate table (the reference: ``NaN.astype(int64)`` as an index)."""

    def __init__(self, fdr: float = 0.01, keep_decoys: bool = False, decoy_generator=None, rehash=None,
                 gather: str = "device", device: int | None = None) -> None:
        _check_builder(keep_decoys, decoy_generator, rehash)
        if gather not in ("device", "host"):
            raise ValueError(f"MBR library: gather is 'device' or 'host', not {gather!r}")
        self.fdr = fdr
        self.keep_decoys = keep_decoys
        self._decoy_generator, self._rehash = decoy_generator, rehash
        self._gather = gather
        self._device = device
        self._session = None

    def __call__(self, psm_df: pd.DataFrame, base_library):
        return self.forward(psm_df, base_library)

    def close(self) -> None:
        if self._session is not None:
            self._session.close()
            self._session = None

    def forward(self, psm_df: pd.DataFrame, base_library) -> ConsensusLibrary:
        from alphadia_amd import runtime

        t0 = time.perf_counter()
        psm = _psm_parts(psm_df, self.keep_decoys, runtime.notnull_objects)  # (pd.notna costs 80 ns a row)
        df, names, columns, mats = _library_parts(base_library)
        if self._session is None:
            self._session = _context(self._device).mbr_library()
        s = self._session
        s.aggregate(psm["qval"], psm["decoy"], psm["eg"], psm["hash"], psm["rt"], psm["pg_notnull"], self.fdr,
                    self.keep_decoys)
        t1 = time.perf_counter()
        on_device = self._gather == "device"
        kept, start, stop, src = s.filter(df["elution_group_idx"].to_numpy(), df["frag_start_idx"].to_numpy(),
                                          df["frag_stop_idx"].to_numpy(), len(mats[0]), mats if on_device else None,
                                          source_rows=not on_device)
        gathered = [s.matrix(m) if on_device else mats[m][src] for m in range(len(names))]
        frames = {n: pd.DataFrame(m, columns=columns) for n, m in zip(names, gathered)}
        lib = _kept_library(df, kept, start, stop, names, columns, frames)
        t2 = time.perf_counter()
        lib = _decoys(lib, self.keep_decoys, self._decoy_generator, self._rehash)
        t3 = time.perf_counter()
        out = lib._precursor_df
        rt, row, missing = s.assign(out["elution_group_idx"].to_numpy(), out["mod_seq_charge_hash"].to_numpy())
        if missing:
            raise ValueError(f"MBR library: {missing} kept precursors have an elution group that no passing PSM has")
        _write_columns(lib, rt, row, psm["pg"])
        t4 = time.perf_counter()
        last_timing.update(aggregate_s=t1 - t0, filter_s=t2 - t1, decoys_s=t3 - t2, assign_s=t4 - t3, total_s=t4 - t0,
                           n_passed=s.n_passed, n_kept=len(kept), n_kept_rows=len(gathered[0]), **s.stats())
        return lib
