"""Loading of tests/golden/mbr_library.npz (written by tests/golden/make_golden_mbr_library.py), the library objects
the tests feed to the builders, the stand-in decoy generator and rehash of the ``keep_decoys`` case, a bit-pattern frame
comparison and a seeded cohort."""

from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mbr_library.npz")
DENSE = ("_fragment_mz_df", "_fragment_intensity_df")
_Z = None


def _z():
    global _Z
    if _Z is None:
        _Z = dict(np.load(PATH))
    return _Z


def meta(case: str) -> dict:
    return json.loads(bytes(_z()[f"{case}/meta"]).decode())


def cases(kind: str | None = None) -> list[str]:
    names = sorted({k.split("/")[0] for k in _z()})
    return [c for c in names if kind is None or meta(c)["kind"] == kind]


# --------------------------------------------------------------------------------------------
# frames in the archive: a column per entry, null masks of object columns, the index
# --------------------------------------------------------------------------------------------
def put_frame(out: dict, prefix: str, df: pd.DataFrame) -> None:
    cols = []
    for c in df.columns:
        v = df[c].to_numpy()
        cols.append([str(c), str(df[c].dtype)])
        if v.dtype == object:
            null = pd.isna(v)
            out[f"{prefix}/{c}__null"] = null
            out[f"{prefix}/{c}"] = np.where(null, "", v).astype(str)
        else:
            out[f"{prefix}/{c}"] = v.copy()
    out[f"{prefix}/__columns__"] = np.frombuffer(json.dumps(cols).encode(), dtype=np.uint8)
    out[f"{prefix}/__index__"] = df.index.to_numpy().copy()


def frame(prefix: str) -> pd.DataFrame:
    z = _z()
    cols = json.loads(bytes(z[f"{prefix}/__columns__"]).decode())
    data = {}
    for name, dtype in cols:
        v = z[f"{prefix}/{name}"]
        if dtype == "object":
            v = v.astype(object)
            v[z[f"{prefix}/{name}__null"]] = None
        else:
            v = v.astype(dtype)
        data[name] = v
    return pd.DataFrame(data, columns=[c for c, _ in cols], index=pd.Index(z[f"{prefix}/__index__"]))


class Library:
    """A library object as the builders take it: ``_precursor_df`` / ``precursor_df`` and dense frames under
    alphabase's names."""

    def __init__(self, precursor_df: pd.DataFrame, frames: dict[str, pd.DataFrame]):
        self._precursor_df = precursor_df
        self._dense = list(frames)
        for name, f in frames.items():
            setattr(self, name, f)

    @property
    def precursor_df(self):
        return self._precursor_df

    def available_dense_fragment_dfs(self):
        return list(self._dense)


def put_library(out: dict, prefix: str, lib) -> None:
    put_frame(out, f"{prefix}/precursor", lib._precursor_df)
    for name in lib.available_dense_fragment_dfs():
        put_frame(out, f"{prefix}/{name}", getattr(lib, name))


def library(prefix: str, dense) -> Library:
    return Library(frame(f"{prefix}/precursor"), {name: frame(f"{prefix}/{name}") for name in dense})


def load(case: str) -> dict:
    """kind "forward": ``psm``, ``library`` and ``out`` (the reference's MBR library) or ``raises`` (the name of the
    exception type the reference raised).  kind "index": the four key columns and the reference's ``fallback``,
    ``mask`` and ``specific`` indices, or ``raises``."""
    m = meta(case)
    z = _z()
    if m["kind"] == "forward":
        return dict(meta=m, psm=frame(f"{case}/psm"), library=library(f"{case}/library", m["dense"]),
                    out=None if m["raises"] else library(f"{case}/out", m["dense"]), raises=m["raises"])
    g = dict(meta=m, raises=m["raises"])
    for k in ("target_keys", "target_fallback_keys", "fallback_lookup_keys", "specific_lookup_keys", "fallback", "mask",
              "specific", "fallback_values", "specific_values", "applied"):
        if f"{case}/{k}" in z:
            g[k] = z[f"{case}/{k}"]
    return g


def assert_frames_identical(got: pd.DataFrame, exp: pd.DataFrame) -> None:
    """Columns, column order, dtypes, index and values; floats bit for bit, nulls of object columns alike."""
    assert list(got.columns) == list(exp.columns), (list(got.columns), list(exp.columns))
    assert [str(t) for t in got.dtypes] == [str(t) for t in exp.dtypes], (list(got.dtypes), list(exp.dtypes))
    assert len(got) == len(exp)
    assert np.array_equal(got.index.to_numpy(), exp.index.to_numpy()), "index"
    for c in exp.columns:
        a, b = np.ascontiguousarray(got[c].to_numpy()), np.ascontiguousarray(exp[c].to_numpy())
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c
        elif a.dtype == object:
            na, nb = pd.isna(a), pd.isna(b)
            assert np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]), c
        else:
            assert np.array_equal(a, b), c


def assert_libraries_identical(got, exp) -> None:
    assert list(got.available_dense_fragment_dfs()) == list(exp.available_dense_fragment_dfs())
    assert_frames_identical(got._precursor_df, exp._precursor_df)
    for name in exp.available_dense_fragment_dfs():
        assert_frames_identical(getattr(got, name), getattr(exp, name))


# --------------------------------------------------------------------------------------------
# the stand-ins of the keep_decoys case (patched into the reference module by the golden script, handed to the
# builders by the tests): they are not alphabase's decoys, only something deterministic between filter and assign
# --------------------------------------------------------------------------------------------
def standin_decoy_generator(lib):
    """One decoy per precursor: same elution group, same hash (the reference's generator leaves the target's hash),
    the reversed rows of the target's block appended to every dense frame; sorted by elution group, fresh index and
    ``precursor_idx``."""
    df = lib._precursor_df
    names = lib.available_dense_fragment_dfs()
    n_rows = len(getattr(lib, names[0]))
    start, stop = df["frag_start_idx"].to_numpy().astype(np.int64), df["frag_stop_idx"].to_numpy().astype(np.int64)
    length = stop - start
    take = np.concatenate([np.arange(b - 1, a - 1, -1) for a, b in zip(start, stop)] + [np.zeros(0, np.int64)]).astype(np.int64)
    decoys = df.copy()
    decoys["decoy"] = 1
    new_stop = n_rows + np.cumsum(length)
    decoys["frag_start_idx"] = (new_stop - length).astype(df["frag_start_idx"].dtype)
    decoys["frag_stop_idx"] = new_stop.astype(df["frag_stop_idx"].dtype)
    targets = df.copy()
    targets["decoy"] = 0
    both = pd.concat([targets, decoys], ignore_index=True)
    both = both.sort_values("elution_group_idx", kind="stable").reset_index(drop=True)
    both["precursor_idx"] = np.arange(len(both))
    lib._precursor_df = both
    for name in names:
        f = getattr(lib, name)
        setattr(lib, name, pd.concat([f, f.iloc[take]], ignore_index=True))
    return lib


def standin_rehash(precursor_df: pd.DataFrame) -> pd.DataFrame:
    """A decoy's hash moves away from its target's (wrapping uint64 arithmetic); targets keep theirs."""
    h = precursor_df["mod_seq_charge_hash"].to_numpy()
    moved = (h.view(np.uint64) + precursor_df["decoy"].to_numpy().astype(np.uint64) * np.uint64(0x51ED270B27B4F3CF))
    precursor_df["mod_seq_charge_hash"] = moved.view(h.dtype)
    return precursor_df


# --------------------------------------------------------------------------------------------
# seeded synthetic cohorts (golden script, GPU tests, benchmark)
# --------------------------------------------------------------------------------------------
def hashes(ident: np.ndarray, signed: bool) -> np.ndarray:
    h = (ident.astype(np.uint64) + np.uint64(3)) * np.uint64(0x9E3779B97F4A7C15)  # about half of them >= 2^63
    return h.view(np.int64) if signed else h


def cohort(rng, n_groups: int, psm_rows_per_group, rt_dtype=np.float32, group_dtype=np.uint32, library_group_dtype=np.int64,
           signed_hash: bool = False, n_columns: int = 4, max_block: int = 6, strings: bool = True, shuffle: bool = True,
           specials: bool = True, fail_fraction: float = 0.1, exact_groups=()):
    """``(psm_df, Library)``: ``n_groups`` elution groups of 1 to 3 precursors; group g has ``psm_rows_per_group[g]``
    PSM rows (0: never identified).  With ``specials``: tied RTs on a quarter grid, NaN RTs inside a group and as the
    whole of group 1, qval at 0.01 exactly and NaN, a null pg in the first row of every third group, group 2 seen as a
    decoy only, zero-length blocks; the last precursor of every group with three is never identified.  Every row of a group in
    ``exact_groups`` passes with a finite RT: its median is over exactly ``psm_rows_per_group[g]`` values."""
    per_group = rng.integers(1, 4, n_groups)
    group_of = np.repeat(np.arange(n_groups), per_group)
    n_prec = len(group_of)
    member = np.arange(n_prec) - np.repeat(np.cumsum(per_group) - per_group, per_group)
    length = rng.integers(0 if specials else 1, max_block + 1, n_prec)
    block_order = rng.permutation(n_prec) if shuffle else np.arange(n_prec)
    gap = rng.integers(0, 2, n_prec) if specials else np.zeros(n_prec, np.int64)  # rows no precursor uses
    stop_sorted = np.cumsum((length + gap)[block_order])
    start = np.empty(n_prec, np.int64)
    start[block_order] = stop_sorted - length[block_order]
    n_rows = int(stop_sorted[-1])
    lib = pd.DataFrame({"precursor_idx": np.arange(n_prec, dtype=np.int64),
                        "elution_group_idx": (group_of * 5 + 11).astype(library_group_dtype),
                        "mod_seq_charge_hash": hashes(np.arange(n_prec), signed_hash),
                        "charge": (member + 2).astype(np.uint8),
                        "frag_start_idx": start, "frag_stop_idx": start + length,
                        "rt": rng.uniform(0, 1, n_prec).astype(np.float32)})
    if strings:
        lib["sequence"] = np.array([f"PEPTIDE{g}K" for g in group_of], dtype=object)
        lib["proteins"] = np.array([f"LIB{g}" for g in group_of], dtype=object)
    if shuffle:
        order = rng.permutation(n_prec)
        lib = lib.iloc[order]
        lib.index = pd.Index(order * 3 + 7)
    cols = [f"f{k}" for k in range(n_columns)]
    frames = {"_fragment_mz_df": pd.DataFrame(rng.uniform(200, 1800, (n_rows, n_columns)).astype(np.float32), columns=cols),
              "_fragment_intensity_df": pd.DataFrame(rng.uniform(0, 1, (n_rows, n_columns)).astype(np.float32), columns=cols)}

    rows = np.asarray(psm_rows_per_group, dtype=np.int64)
    g = np.repeat(np.arange(n_groups), rows)
    n = len(g)
    first_prec = (np.cumsum(per_group) - per_group)[g]
    seen = np.where(per_group[g] == 3, 2, per_group[g])  # the third precursor of a group is never identified
    prec = first_prec + rng.integers(0, 3, n) % seen
    center = rng.uniform(100, 3000, n_groups)
    rt = center[g] + rng.normal(0, 4, n)
    finite_rt = rt.copy()
    qval = np.where(rng.random(n) < fail_fraction, rng.uniform(0.011, 0.5, n), rng.uniform(0, 0.0099, n))
    decoy = np.zeros(n, np.uint8)
    pg = np.array([f"PG{x};ALT{x % 7}" for x in g], dtype=object)
    if specials:
        rt = np.where(rng.random(n) < 0.5, np.round(rt * 4) / 4, rt)
        rt[rng.random(n) < 0.03] = np.nan
        rt[g == 1] = np.nan
        qval[rng.random(n) < 0.03] = 0.01
        qval[rng.random(n) < 0.02] = np.nan
        decoy[g == 2] = 1
        decoy[(g == 3) & (prec == first_prec + 1)] = 1  # a precursor of a passing group seen as a decoy only
        head = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
        for k in head[::3]:
            pg[k] = None
            qval[k] = 0.001  # the null is the first row that passes
    exact = np.isin(g, np.asarray(exact_groups, dtype=np.int64))
    with np.errstate(invalid="ignore"):
        qval[exact & ~(qval <= 0.01)] = 0.002
    rt = np.where(exact & np.isnan(rt), finite_rt, rt)
    psm = pd.DataFrame({"elution_group_idx": (g * 5 + 11).astype(group_dtype),
                        "mod_seq_charge_hash": hashes(prec, signed_hash), "decoy": decoy, "qval": qval,
                        "rt_observed": rt.astype(rt_dtype), "pg": pg,
                        "run": rng.integers(0, 20, n).astype(np.int64)})
    if shuffle:  # a group's rows far apart; the planted null pg stays the first row of its group
        key = np.where(pd.isna(pg), 0, 1 + rng.permutation(n))
        psm = psm.iloc[np.argsort(key, kind="stable")].reset_index(drop=True)
    return psm, Library(lib, frames)
