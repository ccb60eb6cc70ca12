"""Loading of tests/golden/transfer_library.npz (written by tests/golden/make_golden_transfer_library.py), the library
objects the tests feed to the accumulators, a bit-pattern frame comparison and a seeded cohort."""

from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_library.npz")
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


def frame(prefix: str) -> pd.DataFrame:
    z = _z()
    cols = json.loads(bytes(z[f"{prefix}/__columns__"]).decode())
    data = {}
    for name, dtype in cols:
        v = z[f"{prefix}/{name}"]
        data[name] = v.astype(object) if dtype == "object" else v.astype(dtype)
    return pd.DataFrame(data, columns=[c for c, _ in cols])


class Library:
    """A library object as the accumulators take it: ``precursor_df`` and dense frames under alphabase's names."""

    def __init__(self, precursor_df: pd.DataFrame, frames: dict[str, pd.DataFrame]):
        self._precursor_df = precursor_df
        self._dense = list(frames)
        for name, f in frames.items():
            setattr(self, name, f)

    @property
    def precursor_df(self):
        return self._precursor_df

    @property
    def fragment_intensity_df(self):
        return self._fragment_intensity_df

    def available_dense_fragment_dfs(self):
        return list(self._dense)


def library(prefix: str, dense) -> Library:
    return Library(frame(f"{prefix}/precursor"), {name: frame(f"{prefix}/{name}") for name in dense})


def load(case: str) -> dict:
    """kind "update": ``runs`` (fresh Library objects), ``after`` (the reference's consensus after every update) and
    ``post`` (after post_process, or None).  kind "qc": ``lib`` (input) and ``out_precursor`` / ``out_intensity``.
    kind "rt": ``precursor`` and ``out`` (output name -> the reference's rt_norm frame)."""
    m = meta(case)
    if m["kind"] == "update":
        return dict(meta=m, runs=[library(f"{case}/run{r}", m["dense"]) for r in range(m["n_runs"])],
                    after=[library(f"{case}/after{r}", m["dense"]) for r in range(m["n_runs"])],
                    post=library(f"{case}/post", m["dense"]) if m["post"] else None)
    if m["kind"] == "qc":
        lib = Library(frame(f"{case}/in/precursor"), {"_fragment_intensity_df": frame(f"{case}/in/intensity"),
                                                      "_fragment_correlation_df": frame(f"{case}/in/correlation")})
        return dict(meta=m, lib=lib, out_precursor=frame(f"{case}/out/precursor"),
                    out_intensity=frame(f"{case}/out/intensity"))
    return dict(meta=m, precursor=frame(f"{case}/in/precursor"),
                out={k: frame(f"{case}/out_{k}/precursor") for k in m["outputs"]})


def assert_frames_identical(got: pd.DataFrame, exp: pd.DataFrame) -> None:
    """Columns, column order, dtypes, length and values; floats bit for bit."""
    assert list(got.columns) == list(exp.columns), (list(got.columns), list(exp.columns))
    assert [str(t) for t in got.dtypes] == [str(t) for t in exp.dtypes], (list(got.dtypes), list(exp.dtypes))
    assert len(got) == len(exp)
    for c in exp.columns:
        a, b = np.ascontiguousarray(got[c].to_numpy()), np.ascontiguousarray(exp[c].to_numpy())
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c
        else:
            assert np.array_equal(a, b), c


def assert_libraries_identical(got, exp) -> None:
    assert list(got.available_dense_fragment_dfs()) == list(exp.available_dense_fragment_dfs())
    assert_frames_identical(got.precursor_df, exp.precursor_df)
    for name in exp.available_dense_fragment_dfs():
        assert_frames_identical(getattr(got, name), getattr(exp, name))


# --------------------------------------------------------------------------------------------
# seeded synthetic cohorts (GPU tests, benchmark)
# --------------------------------------------------------------------------------------------
DENSE = ("_fragment_mz_df", "_fragment_intensity_df", "_fragment_correlation_df")
FRAG_TYPES = ("b_z1", "b_z2", "y_z1", "y_z2")


def cohort_run(rng, r: int, n_peptides: int, present: float = 0.8, n_columns: int = 4, min_aa: int = 7,
               max_aa: int = 29, strings: bool = True) -> Library:
    """One run of a cohort: a `present` fraction of the peptides, 7 to 29 residues (len - 1 dense rows), quarter-step
    proba ties, about 40 % empty cells."""
    pep = np.flatnonzero(rng.random(n_peptides) < present)
    n = len(pep)
    n_aa = (min_aa + (pep * 7919) % (max_aa - min_aa + 1)).astype(np.int64)  # a peptide keeps its length
    length = n_aa - 1
    stop = np.cumsum(length)
    proba = np.where(rng.random(n) < 0.3, 0.25 * rng.integers(0, 4, n), rng.uniform(0, 1, n)).astype(np.float32)
    lib_rt = (100 + (pep * 104729) % 2900).astype(np.float32)
    cal = (lib_rt * np.float32(1.02) + rng.normal(0, 5, n)).astype(np.float32)
    df = pd.DataFrame({"mod_seq_hash": (pep.astype(np.uint64) + np.uint64(3)) * np.uint64(0x9E3779B97F4A7C15),
                       "proba": proba, "precursor_idx": pep.astype(np.int64) * 4 + rng.integers(0, 3, n),
                       "frag_start_idx": stop - length, "frag_stop_idx": stop, "rt_library": lib_rt,
                       "rt_calibrated": cal, "rt_observed": (cal + rng.normal(0, 8, n)).astype(np.float32)})
    if strings:
        df["raw_name"] = f"run_{r}"
    rows = int(stop[-1])
    cols = list(FRAG_TYPES[:n_columns]) if n_columns <= 4 else [f"b_z{k + 1}" for k in range(n_columns)]
    inten = rng.lognormal(8, 1.5, (rows, n_columns)).astype(np.float32)
    inten[rng.random((rows, n_columns)) < 0.4] = 0
    frames = {"_fragment_mz_df": pd.DataFrame(rng.uniform(200, 1800, (rows, n_columns)).astype(np.float32), columns=cols),
              "_fragment_intensity_df": pd.DataFrame(inten, columns=cols),
              "_fragment_correlation_df": pd.DataFrame(rng.uniform(-0.1, 1, (rows, n_columns)).astype(np.float32),
                                                       columns=cols)}
    return Library(df, frames)


def flat_tables(lib: Library, rng, decoy_fraction: float = 0.1):
    """``(psm_df, frag_df)`` that ``add_run`` turns back into `lib`: a sequence of the right length per precursor, the
    non-zero-intensity cells as flat rows in a random order, some decoy PSMs with fragments of their own, and some
    rows of a fragment type without a column."""
    df = lib.precursor_df
    n_aa = (df["frag_stop_idx"] - df["frag_start_idx"]).to_numpy() + 1
    psm = df.drop(columns=["frag_start_idx", "frag_stop_idx"]).copy()
    psm["sequence"] = ["A" * int(k) for k in n_aa]
    psm["decoy"] = 0
    mz, inten, corr = (getattr(lib, n).to_numpy() for n in DENSE)
    cols = list(lib._fragment_mz_df.columns)
    row, col = np.nonzero(inten)
    owner = np.searchsorted(df["frag_stop_idx"].to_numpy(), row, side="right")
    series = np.array([ord(c[0]) for c in cols])[col]
    charge = np.array([int(c.split("_z")[1]) for c in cols])[col]
    frag = pd.DataFrame({"precursor_idx": psm["precursor_idx"].to_numpy()[owner], "type": series.astype(np.uint8),
                         "loss_type": np.zeros(len(row), np.uint8), "charge": charge.astype(np.uint8),
                         "position": (row - df["frag_start_idx"].to_numpy()[owner]).astype(np.uint8),
                         "mz": mz[row, col], "intensity": inten[row, col], "correlation": corr[row, col]})
    n_decoy = max(int(len(psm) * decoy_fraction), 1)
    decoys = psm.iloc[:n_decoy].copy()
    decoys["decoy"] = 1
    decoys["precursor_idx"] = psm["precursor_idx"].max() + 1 + np.arange(n_decoy)
    extra = frag.iloc[: 3 * n_decoy].copy()
    extra["precursor_idx"] = decoys["precursor_idx"].to_numpy()[np.arange(len(extra)) % n_decoy]
    stray = frag.iloc[:5].copy()
    stray["type"] = np.uint8(ord("c"))  # no c column
    psm_all = pd.concat([decoys, psm], ignore_index=True)
    frag_all = pd.concat([frag, extra, stray], ignore_index=True)
    frag_all = frag_all.iloc[rng.permutation(len(frag_all))].reset_index(drop=True)
    # what add_run leaves: zero where the dense matrices had zero intensity
    keep = inten != 0
    expect = Library(df.copy(), {n: pd.DataFrame(np.where(keep, m, np.float32(0)), columns=cols)
                                 for n, m in zip(DENSE, (mz, inten, corr))})
    return psm_all, frag_all, expect
