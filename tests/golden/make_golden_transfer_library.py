"""Golden vectors of the transfer-learning library, produced by RUNNING THE REFERENCE's
``TransferLearningAccumulator.update`` / ``post_process``, ``ms2_quality_control``, ``normalize_rt_max`` and
``normalize_rt_delta_max`` (alphadia/outputtransform/outputaccumulator.py:272-540) in the build container:

    python tests/golden/make_golden_transfer_library.py

TEST INFRASTRUCTURE, same rules as make_golden_quant.py: the reference is imported from /root/reference with stubs
for the third-party modules that are not installed here (numba through ref_shim, alphabase), fed seeded synthetic
libraries, and inputs + outputs are stored in ``tests/golden/transfer_library.npz``.

alphabase's ``SpecLibBase`` is not installed.  ``DuckLibrary`` below stands in for it: it has the attributes the
reference functions touch, and its ``append``, ``remove_unused_fragments``, ``hash_precursor_df`` and
``available_dense_fragment_dfs`` are written here, not taken from alphabase: ``append`` shifts the new run's
``frag_start_idx`` / ``frag_stop_idx`` behind the consensus' dense rows and concatenates with a fresh index;
``remove_unused_fragments`` keeps the blocks of the remaining precursors in the order of their old start, one block
per precursor, renumbers them by a running sum of their lengths and resets the index; ``hash_precursor_df`` leaves
the ``mod_seq_hash`` the run came with.  The sort, the top-k selection, the normalisations and the quality control are
the reference's own code; what happens to the dense rows of dropped precursors is pinned to this stand-in.

Per case ``<c>``, frames are stored column by column under ``<c>/<frame>/<column>`` with ``<c>/<frame>/__columns__``
(JSON: names and dtypes in order):

    kind "update":  run<r>/precursor, run<r>/<dense name>        the input runs
                    after<r>/precursor, after<r>/<dense name>    the consensus after update r
                    post/precursor, post/<dense name>            after post_process (case "chain" only)
    kind "qc":      in/precursor, in/intensity, in/correlation; out/precursor (use_for_ms2), out/intensity
    kind "rt":      in/precursor; out_max/precursor; out_delta/precursor (when rt_calibrated is there)
    <c>/meta        JSON: kind and parameters
"""

from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402

ref_shim.install()


def _stub(name: str, **attrs) -> types.ModuleType:
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, mod)
    return mod


_stub("alphabase")
_stub("alphabase.spectral_library")
_stub("alphabase.spectral_library.base", SpecLibBase=object)
_stub("alphabase.spectral_library.flat", SpecLibFlat=object)

from alphadia.outputtransform import outputaccumulator as REF  # noqa: E402

F32 = np.float32
DENSE3 = ("_fragment_mz_df", "_fragment_intensity_df", "_fragment_correlation_df")
DENSE2 = ("_fragment_intensity_df", "_fragment_correlation_df")


class DuckLibrary:
    """Stands in for alphabase's SpecLibBase (see the module docstring)."""

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

    def hash_precursor_df(self):
        assert "mod_seq_hash" in self._precursor_df.columns

    def append(self, other, dfs_to_append):
        assert dfs_to_append == ["_precursor_df", *self._dense] and other._dense == self._dense
        n_rows = len(getattr(self, self._dense[0]))
        new = other._precursor_df.copy()
        new["frag_start_idx"] += n_rows
        new["frag_stop_idx"] += n_rows
        self._precursor_df = pd.concat([self._precursor_df, new], ignore_index=True)
        for name in self._dense:
            setattr(self, name, pd.concat([getattr(self, name), getattr(other, name)], ignore_index=True))

    def remove_unused_fragments(self):
        df = self._precursor_df.reset_index(drop=True)
        start, stop = df["frag_start_idx"].to_numpy(), df["frag_stop_idx"].to_numpy()
        rows, cursor = [], 0
        new_start, new_stop = start.copy(), stop.copy()
        for i in np.argsort(start, kind="stable"):
            rows.extend(range(int(start[i]), int(stop[i])))
            new_start[i], new_stop[i] = cursor, cursor + (stop[i] - start[i])
            cursor = int(new_stop[i])
        df["frag_start_idx"], df["frag_stop_idx"] = new_start, new_stop
        self._precursor_df = df
        take = np.asarray(rows, dtype=np.int64)
        for name in self._dense:
            setattr(self, name, getattr(self, name).iloc[take].reset_index(drop=True))


def put_frame(out, prefix: str, df: pd.DataFrame):
    cols = []
    for c in df.columns:
        v = df[c].to_numpy()
        cols.append([str(c), str(df[c].dtype)])
        out[f"{prefix}/{c}"] = v.astype(str) if v.dtype == object else v.copy()  # (the reference writes in place)
    out[f"{prefix}/__columns__"] = np.frombuffer(json.dumps(cols).encode(), dtype=np.uint8)


def put_library(out, prefix: str, lib: DuckLibrary):
    put_frame(out, f"{prefix}/precursor", lib.precursor_df.reset_index(drop=True))
    for name in lib.available_dense_fragment_dfs():
        put_frame(out, f"{prefix}/{name}", getattr(lib, name).reset_index(drop=True))


def put_meta(out, case: str, **meta):
    out[f"{case}/meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)


# --------------------------------------------------------------------------------------------
# quality control
# --------------------------------------------------------------------------------------------
def _qc_block(rng, masked: int, n_columns: int, spare_rows: int):
    """One block with `masked` cells of positive intensity at random places and distinct correlations."""
    rows = -(-masked // n_columns) + spare_rows
    cells = rows * n_columns
    inten = np.zeros(cells, dtype=F32)
    corr = rng.uniform(-0.2, 1.0, cells).astype(F32)
    where = rng.permutation(cells)[:masked]
    inten[where] = rng.lognormal(8.0, 1.5, masked).astype(F32)
    return inten, corr, where


def _plant_median(rng, corr, where, median):
    """Rewrites the masked correlations: their median is exactly `median`, with ties around the middle."""
    n = len(where)
    below, above = (n - 1) // 2, n - 1 - (n - 1) // 2
    lo = np.sort(rng.uniform(0.0, float(median) * 0.98, below).astype(F32))
    hi = np.sort(rng.uniform(float(median) * 1.02, 1.0, above).astype(F32))
    if n % 2 == 0:
        hi[0] = median  # both middle values
    if below > 1:
        lo[-1] = lo[-2]  # a tie just below the middle
    corr[where] = rng.permutation(np.concatenate([lo, [median], hi]).astype(F32))


def case_qc_sizes(out):
    rng = np.random.default_rng(11)
    cutoff, ratio, C = 0.6, 0.9, 4
    counts = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600]
    counts += [int(x) for x in rng.integers(1, 60, 36)]
    blocks = []
    for k, m in enumerate(counts):
        inten, corr, where = _qc_block(rng, m, C, spare_rows=int(rng.integers(0, 3)) + (m == 0))
        if m >= 3 and k % 3 == 0:  # a median exactly at float32(cutoff)
            _plant_median(rng, corr, where, F32(cutoff))
        elif m >= 3 and k % 3 == 1:  # quarter-step correlations: ties everywhere, also around the middle
            corr[where] = (F32(0.25) * rng.integers(0, 5, m)).astype(F32)
        blocks.append([inten, corr, where])
    # correlations exactly at median * ratio, at a masked cell below the middle and at a cell of zero intensity
    for inten, corr, where in blocks:
        m = len(where)
        if m < 5:
            continue
        median = np.median(corr[where])
        thr = F32(median * F32(ratio))
        lowest = where[np.argmin(corr[where])]
        if median > 0 and corr[lowest] < thr < np.sort(corr[where])[(m - 1) // 2]:
            corr[lowest] = thr
            assert np.median(corr[where]) == median
        free = np.flatnonzero(inten == 0)
        if len(free):
            corr[free[0]] = thr
    start, stop, cursor = [], [], 0
    order = rng.permutation(len(blocks) + 1)  # (one empty block: start == stop)
    rows_of = [len(b[0]) // C for b in blocks] + [0]
    first = {}
    for b in range(len(rows_of)):
        first[b] = cursor
        cursor += rows_of[b]
    for b in order:
        start.append(first[b])
        stop.append(first[b] + rows_of[b])
    inten = np.concatenate([b[0] for b in blocks]).reshape(-1, C)
    corr = np.concatenate([b[1] for b in blocks]).reshape(-1, C)
    _run_qc(out, "qc_sizes", start, stop, inten, corr, cutoff, ratio)


def case_qc_special(out):
    rng = np.random.default_rng(12)
    cutoff, ratio, C = 0.6, 0.9, 4
    blocks = []
    for kind in ("nan_corr_masked", "nan_corr_unmasked", "nan_intensity", "negative_intensity", "all_zero_negative_corr",
                 "plain", "plain"):
        inten, corr, where = _qc_block(rng, 9, C, spare_rows=1)
        free = np.flatnonzero(inten == 0)
        if kind == "nan_corr_masked":
            corr[where[2]] = np.nan
        elif kind == "nan_corr_unmasked":
            corr[free[0]] = np.nan
        elif kind == "nan_intensity":
            inten[free[0]] = np.nan
            inten[free[1]] = np.nan
            corr[free[1]] = 0.99
        elif kind == "negative_intensity":
            inten[free[0]] = -5.0
            corr[free[0]] = 0.99
            inten[free[1]] = -7.0
            corr[free[1]] = -0.5
        elif kind == "all_zero_negative_corr":
            inten[:] = 0.0
            corr[::2] = -np.abs(corr[::2]) - F32(0.01)
            inten[3] = -1.0
            inten[4] = np.nan
        blocks.append((inten, corr))
    rows = [len(b[0]) // C for b in blocks]
    stop = np.cumsum(rows)
    inten = np.concatenate([b[0] for b in blocks]).reshape(-1, C)
    corr = np.concatenate([b[1] for b in blocks]).reshape(-1, C)
    _run_qc(out, "qc_special", stop - rows, stop, inten, corr, cutoff, ratio)


def _run_qc(out, case, start, stop, inten, corr, cutoff, ratio):
    cols = [f"c{k}" for k in range(inten.shape[1])]
    prec = pd.DataFrame({"frag_start_idx": np.asarray(start, np.int64), "frag_stop_idx": np.asarray(stop, np.int64)})
    lib = DuckLibrary(prec, {"_fragment_intensity_df": pd.DataFrame(inten.astype(F32), columns=cols),
                             "_fragment_correlation_df": pd.DataFrame(corr.astype(F32), columns=cols)})
    put_frame(out, f"{case}/in/precursor", lib.precursor_df)
    put_frame(out, f"{case}/in/intensity", lib._fragment_intensity_df)
    put_frame(out, f"{case}/in/correlation", lib._fragment_correlation_df)
    with np.errstate(invalid="ignore"):
        REF.ms2_quality_control(lib, cutoff, ratio)
    assert lib._fragment_intensity_df.dtypes.eq(np.float32).all()
    put_frame(out, f"{case}/out/precursor", lib.precursor_df)
    put_frame(out, f"{case}/out/intensity", lib._fragment_intensity_df)
    masked = [int((inten[a:b] > 0).sum()) for a, b in zip(start, stop)]
    put_meta(out, case, kind="qc", cutoff=cutoff, ratio=ratio, masked_counts=sorted(set(masked)))
    return lib


# --------------------------------------------------------------------------------------------
# update
# --------------------------------------------------------------------------------------------
def _hash(peptide: np.ndarray, signed: bool):
    h = (peptide.astype(np.uint64) + np.uint64(3)) * np.uint64(0x9E3779B97F4A7C15)
    return h.view(np.int64) if signed else h


def _run(rng, r, n_peptides, present, signed, proba_dtype, dense, C, rt: bool):
    there = rng.random(n_peptides) < present
    there[:3] = True  # the planted ties and the NaN below
    there[3] = r == 0  # a peptide seen in one run only
    there[4] = True  # and one seen in every run
    pep = np.flatnonzero(there)
    pep = pep[rng.permutation(len(pep))]
    n = len(pep)
    proba = np.where(rng.random(n) < 0.5, 0.25 * rng.integers(0, 4, n), rng.uniform(0, 1, n)).astype(proba_dtype)
    idx = (pep * 4 + rng.integers(0, 3, n)).astype(np.int64)
    if r in (0, 1) and 0 in pep:  # the same (hash, proba, precursor_idx) in two runs
        proba[pep == 0], idx[pep == 0] = 0.25, 0
    if r == 1 and 1 in pep:  # equal proba: precursor_idx decides, against the order of arrival
        proba[pep == 1], idx[pep == 1] = 0.5, 7
    if r == 2 and 1 in pep:
        proba[pep == 1], idx[pep == 1] = 0.5, 6
    if r == 2 and 2 in pep:
        proba[pep == 2] = np.nan
    length = rng.integers(2, 7, n)
    stop = np.cumsum(length)
    df = pd.DataFrame({"mod_seq_hash": _hash(pep, signed), "proba": proba, "precursor_idx": idx,
                       "frag_start_idx": (stop - length).astype(np.int64), "frag_stop_idx": stop.astype(np.int64),
                       "raw_name": np.array([f"run_{r}"] * n, dtype=object),
                       "sequence": np.array([f"PEPTIDE{p}K" for p in pep], dtype=object)})
    if rt:
        df["rt_library"] = rng.uniform(100, 3000, n).astype(F32)
        df["rt_calibrated"] = (df["rt_library"] * F32(1.02) + rng.normal(0, 5, n).astype(F32)).astype(F32)
        df["rt_observed"] = (df["rt_calibrated"] + rng.normal(0, 8, n).astype(F32)).astype(F32)
    cols = [f"f{k}" for k in range(C)]
    rows = int(stop[-1])
    frames = {}
    for name in dense:
        m = rng.uniform(0, 1, (rows, C)).astype(F32)
        if name == "_fragment_intensity_df":
            m = np.where(rng.random((rows, C)) < 0.4, 0, rng.lognormal(8, 1.5, (rows, C))).astype(F32)
        if name == "_fragment_mz_df":
            m = rng.uniform(200, 1800, (rows, C)).astype(F32)
        frames[name] = pd.DataFrame(m, columns=cols)
    return DuckLibrary(df, frames)


def case_update(out, case, seed, keep_top, signed, proba_dtype, n_runs, dense, C, rt=False, post=False):
    rng = np.random.default_rng(seed)
    acc = REF.TransferLearningAccumulator(keep_top=keep_top) if not post else REF.TransferLearningAccumulator()
    for r in range(n_runs):
        lib = _run(rng, r, 40, 0.7, signed, proba_dtype, dense, C, rt)
        put_library(out, f"{case}/run{r}", lib)
        acc.update(lib)
        put_library(out, f"{case}/after{r}", acc.consensus_speclibase)
    if post:
        with np.errstate(invalid="ignore"):
            acc.post_process()
        put_library(out, f"{case}/post", acc.consensus_speclibase)
    put_meta(out, case, kind="update", keep_top=acc._keep_top, n_runs=n_runs, dense=list(dense), post=post)
    return len(acc.consensus_speclibase.precursor_df)


# --------------------------------------------------------------------------------------------
# RT normalisation
# --------------------------------------------------------------------------------------------
def case_rt(out, case, seed, dtypes, nan_row, calibrated=True):
    rng = np.random.default_rng(seed)
    n = 300
    lib_rt = rng.uniform(100, 3000, n)
    cal = lib_rt * 1.02 + rng.normal(0, 5, n)
    obs = cal + rng.normal(0, 8, n)
    df = pd.DataFrame({"rt_observed": obs.astype(dtypes[0]), "rt_library": lib_rt.astype(dtypes[2])})
    if calibrated:
        df["rt_calibrated"] = cal.astype(dtypes[1])
    put_frame(out, f"{case}/in/precursor", df)
    frames = {}
    for which, rows in (("plain", None), ("nan", nan_row)):
        d = df.copy()
        if rows is not None:
            d.loc[rows, "rt_observed"] = np.nan
        a = REF.normalize_rt_max(DuckLibrary(d.copy(), {})).precursor_df
        frames[f"max_{which}"] = a[["rt_norm"]]
        if calibrated:
            with np.errstate(invalid="ignore"):
                b = REF.normalize_rt_delta_max(DuckLibrary(d.copy(), {})).precursor_df
            frames[f"delta_{which}"] = b[["rt_norm"]]
    for k, f in frames.items():
        put_frame(out, f"{case}/out_{k}/precursor", f)
    put_meta(out, case, kind="rt", nan_row=nan_row, calibrated=calibrated, outputs=sorted(frames))


def main():
    out: dict[str, np.ndarray] = {}
    case_qc_sizes(out)
    case_qc_special(out)
    kept = {}
    kept["topk_k1"] = case_update(out, "topk_k1", 21, 1, False, np.float32, 5, DENSE2, 3)
    kept["topk_k2"] = case_update(out, "topk_k2", 22, 2, True, np.float64, 5, DENSE2, 3)
    kept["topk_k3"] = case_update(out, "topk_k3", 23, 3, False, np.float64, 5, DENSE2, 3)
    kept["topk_k5"] = case_update(out, "topk_k5", 24, 5, True, np.float32, 5, DENSE2, 3)
    kept["chain"] = case_update(out, "chain", 25, 3, False, np.float32, 3, DENSE3, 4, rt=True, post=True)
    case_rt(out, "rt_f32", 31, (np.float32, np.float32, np.float32), 17)
    case_rt(out, "rt_mixed", 32, (np.float32, np.float64, np.float32), 5)
    case_rt(out, "rt_mixed_obs64", 33, (np.float64, np.float32, np.float32), 5)
    case_rt(out, "rt_no_calibrated", 34, (np.float32, np.float32, np.float32), 9, calibrated=False)
    path = os.path.join(OUT_DIR, "transfer_library.npz")
    np.savez_compressed(path, **out)
    print(path, kept, f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
