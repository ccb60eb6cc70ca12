"""Golden vectors of the cross-run fragment quantity matrices, produced by RUNNING THE REFERENCE's
``FragmentQuantLoader.accumulate`` (alphadia/outputtransform/quantification/fragment_accumulator.py:51-101) and
``QuantBuilder.filter_frag_df`` (quant_builder.py:132-182) in the build container:

    python tests/golden/make_golden_quant.py

TEST INFRASTRUCTURE, same rules as make_golden.py: the reference is imported from /root/reference with stubs for
the third-party modules that are not installed here (numba through ref_shim, directlfq, quantselect, alphabase -
none of them is on the path these two calls take), fed seeded synthetic frag tables, and inputs + outputs are
stored in ``tests/golden/quant.npz``.

NumPy 2 caveat: the frag tables hold ``number``, ``type``, ``charge`` and ``loss_type`` as uint8
(search/scoring/output.py:39-42) and ``_ion_hash`` shifts them left by up to 56 bits.  Numba types that shift in
int64; plain NumPy 2 keeps ``uint8 << 32`` in uint8, which collapses every ion key to its precursor and turns each
outer merge into a cartesian product.  This script therefore casts those four columns to int64 before it hands the
tables to the reference; the stored inputs keep the uint8 columns the search writes.

Per case ``<c>``:

    <c>/run<r>/<column>      the input frag table of run r (precursor_idx u32, number / type / charge / loss_type u8,
                             intensity / correlation f32)
    <c>/psm/<column>         the PSM table (precursor_idx, pg as text, mod_seq_hash, mod_seq_charge_hash)
    <c>/acc/<q>/<column>     the reference's accumulated frame of quantity q, column by column
    <c>/filt<k>/total, rank  quality_df["total"] / ["rank"] after filter call k
    <c>/filt<k>/keep         the index labels of the rows the call returned
    <c>/meta                 JSON: run names, column order and dtype of every accumulated frame, the filter calls
                             (group column, top_n, min_correlation) in order
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


for _name in ("alphabase", "alphabase.peptide", "alphabase.peptide.precursor", "directlfq", "directlfq.config",
              "directlfq.normalization", "directlfq.protein_intensity_estimation", "directlfq.utils", "quantselect"):
    _stub(_name)
_stub("quantselect.output", run_quantselect=None)

from alphadia.outputtransform.quantification.fragment_accumulator import FragmentQuantLoader  # noqa: E402
from alphadia.outputtransform.quantification.quant_builder import QuantBuilder  # noqa: E402

GROUPS = ("pg", "mod_seq_hash", "mod_seq_charge_hash")


def _psm(rng, n_prec: int, drop: float):
    """PSM table of precursors 0..n_prec-1 without a `drop` fraction (their fragment rows leave); three charge states
    share a mod_seq_hash, two sequences a protein group; every tenth precursor has a second PSM row."""
    keep = np.sort(rng.permutation(n_prec)[: int(round(n_prec * (1 - drop)))]).astype(np.uint32)
    seq = keep // 3
    pg = np.array([f"P{int(s // 2):05d};P{int(s // 2) + 7:05d}" for s in seq], dtype=object)
    msh = (seq.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x1234)
    msch = msh + keep.astype(np.uint64) % np.uint64(3)
    df = pd.DataFrame({"precursor_idx": keep, "pg": pg, "mod_seq_hash": msh, "mod_seq_charge_hash": msch,
                       "decoy": np.zeros(len(keep), dtype=np.int64)})
    if n_prec % 2:  # (an int64 precursor_idx in the PSM table of some cases)
        df["precursor_idx"] = df["precursor_idx"].astype(np.int64)
    extra = df.iloc[::10].copy()
    return pd.concat([df, extra], ignore_index=True).sample(frac=1.0, random_state=int(rng.integers(1 << 30)))


def _frag(rng, n_prec: int, n_frag, present: float, nan_frac: float, ties: bool, exact: float | None):
    """One run's frag table: n_frag fragments per precursor (an int or an array), a `present` fraction of the
    precursors observed, rows in a random order."""
    rows = []
    for p in range(n_prec):
        if rng.random() > present:
            continue
        k = int(n_frag[p]) if np.ndim(n_frag) else int(n_frag)
        number = np.arange(1, k + 1) // 2 + 1
        ftype = (np.arange(k) % 2) * 3 + 98
        charge = 1 + (np.arange(k) % 3 == 2)
        loss = np.where(np.arange(k) % 5 == 4, 18, 0)
        rows.append(np.stack([np.full(k, p), number, ftype, charge, loss], axis=1))
    t = np.concatenate(rows).astype(np.int64)
    t = t[rng.permutation(len(t))]
    n = len(t)
    corr = rng.uniform(0.0, 1.0, n).astype(np.float32)
    if ties:  # a few totals tied inside their precursor's groups: quarter steps, exact in float32 sums
        corr = np.where(rng.random(n) < 0.3, np.float32(0.25) * rng.integers(0, 4, n), corr).astype(np.float32)
    if exact is not None:  # precursor 0's fragments at exactly min_correlation in every run
        corr[t[:, 0] == 0] = np.float32(exact)
    corr[rng.random(n) < nan_frac] = np.nan
    inten = rng.lognormal(10.0, 1.5, n).astype(np.float32)
    inten[rng.random(n) < nan_frac] = np.nan
    return pd.DataFrame({
        "precursor_idx": t[:, 0].astype(np.uint32), "number": t[:, 1].astype(np.uint8),
        "type": t[:, 2].astype(np.uint8), "charge": t[:, 3].astype(np.uint8), "loss_type": t[:, 4].astype(np.uint8),
        "intensity": inten, "correlation": corr,
    })


def _for_reference(df: pd.DataFrame) -> pd.DataFrame:
    out = df.copy()
    for c in ("number", "type", "charge", "loss_type"):
        out[c] = out[c].astype(np.int64)
    return out


# name: (seed, runs, precursors, fragments per precursor, present fraction, NaN fraction, PSM drop, ties, exact
#        total, duplicate key, filter calls)
CASES = {
    "one_run": (1, 1, 40, 8, 1.0, 0.1, 0.2, True, None, False, [("pg", 3, 0.5), ("mod_seq_hash", 2, 0.7),
                                                                ("mod_seq_charge_hash", 3, 0.5)]),
    "two_runs": (2, 2, 60, 6, 0.8, 0.1, 0.15, True, 0.5, False, [("pg", 3, 0.5), ("mod_seq_hash", 3, 0.5),
                                                                 ("mod_seq_charge_hash", 3, 0.5)]),
    "five_runs": (3, 5, 90, "mixed", 0.7, 0.05, 0.1, True, 0.5, False, [("mod_seq_charge_hash", 3, 0.5),
                                                                        ("mod_seq_hash", 3, 0.5), ("pg", 3, 0.5),
                                                                        ("mod_seq_charge_hash", 1, 0.3)]),
    "twelve_runs": (5, 12, 50, 6, 0.75, 0.05, 0.1, True, 0.5, False, [("mod_seq_charge_hash", 3, 0.5),
                                                                      ("pg", 2, 0.5), ("mod_seq_hash", 3, 0.45)]),
    "dup_key": (4, 3, 31, 5, 0.9, 0.0, 0.1, False, None, True, [("pg", 3, 0.5), ("mod_seq_hash", 2, 0.5),
                                                                ("mod_seq_charge_hash", 3, 0.5)]),
}


def run_case(name, spec, out, meta_all):
    seed, n_runs, n_prec, n_frag, present, nan_frac, drop, ties, exact, dup, calls = spec
    rng = np.random.default_rng(seed)
    if n_frag == "mixed":  # exactly top_n = 3 fragments for every seventh precursor, 2..12 for the others
        n_frag = np.where(np.arange(n_prec) % 7 == 0, 3, rng.integers(2, 13, n_prec))
    psm = _psm(rng, n_prec, drop)
    runs = []
    for r in range(n_runs):
        f = _frag(rng, n_prec, n_frag, present, nan_frac, ties, exact)
        if dup and r == 1:  # one fragment row twice in the second run
            f = pd.concat([f, f.iloc[[3]]], ignore_index=True)
        runs.append((f"run_{r:02d}_{name}", f))
    for r, (_, f) in enumerate(runs):
        for c in f.columns:
            out[f"{name}/run{r}/{c}"] = f[c].values
    for c in psm.columns:
        v = psm[c].values
        out[f"{name}/psm/{c}"] = v.astype(str) if v.dtype == object else v

    loader = FragmentQuantLoader(psm[psm["decoy"] == 0], columns=["intensity", "correlation"])
    acc = loader.accumulate(iter([(rn, _for_reference(f)) for rn, f in runs]))
    meta = dict(runs=[rn for rn, _ in runs], frames={}, calls=[list(c) for c in calls])
    for q, df in acc.items():
        meta["frames"][q] = dict(columns=list(df.columns), dtypes=[str(t) for t in df.dtypes], n=len(df),
                                 index_is_range=bool(df.index.equals(pd.RangeIndex(len(df)))))
        for c in df.columns:
            v = df[c].values
            out[f"{name}/acc/{q}/{c}"] = v.astype(str) if v.dtype == object else v
    builder = QuantBuilder(psm[psm["decoy"] == 0])
    for k, (group, top_n, min_corr) in enumerate(calls):
        fi, fq = builder.filter_frag_df(acc["intensity"], acc["correlation"], min_correlation=min_corr, top_n=top_n,
                                        group_column=group)
        assert fi.index.equals(fq.index)
        out[f"{name}/filt{k}/total"] = acc["correlation"]["total"].values
        out[f"{name}/filt{k}/rank"] = acc["correlation"]["rank"].values
        out[f"{name}/filt{k}/keep"] = fq.index.values.astype(np.int64)
    meta["quality_columns_after"] = list(acc["correlation"].columns)
    meta["quality_dtypes_after"] = [str(t) for t in acc["correlation"].dtypes]
    out[f"{name}/meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    meta_all[name] = (n_runs, meta["frames"]["intensity"]["n"])


def main():
    out: dict[str, np.ndarray] = {}
    summary = {}
    for name, spec in CASES.items():
        run_case(name, spec, out, summary)
    path = os.path.join(OUT_DIR, "quant.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v for k, v in summary.items()}, f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
