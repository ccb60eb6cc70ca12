"""Loading of tests/golden/quant.npz (written by tests/golden/make_golden_quant.py) for the quantification tests."""

from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant.npz")


def cases() -> list[str]:
    z = np.load(PATH)
    return sorted({k.split("/")[0] for k in z.files})


def load(case: str):
    """``(runs, psm_df, frames, calls)``: the input runs as (name, frame), the PSM table, the reference's accumulated
    frames by quantity column, and per filter call ``(group, top_n, min_correlation, total, rank, keep)``."""
    z = np.load(PATH)
    meta = json.loads(bytes(z[f"{case}/meta"]).decode())
    runs = []
    for r, name in enumerate(meta["runs"]):
        cols = ["precursor_idx", "number", "type", "charge", "loss_type", "intensity", "correlation"]
        runs.append((name, pd.DataFrame({c: z[f"{case}/run{r}/{c}"] for c in cols})))
    psm = pd.DataFrame({c: z[f"{case}/psm/{c}"] for c in ["precursor_idx", "pg", "mod_seq_hash", "mod_seq_charge_hash",
                                                          "decoy"]})
    psm["pg"] = psm["pg"].astype(object)
    frames = {}
    for q, fm in meta["frames"].items():
        df = pd.DataFrame({c: z[f"{case}/acc/{q}/{c}"] for c in fm["columns"]})
        df = df.astype(dict(zip(fm["columns"], fm["dtypes"])))
        frames[q] = df
    calls = []
    for k, (group, top_n, min_corr) in enumerate(meta["calls"]):
        calls.append((group, top_n, min_corr, z[f"{case}/filt{k}/total"], z[f"{case}/filt{k}/rank"],
                      z[f"{case}/filt{k}/keep"]))
    return runs, psm, frames, calls, meta


def assert_frames_identical(got: pd.DataFrame, exp: pd.DataFrame) -> None:
    """Columns, column order, dtypes, index and values; floats bit for bit."""
    assert list(got.columns) == list(exp.columns)
    assert [str(t) for t in got.dtypes] == [str(t) for t in exp.dtypes], (list(got.dtypes), list(exp.dtypes))
    assert got.index.equals(exp.index)
    for c in exp.columns:
        a, b = got[c].to_numpy(), exp[c].to_numpy()
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c
        else:
            assert np.array_equal(a, b), c
