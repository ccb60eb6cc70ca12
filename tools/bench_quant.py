"""Cross-run fragment quantity matrices: HipFragmentQuantLoader.accumulate over in-memory frag tables plus the three
filter_frag_df calls of one quantification build (precursor, peptide, protein group), host -> host, against the host
restatement of the reference's merges (alphadia_amd.quant.host_accumulate / host_filter_frag_df) on the same box.

    python tools/bench_quant.py --runs 20 60 [--host] [--out profiles/quant_bench.json]

Synthetic cohort: 100 000 precursors, 12 fragments each, 80 % of the precursors present per run.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = ("mod_seq_charge_hash", "mod_seq_hash", "pg")


def cohort(n_runs, n_prec=100_000, n_frag=12, present=0.8, seed=0):
    rng = np.random.default_rng(seed)
    psm = pd.DataFrame({"precursor_idx": np.arange(n_prec, dtype=np.uint32)})
    psm["pg"] = np.array([f"PG{i // 6}" for i in range(n_prec)], dtype=object)
    psm["mod_seq_hash"] = (np.arange(n_prec, dtype=np.uint64) // np.uint64(3)) * np.uint64(2654435761)
    psm["mod_seq_charge_hash"] = psm["mod_seq_hash"] + np.arange(n_prec, dtype=np.uint64) % np.uint64(3)
    f = np.arange(n_frag)
    runs = []
    for r in range(n_runs):
        p = np.flatnonzero(rng.random(n_prec) < present).astype(np.uint32)
        pp, ff = np.repeat(p, n_frag), np.tile(f, len(p))
        order = rng.permutation(len(pp))
        n = len(pp)
        runs.append((f"run_{r:03d}", pd.DataFrame({
            "precursor_idx": pp[order], "number": (ff[order] // 2 + 1).astype(np.uint8),
            "type": (98 + 23 * (ff[order] % 2)).astype(np.uint8), "charge": np.ones(n, np.uint8),
            "loss_type": np.where(ff[order] % 4 == 3, 18, 0).astype(np.uint8),
            "intensity": rng.lognormal(10, 1, n).astype(np.float32), "correlation": rng.random(n, dtype=np.float32),
        })))
    return psm, runs


def run_device(psm, runs):
    from alphadia_amd import quant as Q

    t0 = time.perf_counter()
    loader = Q.HipFragmentQuantLoader(psm)
    acc = loader.accumulate(iter(runs))
    t1 = time.perf_counter()
    filt = {}
    for level in LEVELS:
        s = time.perf_counter()
        fi, _ = Q.filter_frag_df(acc["intensity"], acc["correlation"], min_correlation=0.5, top_n=3, group_column=level)
        filt[level] = dict(seconds=round(time.perf_counter() - s, 4), kept=len(fi))
    t2 = time.perf_counter()
    build_ms = loader.last_device_ms[0]
    filter_ms = Q._resident(acc["correlation"], [n for n, _ in runs]).quant.time_ms()[1]
    return dict(accumulate_s=round(t1 - t0, 4), filters_s=round(t2 - t1, 4), total_s=round(t2 - t0, 4),
                keys=len(acc["intensity"]), build_kernels_ms=round(build_ms, 3),
                last_filter_kernels_ms=round(filter_ms, 3), filters=filt)


def run_host(psm, runs):
    from alphadia_amd import quant as Q

    t0 = time.perf_counter()
    acc = Q.host_accumulate(iter(runs), psm)
    t1 = time.perf_counter()
    for level in LEVELS:
        Q.host_filter_frag_df(acc["intensity"], acc["correlation"], min_correlation=0.5, top_n=3, group_column=level)
    t2 = time.perf_counter()
    return dict(accumulate_s=round(t1 - t0, 3), filters_s=round(t2 - t1, 3), total_s=round(t2 - t0, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, nargs="+", default=[20, 60])
    ap.add_argument("--host", action="store_true", help="also time the host restatement (minutes at 60 runs)")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(cohort=dict(precursors=100_000, fragments=12, present=0.8), results={})
    psm, runs = cohort(2, n_prec=2000)
    run_device(psm, runs)  # warm-up: context, kernels, allocator
    for n in a.runs:
        psm, runs = cohort(n)
        rows = sum(len(df) for _, df in runs)
        res = dict(rows=rows)
        dev = [run_device(psm, runs) for _ in range(a.repeat)]
        res["device"] = min(dev, key=lambda d: d["total_s"])
        res["device_all_total_s"] = [d["total_s"] for d in dev]
        if a.host:
            res["host"] = run_host(psm, runs)
        out["results"][str(n)] = res
        print(json.dumps({n: res}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
