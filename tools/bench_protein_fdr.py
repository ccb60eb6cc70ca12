"""Protein-group FDR: ``alphadia_amd.protein_fdr.perform_protein_fdr`` host -> host on seeded synthetic cohorts, split
into its stages (with the HIP-event times inside them), beside the host restatement ``host_perform_protein_fdr`` on
the same box.

    python tools/bench_protein_fdr.py [--out profiles/protein_fdr_bench.json]

Tables (tests/protein_fdr_golden.py:cohort): 2 000 and 20 000 protein groups per decoy class at about 10 rows per
group over six runs, and a 60-run cohort of 20 000 groups per class at about 75 rows per group (three million rows).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the synthetic tables live with the tests

STAGES = ("prepare_s", "features_s", "scale_s", "train_s", "epoch_s", "qvalues_s", "gather_s")
DEVICE_MS = ("features_ms", "epochs_ms", "predict_ms", "gather_ms")


def tables(small: bool):
    import protein_fdr_golden as G

    yield "groups_2000", G.cohort(2_000, 10.0, n_runs=6, seed=21)
    if small:
        return
    yield "groups_20000", G.cohort(20_000, 10.0, n_runs=6, seed=22)
    yield "runs_60_groups_20000", G.cohort(20_000, 75.0, n_runs=60, seed=23)


def timed(fn, df):
    from alphadia_amd import protein_fdr as PF

    frame = df.copy()
    t0 = time.perf_counter()
    out = fn(frame)
    total = time.perf_counter() - t0
    t = dict(PF.last_timing)
    rec = dict(total_s=round(total, 4), epochs=int(t["epochs"]), groups=int(t["groups"]))
    rec.update({k: round(t[k], 5) for k in STAGES})
    rec.update({k: round(t[k], 3) for k in DEVICE_MS if k in t})
    if "epochs_ms" in t:
        rec["epoch_kernel_ms"] = round(t["epochs_ms"] / max(rec["epochs"], 1), 4)
    return rec, out, dict(PF.last_fit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="the smallest table only")
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    import protein_fdr_golden as G
    from alphadia_amd import protein_fdr as PF

    timed(PF.perform_protein_fdr, G.cohort(100, 5.0, seed=1))  # warm-up: context, kernels, allocator
    out = dict(note="host -> host seconds; prepare_s: factorising pg / sequence / run and the checks; features_s: upload, "
                    "sorts and segment kernels, copy back (features_ms: HIP-event time inside it); scale_s: split and "
                    "scaler in NumPy; train_s: all epochs and the prediction, epoch_s = train_s / epochs (epochs_ms: "
                    "HIP-event time of the epoch kernels alone, epoch_kernel_ms per epoch); qvalues_s: adh_fdr_q_values; "
                    "gather_s: the gather kernel and building the frame; host: host_perform_protein_fdr, same box",
               results={})
    for name, df in tables(a.small):
        dev = [timed(PF.perform_protein_fdr, df) for _ in range(a.repeat)]
        best = min(dev, key=lambda d: d[0]["total_s"])
        res = dict(rows=len(df), device=best[0], device_all_total_s=[d[0]["total_s"] for d in dev])
        if not a.no_host:
            host, host_out, host_fit = timed(PF.host_perform_protein_fdr, df)
            q_dev, q_host = best[1]["pg_qval"].to_numpy(), host_out["pg_qval"].to_numpy()
            res.update(host=host, same_epochs=bool(best[0]["epochs"] == host["epochs"]),
                       qvalues_equal_to_host=bool(np.array_equal(q_dev, q_host, equal_nan=True)),
                       max_rel_proba_deviation=float(np.max(np.abs(best[2]["proba"] - host_fit["proba"]) / host_fit["proba"])))
        out["results"][name] = res
        print(json.dumps({name: res}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
