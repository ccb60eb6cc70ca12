"""Protein inference: ``alphadia_amd.grouping.perform_grouping`` host -> host on seeded synthetic precursor tables,
split into string preparation, the device stages (HIP-event times) and string building, beside the host restatement
``host_perform_grouping`` on the same box.

    python tools/bench_protein_inference.py [--out profiles/protein_inference_bench.json]

Tables (tests/grouping_golden.py): cohorts of 20 000 and 100 000 ids per decoy class with six precursors per id, 30 %
of them shared inside protein families, both classes; and one table whose only component holds 20 000 ids.
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


def tables():
    import grouping_golden as G

    yield "cohort_20000", G.cohort(20_000, 120_000, seed=7)
    yield "cohort_100000", G.cohort(100_000, 600_000, seed=8)
    yield "one_component_20000", G.giant_component(20_000, seed=9)


def timed(fn, df, **mode):
    from alphadia_amd import grouping as PG

    frame = df.copy()
    t0 = time.perf_counter()
    out = fn(frame, **mode)
    total = time.perf_counter() - t0
    t = dict(PG.last_timing)
    rec = dict(total_s=round(total, 4), prepare_s=round(t["prepare_s"], 4), solve_s=round(t["solve_s"], 4),
               build_s=round(t["build_s"], 4))
    for k in ("label_ms", "cover_ms", "filter_ms"):
        if k in t:
            rec[k] = round(t[k], 3)
    for k in ("components", "large_components", "label_rounds", "patterns", "ids", "edges"):
        if k in t:
            rec[k] = int(t[k])
    return rec, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import grouping_golden as G
    from alphadia_amd import grouping as PG

    timed(PG.perform_grouping, G.cohort(500, 3000, seed=1), group=True)  # warm-up: context, kernels, allocator
    out = dict(note="host -> host seconds; prepare_s: duplicates, decoy classes, patterns, id codes, edges and ranks; "
                    "solve_s: upload, kernels, copy back (label_ms / cover_ms / filter_ms: HIP-event times inside it); "
                    "build_s: output strings per pattern and the left merge; host: host_perform_grouping, same box",
               results={})
    for name, df in tables():
        res = dict(rows=len(df), unique_precursors=int(df["precursor_idx"].nunique()))
        for label, mode in (("heuristic", dict(group=True)),
                            ("maximum_parsimony", dict(group=False, return_parsimony_groups=True))):
            dev = [timed(PG.perform_grouping, df, **mode) for _ in range(a.repeat)]
            best = min(dev, key=lambda d: d[0]["total_s"])
            host, host_out = timed(PG.host_perform_grouping, df, **mode)
            same = bool(best[1].equals(host_out))
            res[label] = dict(device=best[0], device_all_total_s=[d[0]["total_s"] for d in dev], host=host,
                              equal_to_host=same)
        out["results"][name] = res
        print(json.dumps({name: res}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
