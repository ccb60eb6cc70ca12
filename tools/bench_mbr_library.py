"""Match-between-runs library: ``HipMbrLibraryBuilder`` host -> host on a seeded synthetic cohort, split into its stages
(with the HIP-event times inside them), with the dense matrices gathered on the device and on the host, beside
``host_build_mbr_library`` on the same box.

    python tools/bench_mbr_library.py [--out profiles/mbr_library_bench.json]

Cohort (tests/mbr_library_golden.py:cohort): 200 000 elution groups of 1 to 3 precursors (about 400 000), blocks of 0
to 35 dense rows (about 7 M rows) x 8 columns x 2 float32 frames, about 2.8 M PSM rows (a Poisson number per group,
four groups in ten never seen), float32 RT, uint32 groups in the PSM table and int64 in the library, uint64 hashes.

The three forms run alternately, ``--repeats`` times after one untimed round at the full size; the record keeps every
time and the median.  The PCIe floor of the matrices is their bytes (all rows up, the kept rows down) over the rate
page-locked copies reach on these boxes (``--link-gbs``, 55 GB/s: DESIGN.md) - a computed bound, not a measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the synthetic cohorts live with the tests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=200_000)
    ap.add_argument("--psm-per-group", type=float, default=14.0)
    ap.add_argument("--max-block", type=int, default=35)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--link-gbs", type=float, default=55.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    import mbr_library_golden as G
    from alphadia_amd import mbr_library as M

    rng = np.random.default_rng(3)
    rows = rng.poisson(a.psm_per_group / 0.6, a.groups) * (rng.random(a.groups) < 0.6)
    psm, lib = G.cohort(rng, a.groups, rows, n_columns=a.columns, max_block=a.max_block, strings=False)
    n_rows = len(lib._fragment_mz_df)
    matrix_bytes = n_rows * a.columns * 4 * len(G.DENSE)

    builders = {"device_gather": M.HipMbrLibraryBuilder(gather="device"), "host_gather": M.HipMbrLibraryBuilder(gather="host")}
    small = G.cohort(np.random.default_rng(1), 300, np.full(300, 8), n_columns=a.columns)
    for b in builders.values():  # context, kernels, allocator
        b(*small)

    def run(name):
        t0 = time.perf_counter()
        out = builders[name](psm, lib) if name in builders else M.host_build_mbr_library(psm, lib)
        dt = time.perf_counter() - t0
        return out, dt, dict(M.last_timing)

    forms = ("device_gather", "host_gather", "host")
    results = {f: dict(seconds=[], stages=[]) for f in forms}
    equal = {}
    for rep in range(a.repeats + 1):
        outs = {}
        for f in forms:
            before = builders[f]._session.stats() if f in builders and builders[f]._session else None
            out, dt, timing = run(f)
            if rep == 0:  # the untimed round at the full size; the results are compared once
                outs[f] = out
                continue
            results[f]["seconds"].append(round(dt, 4))
            keys = ([k for k in timing if k.startswith("host_")] if f == "host" else
                    ["aggregate_s", "filter_s", "assign_s", "aggregate_ms", "filter_ms", "gather_ms", "assign_ms"])
            stage = {k: round(float(timing[k]), 4) for k in keys}
            if before is not None:
                stage["h2d_bytes"] = timing["h2d_bytes"] - before["h2d_bytes"]
                stage["d2h_bytes"] = timing["d2h_bytes"] - before["d2h_bytes"]
            results[f]["stages"].append(stage)
        if rep == 0:
            for f in forms[:2]:
                try:
                    G.assert_libraries_identical(outs[f], outs["host"])
                    equal[f] = True
                except AssertionError:
                    equal[f] = False
            kept_prec, kept_rows = len(outs["host"]._precursor_df), len(outs["host"]._fragment_mz_df)
            del outs
    for f in forms:
        results[f]["median_s"] = round(statistics.median(results[f]["seconds"]), 4)
    kept_bytes = kept_rows * a.columns * 4 * len(G.DENSE)
    floor_s = (matrix_bytes + kept_bytes) / (a.link_gbs * 1e9)
    faster = min(forms[:2], key=lambda f: results[f]["median_s"])
    res = dict(library_precursors=len(lib._precursor_df), dense_rows=n_rows, columns=a.columns, frames=len(G.DENSE),
               psm_rows=len(psm), passed_rows=int(M.last_timing.get("n_passed", -1)), kept_precursors=kept_prec,
               kept_dense_rows=kept_rows, matrix_bytes_up=matrix_bytes, matrix_bytes_down=kept_bytes,
               pcie_floor_of_the_matrices_s=round(floor_s, 4), link_gbs_assumed=a.link_gbs, equal_to_host=equal,
               faster_gather=faster, shipped_default_gather=M.HipMbrLibraryBuilder().__dict__["_gather"], **results)
    for b in builders.values():
        b.close()
    out = dict(note="host -> host seconds of forward(psm_df, base_library), frames in, library object out, the three "
                    "forms alternating.  device_gather: the dense matrices go up whole and the kept rows come back; "
                    "host_gather: the device returns the row map and NumPy gathers.  *_s: host clock around a stage "
                    "(aggregate: the PSM columns up, compaction, sorts, medians; filter: library columns and matrices "
                    "up, membership, renumbering, gather, kept rows back, the new frames; assign: the lookups and the "
                    "three columns); *_ms: HIP-event times inside them; h2d / d2h bytes: what one call moved.  host: "
                    "host_build_mbr_library, NumPy, same box.  pcie_floor_of_the_matrices_s is computed from bytes "
                    "and link_gbs_assumed, not measured.", results=res)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
