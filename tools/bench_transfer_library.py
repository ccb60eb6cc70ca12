"""Transfer-learning library: ``HipTransferLearningAccumulator`` host -> host on a seeded synthetic cohort, split into
its stages (with the HIP-event times inside them), beside the host restatements on the same box and the
per-precursor form of the MS2 quality control (``host_ms2_quality_control(looped=True)``: the reference's loop on NumPy
slices instead of ``DataFrame.iloc``) at 2 000 and 20 000 precursors.

    python tools/bench_transfer_library.py [--out profiles/transfer_library_bench.json]

Cohort (tests/transfer_library_golden.py:cohort_run): 20 runs x 200 000 peptides, 80 % of them seen per run, keep_top 3,
four fragment columns, 7 to 29 residues, float32 m/z, intensity and correlation matrices.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the synthetic cohorts live with the tests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--peptides", type=int, default=200_000)
    ap.add_argument("--keep-top", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement of the cohort")
    ap.add_argument("--loop-sizes", type=int, nargs="*", default=[2_000, 20_000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    import transfer_library_golden as G
    from alphadia_amd import transfer_library as T

    def copy_of(lib):
        return G.Library(lib.precursor_df.copy(), {n: getattr(lib, n).copy() for n in lib.available_dense_fragment_dfs()})

    warm = T.HipTransferLearningAccumulator(keep_top=2)  # warm-up: context, kernels, allocator
    rng = np.random.default_rng(1)
    for r in range(2):
        warm.update(G.cohort_run(rng, r, 500, strings=False))
    warm.post_process()
    warm.close()

    out = dict(note="host -> host seconds.  update_s: all updates (upload of the run, sort, keep mask, renumbering, row "
                    "gathers, the kept index back, truncating the host frame); topk_ms / gather_ms: HIP-event times "
                    "inside it (sort + mask; renumbering + row gathers).  fetch_s: the three consensus matrices back to "
                    "the host.  rt_norm_s / qc_s: normalize_rt_delta_max / ms2_quality_control host -> host (frames in, "
                    "frames out), rt_norm_ms / qc_ms the kernels alone.  host: the NumPy restatements, same box; "
                    "qc_loop: host_ms2_quality_control(looped=True), one precursor at a time on NumPy slices",
               cohort=dict(runs=a.runs, peptides=a.peptides, keep_top=a.keep_top, columns=4), results={})
    rng = np.random.default_rng(7)
    dev = T.HipTransferLearningAccumulator(keep_top=a.keep_top)
    host = None
    host_update_s = 0.0
    rows_in = 0
    for r in range(a.runs):
        run = G.cohort_run(rng, r, a.peptides, strings=False)
        rows_in += len(run.precursor_df)
        dev.update(run)
        if not a.no_host:
            t0 = time.perf_counter()
            host = T.host_update(host, run, a.keep_top)
            host_update_s += time.perf_counter() - t0
        del run
    cons = dev.consensus_speclibase
    t0 = time.perf_counter()
    for name in cons.available_dense_fragment_dfs():
        getattr(cons, name)
    fetch_s = time.perf_counter() - t0
    updates_equal = None
    if host is not None:
        try:
            G.assert_libraries_identical(cons, host)
            updates_equal = True
        except AssertionError:
            updates_equal = False
    pre = copy_of(cons)
    dev.post_process()
    t = dict(dev.timing)
    device = dict(update_s=round(t["update_s"], 4), update_s_per_run=round(t["update_s"] / a.runs, 4),
                  topk_ms=round(t["topk_ms"], 3), gather_ms=round(t["gather_ms"], 3), fetch_s=round(fetch_s, 4),
                  rt_norm_s=round(T.last_timing["rt_norm_s"], 5), rt_norm_ms=round(T.last_timing["rt_norm_ms"], 4),
                  qc_s=round(T.last_timing["qc_s"], 4), qc_ms=round(T.last_timing["qc_ms"], 4),
                  qc_large_blocks=int(T.last_timing["qc_large_blocks"]))
    res = dict(precursor_rows_in=rows_in, consensus_precursors=len(cons.precursor_df),
               consensus_fragment_rows=len(cons._fragment_intensity_df), device=device)
    res["device"]["qc_precursors_per_s"] = round(len(cons.precursor_df) / max(device["qc_s"], 1e-9))
    if not a.no_host:
        t0 = time.perf_counter()
        with np.errstate(invalid="ignore"):
            T.host_normalize_rt_delta_max(pre)
        t1 = time.perf_counter()
        T.host_ms2_quality_control(pre)
        t2 = time.perf_counter()
        try:
            G.assert_libraries_identical(dev.consensus_speclibase, pre)
            post_equal = True
        except AssertionError:
            post_equal = False
        res.update(host=dict(update_s=round(host_update_s, 4), update_s_per_run=round(host_update_s / a.runs, 4),
                             rt_norm_s=round(t1 - t0, 5), qc_s=round(t2 - t1, 4)),
                   consensus_equal_to_host=updates_equal, post_process_equal_to_host=post_equal)
    final = dev.consensus_speclibase
    loops = {}
    for n in a.loop_sizes:
        n = min(n, len(final.precursor_df))
        part = G.Library(pre.precursor_df.iloc[:n].copy() if not a.no_host else final.precursor_df.iloc[:n].copy(),
                         {"_fragment_intensity_df": final._fragment_intensity_df.copy(),
                          "_fragment_correlation_df": final._fragment_correlation_df})
        t0 = time.perf_counter()
        T.host_ms2_quality_control(part, looped=True)
        dt = time.perf_counter() - t0
        loops[str(n)] = dict(seconds=round(dt, 4), precursors_per_s=round(n / dt))
    res["qc_loop"] = loops
    dev.close()
    out["results"]["cohort"] = res
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
