"""The dense library flattened: the device path (alphadia_amd.flatten.HipFlattenLibrary) against the NumPy restatement
(host_flatten_library - this repository's restatement, not alphabase, which is not installed), alternating in one
process, every window closed by a device synchronise; then the flatten that leaves the records staged on a context
against the flatten followed by stage_fragments_columns of the returned frame.  Medians with min - max over the
repetitions after a warm-up go to the record.  No time is fixed in advance: the record is the claim.

The library: elution groups of two charge states (equal row counts, the singly charged columns share m/z) as targets
and again as decoys of the same elution_group_idx; 8 - 30 rows per precursor, 4 columns, 30 % zero intensities.

    python tools/bench_flatten.py --precursors 200000 2000000 --repeat 7 --out profiles/flatten_bench.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = ["b_z1", "b_z2", "y_z1", "y_z2"]
TOP_K, MIN_INTENSITY = 12, 0.01


class Library:
    def __init__(self, n_prec: int, seed: int = 0):
        rng = np.random.default_rng(seed)
        n_groups = n_prec // 4
        n_prec = 4 * n_groups
        g_rows = rng.integers(8, 31, n_groups)
        group = np.repeat(np.arange(n_groups), 4)             # per group: target z2, target z3, decoy z2, decoy z3
        rows = g_rows[group]
        stop = np.cumsum(rows)
        start = stop - rows
        R = int(stop[-1])
        self.precursor_df = pd.DataFrame({
            "frag_start_idx": start, "frag_stop_idx": stop, "elution_group_idx": group.astype(np.uint32),
            "decoy": np.tile(np.array([0, 0, 1, 1], dtype=np.uint8), n_groups),
            "charge": np.tile(np.array([2, 3, 2, 3], dtype=np.uint8), n_groups)})
        mz = rng.uniform(150.0, 1800.0, (R, 4)).astype(np.float32)
        second = np.repeat(np.tile(np.array([False, True, False, True]), n_groups), rows)
        # the second charge state repeats the singly charged columns of the first (which lies `rows` rows above it)
        src = np.flatnonzero(second) - np.repeat(rows[1::2], rows[1::2])
        mz[np.flatnonzero(second)[:, None], [0, 2]] = mz[src[:, None], [0, 2]]
        inten = rng.random((R, 4)).astype(np.float32)
        inten[rng.random((R, 4)) < 0.3] = 0.0
        self.fragment_mz_df = pd.DataFrame(mz, columns=COLUMNS)
        self.fragment_intensity_df = pd.DataFrame(inten, columns=COLUMNS)


def spread(samples, digits=4):
    return dict(median=round(statistics.median(samples), digits), min=round(min(samples), digits),
                max=round(max(samples), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precursors", type=int, nargs="+", default=[200_000, 2_000_000])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from alphadia_amd import flatten as fl
    from alphadia_amd import runtime

    ctx = runtime.get_context(0)
    staged_ctx = runtime.Context(0)
    out = dict(columns=COLUMNS, top_k=TOP_K, min_fragment_intensity=MIN_INTENSITY, repeat=a.repeat,
               host_threads=runtime.host_threads(1 << 20)[1],
               host="alphadia_amd.flatten.host_flatten_library: this repository's NumPy restatement; alphabase is not installed",
               results={})

    def save():  # (after every stage: a run cut short keeps what it measured)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    step = fl.HipFlattenLibrary(TOP_K, MIN_INTENSITY, device=0)

    def device(lib, context=None):
        ctx.synchronize()
        t = time.perf_counter()
        flat = step(lib, context)
        (context or ctx).synchronize()
        return time.perf_counter() - t, dict(fl.last_timing), flat

    def host(lib):
        ctx.synchronize()
        t = time.perf_counter()
        res = fl.host_flatten_library(lib.precursor_df, lib.fragment_mz_df.to_numpy(), lib.fragment_intensity_df.to_numpy(),
                                      COLUMNS, TOP_K, MIN_INTENSITY)
        ctx.synchronize()
        return time.perf_counter() - t, res

    def then_stage(lib):
        staged_ctx.synchronize()
        t = time.perf_counter()
        flat = step(lib)
        frag = flat._fragment_df
        staged_ctx.stage_fragments_columns(frag["mz"].values, frag["mz"].values,
                                           *(frag[c].values for c in fl.FRAGMENT_COLUMNS[1:]))
        staged_ctx.synchronize()
        return time.perf_counter() - t

    device(Library(4000, seed=1))  # warm-up: context, kernels, allocator, page-locked lanes
    device(Library(4000, seed=1), staged_ctx)
    for n in a.precursors:
        lib = Library(n, seed=n % 1000)
        device(lib)  # warm-up at this size
        dev, hst, timings = [], [], []
        same = None
        for r in range(a.repeat):
            s, timing, flat = device(lib)
            dev.append(s)
            timings.append(timing)
            s, (pre, frag) = host(lib)
            hst.append(s)
            if same is None:
                same = bool(all(np.array_equal(flat._fragment_df[c].to_numpy(), frag[c].to_numpy()) for c in frag.columns)
                            and np.array_equal(flat._precursor_df["flat_frag_stop_idx"], pre["flat_frag_stop_idx"]))
            del flat, pre, frag
            print(f"{n}: repeat {r + 1} of {a.repeat}: device {dev[-1]:.3f} s, host {hst[-1]:.3f} s", flush=True)
        res = dict(precursors=len(lib.precursor_df), dense_rows=len(lib.fragment_mz_df), cells=int(lib.fragment_mz_df.size),
                   flat_rows=timings[0]["n_fragments"], device_equals_host=same,
                   device_host_to_host_s=spread(dev), host_restatement_s=spread(hst),
                   device_kernel_ms=spread([t["kernel_ms"] for t in timings], 3),
                   device_prepare_s=spread([t["prepare_s"] for t in timings]),
                   device_call_s=spread([t["device_s"] for t in timings]),
                   device_frames_s=spread([t["frames_s"] for t in timings]),
                   h2d_bytes=timings[0]["h2d_bytes"], d2h_bytes=timings[0]["d2h_bytes"], routes=timings[0]["routes"])
        out["results"][f"{n}_precursors"] = res
        print(json.dumps(res), flush=True)
        save()
        staged, classic = [], []
        for r in range(a.repeat):
            staged.append(device(lib, staged_ctx)[0])
            classic.append(then_stage(lib))
        res["flatten_staged_s"] = spread(staged)
        res["flatten_then_stage_fragments_columns_s"] = spread(classic)
        print(json.dumps({k: res[k] for k in ("flatten_staged_s", "flatten_then_stage_fragments_columns_s")}), flush=True)
        save()
        del lib
    staged_ctx.close()


if __name__ == "__main__":
    main()
