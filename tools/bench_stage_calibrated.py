"""What a calibration update of the fragment library costs until the calibrated library is staged in HBM, three ways,
at the size of a 1e6-precursor library (12 M fragments) and of a batch library (200 000 fragments):

  parent    ``calibration_predict`` (host -> host), ``astype(float32)``, ``stage_fragments(force=True)``
  columns   ``stage_fragments_calibrated``: the columns uploaded, the records packed and calibrated by one kernel
  in_place  ``calibrate_staged_fragments`` alone, on a library staged (outside the clock) with ``stage_fragments``

Every path is warmed up, then the three alternate for ``--repeats`` rounds in this one process; each window ends in a
device synchronise.  Prints one JSON object: per size and path the median, minimum and maximum wall ms, the kernel
time (``adh_calibration_time_ms``), the bytes over the link in each direction, whether the path's median lies below
the parent's by more than the two spreads (max - min) together, and whether the three staged libraries - device
records, host mirror and the float64 column - are bit-equal.

    python tools/bench_stage_calibrated.py [--sizes 12000000,200000] [--repeats 9]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fitted(rng):
    from alphadia_amd.calibration import HipLOESSRegression

    x = rng.uniform(150.0, 2000.0, 5000).astype(np.float32)
    y = x.astype(np.float64) * (1 + 8e-6) + rng.normal(0, 1e-3, x.size)
    return HipLOESSRegression(n_kernels=2).fit(x[:, None], y[:, None])


def library(rng, n):
    """mz_library, intensity, type, loss_type, charge, number, position, cardinality"""
    return [rng.uniform(150, 2000, n).astype(np.float32), rng.random(n, dtype=np.float32),
            rng.integers(97, 123, n).astype(np.uint8), np.zeros(n, np.uint8), rng.integers(1, 3, n).astype(np.uint8),
            rng.integers(1, 40, n).astype(np.uint8), rng.integers(0, 40, n).astype(np.uint8), np.ones(n, np.uint8)]


def run_size(ctx, model, cols, repeats):
    n = cols[0].shape[0]
    nine = lambda mz: (cols[0], mz, *cols[1:])  # noqa: E731

    def parent():
        t0 = time.perf_counter()
        y = ctx.calibration_predict(model, cols[0])
        kernel = ctx.calibration_time_ms()
        ctx.stage_fragments(*nine(y.astype(np.float32)), force=True)
        ctx.synchronize()
        return time.perf_counter() - t0, kernel, y

    def columns():
        t0 = time.perf_counter()
        y = ctx.stage_fragments_calibrated(model, *cols)
        ctx.synchronize()
        return time.perf_counter() - t0, ctx.calibration_time_ms(), y

    def in_place():
        ctx.stage_fragments(*nine(cols[0]), force=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        y = ctx.calibrate_staged_fragments(model)
        ctx.synchronize()
        return time.perf_counter() - t0, ctx.calibration_time_ms(), y

    paths = {"parent": parent, "columns": columns, "in_place": in_place}
    h2d = {"parent": 4 * n + 32 * n, "columns": 14 * n, "in_place": 0}
    for f in paths.values():  # warm-up: page-locked slots, the library's blocks, the mirror's pages
        f()
        f()
    walls = {k: [] for k in paths}
    kernels = {k: [] for k in paths}
    d2h = {}
    for _ in range(repeats):
        for name, f in paths.items():
            before = ctx.d2h_bytes()
            w, k, _y = f()
            d2h[name] = ctx.d2h_bytes() - before
            walls[name].append(w)
            kernels[name].append(k)
    # the three libraries, bit for bit
    states = {}
    for name, f in paths.items():
        _w, _k, y = f()
        states[name] = (ctx.staged_fragment_records().tobytes(), ctx.staged_fragment_records(host_mirror=True).tobytes(),
                        y.tobytes())
    first = states["parent"]
    equal = all(s == first for s in states.values()) and first[0] == first[1]
    out = {"rows": int(n), "repeats": int(repeats), "libraries_bit_equal": bool(equal)}
    spread = {k: 1e3 * (max(v) - min(v)) for k, v in walls.items()}
    median = {k: 1e3 * float(np.median(v)) for k, v in walls.items()}
    for name in paths:
        out[name] = dict(median_ms=median[name], min_ms=1e3 * min(walls[name]), max_ms=1e3 * max(walls[name]),
                         spread_ms=spread[name], kernel_ms=float(np.median(kernels[name])),
                         h2d_bytes=int(h2d[name]), d2h_bytes=int(d2h[name]))
        if name != "parent":
            out[name]["gain"] = bool(median["parent"] - median[name] > spread["parent"] + spread[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12000000,200000")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if args.repeats < 9:
        ap.error("at least nine repetitions")

    from alphadia_amd import runtime

    ctx = runtime.get_context(0)
    rng = np.random.default_rng(20261018)
    model = fitted(rng)
    out = {"device": "cuda:0", "n_kernels": int(model.n_kernels), "host_threads": list(runtime.host_threads(12_000_000))}
    for n in (int(s) for s in args.sizes.split(",")):
        out[str(n)] = run_size(ctx, model, library(rng, n), args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
