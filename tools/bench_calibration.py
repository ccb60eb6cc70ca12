"""Library calibration at the size of a 1e6-precursor library: host -> host prediction of a 12 M-row float32
fragment m/z column (2 kernels) and of a 1 M-row precursor group (m/z 2, RT 6, mobility 2 kernels) through
``adh_calibration_predict``.  Prints one JSON object: per column the kernel time (HIP events), the wall time of the
call, the bytes over the link, and a NumPy evaluation of the same model on this box for comparison (its time on a
sample, scaled to the column); then what re-staging the calibrated fragment column costs the scoring path
(``adh_stage_fragments``), the step an in-place path would save.

    python tools/bench_calibration.py [--fragments 12000000] [--precursors 1000000] [--repeats 5]
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


def numpy_predict(model, x):
    """LOESSRegression.predict (alphadia/calibration/models.py:276-366) in plain NumPy, as the host would run it."""
    col = np.asarray(x).reshape(-1, 1)
    w = model._weights(col)  # noqa: SLF001
    return (model._design(col).astype(np.float64) @ model.beta * w).sum(axis=1)  # noqa: SLF001


def fitted(rng, lo, hi, n_kernels, f):
    from alphadia_amd.calibration import HipLOESSRegression

    x = rng.uniform(lo, hi, 5000).astype(np.float32)
    y = f(x.astype(np.float64)) + rng.normal(0, 1e-3 * (hi - lo), x.size)
    return HipLOESSRegression(n_kernels=n_kernels).fit(x[:, None], y[:, None]), (lo, hi)


def measure(ctx, model, x, repeats, sample):
    ctx.calibration_predict(model, x[: min(x.size, 1 << 16)])  # (first call: page-locked slots)
    walls, kernels = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        y = ctx.calibration_predict(model, x)
        walls.append(time.perf_counter() - t0)
        kernels.append(ctx.calibration_time_ms())
    s = x[:sample]
    t0 = time.perf_counter()
    ref = numpy_predict(model, s)
    numpy_s = (time.perf_counter() - t0) * x.size / s.size
    err = float(np.abs(y[:sample] - ref).max() / max(np.abs(ref).max(), 1e-300))
    return dict(rows=int(x.size), dtype=x.dtype.name, n_kernels=int(model.n_kernels),
                wall_ms=1e3 * float(np.median(walls)), kernel_ms=float(np.median(kernels)),
                link_bytes=int(x.nbytes + 8 * x.size),
                link_gbs=(x.nbytes + 8 * x.size) / float(np.median(walls)) / 1e9,
                numpy_ms=1e3 * numpy_s, speedup=numpy_s / float(np.median(walls)), max_rel_err_sample=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=12_000_000)
    ap.add_argument("--precursors", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1_000_000)
    args = ap.parse_args()

    from alphadia_amd import runtime

    ctx = runtime.get_context(0)
    rng = np.random.default_rng(20261015)
    out = {"device": "cuda:0"}

    frag_mz, (lo, hi) = fitted(rng, 150.0, 2000.0, 2, lambda v: v * (1 + 8e-6))
    x = rng.uniform(lo, hi, args.fragments).astype(np.float32)
    out["fragment_mz"] = measure(ctx, frag_mz, x, args.repeats, args.sample)

    group = {"mz": (400.0, 1200.0, 2, lambda v: v * (1 - 3e-6)),
             "rt": (0.0, 7200.0, 6, lambda v: 1.02 * v + 60 * np.sin(v / 1500)),
             "mobility": (0.6, 1.6, 2, lambda v: 1.01 * v + 0.005)}
    total = dict(wall_ms=0.0, kernel_ms=0.0, numpy_ms=0.0, link_bytes=0)
    for name, (lo, hi, k, f) in group.items():
        model, _ = fitted(rng, lo, hi, k, f)
        x = rng.uniform(lo, hi, args.precursors).astype(np.float32)
        r = measure(ctx, model, x, args.repeats, args.sample)
        out[f"precursor_{name}"] = r
        for key in total:
            total[key] += r[key]
    out["precursor_group"] = total

    # the calibrated fragment column re-staged for selection / scoring (adh_stage_fragments)
    n = args.fragments
    cols = [rng.uniform(150, 2000, n).astype(np.float32), None, rng.random(n, dtype=np.float32),
            np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.ones(n, np.uint8), np.ones(n, np.uint8),
            np.zeros(n, np.uint8), np.ones(n, np.uint8)]  # mz_library, mz, intensity, type, ... cardinality
    stage = []
    for _ in range(max(args.repeats, 1)):
        cols[1] = ctx.calibration_predict(frag_mz, cols[0]).astype(np.float32)
        t1 = time.perf_counter()
        ctx.stage_fragments(*cols, force=True)
        stage.append(time.perf_counter() - t1)
    out["restage_fragments_ms"] = 1e3 * float(np.median(stage))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
