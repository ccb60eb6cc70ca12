"""Multiplex requantification at the size of BASELINE configs[4]: ``requantify()`` plus the q-value filter (the chained
calls: every padded table to the host, the features frame, the channel-decoy FDR on host slices) against
``HipMultiplexingRequantificationHandler.requantify_filtered()`` (tables stay in HBM, only the survivors come back).

The workload is ``syn.make_multiplex_case(75_000, 4800)``: 75 000 elution groups x 4 label channels, the last channel
as decoy channel, and the production FDR hyper-parameters of tools/bench_fdr.py.  Both paths run in one process, on the
same staged run: one warm-up call each, then ``--repeats`` timed calls each, alternating, every call with a fresh FDR
manager of the same seed.  Per path: wall ms per stage (a host clock; every stage ends in a copy to the host, and the
resident scoring stage, which copies nothing, in a device synchronisation), bytes copied device -> host (``ctx.d2h_bytes``), the rows the FDR stage returned and kept; and whether both paths
return the same frame (the bounds of tests/test_fdr_strategies_gpu.py).  Prints one JSON line.

    python tools/bench_multiplex.py [--groups 75000] [--cycles 4800] [--repeats 3] [--out profiles/multiplex_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLASSIFIER = dict(test_size=0.001, batch_size=5000, learning_rate=0.001, epochs=10, experimental_hyperparameter_tuning=True,
                  random_state=1)


def _threads() -> int:
    return max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))


class _TimedManager:
    """Passes ``fit_predict`` on and notes when it was entered and left (the chained path's score / FDR split)."""

    def __init__(self, manager):
        self.manager = manager

    def fit_predict(self, *args, **kwargs):
        self.t_in = time.perf_counter()
        out = self.manager.fit_predict(*args, **kwargs)
        self.t_out = time.perf_counter()
        return out


def same_frame(a, b) -> str:
    if list(a.columns) != list(b.columns):
        return "differ: columns"
    if len(a) != len(b):
        return f"differ: rows {len(a)} / {len(b)}"
    for c in a.columns:
        x, y = a[c], b[c]
        if x.dtype != y.dtype:
            return f"differ: dtype of {c}"
        if c == "proba":
            ok = np.allclose(x.to_numpy(), y.to_numpy(), rtol=0, atol=1e-6)
        elif c == "qval":
            ok = np.allclose(x.to_numpy(), y.to_numpy(), rtol=1e-12, atol=0)
        elif x.dtype == object:
            ok = bool((x.to_numpy() == y.to_numpy()).all())
        else:
            ok = np.array_equal(x.to_numpy(), y.to_numpy(), equal_nan=True)
        if not ok:
            return f"differ: values of {c}"
    return "equal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=75_000)
    ap.add_argument("--cycles", type=int, default=4800)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fdr", type=float, default=0.01)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    from types import SimpleNamespace

    import synthetic as syn
    from alphadia_amd import fdr, runtime
    from alphadia_amd.multiplexing import HipMultiplexingRequantificationHandler
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    t0 = time.perf_counter()
    mc = syn.make_multiplex_case(args.groups, args.cycles, threads=_threads())
    gen_s = time.perf_counter() - t0
    psm_df = mc.psm_df.copy()
    psm_df["channel"] = np.uint32(mc.channels[0])
    features = [c for c in DEFAULT_FEATURE_COLUMNS if c not in ("mobility_observed", "base_width_mobility")] + [
        "delta_rt", "mz_library", "charge", "n_K", "n_R", "n_P"]
    config = {"multiplexing": {"reference_channel": int(mc.channels[0]),
                               "target_channels": ",".join(str(c) for c in mc.channels[1:-1]),
                               "decoy_channel": int(mc.channels[-1]), "competitive_scoring": True},
              "search": {"experimental_xic": True}, "fdr": {"fdr": args.fdr}}
    names = SimpleNamespace(get_rt_column=lambda: "rt_library", get_mobility_column=lambda: "mobility_library",
                            get_precursor_mz_column=lambda: "mz_library", get_fragment_mz_column=lambda: "mz_library")
    lib = SimpleNamespace(precursor_df_unfiltered=mc.library.precursor_df, fragment_df=mc.library.fragment_df,
                          _fragment_df=mc.library.fragment_df)
    reporter = SimpleNamespace(log_string=lambda *a, **k: None)
    ctx = runtime.get_context(0)

    def once(path):
        manager = fdr.HipFDRManager(features, fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=mc.dia.cycle,
                                    random_state=42, device=0)
        ctx.d2h_bytes(reset=True)
        if path == "resident":
            h = HipMultiplexingRequantificationHandler(config, None, manager, reporter, names, lib, device=0)
            out = h.requantify_filtered(mc.dia, psm_df)
            stages = {k: v for k, v in h.last_timings.items() if k.endswith("_ms")}
            assert h.last_timings["path"] == "resident"
            n_fdr = None
        else:
            timed = _TimedManager(manager)
            h = HipMultiplexingRequantificationHandler(config, None, timed, reporter, names, lib, device=0)
            t_0 = time.perf_counter()
            full = h.requantify(mc.dia, psm_df)
            out = full[full["qval"] <= args.fdr].reset_index(drop=True)
            t_1 = time.perf_counter()
            stages = {"score_ms": (timed.t_in - t_0) * 1e3, "fdr_ms": (timed.t_out - timed.t_in) * 1e3,
                      "filter_ms": (t_1 - timed.t_out) * 1e3, "total_ms": (t_1 - t_0) * 1e3}
            n_fdr = len(full)
        return out, stages, ctx.d2h_bytes(), n_fdr

    paths = ("chained", "resident")
    for path in paths:  # warm-up: staging, buffers, kernels loaded
        once(path)
    runs = {p: [] for p in paths}
    frames = {}
    for _ in range(args.repeats):
        for path in paths:
            out, stages, d2h, n_fdr = once(path)
            frames[path] = out
            runs[path].append(dict(stages_ms={k: round(v, 1) for k, v in stages.items()}, d2h_bytes=d2h,
                                   survivors=len(out), **({} if n_fdr is None else {"fdr_rows": n_fdr})))
    result = {"workload": f"{args.groups} elution groups x {len(mc.channels)} channels ({len(mc.library.precursor_df)} "
                          f"table rows), {args.cycles} cycles, decoy channel {mc.channels[-1]}, competitive channel FDR at "
                          f"{args.fdr}, classifier {CLASSIFIER}; all channels of a planted group carry signal",
              "generate_s": round(gen_s, 1), "repeats": args.repeats}
    for path in paths:
        totals = [r["stages_ms"]["total_ms"] for r in runs[path]]
        result[path] = dict(runs[path][int(np.argsort(totals)[len(totals) // 2])], total_ms_all=totals)
    result["same_frame"] = same_frame(frames["resident"], frames["chained"])
    c, r = result["chained"], result["resident"]
    result["d2h_ratio"] = round(r["d2h_bytes"] / max(c["d2h_bytes"], 1), 4)
    result["total_ms_ratio"] = round(r["stages_ms"]["total_ms"] / max(c["stages_ms"]["total_ms"], 1e-9), 3)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
