"""The optimisation lock at the headline size: the chained calls against HipExtractionHandler.process_optimization_batch.

The library and run of bench.py (``syn.make_case(1_000_000, 4800, config_id=2, per_precursor=3)``) and the FDR
hyper-parameters of tools/bench_extraction.py.  A realistic lock sequence (optimization_handler.py:220-343): the
growing batch plan until the target count at 1 % FDR is reached (or the plan ends), each growing step followed by a
recalibration of the batch library; then the reset the lock does when the target is reached and ``--fixed-steps``
steps of the fixed batch, each followed by a recalibration.  Where a step reaches the target, the calibration frames
are built as the integrated optimisation handler builds them (``filter_for_calibration``).  The case's candidate table of the
batch library's precursors stands in for the selection step; a stand-in calibration shifts the calibrated columns.
Each path runs in a child process of its own.  Per step: wall ms, bytes copied device -> host (``ctx.d2h_bytes``),
the lock's feature / fragment rows, the PSMs at 1 % FDR, and the child's peak RSS so far.  Prints one JSON line.

    python tools/bench_optimization.py [--precursors 1000000] [--cycles 4800] [--batch-size 8000] [--target 30000]
                                       [--fixed-steps 3] [--out profiles/optimization_bench.json]
"""

from __future__ import annotations

import argparse
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RUN_ARRAYS = ("rt_values", "peak_start_idx_list", "peak_stop_idx_list", "mz_values", "intensity_values", "cycle")
CLASSIFIER = dict(test_size=0.001, batch_size=5000, learning_rate=0.001, epochs=10, experimental_hyperparameter_tuning=True,
                  random_state=1)


def _threads() -> int:
    return max(1, min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))


class _Calibration:
    """Stands in for the calibration manager: every call shifts the calibrated columns a little more."""

    def __init__(self):
        self.calls = 0

    def predict(self, df, group):
        self.calls += 1
        if group == "precursor":
            df["mz_calibrated"] = df["mz_library"] * (1 + 1e-7 * self.calls)
            df["rt_calibrated"] = df["rt_library"] + 0.1 * self.calls
        else:
            df["mz_calibrated"] = (df["mz_library"] * (1 + 1e-7 * self.calls)).astype(df["mz_library"].dtype)


def child(args):
    from types import SimpleNamespace

    import synthetic as syn
    from alphadia_amd import fdr, runtime
    from alphadia_amd.extraction_handler import HipExtractionHandler
    from alphadia_amd.optimization import HipOptimizationLock
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    light = syn.make_case(args.precursors, args.cycles, config_id=2, per_precursor=3, threads=1, run=False)
    dia = syn.AlphaRawArrays(**{n: np.load(os.path.join(args.work, n + ".npy"), mmap_mode="r") for n in RUN_ARRAYS})
    pre, frag = light.library.precursor_df, light.library.fragment_df
    pre["mz_calibrated"], pre["rt_calibrated"], frag["mz_calibrated"] = pre["mz_library"], pre["rt_library"], frag["mz_library"]
    lib = SimpleNamespace(_precursor_df=pre, _fragment_df=frag)
    cands = light.candidates_df
    features = [c for c in DEFAULT_FEATURE_COLUMNS if c not in ("mobility_observed", "base_width_mobility")] + [
        "delta_rt", "mz_library", "charge", "n_K", "n_R", "n_P"]
    config = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                         "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
              "general": {"thread_count": _threads()},
              "fdr": {"fdr": 0.01, "competitive_scoring": True, "channel_wise_fdr": False},
              "calibration": {"optimization_lock_target": args.target, "batch_size": args.batch_size,
                              "min_correlation": 0.7, "max_fragments": 5000}}
    opt = SimpleNamespace(ms1_error=10, ms2_error=15, score_cutoff=-np.inf, classifier_version=-1)
    names = SimpleNamespace(get_rt_column=lambda: "rt_calibrated", get_mobility_column=lambda: "mobility_library",
                            get_precursor_mz_column=lambda: "mz_calibrated", get_fragment_mz_column=lambda: "mz_calibrated")
    reporter = SimpleNamespace(log_string=lambda *a, **k: None)
    selection = SimpleNamespace(select_candidates=lambda dia, lib, apply_cutoff=False: cands[
        cands["precursor_idx"].isin(lib.precursor_df["precursor_idx"])])
    ctx = runtime.get_context(0)
    manager = fdr.HipFDRManager(features, fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=dia.cycle, random_state=42,
                                device=0)
    h = HipExtractionHandler(config, opt, manager, reporter, names, selection_handler=selection, device=0)
    if args.path == "chained":
        h.resident_refusal = lambda: "chained calls measured"
    lock = HipOptimizationLock(lib, config, device=0)
    calibration = _Calibration()
    steps = []

    def step(kind):
        ctx.d2h_bytes(reset=True)
        t_0 = time.perf_counter()
        psm = h.process_optimization_batch(dia, lock)
        n_feat, n_frag = lock.n_features, lock.n_fragments
        reached = bool(lock.has_target_num_precursors)
        filtered = None
        if reached:  # (where _process_batch's caller calls _filter_for_calibration: INTEGRATION.md)
            pre_f, frag_f = h.filter_for_calibration(psm, config)
            filtered = (len(pre_f), len(frag_f))
        ms = (time.perf_counter() - t_0) * 1e3
        steps.append({"kind": kind, "batch_idx": int(lock.batch_idx), "elution_groups": [int(lock.start_idx), int(lock.stop_idx)],
                      "ms": round(ms, 1), "stages_ms": {k: round(v, 1) for k, v in h.last_timings.items() if k.endswith("_ms")},
                      "d2h_bytes": ctx.d2h_bytes(), "features_rows": n_feat, "fragments_rows": n_frag,
                      "psm_at_1pct": int(((psm["qval"] < 0.01) & (psm["decoy"] == 0)).sum()), "filtered": filtered,
                      "peak_rss_mb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)})
        return reached

    # the growing plan (optimization_handler.py:278-297): recalibrated batch library after every step
    while True:
        reached = step("grow")
        if reached or not lock.batches_remaining():
            break
        lock.update()
        lock.update_with_calibration(calibration)
    # the reset of a reached target (optimization_handler.py:299-314), then fixed steps with a recalibration between
    def advance():
        if lock.has_target_num_precursors or lock.batches_remaining():
            lock.update()
            lock.update_with_calibration(calibration)
        else:  # (the plan is exhausted: start over from the whole plan, as after convergence)
            lock.reset_after_convergence(calibration)

    advance()
    for _ in range(args.fixed_steps):
        step("fixed")
        advance()
    print(json.dumps({"steps": steps, "total_ms": round(sum(s["ms"] for s in steps), 1),
                      "total_d2h_bytes": sum(s["d2h_bytes"] for s in steps)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precursors", type=int, default=1_000_000)
    ap.add_argument("--cycles", type=int, default=4800)
    ap.add_argument("--batch-size", type=int, default=8000)
    ap.add_argument("--target", type=int, default=30000)
    ap.add_argument("--fixed-steps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", choices=("chained", "resident"), dest="path")
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.path:
        return child(args)

    import synthetic as syn

    work = tempfile.mkdtemp(prefix="adh_bench_optimization_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        t0 = time.perf_counter()
        case = syn.make_case(args.precursors, args.cycles, config_id=2, per_precursor=3, threads=_threads())
        for name in RUN_ARRAYS:
            np.save(os.path.join(work, name + ".npy"), getattr(case.dia, name))
        del case
        result = {"workload": f"{args.precursors} precursors x 3 candidates, {args.cycles} cycles (bench.py); lock batch "
                              f"size {args.batch_size} elution groups, target {args.target} at 1 % FDR, "
                              f"{args.fixed_steps} fixed steps; classifier {CLASSIFIER}",
                  "generate_s": round(time.perf_counter() - t0, 1)}
        for path in ("chained", "resident"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--work", work]
            for flag in ("precursors", "cycles", "batch_size", "target", "fixed_steps"):
                cmd += ["--" + flag.replace("_", "-"), str(getattr(args, flag))]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                raise SystemExit(f"{path} child failed with {p.returncode}")
            result[path] = json.loads(p.stdout.strip().splitlines()[-1])
        c, r = result["chained"], result["resident"]
        result["same_trajectory"] = [(s["batch_idx"], s["psm_at_1pct"], s["filtered"]) for s in c["steps"]] == [
            (s["batch_idx"], s["psm_at_1pct"], s["filtered"]) for s in r["steps"]]
        result["d2h_ratio"] = round(r["total_d2h_bytes"] / max(c["total_d2h_bytes"], 1), 4)
        result["total_ms_ratio"] = round(r["total_ms"] / max(c["total_ms"], 1e-9), 3)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
