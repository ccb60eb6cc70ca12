"""Per-file extraction at the headline size: the chained calls against HipExtractionHandler.extract.

The workload of bench.py (1e6 precursors x 3 candidates, 4800 cycles: ``syn.make_case(1_000_000, 4800, config_id=2,
per_precursor=3)``) and the production FDR hyper-parameters of tools/bench_fdr.py.  The case's candidate table
stands in for the selection step (the same table for both paths).  Each path runs in a child process of its own:
one warm-up call, then a timed call with a fresh FDR manager of the same seed.  Per path: wall ms per stage
(the handler's ``last_timings``), bytes copied device -> host (``ctx.d2h_bytes``), survivor and fragment rows, and
the child's peak RSS (``ru_maxrss``; with the resident set before its first call); and whether both paths return
the same frames (the bounds of tests/test_extraction_resident_gpu.py).  Prints one JSON line.

    python tools/bench_extraction.py [--precursors 1000000] [--cycles 4800] [--out profiles/extraction_bench.json]
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


def child(args):
    from types import SimpleNamespace

    import synthetic as syn
    from alphadia_amd import fdr, runtime
    from alphadia_amd.extraction_handler import HipExtractionHandler
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    light = syn.make_case(args.precursors, args.cycles, config_id=2, per_precursor=3, threads=1, run=False)
    dia = syn.AlphaRawArrays(**{n: np.load(os.path.join(args.work, n + ".npy"), mmap_mode="r") for n in RUN_ARRAYS})
    lib = SimpleNamespace(precursor_df=light.library.precursor_df, fragment_df=light.library.fragment_df)
    cands = light.candidates_df
    features = [c for c in DEFAULT_FEATURE_COLUMNS if c not in ("mobility_observed", "base_width_mobility")] + [
        "delta_rt", "mz_library", "charge", "n_K", "n_R", "n_P"]
    config = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                         "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
              "general": {"thread_count": _threads()},
              "fdr": {"fdr": 0.01, "competitive_scoring": True, "channel_wise_fdr": False}}
    opt = SimpleNamespace(ms1_error=10, ms2_error=15, score_cutoff=-np.inf, classifier_version=-1)
    names = SimpleNamespace(get_rt_column=lambda: "rt_library", get_mobility_column=lambda: "mobility_library",
                            get_precursor_mz_column=lambda: "mz_library", get_fragment_mz_column=lambda: "mz_library")
    reporter = SimpleNamespace(log_string=lambda *a, **k: None)
    selection = SimpleNamespace(select_candidates=lambda *a, **k: cands)
    ctx = runtime.get_context(0)
    with open("/proc/self/statm") as f:  # resident set before the first call: imports, library, mapped run untouched
        rss_base_mb = int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2**20

    def once():
        manager = fdr.HipFDRManager(features, fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=dia.cycle, random_state=42,
                                    device=0)
        h = HipExtractionHandler(config, opt, manager, reporter, names, selection_handler=selection, device=0)
        ctx.d2h_bytes(reset=True)
        if args.path == "resident":
            out = h.extract(dia, lib)
        else:
            t_0 = time.perf_counter()
            out = h._extract_chained(h.select_candidates(dia, lib, apply_cutoff=True), dia, lib, t_0)
        return out, dict(h.last_timings), ctx.d2h_bytes()

    once()  # warm-up: staging, buffers, kernels loaded
    (pre, frag), timings, d2h = once()
    assert timings["path"] == args.path
    pre.to_pickle(os.path.join(args.work, args.path + "_precursor.pkl"))
    frag.to_pickle(os.path.join(args.work, args.path + "_fragments.pkl"))
    print(json.dumps({"stages_ms": {k: round(v, 1) for k, v in timings.items() if k.endswith("_ms")}, "d2h_bytes": d2h,
                      "survivors": len(pre), "fragment_rows": len(frag), "table_rows": len(cands),
                      "rss_before_first_call_mb": round(rss_base_mb, 1),
                      "peak_rss_mb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)}))


def same_frames(work) -> dict:
    import pandas as pd

    out = {}
    for what in ("precursor", "fragments"):
        a = pd.read_pickle(os.path.join(work, f"resident_{what}.pkl"))
        b = pd.read_pickle(os.path.join(work, f"chained_{what}.pkl"))
        why = None
        if list(a.columns) != list(b.columns):
            why = "columns"
        elif len(a) != len(b):
            why = f"rows {len(a)} / {len(b)}"
        else:
            for c in a.columns:
                x, y = a[c], b[c]
                if x.dtype != y.dtype:
                    why = f"dtype of {c}"
                elif c == "proba":
                    ok = np.allclose(x.to_numpy(), y.to_numpy(), rtol=0, atol=1e-6)
                elif c == "qval":
                    ok = np.allclose(x.to_numpy(), y.to_numpy(), rtol=1e-12, atol=0)
                elif x.dtype == object:
                    ok = bool((x.to_numpy() == y.to_numpy()).all())
                else:
                    ok = np.array_equal(x.to_numpy(), y.to_numpy(), equal_nan=True)
                if why is None and not ok:
                    why = f"values of {c}"
                if why:
                    break
        out[what] = "equal" if why is None else f"differ: {why}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precursors", type=int, default=1_000_000)
    ap.add_argument("--cycles", type=int, default=4800)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", choices=("chained", "resident"), dest="path")
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.path:
        return child(args)

    import synthetic as syn

    work = tempfile.mkdtemp(prefix="adh_bench_extraction_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        t0 = time.perf_counter()
        case = syn.make_case(args.precursors, args.cycles, config_id=2, per_precursor=3, threads=_threads())
        for name in RUN_ARRAYS:
            np.save(os.path.join(work, name + ".npy"), getattr(case.dia, name))
        del case
        gen_s = time.perf_counter() - t0
        result = {"workload": f"{args.precursors} precursors x 3 candidates, {args.cycles} cycles (bench.py), "
                              f"competitive FDR at 1 %, classifier {CLASSIFIER}", "generate_s": round(gen_s, 1)}
        for path in ("chained", "resident"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--work", work,
                                "--precursors", str(args.precursors), "--cycles", str(args.cycles)],
                               capture_output=True, text=True, cwd=ROOT)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                raise SystemExit(f"{path} child failed with {p.returncode}")
            result[path] = json.loads(p.stdout.strip().splitlines()[-1])
        result["same_frames"] = same_frames(work)
        c, r = result["chained"], result["resident"]
        result["d2h_ratio"] = round(r["d2h_bytes"] / max(c["d2h_bytes"], 1), 4)
        result["total_ms_ratio"] = round(r["stages_ms"]["total_ms"] / max(c["stages_ms"]["total_ms"], 1e-9), 3)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
