"""The selection -> scoring hand-over against the frame path it replaces, from the selection call to the end of
``score_resident``, in one process and alternating:

    frame path   HipCandidateSelection.__call__ (33 B per table row to the host, score > 0, DataFrame, merge), the cutoff
                 filter of the extraction handler, scoring.assemble_candidates, upload, scoring kernels
    hand-over    select_resident (the table stays in HBM, adh_assemble_selected), score_resident(ResidentCandidates)
                 (adh_score_selected_resident; 5 B per kept row to the host for the ids)

Every window is closed by a device synchronise.  Sizes: ``headline`` (1 M precursors x 3 candidates, 4 800 cycles),
``100k`` (100 000 precursors, 4 800 cycles), ``im`` (BASELINE configs[3], the ion-mobility run of tools/bench_timstof.py).
Writes / updates profiles/select_handover_bench.json (``--out`` elsewhere), one entry per size.  Run on the GPU box from
the repo root:  python tools/bench_select_handover.py --size 100k [--reps 9]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # synthetic data generators
import synthetic as syn  # noqa: E402
from alphadia_amd import runtime  # noqa: E402
from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring  # noqa: E402
from alphadia_amd.selection import CandidateSelectionConfig, HipCandidateSelection  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", choices=["headline", "100k", "im"], default="100k")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--precursors", type=int, default=0, help="override the precursor count of the size")
ap.add_argument("--cycles", type=int, default=0, help="override the cycle count of the size")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_handover_bench.json"))
args = ap.parse_args()
threads = min(16, os.cpu_count() or 8)
t_gen = time.time()
names = dict(rt_column="rt_library", mobility_column="mobility_library", precursor_mz_column="mz_library",
             fragment_mz_column="mz_library")
sel_cfg = CandidateSelectionConfig()
if args.size == "im":
    n_prec, n_cycles = args.precursors or 200000, args.cycles or 2000
    case = syn.make_timstof_case(
        n_precursors=n_prec, n_cycles=n_cycles, config_id=4, per_precursor=1, n_ms2_frames=8, windows_per_frame=3,
        scan_max_index=int(os.environ.get("SCAN_MAX", 918)), n_tof=int(os.environ.get("N_TOF", 400000)),
        events_per_push=float(os.environ.get("EVENTS_PER_PUSH", 30.0)), mz_lo=400.0, mz_hi=1000.0, frag_mz_lo=200.0,
        frag_mz_hi=1000.0, tof_mz_lo=195.0, tof_mz_hi=1010.0, planted_fraction=0.3, threads=threads)
    case.dia.has_mobility = True
    sel_cfg.update(dict(rt_tolerance=15.0, mobility_tolerance=0.1, candidate_count=3, peak_len_rt=3.0, sigma_scale_rt=0.5,
                        peak_len_mobility=0.02))
    fwhm = dict(fwhm_rt=3.0, fwhm_mobility=0.02)
    workload = f"BASELINE configs[3]: {case.dia.push_indices.size / 1e6:.0f}M events, {n_cycles} cycles"
else:
    n_prec, n_cycles = args.precursors or (1000000 if args.size == "headline" else 100000), args.cycles or 4800
    case = syn.make_case(n_prec, n_cycles, config_id=2, per_precursor=1, threads=threads)
    sel_cfg.update(dict(rt_tolerance=60.0, candidate_count=3))
    fwhm = dict(fwhm_rt=sel_cfg.peak_len_rt)
    workload = f"{n_cycles} cycles x 61 spectra"
t_gen = time.time() - t_gen
pdf, fdf = case.library.precursor_df, case.library.fragment_df
score_cfg = CandidateScoringConfig()
score_cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                      experimental_xic=True))
selection = HipCandidateSelection(case.dia, pdf, fdf, sel_cfg, device=0, **names, **fwhm)
scorer = HipCandidateScoring(dia_data=case.dia, precursors_flat=pdf, fragments_flat=fdf, config=score_cfg, device=0, **names)
ctx = runtime.get_context(0)
CUTOFF = 0.0  # the optimisation manager's initial score_cutoff: "filter 1" runs and keeps every row


def frame_path():
    ctx.device_synchronize()
    t0 = time.perf_counter()
    frame = selection()
    frame = frame[frame["score"] > CUTOFF]
    ctx.device_synchronize()
    t1 = time.perf_counter()
    res = scorer.score_resident(frame)
    ctx.device_synchronize()
    t2 = time.perf_counter()
    return dict(select_ms=(t1 - t0) * 1e3, score_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3,
                select_kernel_ms=ctx.select_time_ms()), res.n_table


def handover():
    ctx.device_synchronize()
    t0 = time.perf_counter()
    selected = selection.select_resident(apply_cutoff=True, score_cutoff=CUTOFF)
    ctx.device_synchronize()
    t1 = time.perf_counter()
    res = scorer.score_resident(selected)
    ctx.device_synchronize()
    t2 = time.perf_counter()
    return dict(select_ms=(t1 - t0) * 1e3, score_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3,
                select_kernel_ms=ctx.select_time_ms(), assemble_ms=ctx.select_handover_stats()["assemble_ms"]), res.n_table


def summary(runs):
    out = {}
    for key in runs[0]:
        v = np.array([r[key] for r in runs])
        out[key] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
    return out


old_runs, new_runs, rows = [], [], None
for i in range(args.warmup + args.reps):
    ctx.d2h_bytes(reset=True)
    o, n_old = frame_path()
    d2h_old = ctx.d2h_bytes(reset=True)
    n, n_new = handover()
    d2h_new = ctx.d2h_bytes(reset=True)
    assert n_old == n_new, (n_old, n_new)
    rows = n_new
    if i >= args.warmup:
        old_runs.append(o)
        new_runs.append(n)
old, new = summary(old_runs), summary(new_runs)
spread = (old["total_ms"]["max"] - old["total_ms"]["min"]) + (new["total_ms"]["max"] - new["total_ms"]["min"])
gain = old["total_ms"]["median"] - new["total_ms"]["median"]
entry = {
    "workload": f"{n_prec} precursors x {int(sel_cfg.candidate_count)} candidates, {workload}; {rows} rows kept "
                f"(score > 0 and score > {CUTOFF})",
    "timed_region": "selection call -> end of score_resident, device synchronised at every stage boundary",
    "reps": args.reps, "warmup": args.warmup, "alternating": True, "generate_s": t_gen,
    "frame_path": old, "handover": new,
    "d2h_bytes": {"frame_path": int(d2h_old), "handover": int(d2h_new)},
    "handover_stats": ctx.select_handover_stats(),
    "median_gain_ms": gain, "min_max_spreads_ms": spread,
    "clears_the_bar": bool(gain > spread),
    "bar": "median below the frame path's by more than the two min-max spreads together (DESIGN section 8)",
}
record = {}
if os.path.exists(args.out):
    try:
        record = json.load(open(args.out))
    except Exception:
        record = {}
record[args.size if not (args.precursors or args.cycles) else f"{args.size}_{n_prec}x{n_cycles}"] = entry
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
print(json.dumps(entry))
