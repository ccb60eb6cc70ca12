"""Label-free quantification after the fragment matrices: accumulate, then per level (precursor, peptide, protein
group) filter_frag_df and direct_lfq, on the cohort of tools/bench_quant.py.  The device path
(alphadia_amd.lfq.direct_lfq on the matrices in HBM) and the NumPy restatement (host_direct_lfq, pure Python over
every group) alternate in one process; medians with min - max go to the record.  No ratio is fixed: the record is the
claim.  The host side runs at a smaller cohort (--host-precursors, --host-runs), which the record states; the device
runs there too, and at the full cohort on its own.

    python tools/bench_lfq.py --runs 20 60 --repeat 3 --out profiles/lfq_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_quant import LEVELS, cohort  # noqa: E402

SETTINGS = dict(min_nonan=3, num_samples_quadratic=50, normalize=True)


def filtered_frames(psm, runs):
    from alphadia_amd import quant as Q

    t0 = time.perf_counter()
    acc = Q.HipFragmentQuantLoader(psm).accumulate(iter(runs))
    t1 = time.perf_counter()
    frames = {}
    for level in LEVELS:
        frames[level], _ = Q.filter_frag_df(acc["intensity"], acc["correlation"], min_correlation=0.5, top_n=3,
                                            group_column=level)
    return acc, frames, t1 - t0, time.perf_counter() - t1


def device_lfq(frames):
    from alphadia_amd import lfq

    out = {}
    for level, frame in frames.items():
        t = time.perf_counter()
        res = lfq.direct_lfq(frame, level, **SETTINGS)
        s = time.perf_counter() - t
        prepare, sample, groups = lfq._filtered(frame, lfq.run_columns(frame)).quant.lfq_time_ms()
        out[level] = dict(seconds=s, rows=len(frame), groups_out=len(res), prepare_ms=prepare, sample_ms=sample,
                          group_kernels_ms=groups)
    return out


def host_lfq(frames):
    from alphadia_amd import lfq

    out = {}
    for level, frame in frames.items():
        t = time.perf_counter()
        res = lfq.host_direct_lfq(frame, level, **SETTINGS)
        out[level] = dict(seconds=time.perf_counter() - t, rows=len(frame), groups_out=len(res))
    return out


def spread(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4))


def summarise(reps):
    res = {}
    for level in LEVELS:
        res[level] = {k: reps[0][level][k] for k in ("rows", "groups_out")}
        res[level]["seconds"] = spread([r[level]["seconds"] for r in reps])
        for k in ("prepare_ms", "sample_ms", "group_kernels_ms"):
            if k in reps[0][level]:
                res[level][k] = spread([r[level][k] for r in reps])
    res["three_levels_s"] = spread([sum(r[level]["seconds"] for level in LEVELS) for r in reps])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, nargs="+", default=[20, 60])
    ap.add_argument("--precursors", type=int, default=100_000)
    ap.add_argument("--host-precursors", type=int, default=30_000)
    ap.add_argument("--host-runs", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(settings=SETTINGS, fragments=12, present=0.8, repeat=a.repeat,
               host="alphadia_amd.lfq.host_direct_lfq: this repository's NumPy restatement; directlfq is not installed",
               results={})

    def save():  # (after every stage: a run cut short keeps what it measured)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    psm, runs = cohort(3, n_prec=500)
    device_lfq(filtered_frames(psm, runs)[1])  # warm-up: context, kernels, allocator

    # host against device, alternating, at the smaller cohort
    psm, runs = cohort(a.host_runs, n_prec=a.host_precursors)
    acc, frames, _, _ = filtered_frames(psm, runs)
    dev, host = [], []
    for _ in range(a.repeat):
        dev.append(device_lfq(frames))
        host.append(host_lfq(frames))
        print(f"host cohort: repeat {len(host)} of {a.repeat} done", flush=True)
    out["results"]["host_cohort"] = dict(precursors=a.host_precursors, runs=a.host_runs, device=summarise(dev),
                                         host=summarise(host))
    print(json.dumps(out["results"]["host_cohort"]), flush=True)
    save()
    del acc, frames

    # the device alone at the full cohort
    for n in a.runs:
        psm, runs = cohort(n, n_prec=a.precursors)
        acc, frames, acc_s, filt_s = filtered_frames(psm, runs)
        dev = [device_lfq(frames) for _ in range(a.repeat)]
        out["results"][f"device_{n}_runs"] = dict(precursors=a.precursors, runs=n, keys=len(acc["intensity"]),
                                                  accumulate_s=round(acc_s, 4), three_filters_s=round(filt_s, 4),
                                                  device=summarise(dev))
        print(json.dumps(out["results"][f"device_{n}_runs"]), flush=True)
        del acc, frames
        save()


if __name__ == "__main__":
    main()
