"""What the candidate library of transfer-library requantification costs until it is staged and calibrated in HBM,
two ways, for 300 000 identified precursors:

  host    the library built on the host (``host_candidate_library``, the NumPy restatement of alphabase's build),
          then ``stage_fragments_calibrated``: the eight columns go up, one kernel packs and calibrates the records
  device  ``stage_candidate_library``: sequences and modification lists go up, one kernel builds the records

The string columns are turned into byte and offset arrays once, outside both clocks (both routes start from them; the
time is reported as ``tables_ms``).  Both routes are warmed up, then alternate for ``--repeats`` rounds in this one
process; each window ends in a device synchronise.  With ``--requantify N`` the whole ``requantify`` of both routes
(frames, scoring with ``top_k_fragments=9999``, fragment ranges) alternates N times over a synthetic run in which
``--planted`` of the precursors elute.  Prints one JSON object: the inputs (length distribution, series), per route
the median, minimum and maximum wall ms, the kernel ms (``adh_calibration_time_ms``), the bytes over the link in
each direction, and whether the two staged libraries and the two routes' frames are bit-equal.  No target is set.

    python tools/bench_transfer_requant.py [--psms 300000] [--repeats 7] [--requantify 3]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTE_COLUMNS = ("type", "loss_type", "charge", "number", "position", "cardinality")
N_CYCLES = 200


def draw_psms(n: int, seed: int) -> pd.DataFrame:
    """Tryptic-looking identifications: lengths 7 + Poisson(6) capped at 40, charge 2-3, one precursor in five
    carries an oxidation, one in ten an N-terminal acetylation as well."""
    import candidate_library_cases as G

    rng = np.random.default_rng(seed)
    L = np.minimum(7 + rng.poisson(6.0, n), 40)
    flat = rng.choice(G.LETTERS, int(L.sum()))
    stop = np.cumsum(L)
    joined = "".join(flat)
    sequence = np.array([joined[a:b] for a, b in zip(stop - L, stop)], dtype=object)
    mods, sites = np.full(n, "", dtype=object), np.full(n, "", dtype=object)
    inner = rng.integers(1, L + 1)
    ox = np.flatnonzero(rng.random(n) < 0.2)
    for p in ox:
        mods[p], sites[p] = "Oxidation@M", str(inner[p])
    for p in ox[::2]:
        mods[p], sites[p] = "Acetyl@Protein_N-term;" + mods[p], "0;" + sites[p]
    return pd.DataFrame({"sequence": sequence, "mods": mods, "mod_sites": sites,
                         "charge": rng.integers(2, 4, n).astype(np.uint8)})


def fitted_manager():
    from alphadia_amd import calibration as cal

    m = cal.HipCalibrationManager(path=None, load_from_file=False, has_ms1=True, has_mobility=False)
    e = m.get_estimator("fragment", "mz")
    e.model.n_kernels, e.model.polynomial_degree = 2, 1
    e.model.scale_mean, e.model.scale_max = np.array([400.0, 1600.0]), np.array([1500.0, 1500.0])
    e.model.beta = np.array([[0.0, 0.0], [1 + 2e-6, 1 + 3e-6]])
    e.is_fitted = True
    return m


def staging(ctx, model, args, repeats: int) -> dict:
    from alphadia_amd import _abi
    from alphadia_amd import transfer_requantification as trq

    tables = _abi.pack_candidate_library(*args)

    def host():
        t0 = time.perf_counter()
        _start, _stop, cols = trq.host_candidate_library(*args)
        t1 = time.perf_counter()
        y = ctx.stage_fragments_calibrated(model, cols["mz_library"], cols["intensity"], *(cols[k] for k in BYTE_COLUMNS))
        ctx.synchronize()
        return time.perf_counter() - t0, ctx.calibration_time_ms(), y, t1 - t0

    def device():
        t0 = time.perf_counter()
        _start, _stop, _mz_library, y = ctx.stage_candidate_library(tables, model)
        ctx.synchronize()
        return time.perf_counter() - t0, ctx.calibration_time_ms(), y, 0.0

    routes = {"host": host, "device": device}
    for f in routes.values():  # warm-up: page-locked slots, the library's blocks, the mirror's pages
        f()
        f()
    walls, kernels, builds, d2h = ({k: [] for k in routes} for _ in range(4))
    for _ in range(repeats):
        for name, f in routes.items():
            before = ctx.d2h_bytes()
            w, k, _y, b = f()
            d2h[name].append(ctx.d2h_bytes() - before)
            walls[name].append(w)
            kernels[name].append(k)
            builds[name].append(b)
    states = {}
    for name, f in routes.items():
        y = f()[2]
        states[name] = (ctx.staged_fragment_records().tobytes(), ctx.staged_fragment_records(host_mirror=True).tobytes(),
                        y.tobytes())
    rows = len(states["host"][2]) // 8
    n = len(args[0]) - 1
    h2d = {"host": 14 * rows,
           "device": int(args[1].nbytes + 2 * 8 * (n + 1) + 12 * len(args[3]) + 128 * 8 + 4 * (n + 1))}
    out = {"rows": rows, "repeats": repeats,
           "libraries_bit_equal": bool(states["host"] == states["device"] and states["host"][0] == states["host"][1])}
    for name in routes:
        out[name] = dict(median_ms=1e3 * float(np.median(walls[name])), min_ms=1e3 * min(walls[name]),
                         max_ms=1e3 * max(walls[name]), kernel_ms=float(np.median(kernels[name])),
                         host_build_ms=1e3 * float(np.median(builds[name])), h2d_bytes=h2d[name],
                         d2h_bytes=int(np.median(d2h[name])))
    return out


def requantify(psms: pd.DataFrame, args, series, planted_fraction: float, repeats: int, seed: int) -> dict:
    """Both routes' whole ``requantify`` over a synthetic run, alternating."""
    import candidate_library_cases as G
    import synthetic as syn
    from alphadia_amd import transfer_requantification as trq
    from alphadia_amd.extraction_handler import HipExtractionHandler

    n = len(psms)
    start, stop, cols = trq.host_candidate_library(*args)
    at = start.astype(np.int64)
    peptide = cols["mz_library"].astype(np.float64)[at] + cols["mz_library"].astype(np.float64)[at + len(series[0]) // 2] \
        - 2 * G.MASS_PROTON
    rng = np.random.default_rng([seed, 1])
    precursor_df = pd.DataFrame({
        "elution_group_idx": np.arange(n, dtype=np.uint32), "precursor_idx": np.arange(n, dtype=np.uint32),
        "channel": np.zeros(n, dtype=np.uint32), "decoy": np.zeros(n, dtype=np.uint8),
        "flat_frag_start_idx": start, "flat_frag_stop_idx": stop, "charge": psms["charge"].to_numpy(),
        "rt_library": rng.uniform(0, N_CYCLES * 1.5, n).astype(np.float32), "mobility_library": np.zeros(n, dtype=np.float32),
        "mz_library": (peptide / psms["charge"].to_numpy() + G.MASS_PROTON).astype(np.float32),
        "proteins": np.full(n, "P", dtype=object), "genes": np.full(n, "G", dtype=object),
        "sequence": psms["sequence"].to_numpy(), "mods": psms["mods"].to_numpy(), "mod_sites": psms["mod_sites"].to_numpy()})
    for i, share in enumerate((0.5, 0.3, 0.2)):
        precursor_df[f"i_{i}"] = np.float32(share)
    lib = syn.SyntheticLibrary(precursor_df, pd.DataFrame(cols))
    lo, hi = float(precursor_df["mz_library"].min()) - 1, float(precursor_df["mz_library"].max()) + 1
    cycle = syn.make_cycle(n_ms2=40, mz_lo=lo, mz_hi=hi)
    planted = syn.plant_peptides(lib, cycle, N_CYCLES, seed, fraction=planted_fraction)
    dia = syn.make_thermo_run(N_CYCLES, seed, cycle=cycle, ms1_peaks=2000, ms2_peaks=800, planted=planted, threads=8,
                              ms1_mz_range=(lo, hi), ms2_mz_range=(50.0, 4000.0))
    psm = syn.make_candidates(lib, N_CYCLES, cycle.shape[1], seed, per_precursor=1, apex_cycle=planted.apex_cycle)
    for c in ("channel", "rt_library", "mz_library", "mobility_library", "genes", "proteins", "decoy", "mods", "mod_sites",
              "sequence", "charge"):
        psm[c] = precursor_df[c].to_numpy()
    psm["proba"] = rng.random(n).astype(np.float32)
    psm["qval"] = 0.001
    psm["rt_observed"], psm["mobility_observed"], psm["mz_observed"] = psm["rt_library"], psm["mobility_library"], psm["mz_library"]

    config = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                         "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
              "general": {"thread_count": 8}, "fdr": {"fdr": 0.01, "competitive_scoring": True, "channel_wise_fdr": False},
              "transfer_library": {"fragment_types": ["b", "y"], "max_charge": len(series[0]) // 2}}
    names = SimpleNamespace(get_rt_column=lambda: "rt_library", get_mobility_column=lambda: "mobility_library",
                            get_precursor_mz_column=lambda: "mz_library", get_fragment_mz_column=lambda: "mz_calibrated")
    opt = SimpleNamespace(ms1_error=10, ms2_error=15, rt_error=30.0, mobility_error=0.1, num_candidates=1, fwhm_rt=5.0,
                          fwhm_mobility=0.01, score_cutoff=0.0, classifier_version=-1)
    reporter = SimpleNamespace(log_string=lambda *a, **k: None)
    manager = fitted_manager()
    handler = trq.HipTransferLibraryRequantificationHandler(config, manager, opt, None, names, reporter, G.aa_mass_table(),
                                                            G.MOD_MASS, G.MASS_PROTON, G.MASS_H2O, device=0)

    def device():
        return handler.requantify(dia, psm)

    def host():
        scored = trq.candidate_features_to_candidates(psm, trq.OPTIONAL_CANDIDATE_COLUMNS)
        arrays = trq.candidate_library_tables(scored["sequence"].to_numpy(), scored["mods"].to_numpy(),
                                              scored["mod_sites"].to_numpy(), G.MOD_MASS)
        s, e, c = trq.host_candidate_library(arrays["seq_offset"], arrays["residues"], arrays["mod_offset"],
                                             arrays["mod_site"], arrays["mod_mass"], G.aa_mass_table(), G.MASS_PROTON,
                                             G.MASS_H2O, *series[1:])
        scored["nAA"] = np.diff(arrays["seq_offset"])
        scored["flat_frag_start_idx"], scored["flat_frag_stop_idx"] = s, e
        manager.predict(scored, "precursor")
        fragment_df = trq.fragment_frame(c)
        manager.predict_staged(fragment_df, "fragment", device=0)  # (stage_fragments_calibrated + adopt)
        extraction = HipExtractionHandler(config, opt, None, reporter, names, device=0)
        _, frag = extraction.quantify_candidates(scored, None, dia, SimpleNamespace(precursor_df=scored, fragment_df=fragment_df),
                                                 top_k_fragments=9999)
        return trq.index_fragments(scored, frag)

    routes = {"host": host, "device": device}
    results = {k: f() for k, f in routes.items()}  # warm-up, and the frames to compare
    equal = all(a.equals(b) for a, b in zip(results["host"], results["device"]))
    walls = {k: [] for k in routes}
    for _ in range(repeats):
        for name, f in routes.items():
            t0 = time.perf_counter()
            f()
            walls[name].append(time.perf_counter() - t0)
    out = {"repeats": repeats, "planted_fraction": planted_fraction, "n_cycles": N_CYCLES, "peaks": int(len(dia.mz_values)),
           "fragment_rows_returned": int(len(results["device"][1])), "candidates_with_fragments": int(len(results["device"][0])),
           "frames_equal": bool(equal), "device_stages_ms": {k: float(v) for k, v in handler.last_timings.items()}}
    for name in routes:
        out[name] = dict(median_ms=1e3 * float(np.median(walls[name])), min_ms=1e3 * min(walls[name]), max_ms=1e3 * max(walls[name]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--psms", type=int, default=300_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--requantify", type=int, default=3, help="rounds of the whole requantify (0: skip)")
    ap.add_argument("--planted", type=float, default=0.02)
    ap.add_argument("--max-charge", type=int, default=2)
    args = ap.parse_args()

    import candidate_library_cases as G
    from alphadia_amd import runtime

    ctx = runtime.get_context(0)
    seed = 20261020
    psms = draw_psms(args.psms, seed)
    t0 = time.perf_counter()
    _, series, host_args = G.tables_of(psms, max_charge=args.max_charge)
    tables_ms = 1e3 * (time.perf_counter() - t0)
    lengths = psms["sequence"].str.len().to_numpy()
    out = {"device": "cuda:0", "psms": int(args.psms), "series": series[0], "tables_ms": tables_ms,
           "lengths": {"distribution": "7 + Poisson(6), capped at 40", "mean": float(lengths.mean()),
                       "min": int(lengths.min()), "max": int(lengths.max())},
           "modified_fraction": float((psms["mods"] != "").mean()), "host_threads": list(runtime.host_threads(12_000_000)),
           "staging": staging(ctx, fitted_manager().get_estimator("fragment", "mz").model, host_args, args.repeats)}
    if args.requantify:
        out["requantify"] = requantify(psms, host_args, series, args.planted, args.requantify, seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
