"""The shape sweep of tests/box_sweep.py meets its coverage conditions with the ORACLE alone (no GPU): under every
scoring configuration of tests/test_kernel_classes_gpu.py each kernel class the configuration can reach holds enough
candidates the oracle scores as valid, on both sides of every class edge.  These are conditions on the inputs of the
GPU tests, not measurements of the kernels."""

import os
import subprocess
import sys

import numpy as np
import pytest

import box_sweep as bs
import helpers as H

sys.path.insert(0, H.GOLDEN_DIR)
import ref_shim  # noqa: E402  (importing it runs nothing of the reference)

MIN_ROWS, MIN_VALID, MIN_EDGE, MIN_NL = 8, 3, 2, 2
# A library slice of 1, 2 or 3 fragments is in the sweep for the routing and the tables (all zero), but no such row
# can be valid: the reference leaves a candidate with at most three fragments early (candidate.py:190).
NL_NEVER_VALID = (1, 2, 3)


@pytest.fixture(scope="module")
def sweeps():
    out = {}
    for ragged in (False, True):
        case = bs.sweep_case(ragged)
        out[ragged] = (case, H.soa_for(case, bs.config_of("defaults")), bs.spec_rows(ragged))
    return out


def test_sweep_is_what_its_specification_says(sweeps):
    for ragged, (case, soa, spec) in sweeps.items():
        assert len(spec) < 1500
        t = bs.shape_table(case, soa, bs.config_of("defaults"))
        assert np.array_equal(t["F"], spec["F"]) and np.array_equal(t["O"], spec["O"]) and np.array_equal(t["nl"], spec["nl"])
        assert set(spec["F"]) == set(range(2, 37))
        L, n_spectra = case.dia.cycle_len, case.dia.n_spectra
        assert n_spectra % L != 0  # the run ends inside a cycle
        start, stop, centre = soa["frame_start"], soa["frame_stop"], soa["frame_center"]
        assert (start % L == 0).all() and (stop <= n_spectra).all() and (start <= centre).all() and (centre < stop).all()
        for F in range(2, 37):
            m = spec["F"].values == F
            c0, ce = start[m] // L, centre[m] // L
            assert {0, F // 2, F - 1} <= set((ce - c0).tolist()), F                  # centre first / middle / last
            assert (c0 == 0).any() and (stop[m] == n_spectra).any() and (stop[m] == (n_spectra // L) * L).any(), F
            assert ((c0 > 0) & (stop[m] < (n_spectra // L) * L)).any(), F
        # the planted apex lies inside its box
        assert ((case.apex_cycle >= start // L) & (case.apex_cycle < stop // L)).all()
        # one isotope or four: the observation count is what the sweep asked for
        for name in ("isotopes1", "isotopes4"):
            assert np.array_equal(bs.shape_table(case, soa, bs.config_of(name))["O"], spec["O"])
        assert set(spec["nl"]) == ({12} if not ragged else set(bs.NL_ALL) | {bs.NL_LONG_OTHERWISE})


def _feature_lds_bytes(K, O, F, I):
    """feat::Layout::bytes() of the generic kernel (alphadia_amd/csrc/adh_features.hip)."""
    n_double = O * 2 * F + 2 * F + I * O + 2 * K * O + 4 * K + 2 * O + 2 * I
    n_float = 3 * K * O * F + 2 * I * F + 2 * O * F + K * F + 6 * K + 3 * K * O + 4 * O + 3 * I + 3 * F + 46
    n_int = 3 * K + K * O + O
    return n_double * 8 + (n_float * 4 + 7) // 8 * 8 + (n_int * 4 + 7) // 8 * 8 + (5 * K + 7) // 8 * 8


def test_no_batch_of_the_sweep_must_be_refused(sweeps):
    """The generic kernel's tile is sized by the maxima over a batch; with every candidate in that class
    (ADH_DEBUG_NO_FAST) each batch of the sweep stays within the 160 KiB of LDS the plan allows."""
    _, _, spec = sweeps[True]
    for b in (0, 1):
        s = spec[spec["batch"] == b]
        assert len(s) >= 8
        assert _feature_lds_bytes(int(s["nl"].max()), 2, int(s["F"].max()), 4) <= 160 * 1024
    assert _feature_lds_bytes(bs.NL_LONG, 2, 36, 3) > 160 * 1024  # (why there are two batches)


def test_class_rule_restated():
    kw = dict(I=3, experimental_xic=True, quant_all=True)
    assert bs.plan_class(3, 1, 12, 12, **kw) == 0 and bs.plan_class(8, 1, 12, 12, **kw) == 0
    assert bs.plan_class(9, 1, 12, 12, **kw) == 1 and bs.plan_class(32, 1, 12, 12, **kw) == 6
    assert bs.plan_class(32, 2, 12, 64, **kw) == 13 and bs.plan_class(32, 2, 12, 65, **kw) == 16
    assert bs.plan_class(2, 1, 12, 12, **kw) == 36 and bs.plan_class(33, 1, 12, 12, **kw) == 36
    assert bs.plan_class(16, 2, 16, 16, **kw) == 14 and bs.plan_class(17, 2, 13, 13, **kw) == 15
    assert bs.plan_class(29, 1, 16, 200, **kw) == 23 and bs.plan_class(5, 1, 13, 13, **kw) == 17
    assert bs.plan_class(16, 2, 64, 64, **kw) == 24 and bs.plan_class(25, 1, 33, 33, **kw) == 29
    assert bs.plan_class(24, 2, 17, 17, **kw) == 31 and bs.plan_class(3, 1, 32, 32, **kw) == 33
    assert bs.plan_class(16, 1, 65, 65, **kw) == 36
    assert bs.plan_class(16, 2, 64, 64, I=3, experimental_xic=True, quant_all=False) == 36
    assert bs.plan_class(16, 2, 12, 12, I=3, experimental_xic=True, quant_all=False) == 9   # the fused kernel picks one
    assert bs.plan_class(16, 2, 13, 13, I=3, experimental_xic=True, quant_all=False) == 36
    assert bs.plan_class(16, 1, 12, 12, I=3, experimental_xic=False, quant_all=True) == 36
    assert bs.plan_class(16, 1, 12, 12, n_ms1_rows=2, **kw) == 19                           # no fused kernel
    assert bs.plan_class(16, 1, 12, 12, no_fused=True, **kw) == 19
    assert bs.plan_class(16, 2, 12, 12, no_fused2=True, **kw) == 14 and bs.plan_class(16, 1, 12, 12, no_fused2=True, **kw) == 2
    assert bs.plan_class(16, 1, 40, 40, no_wide=True, **kw) == 36 and bs.plan_class(16, 1, 12, 12, no_fast=True, **kw) == 36
    assert bs.plan_class(16, 3, 12, 12, **kw) == 36 and bs.plan_class(16, 0, 12, 12, **kw) == 36


@pytest.mark.parametrize("name", list(bs.CONFIGS))
def test_sweep_covers_every_class_and_edge(oracle_lib, sweeps, name):
    ragged = bs.CONFIGS[name][0]
    case, soa, spec = sweeps[ragged]
    cfg = bs.config_of(name)
    exp, _ = H.oracle_score(oracle_lib, case, cfg, soa=soa, n_threads=4)
    valid = exp["valid"].astype(bool)
    classes = bs.classes_of(case, soa, cfg)
    hist, hist_valid = bs.histogram(classes), bs.histogram(classes[valid])
    print(f"[sweep coverage] {name}: {len(valid)} candidates, {int(valid.sum())} valid\n  all   {hist.tolist()}\n  valid {hist_valid.tolist()}")
    # every class the configuration can reach, and no other
    assert set(np.flatnonzero(hist)) == bs.REACHES[name]
    for c in bs.REACHES[name]:
        assert hist[c] >= MIN_ROWS and hist_valid[c] >= MIN_VALID, (c, hist[c], hist_valid[c])
    # both sides of every edge of the cycle count, for one and for two observations
    F, O, nl = spec["F"].values, spec["O"].values, spec["nl"].values
    for edge in bs.F_EDGES:
        for f in edge:
            for o in (1, 2):
                assert (valid & (F == f) & (O == o)).sum() >= MIN_EDGE, (f, o)
    for f in (5, 30, 31, 32, 33):  # (the shapes no other generator makes)
        assert (valid & (F == f)).sum() >= MIN_EDGE, f
    # every slice length
    for k in sorted(set(nl.tolist())):
        if k in NL_NEVER_VALID:
            assert not (valid & (nl == k)).any()
        else:
            assert (valid & (nl == k)).sum() >= MIN_NL, k
    if ragged:  # the register axes at the slice lengths where the kernel family changes
        for k in (16, 17, 32, 33, 64, 65):
            for f in bs.F_EDGE_VALUES:
                for o in (1, 2):
                    assert (valid & (nl == k) & (F == f) & (O == o)).any(), (k, f, o)
        assert {62, 63, 64, 65, 80, 200} <= set(nl[valid].tolist())


def test_configurations_reach_all_classes():
    assert set().union(*bs.REACHES.values()) == set(range(bs.N_CLASSES))


def test_fixtures_hold_the_shapes_they_are_for():
    """tests/golden/scoring_boxes*.npz (the thinned sweep through the reference): every cycle count 2 ... 36 on a valid
    row, both observation counts, slices of 62 ... 65 and more fragments, and a batch the plan does not refuse."""
    for name, ragged in (("boxes", False), ("boxes_ragged", True)):
        g = H.load_scoring_golden(name)
        spec = bs.spec_rows(ragged, golden=True)
        assert len(spec) == len(g.candidates_df) and os.path.getsize(H.golden_path(f"scoring_{name}.npz")) < 1024 * 1024
        v = g.expected["valid"].astype(bool)
        assert set(spec["F"][v]) == set(range(2, 37)) and {1, 2} == set(spec["O"][v])
        assert (g.expected["features"][v][:, 17] == spec["O"][v]).all()
        assert _feature_lds_bytes(int(spec["nl"].max()), 2, int(spec["F"].max()), 4) <= 160 * 1024
        if ragged:
            assert {16, 17, 32, 33, 62, 63, 64, 65, 80, 120} <= set(spec["nl"][v])
            assert int(g.config.top_k_fragments) == 9999 and not g.config.quant_all
        else:
            assert int(g.config.quant_window) == 5 and g.config.quant_all


@pytest.mark.skipif(not os.path.isdir(ref_shim.REFERENCE_ROOT), reason="the reference checkout is not on this machine")
def test_regenerating_the_box_goldens_reproduces_the_committed_files(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(H.GOLDEN_DIR, "make_golden.py"), "--out", str(tmp_path), "--boxes-only"],
                       capture_output=True, text=True, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for name in ("scoring_boxes.npz", "scoring_boxes_ragged.npz"):
        fresh, golden = np.load(tmp_path / name), np.load(H.golden_path(name))
        assert sorted(fresh.files) == sorted(golden.files), name
        for key in golden.files:
            assert fresh[key].dtype == golden[key].dtype, (name, key)
            assert np.array_equal(fresh[key], golden[key], equal_nan=golden[key].dtype.kind == "f"), (name, key)
