"""The ion-mobility shape sweep of tests/box_sweep_im.py meets its coverage conditions with the ORACLE alone (no GPU):
the boxes are what the specification says, the two restated routing rules are pinned on hand-written cases on both sides
of every limit and the launch rule is held equal to the library's own (``adh_im_launch_routes``), every (plan class, layout, launch) a configuration can reach holds enough candidates the oracle scores as
valid, the designed event counts of the density rows - counted from the run arrays - lie on the designed side of the
capacities of the gather kernel, and no batch needs more LDS than a launch may have.  These are conditions on the
inputs of tests/test_kernel_classes_im_gpu.py, not measurements of the kernels."""

import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import box_sweep_im as bi
import helpers as H
from alphadia_amd.scoring import fragment_columns, pack_assembled

sys.path.insert(0, H.GOLDEN_DIR)
import ref_shim  # noqa: E402  (importing it runs nothing of the reference)

MIN_ROWS, MIN_VALID, MIN_EDGE = 8, 3, 2
NL_NEVER_VALID = (1, 2, 3)   # the reference leaves a candidate with at most three fragments early (candidate.py:190)
# A tile with every cell of every plane non-zero holds 1.5 times the entries that fit where the tiles would be (8-byte
# cells against 12-byte entries) and cannot hold more; the 32-byte round-up of the smallest block (2 scans x 3 cycles:
# 90 entries against 61) takes 0.025 off that.  Every other designed count keeps the factor bi.MARGIN.
FULL_TILE_MARGIN = 1.45


@pytest.fixture(scope="module")
def sweeps():
    out = {}
    for run in bi.RUNS:
        case = bi.sweep_case(run)
        out[run] = (case, H.soa_for(case, bi.config_of("defaults")), bi.spec_rows(run))
    return out


def oracle_tables(oracle_lib, case, soa, cfg):
    return oracle_lib.score_timstof(case.dia, fragment_columns(case.library.fragment_df, "mz_library"), pack_assembled(soa),
                                    cfg.to_jitclass(), n_threads=4, with_stats=True)


def _uncovered(case, soa):
    """Boxes that lie in the scans no isolation window covers: no observation, whatever the precursor."""
    cyc = case.dia.cycle
    return np.array([(cyc[0, :, a:b, 0] < 0).all() for a, b in zip(soa["scan_start"], soa["scan_stop"])])


def test_sweep_is_what_its_specification_says(sweeps):
    total = 0
    for run, (case, soa, spec) in sweeps.items():
        total += len(spec)
        dia = case.dia
        L, n_frames, S_max = dia.cycle_len, len(dia.rt_values), dia.scan_max_index
        z = int(dia.zeroth_frame)
        assert (n_frames - z) % L != 0                                            # the run ends inside a cycle
        assert int(dia.push_indices.max()) < n_frames * S_max
        complete = (n_frames - z) // L
        fs, fe, fc = soa["frame_start"].astype(np.int64), soa["frame_stop"].astype(np.int64), soa["frame_center"].astype(np.int64)
        ss, se, sc = soa["scan_start"].astype(np.int64), soa["scan_stop"].astype(np.int64), soa["scan_center"].astype(np.int64)
        assert ((fs - z) % L == 0).all() and (fs >= z).all() and (fe <= n_frames).all() and (fs <= fc).all() and (fc < fe).all()
        assert (ss >= 0).all() and (se <= S_max).all() and (sc >= ss).all() and (sc < se).all() and (sc < S_max).all()
        t = bi.shape_table(case, soa, bi.config_of("defaults"))
        assert np.array_equal(t["S"], spec["S"]) and np.array_equal(t["F"], spec["F"]) and np.array_equal(t["nl"], spec["nl"])
        # observations: what the sweep asked for (three times that on the cycle with every MS2 frame three times),
        # none in the scans without an isolation window; one isotope or four change nothing
        want_o = np.where(_uncovered(case, soa), 0, spec["O"].values * (3 if run == "obs3" else 1))
        for name in ("defaults", "isotopes1", "isotopes4"):
            assert np.array_equal(bi.shape_table(case, soa, bi.config_of(name))["O"], want_o), (run, name)
        assert (want_o > 0).mean() > 0.9
        want_p = 2 if run == "ms1x2" else 1   # (a box in the scans without a window sees every frame as an MS1 frame)
        assert (t["Op"].values[~(se > S_max - 2)] == want_p).all() and t["Op"].max() <= 16
        # positions and centres
        c0, c1 = (fs - z) // L, (fe - z) // L
        pos_f = spec["pos_f"].values
        assert (c0[pos_f == 0] == 0).all() and (fs[pos_f == 0] == z).all()
        assert (c1[pos_f >= 2] == complete).all() and (fe[pos_f == 2] == complete * L + z).all() and (fe[pos_f == 3] == n_frames).all()
        assert ((c0[pos_f == 1] > 0) & (c1[pos_f == 1] < complete)).all()
        pos_s = spec["pos_s"].values
        plain = spec["density"].values == ""
        assert (ss[pos_s == 0] == 0).all() and (se[pos_s == 2] == S_max).all()
        assert ((ss[(pos_s == 1) & plain] > 0) & (se[(pos_s == 1) & plain] < S_max)).all()
        F, S = spec["F"].values, spec["S"].values
        ce_f, ce_s = spec["ce_f"].values, spec["ce_s"].values
        assert np.array_equal((fc - z) // L - c0, np.where(ce_f == 0, 0, np.where(ce_f == 1, F // 2, F - 1)))
        assert np.array_equal(sc - ss, np.where(ce_s == 0, 0, np.where(ce_s == 1, S // 2, S - 1)))
        for col, values in (("pos_f", range(4)), ("pos_s", range(3)), ("ce_f", range(3)), ("ce_s", range(3))):
            assert set(spec[col]) == set(values), (run, col)
    assert total < 2000
    spec = sweeps["base"][2]
    plain = spec[spec["density"] == ""]
    assert set(plain["F"]) == set(bi.F_ALL) and set(plain["S"]) == set(bi.S_ALL) and set(plain["nl"]) == set(bi.NL_ALL)
    planes = set((spec["S"] * spec["F"]).tolist())
    assert {640, 1152} <= planes and planes & set(range(641, 673)) and planes & set(range(1153, 1161))
    for shapes in bi.PLANES_AT.values():
        for S, F in shapes:
            assert ((spec["S"] == S) & (spec["F"] == F)).sum() >= 2, (S, F)
    # each batch's maxima are what the batch is for
    mx = {b: (int(g["S"].max()), int(g["F"].max())) for b, g in spec.groupby("batch")}
    assert mx["a"] == (32, 24) and all(bi._is_small(S, F) for S, F in zip(spec["S"][spec["batch"] == "a"], spec["F"][spec["batch"] == "a"]))
    assert mx["b1"] == (36, 32) and 36 * 32 == bi.COMMON_SF and mx["b2"] == (40, 28)
    assert mx["c_s"][0] == 48 and 41 in set(spec["S"][spec["batch"] == "c_s"]) and mx["c_s"][0] * mx["c_s"][1] > bi.COMMON_SF
    assert mx["c_f"][1] == 36 and 33 in set(spec["F"][spec["batch"] == "c_f"]) and mx["c_f"][0] <= bi.COMMON_S
    assert mx["c_sf"] == (40, 32) and ((spec["S"] == 40) & (spec["F"] == 29) & (spec["batch"] == "c_sf")).any()
    assert mx["f2"] == (40, 2)
    assert set(spec["density"]) == set(bi.DENSITIES) | {""}


def test_plan_class_rule_restated():
    c = bi.plan_class_im
    assert c(1, 12, 32, 20) == bi.CLASS_SMALL and c(1, 12, 32, 21) == bi.CLASS_ONE          # 640 / 672 cells
    assert c(1, 12, 27, 24) == bi.CLASS_ONE and c(1, 12, 26, 24) == bi.CLASS_SMALL          # 648 / 624 cells
    assert c(1, 12, 33, 2) == bi.CLASS_ONE and c(1, 12, 32, 2) == bi.CLASS_SMALL            # S = 33 / 32
    assert c(1, 12, 2, 25) == bi.CLASS_ONE and c(1, 12, 2, 24) == bi.CLASS_SMALL            # F = 25 / 24
    assert c(1, 13, 2, 2) == bi.CLASS_ONE and c(1, 12, 2, 2) == bi.CLASS_SMALL              # 13 / 12 kept fragments
    assert c(0, 12, 2, 2) == bi.CLASS_SMALL and c(0, 16, 2, 2) == bi.CLASS_ONE              # no observation counts as one
    assert c(2, 12, 2, 2) == bi.CLASS_TWO and c(2, 16, 48, 36) == bi.CLASS_TWO
    assert c(3, 12, 2, 2) == bi.CLASS_GENERIC and c(8, 12, 2, 2) == bi.CLASS_GENERIC
    assert c(1, 12, 2, 2, skipped=True) == bi.CLASS_GENERIC


def test_instantiation_rule_restated():
    cfg, no_xic, iso4 = bi.config_of("defaults"), bi.config_of("no_xic"), bi.config_of("isotopes4")
    every = {bi.CLASS_ONE: 5, bi.CLASS_TWO: 5, bi.CLASS_SMALL: 5, bi.CLASS_GENERIC: 5}

    def inst(k=12, o=2, s=36, f=32, i=3, cfg=cfg, env=None, n_class=every):
        return bi.instantiation_of(dict(k=k, o=o, s=s, f=f, i=i), n_class, cfg, env)

    at = inst()                                                     # maxima exactly at the common limits
    assert at == {bi.CLASS_ONE: ("common", "fused4"), bi.CLASS_TWO: ("common2", "tile4"), bi.CLASS_SMALL: ("small", "fused4"),
                  bi.CLASS_GENERIC: ("dynamic", "one")}
    assert inst(s=40, f=28) == at and inst(s=40, f=28, o=8) == at   # (the classes cap the observations of their launches)
    for past in (dict(s=41, f=28), dict(s=34, f=33), dict(s=40, f=29), dict(s=37, f=32)):   # S, F, the plane, the plane
        got = inst(**past)
        assert got[bi.CLASS_ONE] == got[bi.CLASS_TWO] == ("dynamic", "one") and got[bi.CLASS_SMALL] == ("small", "fused4"), past
    assert inst(k=13)[bi.CLASS_ONE] == ("dynamic", "one") and inst(k=13)[bi.CLASS_SMALL] == ("small", "fused4")
    # f >= 3 of the split path: not asked of the small class
    two = inst(s=40, f=2)
    assert two == {bi.CLASS_ONE: ("common", "one"), bi.CLASS_TWO: ("dynamic", "one"), bi.CLASS_SMALL: ("small", "fused4"),
                   bi.CLASS_GENERIC: ("dynamic", "one")}
    assert inst(s=40, f=3) == at
    # experimental_xic = False, four isotopes: no split; four isotopes fit no fixed layout
    assert inst(cfg=no_xic) == {bi.CLASS_ONE: ("common", "one"), bi.CLASS_TWO: ("dynamic", "one"), bi.CLASS_SMALL: ("small", "one"),
                                bi.CLASS_GENERIC: ("dynamic", "one")}
    assert set(inst(cfg=iso4, i=4).values()) == {("dynamic", "one")}
    assert inst(cfg=bi.config_of("isotopes1"), i=1) == at
    # the switches
    assert inst(env={"ADH_DEBUG_IM_NO_SPLIT": "1"}) == inst(cfg=no_xic)
    assert set(inst(env={"ADH_DEBUG_IM_DYNAMIC_LAYOUT": "1"}).values()) == {("dynamic", "one")}
    t1 = inst(env={"ADH_DEBUG_IM_TILE1": "1"})
    assert t1[bi.CLASS_ONE] == ("common", "split1") and t1[bi.CLASS_SMALL] == ("small", "split1") and t1[bi.CLASS_TWO] == ("common2", "split1")
    nf = inst(env={"ADH_DEBUG_IM_NO_FUSE4": "1"})
    assert nf[bi.CLASS_ONE] == ("common", "tile4") and nf[bi.CLASS_SMALL] == ("small", "tile4") and nf[bi.CLASS_TWO] == ("common2", "tile4")
    assert inst(env={"ADH_DEBUG_IM4": "1"}) == nf                   # (an ablation stop of the tile4 kernel: not fused)
    assert inst(env={"ADH_DEBUG_IM_TILE1_TWO": "1"}) =={**at, bi.CLASS_TWO: ("common2", "split1")}
    assert inst(env={"ADH_DEBUG_IM_NO_SPLIT2": "1"}) == {**at, bi.CLASS_TWO: ("dynamic", "one")}
    assert inst(env={"ADH_DEBUG_IM": "8"}) == at and inst(env={"ADH_DEBUG_IM": "14"}) == inst(cfg=no_xic)
    assert inst(n_class={bi.CLASS_TWO: 3}) == {bi.CLASS_TWO: ("common2", "tile4")}


# every switch of the routing rule, each on its own: the launch switches of WAYS in test_kernel_classes_im_gpu.py, and the
# ablation stop of the tile4 kernel
ROUTING_SWITCHES = [("ADH_DEBUG_IM_NO_SPLIT", "1"), ("ADH_DEBUG_IM_TILE1", "1"), ("ADH_DEBUG_IM_NO_FUSE4", "1"),
                    ("ADH_DEBUG_IM_TILE1_TWO", "1"), ("ADH_DEBUG_IM_NO_SPLIT2", "1"), ("ADH_DEBUG_IM_DYNAMIC_LAYOUT", "1"),
                    ("ADH_DEBUG_IM", "8"), ("ADH_DEBUG_IM", "14"), ("ADH_DEBUG_IM4", "1")]


def test_instantiation_rule_is_the_librarys(monkeypatch):
    """``bi.instantiation_of`` - what ``routes_of`` and ``REACHES`` reason with - against the rule the launches follow
    (``adh_im_launch_routes``, no GPU) on a grid that straddles every limit of the rule: 12 / 13 kept fragments, one,
    two and more observations, the scan, cycle and plane limits of the small and the common layouts, f >= 3 of the
    split path, with and without the split path, one, three and four isotopes, all four classes and each alone, no
    switch and each routing switch on its own."""
    from alphadia_amd import _abi, runtime

    for name in {s for s, _ in ROUTING_SWITCHES}:
        monkeypatch.delenv(name, raising=False)
    classes = (bi.CLASS_ONE, bi.CLASS_TWO, bi.CLASS_SMALL, bi.CLASS_GENERIC)
    populations = [{c: 5 for c in classes}] + [{c: 3} for c in classes]
    configs = [(cfg, _abi.pack_config(cfg), max(min(int(cfg.top_k_isotopes), bi.N_ISOTOPE_COLUMNS), 1))
               for cfg in (bi.config_of(n) for n in ("defaults", "no_xic", "isotopes1", "isotopes4"))]
    assert sorted(i for _, _, i in configs) == [1, 3, 3, 4]
    n, seen = 0, set()
    for switch in [None] + ROUTING_SWITCHES:
        with monkeypatch.context() as mp:
            env = {}
            if switch is not None:
                mp.setenv(*switch)
                env = dict([switch])
            for cfg, packed, i in configs:
                for k in (12, 13):
                    for o in (1, 2, 3, 8):
                        for s in (2, 32, 33, 36, 37, 40, 41, 48):
                            for f in (2, 3, 24, 25, 28, 29, 32, 33, 36):
                                caps = dict(k=k, o=o, s=s, f=f, i=i)
                                for n_class in populations:
                                    want = runtime.im_launch_routes(caps, n_class, packed)
                                    assert bi.instantiation_of(caps, n_class, cfg, env) == want, (switch, caps, n_class)
                                    seen.update(want.values())
                                    n += 1
    assert n == 10 * 4 * 2 * 4 * 8 * 9 * 5
    # (the grid reaches every pair the rule can give)
    assert seen == {("small", "fused4"), ("small", "tile4"), ("small", "split1"), ("small", "one"), ("common", "fused4"),
                    ("common", "tile4"), ("common", "split1"), ("common", "one"), ("common2", "tile4"), ("common2", "split1"),
                    ("dynamic", "one")}


@pytest.mark.parametrize("name", list(bi.CONFIGS))
def test_sweep_covers_every_route_and_edge(oracle_lib, sweeps, name):
    cfg = bi.config_of(name)
    case, soa, spec = sweeps["base"]
    exp = oracle_tables(oracle_lib, case, soa, cfg)
    valid = exp["valid"].astype(bool)
    table = bi.shape_table(case, soa, cfg)
    routes = bi.routes_of(table, spec["batch"].values, cfg)
    hist, hist_valid = collections.Counter(routes.tolist()), collections.Counter(routes[valid].tolist())
    print(f"[ion-mobility sweep coverage] {name}: {len(valid)} candidates, {int(valid.sum())} valid")
    for r in sorted(hist):
        print(f"  class {r[0]:2d} {r[1]:8s} {r[2]:7s} all {hist[r]:4d} valid {hist_valid.get(r, 0):4d}")
    # every (class, layout, launch) the configuration can reach, and no other
    assert set(hist) == bi.REACHES[name]
    for r in bi.REACHES[name]:
        assert hist[r] >= MIN_ROWS and hist_valid.get(r, 0) >= MIN_VALID, (r, hist[r], hist_valid.get(r, 0))
    # both sides of every edge of S, F and S x F, for one and for two observations
    S, F, O, nl = spec["S"].values, spec["F"].values, table["O"].values, spec["nl"].values
    for o in (1, 2):
        for edge in bi.S_EDGES:
            for s in edge:
                assert (valid & (S == s) & (O == o)).sum() >= MIN_EDGE, ("S", s, o)
        for edge in bi.F_EDGES:
            for f in edge:
                assert (valid & (F == f) & (O == o)).sum() >= MIN_EDGE, ("F", f, o)
        for shapes in bi.PLANES_AT.values():
            for s, f in shapes:
                assert (valid & (S == s) & (F == f) & (O == o)).sum() >= MIN_EDGE, ("plane", s, f, o)
    for s in bi.S_ALL:
        assert (valid & (S == s)).sum() >= MIN_EDGE, s
    for f in bi.F_ALL:
        assert (valid & (F == f)).sum() >= MIN_EDGE, f
    # every box position and centre position
    for col, n in (("pos_f", 4), ("pos_s", 3), ("ce_f", 3), ("ce_s", 3)):
        for v in range(n):
            assert (valid & (spec[col].values == v)).sum() >= 20, (col, v)
    # every slice length
    for k in bi.NL_ALL:
        if k in NL_NEVER_VALID:
            assert not (valid & (nl == k)).any()
        else:
            assert (valid & (nl == k)).sum() >= 20, k
    # two-cycle boxes in a split launch of each layout: small (24 cycle registers), common and two observations (32)
    for r in bi.REACHES[name] & bi._SPLIT:
        at = np.array([x == r for x in routes])
        assert (valid & at & (F == 2)).sum() >= MIN_EDGE, r
    # the density rows are valid: what they took is seen in the output
    assert valid[spec["density"].values != ""].all()
    # the other cycles: three and six observations in the generic class, two MS1 rows in every class
    for run, want in (("obs3", {(bi.CLASS_GENERIC, "dynamic", "one")}), ("ms1x2", None)):
        case_r, soa_r, spec_r = sweeps[run]
        v = oracle_tables(oracle_lib, case_r, soa_r, cfg)["valid"].astype(bool)
        t = bi.shape_table(case_r, soa_r, cfg)
        r = bi.routes_of(t, spec_r["batch"].values, cfg)
        h = collections.Counter(r[v].tolist())
        print(f"  {run}: {dict(collections.Counter(r.tolist()))}, valid {dict(h)}")
        if want is not None:
            assert want <= set(h) and all(h[w] >= 20 for w in want)
            assert {3, 6} <= set(t["O"].values[v].tolist())
        else:
            # (a box that reaches the scans without a window sees every frame of the cycle as an MS1 frame: 7 rows)
            assert len(h) == 3 and min(h.values()) >= MIN_VALID
            assert set(t["Op"].values[v].tolist()) == {2, 7} and (t["Op"].values[v] == 2).sum() >= 20


def test_density_rows_are_on_the_designed_side_of_every_capacity(sweeps):
    case, soa, spec = sweeps["base"]
    cfg = bi.config_of("defaults")
    table = bi.shape_table(case, soa, cfg)
    over, fits = bi.MARGIN * bi.SORT_CAP, bi.SORT_CAP / bi.MARGIN
    seen = collections.Counter()
    for i in np.flatnonzero(spec["density"].values != ""):
        d, t = spec["density"].values[i], table.iloc[i]
        ev = bi.window_events(case, soa, cfg, int(i))
        cap = bi.entry_capacity(int(t["k_cap"]), int(t["O"]), int(t["S"]), int(t["F"]), 3, int(t["Op"]))
        assert t["O"] == spec["O"].values[i] and t["k_cap"] == 12
        assert ev["bins"] <= bi.PAIR_CAP / bi.MARGIN                      # (the pair capacity has a run of its own: "fine")
        w = sorted(ev["fragment_windows"])
        what = (int(i), d, w, ev["isotope_group"], ev["entries"], cap)
        if d in ("window_over_one", "window_over_two"):
            assert w[-1] >= over and w[-2] <= fits and ev["isotope_group"] <= fits and ev["entries"] <= cap / bi.MARGIN, what
            assert t["O"] == (1 if d == "window_over_one" else 2)
        elif d == "isotopes_over":
            assert ev["isotope_group"] >= over and w[-1] <= fits and ev["entries"] <= cap / bi.MARGIN and t["O"] == 1, what
        elif d == "many_batches":   # every window around 200 events: two or three of them fill the list of 512
            assert 150 <= w[0] and w[-1] <= fits and ev["isotope_group"] <= fits and ev["entries"] <= cap / bi.MARGIN, what
            assert sum(w) >= 4 * bi.SORT_CAP
        elif d == "full_tile":
            assert ev["entries"] > cap and ev["entries"] >= FULL_TILE_MARGIN * cap, what
            cells = int(t["S"]) * int(t["F"])
            assert ev["entries"] == (12 * int(t["O"]) + 3) * cells     # every cell of every plane
        seen[(d, int(t["O"]))] += 1
    assert seen == {("window_over_one", 1): 4, ("window_over_two", 2): 8, ("isotopes_over", 1): 4, ("many_batches", 1): 4,
                    ("many_batches", 2): 4, ("full_tile", 1): 10, ("full_tile", 2): 10}
    # the fragment windows of planted rows stay well inside: the peptide's peak is a few dozen cells per window (their
    # isotope windows, 20 ppm wide in the MS1 frames all precursors share, do not: many take the scan-parts path)
    for i in np.flatnonzero((spec["density"].values == "") & (spec["nl"].values == 12))[::37]:
        ev = bi.window_events(case, soa, cfg, int(i))
        assert max(ev["fragment_windows"]) <= fits, (int(i), ev)


def test_pair_rows_are_on_the_designed_side_of_the_pair_capacity(oracle_lib, sweeps):
    """The run "fine" under the wide tolerance: the (window, TOF bin) pairs of the designed rows, counted from the m/z
    table, are 1.5 x ADH_IM_PAIR_CAP and more or ADH_IM_PAIR_CAP / 1.5 at most; no window has more than 256 bins (the
    tile layout's limit, another way to the dense tiles); events and entries stay well inside their capacities, so
    the pair capacity alone decides; and each split launch holds valid rows of both kinds."""
    case, soa, spec = sweeps["fine"]
    cfg = bi.config_of("wide_tolerance")
    table = bi.shape_table(case, soa, cfg)
    valid = oracle_tables(oracle_lib, case, soa, cfg)["valid"].astype(bool)
    routes = bi.routes_of(table, spec["batch"].values, cfg)
    assert set(routes.tolist()) == bi._SPLIT and valid.all()
    density = spec["density"].values
    assert set(density) == set(bi.PAIR_DENSITIES)
    fits = bi.SORT_CAP / bi.MARGIN
    for i in range(len(spec)):
        t = table.iloc[i]
        ev = bi.window_events(case, soa, cfg, i)
        cap = bi.entry_capacity(int(t["k_cap"]), int(t["O"]), int(t["S"]), int(t["F"]), 3, int(t["Op"]))
        what = (i, density[i], ev)
        assert ev["widest_window"] <= 256 / bi.MARGIN and max(ev["fragment_windows"]) <= fits and ev["isotope_group"] <= fits, what
        assert ev["entries"] <= cap / bi.MARGIN and sum(ev["fragment_windows"]) + ev["isotope_group"] <= bi.SORT_CAP * bi.MARGIN, what
        if density[i] == "pairs_over":
            assert ev["bins"] >= bi.MARGIN * bi.PAIR_CAP and t["k_cap"] == 12, what
        else:
            assert ev["bins"] <= bi.PAIR_CAP / bi.MARGIN and t["k_cap"] == 4, what
    for r in bi._SPLIT:
        at = np.array([x == r for x in routes])
        assert (at & (density == "pairs_over")).sum() >= 4 and (at & (density == "pairs_fit")).sum() >= 4, r
    # under the default tolerance the same rows are far below the capacity
    cfg = bi.config_of("defaults")
    assert max(bi.window_events(case, soa, cfg, i)["bins"] for i in range(0, len(spec), 5)) <= bi.PAIR_CAP / bi.MARGIN


def test_no_batch_of_the_sweep_must_be_refused(sweeps):
    """launch_scoring_im refuses a launch whose feature layout needs more than 160 KiB less the static LDS, or whose
    gather needs more than 160 KiB: under every configuration every batch of the sweep stays within both."""
    assert bi._layout_bytes(bi.COMMON_K, 1, bi.COMMON_S, bi.COMMON_F, 3, bi.COMMON_SF) == 13704  # (adh_features_im.hip: "13 704 + ...")
    assert bi._layout_bytes(bi.SMALL_K, 1, bi.SMALL_S, bi.SMALL_F, 3, bi.SMALL_SF) == 10216
    worst = 0
    for name in bi.CONFIGS:
        cfg = bi.config_of(name)
        for run, (case, soa, spec) in sweeps.items():
            table = bi.shape_table(case, soa, cfg)
            for b in spec["batch"].unique():
                caps = bi.batch_caps(table, np.flatnonzero(spec["batch"].values == b), cfg)
                f_lds, g_lds = bi.feature_lds_bytes(caps), bi.gather_lds_bytes(caps)
                assert f_lds <= bi.LDS_LIMIT - bi.IM_STATIC_LDS and g_lds <= bi.LDS_LIMIT, (name, run, b, caps)
                worst = max(worst, f_lds)
    assert worst > 64 * 1024   # (the three-observation batch is the large one)


def test_fixture_holds_the_shapes_it_is_for():
    """tests/golden/scoring_boxes_timstof.npz (the thinned sweep through the reference)."""
    g = np.load(H.golden_path("scoring_boxes_timstof.npz"))
    spec = bi.golden_spec()
    assert len(spec) == len(g["cand_precursor_idx"]) and os.path.getsize(H.golden_path("scoring_boxes_timstof.npz")) < 1024 * 1024
    assert all(g[k].dtype.kind in "biufU" for k in g.files)                # arrays of numbers (and the caveat string) only
    v = g["out_valid"].astype(bool)
    S, F = spec["S"].values, spec["F"].values
    assert set(F[v]) == set(bi.F_ALL) and set(S[v]) == set(bi.S_ALL)
    assert {1, 2, 3} <= set(g["out_features"][v][:, 17].astype(int).tolist())
    planes = set((S * F)[v].tolist())
    assert {640, 1152} <= planes and planes & set(range(641, 673)) and planes & set(range(1153, 1161))
    assert set(spec["pos_f"][v]) == {0, 1, 2} and set(spec["pos_s"][v]) == {0, 1, 2}
    assert set(spec["ce_f"][v]) == {0, 1, 2} and set(spec["ce_s"][v]) == {0, 1, 2}
    assert v.sum() >= 100


def test_oracle_reproduces_the_fixture(oracle_lib):
    """The oracle against the reference on the thinned sweep, at the tolerances of test_timstof_scoring_matches_reference."""
    from test_oracle_golden import _compare, _tims_golden

    z, dia, fragment_df, precursor_df, cand, cfg = _tims_golden("scoring_boxes_timstof.npz")
    from alphadia_amd.scoring import assemble_candidates

    soa = assemble_candidates(cand, precursor_df, "mz_library")
    got = oracle_lib.score_timstof(dia, fragment_columns(fragment_df, "mz_library"), pack_assembled(soa), cfg.to_jitclass())
    exp = {n: z["out_" + n] for n in H.OUT_NAMES}
    _compare(got, exp, ppm_tol=0.15, rel_tol=1e-4, corr_abs=1e-3)


@pytest.mark.skipif(not os.path.isdir(ref_shim.REFERENCE_ROOT), reason="the reference checkout is not on this machine")
def test_regenerating_the_fixture_reproduces_the_committed_file(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(H.GOLDEN_DIR, "make_golden.py"), "--out", str(tmp_path), "--boxes-timstof-only"],
                       capture_output=True, text=True, cwd=root)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    name = "scoring_boxes_timstof.npz"
    fresh, golden = np.load(tmp_path / name), np.load(H.golden_path(name))
    assert sorted(fresh.files) == sorted(golden.files)
    for key in golden.files:
        assert fresh[key].dtype == golden[key].dtype, key
        assert np.array_equal(fresh[key], golden[key], equal_nan=golden[key].dtype.kind == "f"), key
