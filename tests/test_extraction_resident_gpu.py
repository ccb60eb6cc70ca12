"""Resident extraction on the GPU: HipExtractionHandler.extract scores into HBM, runs the FDR stage there and copies
back only the survivors.  It must return what the python branch of PeptideCentricWorkflow.extraction
(alphadia/workflow/peptidecentric/peptidecentric.py:202-246) returns from the chained calls, while moving less."""

from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import synthetic as syn

pytestmark = pytest.mark.gpu

NAMES = SimpleNamespace(get_rt_column=lambda: "rt_library", get_mobility_column=lambda: "mobility_library",
                        get_precursor_mz_column=lambda: "mz_library", get_fragment_mz_column=lambda: "mz_library")
CLASSIFIER = dict(test_size=0.2, batch_size=500, learning_rate=0.001, epochs=4, random_state=11)


def _features():
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    # kernel features, the host-derived delta_rt, and library / sequence columns of the reference's list
    return [c for c in DEFAULT_FEATURE_COLUMNS if c not in ("mobility_observed", "base_width_mobility")] + [
        "delta_rt", "mz_library", "charge", "n_K", "n_R", "n_P"]


def _manager(dia, seed=7):
    from alphadia_amd import fdr

    return fdr.HipFDRManager(_features(), fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=dia.cycle,
                             random_state=seed, device=0)


def _handler(candidates_df, manager, competitive, fdr=0.01, channel_wise=False):
    from alphadia_amd.extraction_handler import HipExtractionHandler

    config = {"search": {"extraction_backend": "hip", "exclude_shared_ions": True, "quant_window": 3, "quant_all": True,
                         "experimental_xic": True, "top_k_fragments_scoring": 12, "top_k_fragments_selection": 12},
              "general": {"thread_count": 4},
              "fdr": {"fdr": fdr, "competitive_scoring": competitive, "channel_wise_fdr": channel_wise}}
    opt = SimpleNamespace(ms1_error=10, ms2_error=15, rt_error=30.0, mobility_error=0.1, num_candidates=2, fwhm_rt=5.0,
                          fwhm_mobility=0.01, score_cutoff=0.0, classifier_version=-1)
    log = []
    reporter = SimpleNamespace(log_string=lambda msg, **k: log.append(msg))
    # the candidates of the case stand in for the selection step (the same table for both paths)
    selection = SimpleNamespace(select_candidates=lambda dia, lib, apply_cutoff=False: candidates_df)
    h = HipExtractionHandler(config, opt, manager, reporter, NAMES, selection_handler=selection, device=0)
    h.log = log
    return h


def _chained(handler, dia, lib, manager, competitive, fdr=0.01, channel_wise=False):
    """peptidecentric.py:202-246 as written, on the handler's chained calls."""
    from alphadia_amd.fragcomp import candidate_hash

    cands = handler.select_candidates(dia, lib, apply_cutoff=True)
    features_df, fragments_df = handler.score_and_quantify_candidates(cands, dia, lib)
    precursor_df = manager.fit_predict(features_df, decoy_strategy="precursor_channel_wise" if channel_wise else "precursor",
                                       competitive=competitive, df_fragments=fragments_df, version=-1)
    precursor_df = precursor_df[precursor_df["qval"] <= fdr].copy()
    fragments_df["candidate_idx"] = candidate_hash(fragments_df["precursor_idx"].values, fragments_df["rank"].values)
    precursor_df["candidate_idx"] = candidate_hash(precursor_df["precursor_idx"].values, precursor_df["rank"].values)
    fragments_df = fragments_df[fragments_df["candidate_idx"].isin(precursor_df["candidate_idx"])]
    return precursor_df, fragments_df


def _assert_same(got: pd.DataFrame, exp: pd.DataFrame, what: str):
    assert isinstance(got.index, pd.RangeIndex) and got.index.start == 0, what
    exp = exp.reset_index(drop=True)
    assert list(got.columns) == list(exp.columns), what
    assert len(got) == len(exp), (what, len(got), len(exp))
    for c in exp.columns:
        a, b = got[c], exp[c]
        assert a.dtype == b.dtype, (what, c, a.dtype, b.dtype)
        if c == "proba":  # (the bounds of tests/test_fdr_resident.py)
            assert np.allclose(a.to_numpy(), b.to_numpy(), rtol=0, atol=1e-6), (what, c)
        elif c == "qval":
            assert np.allclose(a.to_numpy(), b.to_numpy(), rtol=1e-12, atol=0), (what, c)
        elif a.dtype == object:
            assert (a.to_numpy() == b.to_numpy()).all(), (what, c)
        else:
            assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True), (what, c)


def _lib(case):
    return SimpleNamespace(precursor_df=case.library.precursor_df, fragment_df=case.library.fragment_df)


@pytest.fixture(scope="module")
def case():
    return syn.make_case(5000, 260, config_id=78, per_precursor=2, planted_fraction=0.5, threads=4)


def _scorer(case):
    from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring

    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                    experimental_xic=True))
    return HipCandidateScoring(dia_data=case.dia, precursors_flat=case.library.precursor_df,
                               fragments_flat=case.library.fragment_df, config=cfg, device=0, rt_column="rt_library",
                               mobility_column="mobility_library", precursor_mz_column="mz_library",
                               fragment_mz_column="mz_library")


@pytest.mark.parametrize("competitive", [True, False])
def test_extract_equals_the_chained_path(case, competitive):
    from alphadia_amd import runtime

    ctx = runtime.get_context(0)
    lib = _lib(case)
    m_res, m_chain = _manager(case.dia), _manager(case.dia)
    ctx.d2h_bytes(reset=True)
    pre, frag = _handler(case.candidates_df, m_res, competitive).extract(case.dia, lib)
    moved = ctx.d2h_bytes(reset=True)
    pre_c, frag_c = _chained(_handler(case.candidates_df, m_chain, competitive), case.dia, lib, m_chain, competitive)
    moved_chained = ctx.d2h_bytes()
    assert len(pre) > 300 and len(frag) > 5 * len(pre)
    assert {"_decoy", "proba", "qval", "_candidate_idx", "valid", "candidate_idx"} <= set(pre.columns)
    _assert_same(pre, pre_c, "precursor_df")
    _assert_same(frag, frag_c, "fragments_df")
    assert m_res.current_version == m_chain.current_version == 0
    assert list(m_res.classifier_store) == list(m_chain.classifier_store)
    # copy-out: the survivors' compact rows (193 bytes per row, 42 per slot, column padding) and at most 64 bytes
    # per table row for the FDR stage
    n_table = len(case.candidates_df)
    assert moved < moved_chained, (moved, moved_chained)
    assert moved <= 64 * n_table + 193 * len(pre) + 42 * len(frag) + 16 * 80, (moved, n_table, len(pre), len(frag))


def test_extract_equals_the_chained_path_with_ion_mobility():
    from alphadia_amd import runtime

    tcase = syn.make_timstof_case(n_precursors=300, n_cycles=60, config_id=46, per_precursor=2, n_ms2_frames=6,
                                  windows_per_frame=3, scan_max_index=96)
    lib = _lib(tcase)
    ctx = runtime.get_context(0)
    m_res, m_chain = _manager(tcase.dia, 3), _manager(tcase.dia, 3)
    ctx.d2h_bytes(reset=True)
    pre, frag = _handler(tcase.candidates_df, m_res, True, fdr=0.5).extract(tcase.dia, lib)
    moved = ctx.d2h_bytes(reset=True)
    pre_c, frag_c = _chained(_handler(tcase.candidates_df, m_chain, True, fdr=0.5), tcase.dia, lib, m_chain, True, fdr=0.5)
    assert len(pre) > 0
    _assert_same(pre, pre_c, "precursor_df (ion mobility)")
    _assert_same(frag, frag_c, "fragments_df (ion mobility)")
    assert moved < ctx.d2h_bytes()


def test_score_resident_moves_nothing_and_leaves_the_tables_of_score_host(case):
    from alphadia_amd import runtime
    from alphadia_amd.scoring import assemble_candidates, pack_assembled

    ctx = runtime.get_context(0)
    scorer = _scorer(case)
    soa = assemble_candidates(case.candidates_df, scorer.precursors_flat_df, "mz_library")
    ctx.score_host(pack_assembled(soa), scorer._kernel_config())
    host = ctx.device_tables_to_host()
    ctx.d2h_bytes(reset=True)
    res = scorer.score_resident(case.candidates_df)
    assert ctx.d2h_bytes() == 0
    assert res.n_table == len(case.candidates_df) == int(ctx.device_tables().n)
    dev = ctx.device_tables_to_host()
    assert sorted(dev) == sorted(host)
    for name in host:
        assert host[name].dtype == dev[name].dtype and host[name].shape == dev[name].shape, name
        assert np.array_equal(host[name], dev[name], equal_nan=True), name


def test_take_rows_copies_the_listed_rows_of_the_padded_tables(case):
    from alphadia_amd import _abi, runtime
    from alphadia_amd.runtime import HipBackendError

    ctx = runtime.get_context(0)
    scorer = _scorer(case)
    res = scorer.score_resident(case.candidates_df)
    tab = ctx.device_tables_to_host()
    n = res.n_table
    valid = tab["valid"].astype(bool)
    assert (~valid).any() and valid.any()
    rows = np.random.default_rng(5).permutation(n)[: (2 * n) // 3]
    rows = np.concatenate([rows, np.flatnonzero(~valid)[:5]])  # invalid rows listed on purpose
    ctx.d2h_bytes(reset=True)
    comp = ctx.take_rows(rows)
    moved = ctx.d2h_bytes()
    keep = rows[valid[rows]]
    assert comp["row"].dtype == np.uint32 and np.array_equal(comp["row"], keep)
    assert np.array_equal(comp["precursor_idx"], tab["precursor_idx"][keep])
    assert np.array_equal(comp["rank"], tab["rank"][keep])
    assert comp["features"].shape == (_abi.NUM_FEATURES, len(keep))
    assert np.array_equal(comp["features"], tab["features"][keep].T, equal_nan=True)
    filled = tab["fragment_mz_library"][keep] > 0  # (output.py:89-97)
    assert np.array_equal(comp["fragment_row"], np.repeat(keep, filled.sum(axis=1)))
    for name, dt in _abi.COMPACT_SLOT_FIELDS:
        if name != "fragment_row":
            assert comp[name].dtype == dt and np.array_equal(comp[name], tab[name][keep][filled], equal_nan=True), name
    assert moved <= 8 + 193 * len(keep) + 42 * len(comp["fragment_row"]) + 16 * 80
    assert len(ctx.take_rows(np.zeros(0, np.int64))["row"]) == 0
    for bad in ([n], [-1], [0, n + 5]):
        with pytest.raises(HipBackendError):
            ctx.take_rows(np.asarray(bad))
    # a later scoring call replaces the tables the result refers to; staging the run again ends them for take_rows
    res2 = scorer.score_resident(case.candidates_df.iloc[:100])
    with pytest.raises(HipBackendError):
        res.frames(keep[:3])
    assert len(res2.frames(np.arange(10))[0]) <= 10
    ctx.stage_run(case.dia, force=True)
    with pytest.raises(HipBackendError):
        ctx.take_rows(keep[:3])
    with pytest.raises(HipBackendError):
        res2.frames(np.arange(3))


def test_extract_without_survivors_and_with_too_few_psms(case):
    lib = _lib(case)
    m_res, m_chain = _manager(case.dia), _manager(case.dia)
    pre, frag = _handler(case.candidates_df, m_res, True, fdr=-1.0).extract(case.dia, lib)
    pre_c, frag_c = _chained(_handler(case.candidates_df, m_chain, True, fdr=-1.0), case.dia, lib, m_chain, True, fdr=-1.0)
    assert len(pre) == len(frag) == 0
    _assert_same(pre, pre_c, "precursor_df (no survivors)")
    _assert_same(frag, frag_c, "fragments_df (no survivors)")

    small = syn.make_case(40, 80, config_id=79, per_precursor=1, n_ms2=8, ms1_peaks=400, ms2_peaks=150, mz_lo=400,
                          mz_hi=480, frag_mz_lo=200, frag_mz_hi=350, ms1_mz_range=(395, 500), ms2_mz_range=(195, 355),
                          planted_fraction=1.0, threads=1)
    lib = _lib(small)
    for keep in (2, 1):  # too few PSMs for a train / test split: every usable PSM with qval = proba = 1
        cands = small.candidates_df.iloc[:keep]
        m_res, m_chain = _manager(small.dia), _manager(small.dia)
        pre, frag = _handler(cands, m_res, True, fdr=1.0).extract(small.dia, lib)
        pre_c, frag_c = _chained(_handler(cands, m_chain, True, fdr=1.0), small.dia, lib, m_chain, True, fdr=1.0)
        assert 0 < len(pre) <= keep and list(pre.columns[-3:]) == ["qval", "proba", "candidate_idx"]
        _assert_same(pre, pre_c, "precursor_df (too few PSMs)")
        _assert_same(frag, frag_c, "fragments_df (too few PSMs)")
        assert m_res.current_version == m_chain.current_version == 0


def test_channel_wise_fdr_falls_back_to_the_chained_calls():
    mc = syn.make_multiplex_case(300, 120, config_id=81, threads=4)
    pdf = mc.library.precursor_df.copy()
    pdf["decoy"] = (pdf["elution_group_idx"].to_numpy() % 2).astype(pdf["decoy"].dtype)  # decoys in every channel
    lib = SimpleNamespace(precursor_df=pdf, fragment_df=mc.library.fragment_df)
    cands = syn.make_candidates(SimpleNamespace(precursor_df=pdf, fragment_df=mc.library.fragment_df), 120,
                                mc.dia.cycle.shape[1], 81, per_precursor=1, apex_cycle=mc.apex_cycle)
    m_res, m_chain = _manager(mc.dia), _manager(mc.dia)
    h = _handler(cands, m_res, False, fdr=0.5, channel_wise=True)
    assert h.resident_refusal() is not None
    pre, frag = h.extract(mc.dia, lib)
    h.extract(mc.dia, lib)
    assert sum("not used" in msg for msg in h.log) == 1  # the reason is logged once
    pre_c, frag_c = _chained(_handler(cands, m_chain, False, fdr=0.5, channel_wise=True), mc.dia, lib, m_chain, False,
                             fdr=0.5, channel_wise=True)
    assert len(pre) > 0
    # the same chained calls: equal to the bit (a fresh RangeIndex on both frames)
    pd.testing.assert_frame_equal(pre, pre_c.reset_index(drop=True))
    pd.testing.assert_frame_equal(frag, frag_c.reset_index(drop=True))
