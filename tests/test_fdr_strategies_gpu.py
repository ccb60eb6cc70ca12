"""The channel-wise decoy strategies of the FDR manager (fdr_manager.py:178-223) on the GPU: the host strategies
against the reference golden, the part staging of the device classifier against its NumPy restatement, the strategies
on tables in HBM against the host strategies on the frames of the same scoring call, and multiplex requantification
without the round trip against the chained calls."""

import logging
import os
import sys
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import synthetic as syn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_fdr_strategies as gen  # noqa: E402  (importing it runs nothing of the reference)

pytestmark = pytest.mark.gpu

NAMES = dict(rt_column="rt_library", mobility_column="mobility_library", precursor_mz_column="mz_library",
             fragment_mz_column="mz_library")
NAME_HANDLER = SimpleNamespace(**{"get_" + k: (lambda v=v: v) for k, v in NAMES.items()})
CLASSIFIER = dict(test_size=0.2, batch_size=500, learning_rate=0.001, epochs=4, random_state=11)
ID_COLUMNS = ["precursor_idx", "rank", "elution_group_idx", "channel", "decoy"]


def _features():
    from alphadia_amd.scoring import DEFAULT_FEATURE_COLUMNS

    return [c for c in DEFAULT_FEATURE_COLUMNS if c not in ("mobility_observed", "base_width_mobility")] + [
        "delta_rt", "mz_library", "charge", "n_K", "n_R", "n_P"]


def _manager(dia, seed=7):
    from alphadia_amd import fdr

    return fdr.HipFDRManager(_features(), fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=dia.cycle,
                             random_state=seed, device=0)


def _scorer(dia, precursor_df, fragment_df):
    from alphadia_amd.scoring import CandidateScoringConfig, HipCandidateScoring

    cfg = CandidateScoringConfig()
    cfg.update(dict(top_k_isotopes=3, precursor_mz_tolerance=10, fragment_mz_tolerance=15, quant_all=True,
                    experimental_xic=True))
    return HipCandidateScoring(dia_data=dia, precursors_flat=precursor_df, fragments_flat=fragment_df, config=cfg,
                               device=0, **NAMES)


# ------------------------------------------------------------------ the host strategies against the reference
@pytest.mark.parametrize("competitive", [False, True])
@pytest.mark.parametrize("strategy", gen.STRATEGIES)
def test_host_strategies_reproduce_the_reference(strategy, competitive):
    from alphadia_amd import fdr

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fdr_strategies.npz"))
    table = pd.DataFrame({c: g["in/" + c] for c in gen.INPUT_COLUMNS})
    manager = fdr.HipFDRManager(gen.FEATURES, gen.StandInClassifier(), compete_for_fragments=False, random_state=3,
                                device=0)
    res = manager.fit_predict(table, strategy, competitive,
                              decoy_channel=gen.DECOY_CHANNEL if strategy == "channel" else -1)
    exp = pd.DataFrame({c: g[f"{gen.tag(strategy, competitive)}/{c}"] for c in gen.RESULT_COLUMNS})
    assert len(res) == len(exp) > 1000
    # the order of the parts of "channel" is a set's iteration order in the reference: compare as sorted rows
    res = res.sort_values(["precursor_idx", "qval", "proba"], kind="stable")
    exp = exp.sort_values(["precursor_idx", "qval", "proba"], kind="stable")
    for c in ("precursor_idx", "channel", "decoy", "_decoy"):
        assert np.array_equal(res[c].to_numpy(), exp[c].to_numpy()), c
    assert np.allclose(res["proba"].to_numpy(), exp["proba"].to_numpy(), rtol=0, atol=1e-6)
    assert np.allclose(res["qval"].to_numpy(), exp["qval"].to_numpy(), rtol=1e-12, atol=0)
    if strategy == "channel":  # a row of the decoy channel comes back once per part
        assert res["precursor_idx"].duplicated().any() and (res.loc[res["channel"] == gen.DECOY_CHANNEL, "decoy"] == 1).all()


# ------------------------------------------------------------------ staging
def _multiplex_inputs(n_groups, n_cycles, config_id, planted_fraction=0.3, empty_decoy_channel=False):
    """A multiplex case as the requantification handler sees it: the library of all channels, the identifications of
    the reference channel.  ``empty_decoy_channel``: the precursors of the last channel point at the fragments of the
    next elution group, as a label channel without sample looks to the scoring (nothing elutes where they are sought)."""
    mc = syn.make_multiplex_case(n_groups, n_cycles, config_id=config_id, planted_fraction=planted_fraction, threads=4)
    pdf = mc.library.precursor_df.copy()
    if empty_decoy_channel:
        last = np.flatnonzero(pdf["channel"].to_numpy() == mc.channels[-1])
        for c in ("flat_frag_start_idx", "flat_frag_stop_idx"):
            col = pdf[c].to_numpy().copy()
            col[last] = np.roll(col[last], 1)
            pdf[c] = col
    psm_df = mc.psm_df.copy()
    psm_df["channel"] = np.uint32(mc.channels[0])
    return mc, pdf, psm_df


def _requant_handler(mc, pdf, manager, fdr=0.01, competitive=True):
    from alphadia_amd.multiplexing import HipMultiplexingRequantificationHandler

    config = {"multiplexing": {"reference_channel": int(mc.channels[0]),
                               "target_channels": ",".join(str(c) for c in mc.channels[1:-1]),
                               "decoy_channel": int(mc.channels[-1]), "competitive_scoring": competitive},
              "search": {"experimental_xic": True}, "fdr": {"fdr": fdr}}
    log = []
    lib = SimpleNamespace(precursor_df_unfiltered=pdf, fragment_df=mc.library.fragment_df,
                          _fragment_df=mc.library.fragment_df)
    h = HipMultiplexingRequantificationHandler(config, None, manager, SimpleNamespace(
        log_string=lambda msg, **k: log.append(msg)), NAME_HANDLER, lib, device=0)
    h.log = log
    return h


def test_part_staging_equals_the_numpy_restatement():
    from alphadia_amd import runtime
    from alphadia_amd.fdr import part_rows
    from alphadia_amd.runtime import HipBackendError
    from alphadia_amd.scoring import requantify_multiplexed

    ctx = runtime.get_context(0)
    mc, pdf, psm_df = _multiplex_inputs(300, 120, 81)
    res = requantify_multiplexed(mc.dia, psm_df, pdf, mc.library.fragment_df, list(mc.channels), int(mc.channels[0]),
                                 True, NAMES, device=0, resident=True)
    n = res.n_table
    assert n == int(ctx.device_tables().n) > 1000
    channel, decoy = res.metadata["channel"].to_numpy(), res.metadata["decoy"].to_numpy().copy()
    decoy[::3] = 1  # (the library of requantification holds targets only: some decoys by column for the label test)
    valid = res.valid()
    assert valid.dtype == bool and valid.shape == (n,) and valid.sum() > 50
    # classifier columns: three kernel features, delta_rt and one host column with NaN in rows of every channel
    extra = np.random.default_rng(3).normal(size=n).astype(np.float32)
    extra[::7] = np.nan
    assert all(np.isnan(extra[valid & (channel == c)]).any() for c in mc.channels)
    rt = res.table_column("rt_library").astype(np.float32)
    src_cols, extras = [0, 5, 2, -1, 47], [rt, extra]
    features = ctx.device_tables_to_host(["features"])["features"]
    usable = ~(np.isnan(features[:, [0, 5, 2]]).any(axis=1) | np.isnan(extra) | np.isnan(rt))
    dc = int(mc.channels[-1])
    parts = [(int(c), -1, 0) for c in mc.channels] + [(int(c), dc, 1) for c in mc.channels[:-1]] + [
        (int(mc.channels[1]), dc, 0), (dc, dc, 1), (int(mc.channels[0]), -1, 1)]
    mlp = runtime.DeviceMlp(ctx, len(src_cols), [8], 2)
    try:
        for part in parts:
            counts = mlp.stage_rows_device(src_cols, decoy, extras, channel=channel, part=part)
            rows, n_t, n_d = part_rows(valid, usable, decoy, channel, part)
            assert counts == (n_t, n_d) and mlp.n_rows == n_t + n_d, part
            assert np.array_equal(mlp.staged_rows(), rows), part
            assert n_t + n_d > 10, part
        # no part: the old entry, with or without the channel column
        rows, n_t, n_d = part_rows(valid, usable, decoy, channel)
        assert mlp.stage_rows_device(src_cols, decoy, extras) == (n_t, n_d) and np.array_equal(mlp.staged_rows(), rows)
        assert mlp.stage_rows_device(src_cols, decoy, extras, channel=channel, part=None) == (n_t, n_d)
        assert np.array_equal(mlp.staged_rows(), rows) and n_t + n_d == int((valid & usable).sum())
        # a target channel the table does not hold
        assert mlp.stage_rows_device(src_cols, decoy, extras, channel=channel, part=(5, -1, 0)) == (0, 0)
        assert len(mlp.staged_rows()) == 0
        assert mlp.stage_rows_device(src_cols, decoy, extras, channel=channel, part=(5, -1, 1)) == (0, 0)
        for bad in (channel[:-1], np.r_[channel, channel[:2]]):
            with pytest.raises(HipBackendError):
                mlp.stage_rows_device(src_cols, decoy, extras, channel=bad, part=parts[0])
        with pytest.raises(ValueError):
            mlp.stage_rows_device(src_cols, decoy, extras, part=parts[0])
        # an empty table stages nothing and does not fail
        empty = res._scorer.score_resident(res._candidates_df.iloc[:0])
        assert empty.n_table == 0 and len(empty.valid()) == 0
        none = np.zeros(0, np.int64)
        assert mlp.stage_rows_device(src_cols, none, [none, none], channel=none, part=parts[0]) == (0, 0)
        assert len(mlp.staged_rows()) == 0
    finally:
        mlp.close()


# ------------------------------------------------------------------ the strategies: resident == host
@pytest.fixture(scope="module")
def channel_case():
    """1 500 elution groups x 4 channels with decoys (by column) in every channel; the precursor indices of a group
    are permuted against its channels, so the table (elution group, decoy, rank, precursor) meets the channels in the
    order 8, 0, 4, 12."""
    mc = syn.make_multiplex_case(1500, 260, config_id=81, threads=4)
    pdf = mc.library.precursor_df.copy()
    pdf["decoy"] = (pdf["elution_group_idx"].to_numpy() % 2).astype(pdf["decoy"].dtype)
    n_c = len(mc.channels)
    slot = np.asarray([1, 2, 0, 3])[np.searchsorted(np.asarray(mc.channels), pdf["channel"].to_numpy())]
    pdf["precursor_idx"] = ((pdf["precursor_idx"].to_numpy() // n_c) * n_c + slot).astype(pdf["precursor_idx"].dtype)
    lib = SimpleNamespace(precursor_df=pdf, fragment_df=mc.library.fragment_df)
    cands = syn.make_candidates(lib, 260, mc.dia.cycle.shape[1], 81, per_precursor=1, apex_cycle=mc.apex_cycle)
    return SimpleNamespace(dia=mc.dia, library=lib, candidates_df=cands, channels=mc.channels)


def _assert_same_fdr(res, host, m_res, m_host, what):
    assert len(res) == len(host), (what, len(res), len(host))
    for c in ID_COLUMNS:  # the identifying columns and the order
        assert np.array_equal(res[c].to_numpy(), host[c].to_numpy()), (what, c)
    assert np.array_equal(res["_decoy"].to_numpy(), host["_decoy"].to_numpy()), what
    assert np.allclose(res["proba"].to_numpy(), host["proba"].to_numpy(), rtol=0, atol=1e-6), what
    assert np.allclose(res["qval"].to_numpy(), host["qval"].to_numpy(), rtol=1e-12, atol=0), what
    assert m_res.current_version == m_host.current_version == 0, what
    assert list(m_res.classifier_store) == list(m_host.classifier_store), what
    assert [len(v) for v in m_res.classifier_store.values()] == [len(v) for v in m_host.classifier_store.values()] == [1]


def _assert_not_vacuous(host, strategy, channels):
    assert len(host) > 500
    targets = set(channels[:-1]) if strategy == "channel" else set(channels)
    assert targets <= set(host.loc[host["_decoy"] == 0, "channel"]), "a part contributed no rows"
    assert (host["_decoy"] == 1).sum() > 100
    if strategy == "channel":
        assert set(host.loc[host["_decoy"] == 1, "channel"]) == {channels[-1]}
        assert (host.loc[host["channel"] == channels[-1], "decoy"] == 1).all()


@pytest.mark.parametrize("competitive", [True, False])
@pytest.mark.parametrize("strategy", ["precursor_channel_wise", "channel"])
def test_resident_strategies_equal_the_host_strategies(channel_case, strategy, competitive):
    from alphadia_amd.fdr import strategy_parts

    case = channel_case
    dc = int(case.channels[-1]) if strategy == "channel" else -1
    scorer = _scorer(case.dia, case.library.precursor_df, case.library.fragment_df)
    resident = scorer.score_resident(case.candidates_df)
    features_df, fragments_df = resident.frames(np.arange(resident.n_table))
    first_seen = [p[0] for p in strategy_parts("precursor_channel_wise", resident.metadata["channel"].to_numpy(),
                                               resident.valid())]
    assert first_seen == list(features_df["channel"].unique()) and first_seen != sorted(first_seen)
    m_res, m_host = _manager(case.dia), _manager(case.dia)
    res = m_res.fit_predict_resident(resident, competitive, decoy_strategy=strategy, decoy_channel=dc)
    host = m_host.fit_predict(features_df, strategy, competitive, df_fragments=fragments_df, decoy_channel=dc)
    _assert_not_vacuous(host, strategy, list(case.channels))
    _assert_same_fdr(res, host, m_res, m_host, (strategy, competitive))
    assert [p[0][0] for p in res.attrs["parts"]] == (sorted(set(first_seen) - {dc}) if strategy == "channel" else first_seen)
    assert sum(p[1] for p in res.attrs["parts"]) == len(res) and not any(p[2] for p in res.attrs["parts"])
    assert res.attrs["fragment_competition"] == (strategy != "channel")
    assert np.array_equal(resident.metadata["precursor_idx"].to_numpy()[res["table_row"].to_numpy()],
                          res["precursor_idx"].to_numpy())
    assert list(res.columns) == [*ID_COLUMNS, "_decoy", "proba", "qval", "table_row"]  # (those of "precursor")


def test_resident_strategies_check_their_input(channel_case):
    case = channel_case
    scorer = _scorer(case.dia, case.library.precursor_df, case.library.fragment_df)
    resident = scorer.score_resident(case.candidates_df.iloc[:400])
    manager = _manager(case.dia)
    with pytest.raises(ValueError, match="decoy_channel must be set"):
        manager.fit_predict_resident(resident, True, decoy_strategy="channel")
    with pytest.raises(ValueError, match="not found"):
        manager.fit_predict_resident(resident, True, decoy_strategy="channel", decoy_channel=5)
    with pytest.raises(ValueError, match="Invalid decoy_strategy"):
        manager.fit_predict_resident(resident, True, decoy_strategy="precursors")
    assert manager.current_version == -1 and not manager.classifier_store


def test_accumulated_scores_run_the_strategies(channel_case):
    """Two appended batches of different width (the first with library slices of 5 fragments)."""
    from alphadia_amd import runtime
    from alphadia_amd.scoring import AccumulatedScores

    case = channel_case
    pre = case.library.precursor_df.copy()
    in_a_lib = ((pre["elution_group_idx"] // 2) % 2 == 0).to_numpy()
    pre.loc[in_a_lib, "flat_frag_stop_idx"] = pre.loc[in_a_lib, "flat_frag_start_idx"] + 5
    scorer = _scorer(case.dia, pre, case.library.fragment_df)
    in_a = ((case.candidates_df["elution_group_idx"] // 2) % 2 == 0).to_numpy()
    acc = AccumulatedScores(0)
    acc.append(scorer, case.candidates_df[in_a])
    width_a = int(runtime.get_context(0).device_tables().top_k)
    acc.append(scorer, case.candidates_df[~in_a])
    assert (width_a, int(runtime.get_context(0).device_tables().top_k)) == (5, 12)
    assert np.array_equal(acc.valid(), np.concatenate([acc.valid(0, 100), acc.valid(100)]))
    feats, frags = acc.batch_frames()
    features_df, fragments_df = pd.concat(feats, ignore_index=True), pd.concat(frags, ignore_index=True)
    for strategy, dc in (("precursor_channel_wise", -1), ("channel", int(case.channels[-1]))):
        m_res, m_host = _manager(case.dia), _manager(case.dia)
        res = m_res.fit_predict_resident(acc, True, decoy_strategy=strategy, decoy_channel=dc)
        host = m_host.fit_predict(features_df, strategy, True, df_fragments=fragments_df, decoy_channel=dc)
        _assert_not_vacuous(host, strategy, list(case.channels))
        _assert_same_fdr(res, host, m_res, m_host, ("accumulated", strategy))


# ------------------------------------------------------------------ multiplex requantification
def _assert_same(got: pd.DataFrame, exp: pd.DataFrame, what: str):
    """tests/test_extraction_resident_gpu.py::_assert_same"""
    assert isinstance(got.index, pd.RangeIndex) and got.index.start == 0, what
    exp = exp.reset_index(drop=True)
    assert list(got.columns) == list(exp.columns), what
    assert len(got) == len(exp), (what, len(got), len(exp))
    for c in exp.columns:
        a, b = got[c], exp[c]
        assert a.dtype == b.dtype, (what, c, a.dtype, b.dtype)
        if c == "proba":
            assert np.allclose(a.to_numpy(), b.to_numpy(), rtol=0, atol=1e-6), (what, c)
        elif c == "qval":
            assert np.allclose(a.to_numpy(), b.to_numpy(), rtol=1e-12, atol=0), (what, c)
        elif a.dtype == object:
            assert (a.to_numpy() == b.to_numpy()).all(), (what, c)
        else:
            assert np.array_equal(a.to_numpy(), b.to_numpy(), equal_nan=True), (what, c)


@pytest.fixture(scope="module")
def requant_case():
    return _multiplex_inputs(1200, 260, 82, planted_fraction=0.5, empty_decoy_channel=True)


@pytest.mark.parametrize("competitive", [True, False])
def test_requantify_filtered_equals_requantify_and_the_filter(requant_case, competitive):
    from alphadia_amd import runtime

    mc, pdf, psm_df = requant_case
    ctx = runtime.get_context(0)
    # the chained calls first: their q-values place the threshold - halfway between the two distinct q-values next to
    # the median, so that about half of the rows survive and no row sits on the threshold itself
    m_chain = _manager(mc.dia)
    ctx.d2h_bytes(reset=True)
    full = _requant_handler(mc, pdf, m_chain, 1.0, competitive).requantify(mc.dia, psm_df)
    moved_chained = ctx.d2h_bytes(reset=True)
    q = np.unique(full["qval"].to_numpy())
    at = min(max(int(np.searchsorted(q, np.median(full["qval"].to_numpy()))), 1), len(q) - 1)
    threshold = float(0.5 * (q[at - 1] + q[at]))
    assert q[at - 1] < threshold < q[at]
    exp = full[full["qval"] <= threshold]
    m_res = _manager(mc.dia)
    h_res = _requant_handler(mc, pdf, m_res, threshold, competitive)
    ctx.d2h_bytes(reset=True)
    got = h_res.requantify_filtered(mc.dia, psm_df)
    moved = ctx.d2h_bytes(reset=True)
    dc = int(mc.channels[-1])
    assert len(exp) >= 100 and len(full) - len(exp) >= 100
    assert exp.loc[exp["channel"] == dc, "precursor_idx"].duplicated().any()  # a decoy-channel row kept in two parts
    assert (exp.loc[exp["channel"] == dc, "decoy"] == 1).all() and (exp.loc[exp["channel"] != dc, "decoy"] == 0).all()
    assert h_res.last_timings["path"] == "resident" and not h_res.log[1:]
    assert {"_decoy", "proba", "qval"} <= set(got.columns)
    _assert_same(got, exp, f"requantify_filtered (competitive={competitive})")
    assert m_res.current_version == m_chain.current_version == 0
    assert list(m_res.classifier_store) == list(m_chain.classifier_store)
    # copy-out: at most 64 bytes per table row and part for the FDR stage, and the survivors' compact rows (193 bytes
    # per distinct row, 42 per filled fragment slot of those rows, column padding)
    from alphadia_amd.scoring import requantify_multiplexed

    _, fragments = requantify_multiplexed(mc.dia, psm_df, pdf, mc.library.fragment_df, list(mc.channels),
                                          int(mc.channels[0]), True, NAMES, device=0)
    n_table, n_parts = len(psm_df) * len(mc.channels), len(mc.channels) - 1
    survivors = exp.drop_duplicates(["precursor_idx", "rank"])
    assert not survivors["precursor_idx"].duplicated().any()  # (one table row per precursor)
    n_rows, n_slots = len(survivors), int(fragments["precursor_idx"].isin(survivors["precursor_idx"]).sum())
    assert n_rows < n_slots <= 12 * n_rows
    assert moved < moved_chained, (moved, moved_chained)
    assert moved <= 64 * n_table * n_parts + 193 * n_rows + 42 * n_slots + 16 * 80, (moved, n_table, n_rows, n_slots)


# ------------------------------------------------------------------ parts with too few PSMs
class _WithColumn:
    """A ``ResidentScores`` with one more host column of the features frame, ``extra``: NaN for the precursors in
    ``unusable``, 0 elsewhere (a part whose rows are NaN there has no usable PSM)."""

    def __init__(self, resident, unusable):
        self._resident, self._unusable = resident, unusable

    def __getattr__(self, name):
        return getattr(self._resident, name)

    def extra(self, precursor_idx):
        return np.where(np.isin(precursor_idx, self._unusable), np.nan, 0.0).astype(np.float32)

    def feature_columns(self):
        return [*self._resident.feature_columns(), "extra"]

    def table_column(self, name):
        if name == "extra":
            return self.extra(self._resident.metadata["precursor_idx"].to_numpy())
        return self._resident.table_column(name)

    def frames(self, table_rows):
        features_df, fragments_df = self._resident.frames(table_rows)
        features_df["extra"] = self.extra(features_df["precursor_idx"].to_numpy())
        return features_df, fragments_df


def _manager_with_extra(dia):
    from alphadia_amd import fdr

    return fdr.HipFDRManager([*_features(), "extra"], fdr.HipBinaryClassifier(**CLASSIFIER), dia_cycle=dia.cycle,
                             random_state=7, device=0)


def test_a_part_with_too_few_psms_does_not_stop_the_others(channel_case):
    """A part with fewer than two usable rows has no train split (``TooFewPSMError``): it answers qval = proba = 1 for
    its rows, the other parts are classified, and ``_decoy`` of its rows is NaN as in the host manager's
    concatenation.  Here all rows but one of the channel that is seen first carry NaN in a classifier column."""
    case = channel_case
    scorer = _scorer(case.dia, case.library.precursor_df, case.library.fragment_df)
    inner = scorer.score_resident(case.candidates_df)
    channel, ids = inner.metadata["channel"].to_numpy(), inner.metadata["precursor_idx"].to_numpy()
    first = int(channel[np.flatnonzero(inner.valid())[0]])
    scored, _ = inner.frames(np.arange(inner.n_table))
    in_first = scored[scored["channel"] == first].dropna(subset=_features())["precursor_idx"].to_numpy()
    resident = _WithColumn(inner, np.setdiff1d(ids[channel == first], in_first[:1]))
    features_df, fragments_df = resident.frames(np.arange(inner.n_table))
    assert features_df["extra"].isna().sum() == (scored["channel"] == first).sum() - 1 > 100
    m_res, m_host = _manager_with_extra(case.dia), _manager_with_extra(case.dia)
    res = m_res.fit_predict_resident(resident, True, decoy_strategy="precursor_channel_wise")
    host = m_host.fit_predict(features_df, "precursor_channel_wise", True, df_fragments=fragments_df)
    assert [p[0][0] for p in res.attrs["parts"]][0] == first
    assert [p[2] for p in res.attrs["parts"]] == [True, False, False, False] and "too_few_psms" not in res.attrs
    assert res.attrs["parts"][0][1] == 1 and len(host) > 500
    assert len(res) == len(host)
    for c in [*ID_COLUMNS, "_decoy"]:
        assert np.array_equal(res[c].to_numpy(), host[c].to_numpy(), equal_nan=True), c
    assert np.isnan(host["_decoy"].to_numpy()[0]) and not host["_decoy"].iloc[1:].isna().any()
    assert host["qval"].iloc[0] == host["proba"].iloc[0] == res["qval"].iloc[0] == res["proba"].iloc[0] == 1.0
    assert np.allclose(res["proba"].to_numpy(), host["proba"].to_numpy(), rtol=0, atol=1e-6)
    assert np.allclose(res["qval"].to_numpy(), host["qval"].to_numpy(), rtol=1e-12, atol=0)
    assert m_res.current_version == m_host.current_version == 0


@pytest.mark.parametrize("which", ["first part", "every part"])
def test_requantify_filtered_with_too_few_psms_in_parts(which):
    """The frame of ``requantify_filtered`` is that of the chained calls also where parts have too few PSMs: its last
    columns then follow perform_fdr's answer for such a part (``qval``, ``proba``; ``_decoy`` from the classified
    parts only).  "first part": all rows of the reference and the decoy channel but one are unusable, so the first
    part has one row and the others hold targets only; "every part": all rows but one are unusable."""
    from alphadia_amd.multiplexing import HipMultiplexingRequantificationHandler
    from alphadia_amd.scoring import requantify_multiplexed

    mc, pdf, psm_df = _multiplex_inputs(300, 120, 81)
    c_ref, c_decoy = int(mc.channels[0]), int(mc.channels[-1])
    scored, _ = requantify_multiplexed(mc.dia, psm_df, pdf, mc.library.fragment_df, list(mc.channels), c_ref, True,
                                       NAMES, device=0)
    kept = scored[scored["channel"] == c_ref].dropna(subset=_features())["precursor_idx"].to_numpy()[:1]
    assert len(kept) == 1  # (a valid row without NaN in a classifier column)
    channel = pdf["channel"].to_numpy()
    of = np.isin(channel, [c_ref, c_decoy]) if which == "first part" else np.ones(len(pdf), bool)
    unusable = np.setdiff1d(pdf["precursor_idx"].to_numpy()[of], kept)

    class Handler(HipMultiplexingRequantificationHandler):
        def _score(self, dia_data, psm_df, resident):
            out = super()._score(dia_data, psm_df, resident)
            if resident:
                return _WithColumn(out, unusable)
            out[0]["extra"] = _WithColumn(None, unusable).extra(out[0]["precursor_idx"].to_numpy())
            return out

    def handler(manager):
        h = _requant_handler(mc, pdf, manager, 1.0)
        h.__class__ = Handler
        return h

    m_res, m_chain = _manager_with_extra(mc.dia), _manager_with_extra(mc.dia)
    full = handler(m_chain).requantify(mc.dia, psm_df)
    h_res = handler(m_res)
    got = h_res.requantify_filtered(mc.dia, psm_df)
    assert h_res.last_timings["path"] == "resident"
    few = full["channel"].isin([c_ref, c_decoy]).to_numpy()
    if which == "first part":
        assert list(full.columns[-3:]) == ["qval", "proba", "_decoy"]
        assert few.sum() == 1 and (~few).sum() > 100
        assert full.loc[few, "_decoy"].isna().all() and (full.loc[few, ["qval", "proba"]] == 1.0).all(axis=None)
        assert (full.loc[~few, "_decoy"] == 0).all() and set(full.loc[~few, "channel"]) == set(mc.channels[1:-1])
    else:
        assert list(full.columns[-2:]) == ["qval", "proba"] and "_decoy" not in full.columns
        assert len(full) == 1 and (full[["qval", "proba"]] == 1.0).all(axis=None)
    _assert_same(got, full, f"requantify_filtered, too few PSMs in {which}")
    assert m_res.current_version == m_chain.current_version == 0


def test_requantify_filtered_takes_the_chained_calls_for_another_manager(caplog):
    mc, pdf, psm_df = _multiplex_inputs(300, 120, 81)
    calls = []

    def fit_predict(features, **kw):
        calls.append(kw)
        return features.assign(qval=np.where(np.arange(len(features)) % 2 == 0, 0.001, 0.5))

    h = _requant_handler(mc, pdf, SimpleNamespace(fit_predict=fit_predict), 0.01)
    assert h.resident_refusal() is not None
    with caplog.at_level(logging.INFO, logger="alphadia_amd.multiplexing"):
        out = h.requantify_filtered(mc.dia, psm_df)
        out2 = h.requantify_filtered(mc.dia, psm_df)
    assert sum("not used" in msg for msg in h.log) == 1  # the reason is logged once
    assert sum("not used" in r.getMessage() for r in caplog.records) == 1
    assert calls == [dict(decoy_strategy="channel", competitive=True, decoy_channel=int(mc.channels[-1]))] * 2
    full = h.requantify(mc.dia, psm_df)
    assert 0 < len(out) == (len(full) + 1) // 2 and (out["qval"] <= 0.01).all()
    assert isinstance(out.index, pd.RangeIndex) and h.last_timings["path"] == "chained"
    pd.testing.assert_frame_equal(out, out2)
    pd.testing.assert_frame_equal(out, full[full["qval"] <= 0.01].reset_index(drop=True))
