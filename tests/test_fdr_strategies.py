"""The channel-wise decoy strategies on resident tables, host side (no GPU): the C prototype of the part-staging
entry against its ctypes declaration, the NumPy restatement of the staging against the host manager's slicing
(fdr_manager.py:178-223) on the golden's input table, and the golden's generator against the committed fixture."""

import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from alphadia_amd import _abi, runtime
from alphadia_amd.fdr import part_labels, part_rows, strategy_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden_fdr_strategies as gen  # noqa: E402  (importing it runs nothing of the reference)


def _header_types(name):
    header = open(os.path.join(ROOT, "include", "alphadia_hip.h")).read()
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", header)
    assert m, name
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    return [re.sub(r"\s*\w+$", "", p).strip() for p in params]


def test_part_staging_entry_matches_the_header():
    """tests/test_abi.py holds every prototype against the header; here, what the loaded library got and how the
    part entry extends the whole-table one."""
    for name in ("adh_mlp_stage_rows_device", "adh_mlp_stage_rows_device_part"):
        restype, argtypes = _abi.PROTOTYPES[name]
        assert len(_header_types(name)) == len(argtypes)
        assert name in runtime.EXPORTED_SYMBOLS
        assert getattr(runtime.lib, name).argtypes == argtypes and getattr(runtime.lib, name).restype is restype
    # the arguments of the existing entry plus channel, target_channel, decoy_channel, label_by_channel
    old, new = _header_types("adh_mlp_stage_rows_device"), _header_types("adh_mlp_stage_rows_device_part")
    assert new[: len(old) - 2] == old[:-2] and new[-2:] == old[-2:]
    assert new[len(old) - 2: -2] == ["const int64_t *", "int64_t", "int64_t", "int32_t"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "fdr_strategies.npz"))


def _table(golden) -> pd.DataFrame:
    return pd.DataFrame({c: golden["in/" + c] for c in gen.INPUT_COLUMNS})


def test_golden_input_table_is_what_the_strategies_need(golden):
    tab = _table(golden)
    assert list(pd.unique(tab["channel"])) == list(gen.CHANNELS) != sorted(gen.CHANNELS)
    assert all(0 < int(tab[c].isna().sum()) < 20 for c in gen.FEATURES)
    for c in gen.CHANNELS:  # decoys by column in every channel, NaN rows in the decoy channel too
        assert set(tab.loc[tab["channel"] == c, "decoy"]) == {0, 1}
    assert tab.loc[tab["channel"] == gen.DECOY_CHANNEL, gen.FEATURES].isna().any(axis=None)
    pd.testing.assert_frame_equal(tab, gen.input_table())


def _host_slicing(features_df, part):
    """fdr_manager.py:181-220 and fdr.py:86-119 as written: the rows perform_fdr concatenates, and their labels."""
    target, decoy_channel, by_channel = part
    sub = features_df[features_df["channel"].isin([target, decoy_channel])]
    if by_channel:
        df_t, df_d = sub[sub["channel"] != decoy_channel], sub[sub["channel"] == decoy_channel]
    else:
        df_t, df_d = sub[sub["decoy"] == 0], sub[sub["decoy"] == 1]
    df_t, df_d = df_t.dropna(subset=gen.FEATURES), df_d.dropna(subset=gen.FEATURES)
    return np.concatenate([df_t.index.to_numpy(), df_d.index.to_numpy()]), len(df_t), len(df_d)


def test_numpy_restatement_selects_what_the_host_manager_slices(golden):
    tab = _table(golden)
    n = len(tab)
    valid = np.random.default_rng(4).random(n) < 0.85  # the features frame holds the valid table rows only
    valid[: 2 * len(gen.CHANNELS)] = [False, True, False, False, False, False, True, False]  # first valid: 0, then 4
    features_df = tab[valid]  # (index = table row)
    usable = ~tab[gen.FEATURES].isna().any(axis=1).to_numpy()
    decoy, channel = tab["decoy"].to_numpy(), tab["channel"].to_numpy()

    cw = strategy_parts("precursor_channel_wise", channel, valid)
    assert cw == [(int(c), -1, 0) for c in features_df["channel"].unique()]
    assert [p[0] for p in cw][:2] == [0, 4] and sorted(p[0] for p in cw) == sorted(gen.CHANNELS)
    ch = strategy_parts("channel", channel, valid, gen.DECOY_CHANNEL)
    assert ch == [(c, gen.DECOY_CHANNEL, 1) for c in sorted(set(gen.CHANNELS) - {gen.DECOY_CHANNEL})]
    with pytest.raises(ValueError):
        strategy_parts("precursor", channel, valid)
    # a channel whose rows are all invalid is no part (features_df["channel"].unique() does not see it)
    gone = valid & (channel != 4)
    assert 4 not in [p[0] for p in strategy_parts("precursor_channel_wise", channel, gone)]
    assert 4 not in [p[0] for p in strategy_parts("channel", channel, gone, gen.DECOY_CHANNEL)]

    extra = [(0, -1, 1), (8, -1, 0), (5, gen.DECOY_CHANNEL, 1), (5, -1, 0), (5, -1, 1), (gen.DECOY_CHANNEL, 0, 0)]
    for part in cw + ch + extra:  # decoy_channel = -1 matches nothing; channel 5 has no rows
        rows, n_t, n_d = part_rows(valid, usable, decoy, channel, part)
        exp_rows, exp_t, exp_d = _host_slicing(features_df, part)
        assert np.array_equal(rows, exp_rows) and (n_t, n_d) == (exp_t, exp_d), part
        labels = part_labels(decoy, channel, part)[rows]
        assert np.array_equal(labels, np.r_[np.zeros(n_t), np.ones(n_d)]), part
    assert part_rows(valid, usable, decoy, channel, (5, -1, 1))[1:] == (0, 0)
    assert part_rows(valid, usable, decoy, channel, (0, -1, 1))[2] == 0
    assert part_rows(valid, usable, decoy, channel, (5, gen.DECOY_CHANNEL, 1))[1] == 0
    # no part: every usable row, split by the decoy column (the "precursor" strategy)
    rows, n_t, n_d = part_rows(valid, usable, decoy, channel)
    ok = features_df.dropna(subset=gen.FEATURES)
    assert np.array_equal(rows, np.r_[ok.index[ok["decoy"] == 0], ok.index[ok["decoy"] == 1]])
    assert n_t + n_d == len(ok) > 1000


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference checkout is not on this machine")
def test_regenerating_the_golden_reproduces_the_committed_file(golden, tmp_path):
    p = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_fdr_strategies.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    fresh = np.load(tmp_path / "fdr_strategies.npz")
    assert sorted(fresh.files) == sorted(golden.files)
    expected = {"in/" + c for c in gen.INPUT_COLUMNS} | {
        f"{gen.tag(s, comp)}/{c}" for s in gen.STRATEGIES for comp in (False, True) for c in gen.RESULT_COLUMNS}
    assert set(golden.files) == expected
    for name in golden.files:
        assert fresh[name].dtype == golden[name].dtype, name
        assert np.array_equal(fresh[name], golden[name], equal_nan=True), name
