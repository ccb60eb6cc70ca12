"""Golden vectors of the decoy strategies of the FDR manager, produced by RUNNING THE REFERENCE
(alphadia/workflow/managers/fdr_manager.py: ``FDRManager.fit_predict``) in the build container:

    python tests/golden/make_golden_fdr_strategies.py

TEST INFRASTRUCTURE, same rules as make_golden.py: the reference is imported from /root/reference through
``ref_shim`` (third-party stubs only), fed a seeded synthetic table, and the table + the results are stored in
``tests/golden/fdr_strategies.npz``.  The classifier is a stand-in whose probability is a fixed function of the feature
row, so the same row scores the same in every part of a strategy and no network training enters: what is pinned is the
manager's slicing, labelling, grouping and concatenation.

Importing this module runs nothing of the reference (``input_table`` and ``StandInClassifier`` are shared with the
tests); ``main`` does.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))

FEATURES = ["f0", "f1"]
CHANNELS = (8, 0, 4, 12)  # interleaved in this order: first appearance is not ascending
DECOY_CHANNEL = 12
N_GROUPS = 400
STRATEGIES = ("precursor", "precursor_channel_wise", "channel")
RESULT_COLUMNS = ("precursor_idx", "channel", "decoy", "_decoy", "proba", "qval")
INPUT_COLUMNS = (*FEATURES, "precursor_idx", "elution_group_idx", "channel", "decoy", "rank")


class StandInClassifier:
    """Class-1 probability = a rounded squashing of the sum of the feature row: plain IEEE arithmetic, so every
    platform agrees, and symmetric in the columns, because the reference manager lists them in a set's iteration
    order; the rounding makes ties.  ``fit`` learns nothing."""

    fitted = True

    def fit(self, x, y):
        pass

    def predict_proba(self, x):
        x = np.asarray(x).astype(np.float64)
        assert x.shape[1] == 2
        v = x[:, 0] + x[:, 1]
        p = np.round(0.5 + 0.5 * v / (1.0 + np.abs(v)), 3)
        return np.stack([1.0 - p, p], axis=1)

    def predict(self, x):
        return np.argmax(self.predict_proba(x), axis=1)

    def to_state_dict(self):
        return {}

    def from_state_dict(self, state_dict, **kwargs):  # (the reference manager's constructor loads its classifier store)
        pass


def input_table(seed: int = 20261018) -> pd.DataFrame:
    """``N_GROUPS`` elution groups x ``CHANNELS``, channels interleaved; decoys (by column) are the odd groups of every
    channel; true hits sit among the target rows outside the decoy channel; a few NaN features.  Every third group has a
    second precursor per channel, with the other decoy flag, so that competitive scoring (one row per elution group and
    channel) keeps fewer rows than plain scoring (one per precursor); every fifth group has its first precursors at a
    second rank as well, so that the best row of a precursor is chosen among two."""
    rng = np.random.default_rng(seed)
    n_c = len(CHANNELS)
    n_base = N_GROUPS * n_c
    base_group = np.repeat(np.arange(N_GROUPS), n_c)
    second = np.flatnonzero(base_group % 3 == 0)  # a second precursor of the same group and channel
    ranked = np.flatnonzero(base_group % 5 == 0)  # the same precursor at rank 1
    source = np.concatenate([np.arange(n_base), second, ranked])
    n = len(source)
    group = base_group[source]
    channel = np.tile(np.asarray(CHANNELS), N_GROUPS)[source]
    decoy = (group % 2).astype(np.uint8)
    decoy[n_base: n_base + len(second)] ^= 1
    precursor_idx = rng.permutation(n_base + len(second))[np.concatenate([np.arange(n_base + len(second)), ranked])]
    rank = np.zeros(n, np.uint8)
    rank[n_base + len(second):] = 1
    true_hit = (decoy == 0) & (channel != DECOY_CHANNEL) & (rng.random(n) < 0.6)
    f0 = (rng.normal(size=n) - 2.5 * true_hit).astype(np.float32)
    f1 = (0.3 * rng.normal(size=n)).astype(np.float32)
    f0[rng.choice(n, 13, replace=False)] = np.nan
    f1[rng.choice(n, 11, replace=False)] = np.nan
    table = pd.DataFrame({
        "f0": f0, "f1": f1,
        "precursor_idx": precursor_idx.astype(np.uint32),
        "elution_group_idx": group.astype(np.uint32),
        "channel": channel.astype(np.uint32),
        "decoy": decoy,
        "rank": rank,
    })
    # group by group, the first precursors first: the channels still appear in the order of CHANNELS
    return table.iloc[np.argsort(group, kind="stable")].reset_index(drop=True)


def tag(strategy: str, competitive: bool) -> str:
    return f"{strategy}/{'competitive' if competitive else 'plain'}"


def main():
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    sys.path.insert(0, HERE)
    import ref_shim

    ref_shim.install()
    from alphadia.workflow.managers.fdr_manager import FDRManager

    table = input_table()
    d = {"in/" + c: table[c].to_numpy() for c in INPUT_COLUMNS}
    for strategy in STRATEGIES:
        for competitive in (False, True):
            manager = FDRManager(FEATURES, StandInClassifier(), config={"search": {"compete_for_fragments": False}},
                                 path=None, load_from_file=False, random_state=3)
            res = manager.fit_predict(table.copy(), strategy, competitive,
                                      decoy_channel=DECOY_CHANNEL if strategy == "channel" else -1)
            for c in RESULT_COLUMNS:
                d[f"{tag(strategy, competitive)}/{c}"] = res[c].to_numpy()
            print(f"{tag(strategy, competitive)}: {len(res)} rows, {int((res['qval'] <= 0.05).sum())} at q <= 0.05")
    path = os.path.join(out_dir, "fdr_strategies.npz")
    np.savez_compressed(path, **d)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
