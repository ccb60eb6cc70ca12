"""Dense libraries for tests/test_flatten.py (hand-computed answers) and tests/test_flatten_gpu.py (device against the
restatement): small ones written out cell by cell, and a seeded random one."""

from __future__ import annotations

import numpy as np
import pandas as pd

COLS4 = ["b_z1", "b_z2", "y_z1", "y_z2"]
COLS8 = COLS4 + ["b_H2O_z1", "y_NH3_z1", "b_modloss_z1", "y_modloss_z2"]
COLS32 = [f"{s}{loss}_z{z}" for s in "by" for loss in ("", "_H2O", "_NH3", "_modloss") for z in (1, 2, 3, 4)]


class Dense:
    """A dense library: ``precursor_df`` and the two frames, plus the flatten's two parameters."""

    def __init__(self, blocks, groups, mz, intensity, cols=COLS4, decoy=None, top_k=12, min_intensity=0.01, index=None):
        blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 2)
        frame = {"frag_start_idx": blocks[:, 0], "frag_stop_idx": blocks[:, 1],
                 "elution_group_idx": np.asarray(groups, dtype=np.uint32)}
        if decoy is not None:
            frame["decoy"] = np.asarray(decoy, dtype=np.uint8)
        self.precursor_df = pd.DataFrame(frame, index=index)
        mz = np.asarray(mz, dtype=np.float32).reshape(-1, len(cols))
        intensity = np.asarray(intensity, dtype=np.float32).reshape(-1, len(cols))
        self.fragment_mz_df = pd.DataFrame(mz, columns=cols)
        self.fragment_intensity_df = pd.DataFrame(intensity, columns=cols)
        self.top_k, self.min_intensity = top_k, min_intensity

    def host(self):
        from alphadia_amd.flatten import host_flatten_library

        return host_flatten_library(self.precursor_df, self.fragment_mz_df.to_numpy(), self.fragment_intensity_df.to_numpy(),
                                    list(self.fragment_mz_df.columns), self.top_k, self.min_intensity)


def two_charge_states():
    """One elution group, charge 2 and 3 of a peptide: the singly charged columns (0, 2) share m/z."""
    mz = [[100, 50.5, 300, 150.5], [200, 100.5, 250, 125.5],        # precursor 0
          [100, 50.7, 300, 150.7], [200, 100.7, 250, 125.7]]        # precursor 1
    return Dense([[0, 2], [2, 4]], [7, 7], mz, np.ones((4, 4)))


def target_and_decoy():
    """A target and a decoy of one elution_group_idx with identical m/z: they do not see each other."""
    mz = [[100, 50.5, 300, 150.5]] * 2
    return Dense([[0, 1], [1, 2]], [3, 3], mz, np.ones((2, 4)), decoy=[0, 1])


def unequal_row_counts():
    """Two and three rows in one group, equal m/z where both have a row: every cell stays at 1."""
    row = [100, 50.5, 300, 150.5]
    return Dense([[0, 2], [2, 5]], [1, 1], [row] * 5, np.ones((5, 4)))


def group_of(m, cols=COLS4, rows=1):
    """``m`` precursors in one group, scattered among ``m`` single precursors of other groups, all with equal m/z."""
    n = 2 * m
    blocks = [[i * rows, (i + 1) * rows] for i in range(n)]
    groups = [5 if i % 2 == 0 else 1000 + i for i in range(n)]
    mz = np.full((n * rows, len(cols)), 123.25)
    inten = np.tile(np.arange(1, len(cols) + 1), (n * rows, 1))
    return Dense(blocks, groups, mz, inten, cols=cols)


def one_ulp_apart():
    """Two m/z one float32 ulp apart: under 1e-5 below 128 (column 0), above it beyond 256 (column 2)."""
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))  # noqa: E731
    mz = [[100, 50.5, 300, 150.5], [up(100), 50.7, up(300), 150.7]]
    return Dense([[0, 1], [1, 2]], [2, 2], mz, np.ones((2, 4)))


def at_the_threshold():
    """Intensities around float32(0.01): the cell exactly at min_fragment_intensity is dropped."""
    t = np.float32(0.01)
    inten = [[t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 0.5]]
    return Dense([[0, 1]], [0], [[100, 50.5, 300, 150.5]], inten)


def four_cells(top_k):
    """One block of 2 x 2 cells with the intensities 4 1 / 3 2."""
    return Dense([[0, 2]], [0], [[100, 300], [200, 250]], [[4, 1], [3, 2]], cols=["b_z1", "y_z1"], top_k=top_k)


def ties_at_rank_k():
    """Five cells 5 3 3 3 1 and top_k = 2: of the equal ones the highest flat index stays."""
    return Dense([[0, 5]], [0], [[101], [102], [103], [104], [105]], [[5], [3], [3], [3], [1]], cols=["y_z1"], top_k=2)


def nan_intensity(top_k):
    """NaN 2 1 -0.0: NaN is never kept and takes nobody's place."""
    return Dense([[0, 4]], [0], [[101], [102], [103], [104]], [[np.nan], [2], [1], [-0.0]], cols=["b_z1"], top_k=top_k,
                 min_intensity=-1.0)


def descending_starts():
    """Blocks in descending start order, rows 1, 4 and 7 owned by nobody, the middle precursor keeps nothing."""
    mz = np.arange(16, dtype=np.float32).reshape(8, 2) + 100
    inten = np.ones((8, 2))
    inten[2:4] = 0.0
    inten[5, 1] = 0.0
    return Dense([[5, 7], [2, 4], [0, 1]], [0, 1, 2], mz, inten, cols=["b_z1", "y_z1"], index=[30, 10, 20])


def overlapping():
    return Dense([[0, 3], [2, 4]], [0, 1], np.ones((4, 4)), np.ones((4, 4)))


def empty_library():
    return Dense(np.empty((0, 2)), [], np.empty((0, 4)), np.empty((0, 4)))


def nothing_kept_at(where, n=5):
    """``n`` precursors of two rows; the one at ``where`` (0, the middle, the last) has only zero intensities.  The last
    block ends on the matrix's last row."""
    rng = np.random.default_rng(11 + where)
    blocks = [[2 * i, 2 * i + 2] for i in range(n)]
    inten = rng.uniform(0.1, 1.0, (2 * n, 4))
    inten[2 * where:2 * where + 2] = 0.0
    return Dense(blocks, np.arange(n), rng.uniform(100, 900, (2 * n, 4)), inten)


def one_block(rows, cols, top_k=12, seed=0):
    """One precursor of ``rows`` x ``len(cols)`` cells with duplicate intensities, between two small neighbours."""
    rng = np.random.default_rng(seed + 31 * rows + len(cols))
    R = rows + 3
    inten = rng.integers(0, 9, (R, len(cols))).astype(np.float32) / 8
    return Dense([[0, 1], [1, 1 + rows], [1 + rows, R]], [0, 1, 2], rng.uniform(100, 900, (R, len(cols))), inten,
                 cols=cols, top_k=top_k)


def random_library(n_prec=3000, cols=COLS4, seed=5, max_rows=60, top_k=12, max_group=4):
    """Mixed row counts 1 .. max_rows, 30 % zero intensities, duplicate intensities, groups of 1 .. max_group
    precursors scattered in row order (members of a group share a row count and most m/z), half of them with decoys
    of the same elution_group_idx, blocks in shuffled order with unowned rows between them."""
    rng = np.random.default_rng(seed)
    C = len(cols)
    sizes = []
    while sum(sizes) < n_prec:
        sizes.append(int(rng.integers(1, max_group + 1)))
    sizes[-1] -= sum(sizes) - n_prec
    group = np.repeat(np.arange(len(sizes)), sizes)
    g_rows = rng.integers(1, max_rows + 1, len(sizes))
    rows = g_rows[group]
    odd = rng.random(n_prec) < 0.03                      # a few members with a row count of their own
    rows = np.where(odd, rng.integers(0, max_rows + 1, n_prec), rows)
    decoy = (rng.random(len(sizes)) < 0.5)[group] & (rng.random(n_prec) < 0.5)
    perm = rng.permutation(n_prec)                       # scatter the groups
    group, rows, decoy = group[perm], rows[perm], decoy[perm]
    place = rng.permutation(n_prec)                      # block order differs from row order
    gaps = rng.integers(0, 2, n_prec)
    begin = np.empty(n_prec, dtype=np.int64)
    begin[place] = np.cumsum(gaps[place] + np.concatenate([[0], rows[place][:-1]]))
    R = int((begin + rows).max())
    base = rng.uniform(100, 1500, (len(sizes), max_rows + 1, C)).astype(np.float32)
    mz = rng.uniform(100, 1500, (R, C)).astype(np.float32)
    for p in range(n_prec):
        block = base[group[p], :rows[p]].copy()
        jitter = rng.random(block.shape) < 0.3          # 30 % of a member's cells move away from the group's m/z
        block[jitter] += np.float32(0.5)
        mz[begin[p]:begin[p] + rows[p]] = block
    inten = (rng.integers(1, 40, (R, C)) / 32).astype(np.float32)
    inten[rng.random((R, C)) < 0.3] = 0.0
    return Dense(np.stack([begin, begin + rows], axis=1), group, mz, inten, cols=cols, decoy=decoy.astype(np.uint8),
                 top_k=top_k)
