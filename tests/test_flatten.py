"""``flatten.host_flatten_library`` - the NumPy restatement the device flatten is pinned to - against answers computed
by hand, invariants on a seeded random library, the dtype table of the reference's flat schemas and the column-name
rule.  The restatement needs no GPU; the module it lives in loads the built library, as every device module does."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import flatten_cases as fc
from alphadia_amd import flatten as fl

B, Y = ord("b"), ord("y")


def f32(v: float) -> float:
    return float(np.float32(v))


def frame(frag: pd.DataFrame) -> dict:
    return {c: frag[c].tolist() for c in frag.columns}


def test_two_charge_states_share_their_singly_charged_columns():
    pre, frag = fc.two_charge_states().host()
    assert pre["flat_frag_start_idx"].tolist() == [0, 8] and pre["flat_frag_stop_idx"].tolist() == [8, 16]
    assert frame(frag) == {
        "mz": [100, 50.5, 300, 150.5, 200, 100.5, 250, 125.5, 100, f32(50.7), 300, f32(150.7), 200, f32(100.7), 250, f32(125.7)],
        "intensity": [1.0] * 16,
        "type": [B, B, Y, Y] * 4,
        "loss_type": [0] * 16,
        "charge": [1, 2, 1, 2] * 4,
        "number": [1, 1, 2, 2, 2, 2, 1, 1] * 2,     # b counts from the N-terminus, y from the C-terminus: 2 - position
        "position": [0, 0, 0, 0, 1, 1, 1, 1] * 2,
        "cardinality": [2, 1, 2, 1] * 4,
    }
    assert pre["flat_frag_start_idx"].dtype == pre["flat_frag_stop_idx"].dtype == np.uint32


def test_target_and_decoy_of_one_elution_group_do_not_see_each_other():
    case = fc.target_and_decoy()
    assert case.host()[1]["cardinality"].tolist() == [1] * 8
    del case.precursor_df["decoy"]  # without the column they are one group
    assert case.host()[1]["cardinality"].tolist() == [2] * 8


def test_a_group_with_unequal_row_counts_stays_at_one():
    pre, frag = fc.unequal_row_counts().host()
    assert frag["cardinality"].tolist() == [1] * 20
    assert pre["flat_frag_start_idx"].tolist() == [0, 8] and pre["flat_frag_stop_idx"].tolist() == [8, 20]


def test_a_group_of_255_counts_to_255_and_one_of_256_raises():
    pre, frag = fc.group_of(255).host()
    in_group = np.repeat(pre["elution_group_idx"].to_numpy() == 5, 4)
    assert frag["cardinality"][in_group].tolist() == [255] * (255 * 4)
    assert frag["cardinality"][~in_group].tolist() == [1] * (255 * 4)
    with pytest.raises(ValueError, match="more than 255"):
        fc.group_of(256).host()


def test_one_ulp_matches_below_128_and_not_above_256():
    case = fc.one_ulp_apart()
    mz = case.fragment_mz_df.to_numpy()
    assert 0 < mz[1, 0] - mz[0, 0] < 1e-5 < mz[1, 2] - mz[0, 2]
    assert case.host()[1]["cardinality"].tolist() == [2, 1, 1, 1] * 2


def test_the_cell_at_the_threshold_is_dropped():
    pre, frag = fc.at_the_threshold().host()
    t = float(np.float32(0.01))
    assert frag["intensity"].tolist() == [float(np.nextafter(np.float32(t), np.float32(1))), 0.5]
    assert frag["charge"].tolist() == [2, 2] and frag["type"].tolist() == [B, Y]
    assert pre["flat_frag_stop_idx"].tolist() == [2]


@pytest.mark.parametrize("top_k, kept", [(1, [4]), (2, [4, 3]), (4, [4, 1, 3, 2]), (5, [4, 1, 3, 2])])
def test_top_k_of_one_of_the_cell_count_and_one_more(top_k, kept):
    pre, frag = fc.four_cells(top_k).host()
    assert frag["intensity"].tolist() == kept  # (in flat order: 4 1 / 3 2)
    assert pre["flat_frag_stop_idx"].tolist() == [len(kept)]


def test_top_k_below_one_raises():
    with pytest.raises(ValueError, match="top_k"):
        fc.four_cells(0).host()


def test_of_equal_intensities_at_rank_k_the_higher_flat_index_stays():
    _, frag = fc.ties_at_rank_k().host()
    assert frame(frag) == {"mz": [101, 104], "intensity": [5, 3], "type": [Y, Y], "loss_type": [0, 0], "charge": [1, 1],
                           "number": [5, 2], "position": [0, 3], "cardinality": [1, 1]}
    values = fc.ties_at_rank_k().fragment_intensity_df.to_numpy().ravel()
    assert sorted(np.argsort(values, kind="stable")[-2:].tolist()) == frag["position"].tolist()


@pytest.mark.parametrize("top_k, kept", [(1, [2]), (2, [2, 1]), (3, [2, 1, -0.0]), (4, [2, 1, -0.0])])
def test_nan_intensity_is_never_kept_and_ranks_last(top_k, kept):
    _, frag = fc.nan_intensity(top_k).host()
    assert frag["intensity"].tolist() == kept and frag["position"].tolist() == [1, 2, 3][:len(kept)]


def test_blocks_in_descending_start_order_with_unowned_rows():
    pre, frag = fc.descending_starts().host()
    # block order: precursor 2 (row 0), precursor 1 (rows 2-3, all zero), precursor 0 (rows 5-6 without cell (5, 1))
    assert frag["mz"].tolist() == [100, 101, 110, 112, 113]
    assert frag["position"].tolist() == [0, 0, 0, 1, 1] and frag["number"].tolist() == [1, 1, 1, 2, 1]
    assert pre.index.tolist() == [30, 10, 20]
    assert pre["flat_frag_start_idx"].tolist() == [2, 2, 0] and pre["flat_frag_stop_idx"].tolist() == [5, 2, 2]


def test_overlapping_blocks_raise():
    with pytest.raises(ValueError, match="precursors 0 and 1 overlap"):
        fc.overlapping().host()


def test_a_block_outside_the_matrices_or_too_long_raises():
    case = fc.overlapping()
    case.precursor_df["frag_stop_idx"] = [3, 5]
    with pytest.raises(ValueError, match="precursor 1 lie outside"):
        case.host()
    long = fc.Dense([[0, 256]], [0], np.ones((256, 4)), np.ones((256, 4)))
    with pytest.raises(ValueError, match="256 fragment rows"):
        long.host()


def test_an_empty_library():
    pre, frag = fc.empty_library().host()
    assert len(pre) == 0 and len(frag) == 0
    assert list(frag.columns) == list(fl.FRAGMENT_COLUMNS)
    assert pre["flat_frag_start_idx"].dtype == np.uint32 and frag["mz"].dtype == np.float32


def test_invariants_on_a_random_library():
    case = fc.random_library(n_prec=600, cols=fc.COLS8, seed=3, max_rows=20, top_k=6)
    pre, frag = case.host()
    start, stop = pre["flat_frag_start_idx"].to_numpy().astype(np.int64), pre["flat_frag_stop_idx"].to_numpy().astype(np.int64)
    rows = (pre["frag_stop_idx"] - pre["frag_start_idx"]).to_numpy()
    assert ((stop - start) <= 6).all() and ((stop - start) <= rows * 8).all() and (stop - start).max() == 6
    by_block = np.lexsort((rows, pre["frag_start_idx"].to_numpy()))
    assert start[by_block][0] == 0 and stop[by_block][-1] == len(frag)
    assert (start[by_block][1:] == stop[by_block][:-1]).all()  # the ranges tile [0, total) in block order
    owner = np.repeat(np.arange(len(pre))[by_block], (stop - start)[by_block])
    assert (frag["position"].to_numpy() < rows[owner]).all()
    nterm = frag["type"].to_numpy() == B
    assert set(frag["type"]) == {B, Y} and set(frag["loss_type"]) == {0, 17, 18, 98}
    pos, num = frag["position"].to_numpy().astype(int), frag["number"].to_numpy().astype(int)
    assert (num[nterm] == pos[nterm] + 1).all() and (num[~nterm] == rows[owner][~nterm] - pos[~nterm]).all()
    assert (frag["intensity"] > 0.01).all() and frag["cardinality"].min() == 1 and frag["cardinality"].max() > 1
    # every kept cell is a cell of its owner's block, in flat order, at least as intense as any cell left out
    mz, inten = case.fragment_mz_df.to_numpy(), case.fragment_intensity_df.to_numpy()
    for p in by_block[:50]:
        a, b = pre["frag_start_idx"].iloc[p], pre["frag_stop_idx"].iloc[p]
        got = frag.iloc[start[p]:stop[p]]
        col = np.array([case.fragment_mz_df.columns.get_loc(
            f"{chr(t)}{ {0: '', 17: '_NH3', 18: '_H2O', 98: '_modloss'}[l]}_z{z}")
            for t, l, z in zip(got["type"], got["loss_type"], got["charge"])], dtype=int)
        cells = got["position"].to_numpy().astype(int) * 8 + col
        assert (np.diff(cells) > 0).all()
        assert np.array_equal(mz[a:b].ravel()[cells], got["mz"]) and np.array_equal(inten[a:b].ravel()[cells], got["intensity"])
        left = np.delete(inten[a:b].ravel(), cells)
        if len(got) and len(left):
            assert left[left > 0.01].max(initial=0) <= got["intensity"].min()
        if len(got) < 6:
            assert (left <= np.float32(0.01)).all()


def test_the_flat_schemas_hold_after_init_flat_columns():
    case = fc.two_charge_states()
    n = len(case.precursor_df)
    for name, dtype, value in (("precursor_idx", np.uint32, 1), ("channel", np.uint32, 0), ("decoy", np.uint8, 0),
                               ("charge", np.uint8, 2), ("rt_pred", np.float32, 1.5), ("precursor_mz", np.float32, 500.25),
                               ("proteins", object, "P"), ("genes", object, "G")):
        case.precursor_df[name] = np.full(n, value, dtype=dtype)
    pre, frag = case.host()
    lib = fl.init_flat_columns(fl.BatchLibrary(pre, frag))
    # validation/schemas.py:11-48, the required columns
    precursors_flat = {"elution_group_idx": np.uint32, "precursor_idx": np.uint32, "channel": np.uint32, "decoy": np.uint8,
                       "flat_frag_start_idx": np.uint32, "flat_frag_stop_idx": np.uint32, "charge": np.uint8,
                       "rt_library": np.float32, "mobility_library": np.float32, "mz_library": np.float32,
                       "proteins": object, "genes": object}
    fragments_flat = {"mz_library": np.float32, "intensity": np.float32, "cardinality": np.uint8, "type": np.uint8,
                      "loss_type": np.uint8, "charge": np.uint8, "number": np.uint8, "position": np.uint8}
    assert {c: lib.precursor_df[c].dtype for c in precursors_flat} == {c: np.dtype(t) for c, t in precursors_flat.items()}
    assert {c: lib.fragment_df[c].dtype for c in fragments_flat} == {c: np.dtype(t) for c, t in fragments_flat.items()}
    assert (lib.precursor_df["mobility_library"] == 0).all() and "mz" not in lib.fragment_df.columns
    assert "rt_pred" not in lib.precursor_df.columns and "precursor_mz" not in lib.precursor_df.columns


def test_column_names():
    codes = fl.parse_columns(["a_z1", "b_H2O_z2", "c_NH3_z3", "x_modloss_z1", "y_z4", "z_z1"])
    assert codes.tolist() == [[97, 98, 99, 120, 121, 122], [0, 18, 17, 98, 0, 0], [1, 2, 3, 1, 4, 1], [1, 1, 1, 0, 0, 0]]
    assert codes.dtype == np.uint8
    for bad in ("b_z", "q_z1", "b_CO_z1", "b_z0", "bz1", "B_z1", "b_z1 ", 7):
        with pytest.raises(ValueError, match="fragment column"):
            fl.parse_columns(["b_z1", bad])
    with pytest.raises(ValueError, match="1 to 32"):
        fl.parse_columns(fc.COLS32 + ["b_z9"])
    assert fl.parse_columns(fc.COLS32).shape == (4, 32)
