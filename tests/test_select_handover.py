"""The selection -> scoring hand-over, host side: ``selection.host_assemble_selected`` - the NumPy restatement of
``adh_assemble_selected`` and the parity reference of the device - must give what the frame path gives: the frame logic
of ``HipCandidateSelection.__call__`` (``candidate_frame``), the cutoff filter of the extraction handler and
``scoring.assemble_candidates``.  No GPU."""

import os
import re

import numpy as np
import pandas as pd
import pytest

from alphadia_amd import _abi
from alphadia_amd.scoring import assemble_candidates
from alphadia_amd.selection import CANDIDATE_COLUMNS, candidate_frame, cutoff_threshold, host_assemble_selected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOA_KEYS = ["order", "prec_row", "score_group_idx", "elution_group_idx", "decoy", "channel", "precursor_idx", "rank", "flags",
            "frag_start_idx", "frag_stop_idx", "charge", "precursor_mz", "isotope_intensity", "scan_start", "scan_stop",
            "scan_center", "frame_start", "frame_stop", "frame_center"]


def _library(n, rng, presorted, channels=1):
    """A precursor table sorted by precursor_idx (as the selection operator keeps it).  ``presorted``: elution groups
    ascend with the precursors, targets before decoys; otherwise they are shuffled, so that precursor order is not
    score-group order."""
    groups = np.repeat(np.arange((n + 2 * channels - 1) // (2 * channels)), 2 * channels)[:n]
    decoy = (np.arange(n) // channels) % 2
    channel = (np.arange(n) % channels) * 4
    if not presorted:
        groups = rng.permutation(groups.max() + 1)[groups]
    fs = np.cumsum(rng.integers(1, 9, n))
    return pd.DataFrame({
        "precursor_idx": np.arange(n, dtype=np.uint32) * 3 + 5,  # (not the row number)
        "elution_group_idx": groups.astype(np.uint32), "decoy": decoy.astype(np.uint8), "channel": channel.astype(np.uint8),
        "flat_frag_start_idx": (fs - 1).astype(np.uint32), "flat_frag_stop_idx": (fs + rng.integers(0, 5, n)).astype(np.uint32),
        "charge": rng.integers(1, 5, n).astype(np.uint8), "mz_library": rng.uniform(300, 900, n).astype(np.float32),
        "i_0": rng.random(n).astype(np.float32), "i_1": rng.random(n).astype(np.float32), "i_2": rng.random(n).astype(np.float32),
    })


def _table(lib, cc, rng, zero_fraction=0.3):
    n = len(lib) * cc
    score = rng.integers(1, 40, n).astype(np.float32) / 4  # (few distinct values: cutoffs hit existing scores)
    score[rng.random(n) < zero_fraction] = 0
    t = {"precursor_idx": np.repeat(lib["precursor_idx"].to_numpy(), cc), "rank": np.tile(np.arange(cc, dtype=np.uint8), len(lib)),
         "score": score}
    for c in CANDIDATE_COLUMNS[3:]:
        t[c] = rng.integers(0, 5000, n).astype(np.uint32)
    for c in CANDIDATE_COLUMNS:
        t[c] = np.where(score > 0, t[c], 0).astype(t[c].dtype)  # (rows without a candidate stay zero)
    return t


def _precursor_columns(lib):
    return {"frag_start_idx": lib["flat_frag_start_idx"].to_numpy(), "frag_stop_idx": lib["flat_frag_stop_idx"].to_numpy(),
            "charge": lib["charge"].to_numpy(), "precursor_mz": lib["mz_library"].to_numpy(),
            "isotope_intensity": lib[["i_0", "i_1", "i_2"]].to_numpy(), "elution_group_idx": lib["elution_group_idx"].to_numpy(),
            "decoy": lib["decoy"].to_numpy(), "channel": lib["channel"].to_numpy()}


def _frame_path(table, lib, apply_cutoff, cutoff, score_grouped, reference_channel):
    frame = candidate_frame(table, lib)
    n_selected = len(frame)
    if apply_cutoff:
        frame = frame[frame["score"] > cutoff]
    return frame, n_selected, assemble_candidates(frame, lib, "mz_library", score_grouped=score_grouped,
                                                  reference_channel=reference_channel)


def _check(table, lib, cc, apply_cutoff=False, cutoff=0.0, score_grouped=False, reference_channel=-1):
    frame, n_selected, exp = _frame_path(table, lib, apply_cutoff, cutoff, score_grouped, reference_channel)
    got = host_assemble_selected(table, _precursor_columns(lib), cc, apply_cutoff, cutoff, score_grouped, reference_channel)
    assert got["n_selected"] == n_selected and got["n_kept"] == len(frame)
    for k in SOA_KEYS:
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        assert a.shape == b.shape and np.array_equal(a, b), k
        if k not in ("order", "prec_row"):
            assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
    # the ids the host derives: the join is a division, the index labels are the positions among the score > 0 rows
    assert np.array_equal(got["table_row"] // cc, exp["prec_row"])
    assert np.array_equal(np.sort(got["selected_pos"]), frame.index.to_numpy())
    assert np.array_equal(got["selected_pos"], frame.index.to_numpy()[exp["order"]])
    return got, exp


@pytest.mark.parametrize("presorted", [True, False])
@pytest.mark.parametrize("cc", [1, 3])
def test_restatement_equals_the_frame_path(presorted, cc):
    rng = np.random.default_rng(17 + cc + 10 * presorted)
    lib = _library(700, rng, presorted)
    table = _table(lib, cc, rng)
    got, _ = _check(table, lib, cc)
    assert got["was_sorted"] == presorted
    assert 0 < got["n_kept"] < len(lib) * cc  # zero-score rows were dropped
    scores = table["score"][table["score"] > 0]
    existing = float(np.median(scores))
    assert (scores == existing).any()
    got, _ = _check(table, lib, cc, apply_cutoff=True, cutoff=existing)  # strict >: rows at the cutoff go
    assert got["n_kept"] == int((scores > existing).sum()) <= got["n_selected"] - int((scores == existing).sum())
    got, _ = _check(table, lib, cc, apply_cutoff=True, cutoff=float(scores.max()) + 1)
    assert got["n_kept"] == 0 and got["n_selected"] == len(scores)
    _check(table, lib, cc, apply_cutoff=True, cutoff=-1.0)  # (score > 0 still applies)


def test_cutoff_compares_in_the_dtype_numpy_picks():
    rng = np.random.default_rng(3)
    lib = _library(50, rng, True)
    table = _table(lib, 2, rng, zero_fraction=0.0)
    table["score"][:] = np.float32(0.1)
    # float32(0.1) > 0.1 is False where NumPy compares in float32 and True in float64
    expected = bool((table["score"] > 0.1).any())
    got, _ = _check(table, lib, 2, apply_cutoff=True, cutoff=0.1)
    assert (got["n_kept"] > 0) == expected
    assert cutoff_threshold(0.1) == float(np.asarray(0.1).astype(np.result_type(np.float32, 0.1)))
    _check(table, lib, 2, apply_cutoff=True, cutoff=np.float64(0.1))


@pytest.mark.parametrize("presorted", [True, False])
@pytest.mark.parametrize("reference_channel", [-1, 0, 4, 9])
def test_score_groups_and_reference_channel(presorted, reference_channel):
    rng = np.random.default_rng(40 + reference_channel)
    lib = _library(600, rng, presorted, channels=3)  # channels 0, 4, 8 share an elution group and a decoy flag
    table = _table(lib, 2, rng)
    got, exp = _check(table, lib, 2, score_grouped=True, reference_channel=reference_channel)
    assert got["score_group_idx"].max() + 1 < got["n_kept"]  # groups of several rows
    skipped = int((got["flags"] == _abi.FLAG_SKIP).sum())
    if reference_channel < 0:
        assert skipped == 0
    elif reference_channel == 9:
        assert skipped == got["n_kept"]  # no group has a row of that channel
    else:
        assert 0 < skipped < got["n_kept"]  # (zero-score rows took the reference row out of some groups)
    _check(table, lib, 2, score_grouped=False, reference_channel=reference_channel)
    _check(table, lib, 2, apply_cutoff=True, cutoff=3.0, score_grouped=True, reference_channel=reference_channel)


def test_duplicate_precursor_in_a_score_group_is_the_hosts_error():
    rng = np.random.default_rng(9)
    lib = _library(40, rng, True)
    lib.loc[11, "precursor_idx"] = lib.loc[10, "precursor_idx"]  # two library rows, one precursor_idx, one group
    lib.loc[11, ["elution_group_idx", "decoy"]] = lib.loc[10, ["elution_group_idx", "decoy"]].to_numpy()
    table = _table(lib, 1, rng, zero_fraction=0.0)
    frame = pd.DataFrame({c: table[c] for c in CANDIDATE_COLUMNS}).assign(elution_group_idx=np.repeat(lib["elution_group_idx"].to_numpy(), 1),
                                                                        decoy=lib["decoy"].to_numpy())
    with pytest.raises(ValueError, match="precursor_idx must be unique within a score group") as host:
        assemble_candidates(frame, lib.drop_duplicates("precursor_idx"), "mz_library", score_grouped=True)
    with pytest.raises(ValueError, match="precursor_idx must be unique within a score group") as ours:
        host_assemble_selected(table, _precursor_columns(lib), 1, score_grouped=True)
    assert str(host.value) == str(ours.value)
    host_assemble_selected(table, _precursor_columns(lib), 1, score_grouped=False)  # every row its own group


def test_empty_tables():
    rng = np.random.default_rng(1)
    lib = _library(30, rng, True)
    table = _table(lib, 2, rng, zero_fraction=1.1)
    got, _ = _check(table, lib, 2, score_grouped=True, reference_channel=0)
    assert got["n_kept"] == got["n_selected"] == 0 and got["was_sorted"]


def test_handover_abi_declarations_agree():
    """Every hand-over entry is in the prototype table (tests/test_abi.py holds it against the header), one after the
    other as in the header, and defined in adh_select_handover.hip, which adh_api.hip includes (no library loaded)."""
    names = ["adh_select_candidates_resident", "adh_assemble_selected", "adh_select_handover_stats",
             "adh_score_selected_resident", "adh_selected_ids", "adh_take_selected"]
    table = list(_abi.PROTOTYPES)
    assert table[table.index(names[0]):][: len(names)] == names
    csrc = open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_select_handover.hip")).read()
    for name in names:
        assert re.search(rf"\bint {name}\(", csrc), name
    assert '#include "adh_select_handover.hip"' in open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_api.hip")).read()
