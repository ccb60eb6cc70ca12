"""The candidate library of transfer-library requantification, host side: the NumPy restatement of the mass rules
and the row order on hand-checked cases, the scan, the ABI against the header, the handler's error paths and the
fragment ranges of the candidates.  The device side is in tests/test_candidate_library_gpu.py."""

from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import candidate_library_cases as G
from alphadia_amd import _abi
from alphadia_amd import transfer_requantification as trq
from alphadia_amd.fragcomp import candidate_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# PEPTIDEK, singly charged, from the residue masses by hand: b1 .. b7 and y7 .. y1 (position 0 .. 6)
PEPTIDEK_B = [98.06004032, 227.10263341, 324.15539726, 425.20307573, 538.28713971, 653.31408274, 782.35667583]
PEPTIDEK_Y = [831.40943970, 702.36684661, 605.31408276, 504.26640429, 391.18234031, 276.15539728, 147.11280419]


def _frame(sequence, mods="", sites=""):
    one = isinstance(sequence, str)
    sequence = [sequence] if one else list(sequence)
    mods = [mods] * len(sequence) if isinstance(mods, str) else list(mods)
    sites = [sites] * len(sequence) if isinstance(sites, str) else list(sites)
    return pd.DataFrame({"sequence": np.array(sequence, dtype=object), "mods": np.array(mods, dtype=object),
                         "mod_sites": np.array(sites, dtype=object), "charge": np.full(len(sequence), 2, np.uint8)})


def _library(frame, max_charge=1, mz_dtype=np.float64):
    _, series, args = G.tables_of(frame, max_charge=max_charge)
    return series, trq.host_candidate_library(*args, mz_dtype=mz_dtype)


def test_peptidek_masses():
    series, (start, stop, cols) = _library(_frame("PEPTIDEK"))
    assert series[0] == ["b_z1", "y_z1"]
    assert start.tolist() == [0] and stop.tolist() == [14]
    mz = cols["mz_library"].reshape(7, 2)
    assert np.abs(mz[:, 0] - PEPTIDEK_B).max() < 1e-6
    assert np.abs(mz[:, 1] - PEPTIDEK_Y).max() < 1e-6
    # the float32 column is the rounding of those values
    _, (_, _, cols32) = _library(_frame("PEPTIDEK"), mz_dtype=np.float32)
    assert cols32["mz_library"].dtype == np.float32
    assert np.array_equal(cols32["mz_library"], cols["mz_library"].astype(np.float32))
    # doubly charged: (m + 2 p) / 2 from the singly charged (m + p)
    _, (_, _, cols2) = _library(_frame("PEPTIDEK"), max_charge=2)
    mz2 = cols2["mz_library"].reshape(7, 4)
    assert np.abs(mz2[:, 1] - ((np.array(PEPTIDEK_B) - G.MASS_PROTON) / 2 + G.MASS_PROTON)).max() < 1e-6
    assert np.abs(mz2[:, 3] - ((np.array(PEPTIDEK_Y) - G.MASS_PROTON) / 2 + G.MASS_PROTON)).max() < 1e-6


def test_row_order_number_and_position():
    series, (start, stop, cols) = _library(_frame(["PEPTIDEK", "AG", "GASP"]), max_charge=2)
    assert series[0] == ["b_z1", "b_z2", "y_z1", "y_z2"]
    assert series[1].tolist() == [98, 98, 121, 121] and series[2].tolist() == [1, 1, 0, 0] and series[3].tolist() == [1, 2, 1, 2]
    assert start.tolist() == [0, 28, 32] and stop.tolist() == [28, 32, 44]
    assert start.dtype == np.uint32 and stop.dtype == np.uint32
    # position-major: the four series of position 0, then of position 1, ...
    assert cols["position"][:28].tolist() == [i for i in range(7) for _ in range(4)]
    assert cols["type"][:8].tolist() == [98, 98, 121, 121] * 2
    assert cols["charge"][:8].tolist() == [1, 2, 1, 2] * 2
    assert cols["number"][:28].tolist() == [v for i in range(7) for v in (i + 1, i + 1, 7 - i, 7 - i)]
    assert cols["position"][28:32].tolist() == [0] * 4 and cols["number"][28:32].tolist() == [1, 1, 1, 1]
    assert cols["number"][32:44].tolist() == [1, 1, 3, 3, 2, 2, 2, 2, 3, 3, 1, 1]
    assert (cols["intensity"] == 1).all() and cols["intensity"].dtype == np.float32
    assert not cols["loss_type"].any() and not cols["cardinality"].any()
    for name in ("type", "loss_type", "charge", "number", "position", "cardinality"):
        assert cols[name].dtype == np.uint8 and cols[name].shape == (44,)
    # b_i + y_i of a position add up to the peptide: (b - p) + (y - p) = pep
    mz = cols["mz_library"][:28].reshape(7, 4)
    pep = sum(G.RESIDUE_MASS[a] for a in "PEPTIDEK") + G.MASS_H2O
    assert np.abs(mz[:, 0] + mz[:, 2] - 2 * G.MASS_PROTON - pep).max() < 1e-9


def test_modification_sites():
    ac, am, ox, ph = (G.MOD_MASS[k] for k in ("Acetyl@Protein_N-term", "Amidated@Any_C-term", "Oxidation@M", "Phospho@S"))
    plain = _library(_frame("PEPTIDEK"))[1][2]["mz_library"].reshape(7, 2)

    def shifted(mods, sites):
        return _library(_frame("PEPTIDEK", mods, sites))[1][2]["mz_library"].reshape(7, 2) - plain

    d = shifted("Acetyl@Protein_N-term", "0")  # site 0 is residue 0: every b ion, no y ion
    assert np.abs(d[:, 0] - ac).max() < 1e-9 and np.abs(d[:, 1]).max() < 1e-9
    d = shifted("Amidated@Any_C-term", "-1")  # site -1 is the last residue: every y ion, no b ion
    assert np.abs(d[:, 0]).max() < 1e-9 and np.abs(d[:, 1] - am).max() < 1e-9
    d = shifted("Oxidation@M", "8")  # site s >= 1 is residue s - 1: here the last one as well
    assert np.abs(d[:, 0]).max() < 1e-9 and np.abs(d[:, 1] - ox).max() < 1e-9
    d = shifted("Oxidation@M", "1")  # ... and residue 0
    assert np.abs(d[:, 0] - ox).max() < 1e-9 and np.abs(d[:, 1]).max() < 1e-9
    d = shifted("Oxidation@M;Phospho@S", "3;3")  # two on residue 2: b3 and up, y7 and y6
    assert np.abs(d[:2, 0]).max() < 1e-9 and np.abs(d[2:, 0] - (ox + ph)).max() < 1e-9
    assert np.abs(d[:2, 1] - (ox + ph)).max() < 1e-9 and np.abs(d[2:, 1]).max() < 1e-9


def test_modifications_are_added_in_list_order():
    """(aa + big) + small and (aa + small) + big differ in the last bit for these values: the list order decides."""
    big, small = 2.0**30, 2.0**-24 * 3
    table = {"big": big, "small": small}
    aa = G.RESIDUE_MASS["P"]
    assert (aa + big) + small != (aa + small) + big
    out = []
    for mods in ("big;small", "small;big"):
        arrays = trq.candidate_library_tables(["PK"], [mods], ["1;1"], table)
        series = trq.charged_series(["b"], 1)
        _, _, cols = trq.host_candidate_library(arrays["seq_offset"], arrays["residues"], arrays["mod_offset"],
                                                arrays["mod_site"], arrays["mod_mass"], G.aa_mass_table(), 0.0, 0.0,
                                                *series[1:], mz_dtype=np.float64)
        out.append(float(cols["mz_library"][0]))
    assert out == [(aa + big) + small, (aa + small) + big]


def test_prefix_is_summed_left_to_right():
    frame = G.draw_precursors(40, seed=3)
    arrays, _, args = G.tables_of(frame, max_charge=1)
    _, _, cols = trq.host_candidate_library(*args, mz_dtype=np.float64)
    table = G.aa_mass_table()
    row = 0
    for p in range(len(frame)):
        res = arrays["residues"][arrays["seq_offset"][p]:arrays["seq_offset"][p + 1]]
        m = [float(table[r]) for r in res]
        for k in range(arrays["mod_offset"][p], arrays["mod_offset"][p + 1]):
            s = int(arrays["mod_site"][k])
            m[0 if s == 0 else len(m) - 1 if s == -1 else s - 1] += float(arrays["mod_mass"][k])
        acc, prefix = 0.0, []
        for v in m:  # (0.0 + m[0] is m[0])
            acc = acc + v
            prefix.append(acc)
        pep = prefix[-1] + G.MASS_H2O
        for i in range(len(m) - 1):
            assert cols["mz_library"][row] == prefix[i] / 1.0 + G.MASS_PROTON
            assert cols["mz_library"][row + 1] == (pep - prefix[i]) / 1.0 + G.MASS_PROTON
            row += 2
    assert row == len(cols["mz_library"])


def test_scan_and_integer_columns():
    frame = G.draw_precursors(60, seed=4)
    for max_charge in (1, 2, 3):
        arrays, series, args = G.tables_of(frame, max_charge=max_charge)
        start, stop, cols = trq.host_candidate_library(*args)
        L = np.diff(arrays["seq_offset"])
        rows = (L - 1) * 2 * max_charge
        assert np.array_equal(stop, np.cumsum(rows)) and np.array_equal(start, np.cumsum(rows) - rows)
        assert len(cols["mz_library"]) == rows.sum()
        ints = trq.integer_columns(L, start, *series[1:])
        for name, column in ints.items():
            assert np.array_equal(column, cols[name]) and column.dtype == cols[name].dtype, name
        assert list(trq.fragment_frame(cols, cols["mz_library"].astype(np.float64)).columns) == list(trq.FRAGMENT_COLUMNS)
        assert list(trq.fragment_frame(cols).columns) == [c for c in trq.FRAGMENT_COLUMNS if c != "mz_calibrated"]
    # the longest sequence: number and position reach 254 without wrapping
    _, _, cols = trq.host_candidate_library(*G.tables_of(_frame("G" * 255), max_charge=1)[2])
    assert cols["position"].max() == 253 and cols["number"].max() == 254 and cols["number"].min() == 1


def test_restatement_refusals():
    def build(frame, **kw):
        return trq.host_candidate_library(*G.tables_of(frame, **kw)[2])

    with pytest.raises(ValueError, match="2 .. 255"):
        build(_frame(["PEPTIDEK", "K"]))
    with pytest.raises(ValueError, match="2 .. 255"):
        build(_frame("G" * 256))
    with pytest.raises(ValueError, match="outside"):
        build(_frame("PEPTIDEK", "Oxidation@M", "9"))
    with pytest.raises(ValueError, match="outside"):
        build(_frame("PEPTIDEK", "Oxidation@M", "-2"))
    _, _, args = G.tables_of(_frame("PEPTIDEK"))
    high = list(args)
    high[1] = args[1].copy()
    high[1][3] = 200
    with pytest.raises(ValueError, match="128"):
        trq.host_candidate_library(*high)
    none = list(args)
    none[8:] = [np.zeros(0, np.uint8)] * 3
    with pytest.raises(ValueError, match="no fragment series"):
        trq.host_candidate_library(*none)
    start, stop, cols = build(_frame([]))
    assert len(start) == len(stop) == 0 and all(len(c) == 0 for c in cols.values())


def test_tables_from_strings():
    with pytest.raises(KeyError, match="Unobtainium@X"):
        trq.candidate_library_tables(["PEPTIDEK"], ["Oxidation@M;Unobtainium@X"], ["1;2"], G.MOD_MASS)
    with pytest.raises(ValueError, match="different numbers"):
        trq.candidate_library_tables(["PEPTIDEK"], ["Oxidation@M;Phospho@S"], ["1"], G.MOD_MASS)
    with pytest.raises(ValueError, match="different numbers"):
        trq.candidate_library_tables(["PEPTIDEK"], [""], ["1"], G.MOD_MASS)
    with pytest.raises(ValueError, match="ASCII"):
        trq.candidate_library_tables(["PEPTIDÉK"], [""], [""], G.MOD_MASS)
    t = trq.candidate_library_tables(["PEPTIDEK", "AG", "GASP"], ["Oxidation@M;Phospho@S", "", "Acetyl@Protein_N-term"],
                                     ["3;-1", "", "0"], G.MOD_MASS)
    assert t["seq_offset"].tolist() == [0, 8, 10, 14] and bytes(t["residues"]) == b"PEPTIDEKAGGASP"
    assert t["mod_offset"].tolist() == [0, 2, 2, 3] and t["mod_site"].tolist() == [3, -1, 0]
    assert t["mod_mass"].tolist() == [G.MOD_MASS["Oxidation@M"], G.MOD_MASS["Phospho@S"], G.MOD_MASS["Acetyl@Protein_N-term"]]
    assert t["mod_site"].dtype == np.int32 and t["mod_mass"].dtype == np.float64 and t["seq_offset"].dtype == np.int64
    with pytest.raises(ValueError, match="not supported"):
        trq.charged_series(["b", "y", "b_modloss"], 2)
    with pytest.raises(ValueError, match="at most"):
        trq.charged_series(["b", "y"], 33)


# ---- the ABI --------------------------------------------------------------------------------------------------------

def _header() -> str:
    with open(os.path.join(ROOT, "include", "alphadia_hip.h")) as f:
        return f.read()


def test_struct_matches_the_header():
    body = re.search(r"typedef struct adh_candidate_library \{(.*?)\} adh_candidate_library_t;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint8_t": C.c_uint8, "double": C.c_double}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, decl
        fields.append((m.group(4), C.POINTER(ctype[m.group(2)]) if m.group(3) else ctype[m.group(2)]))
    assert fields == list(_abi.CandidateLibrary._fields_)
    limit = int(re.search(r"#define ADH_CANDIDATE_LIBRARY_MAX_SERIES (\d+)", _header()).group(1))
    assert limit == _abi.CANDIDATE_LIBRARY_MAX_SERIES
    m = _abi.pack_candidate_library(*G.tables_of(_frame(["PEPTIDEK", "AG"]))[2])
    assert m.struct.n == 2 and m.struct.n_series == 4 and m.struct.mass_h2o == G.MASS_H2O
    with pytest.raises(ValueError, match="128"):
        _abi.pack_candidate_library(*G.tables_of(_frame("AG"))[2][:5], np.zeros(26), 1.0, 18.0, [98], [1], [1])


# ---- the handler ----------------------------------------------------------------------------------------------------

CONFIG = {"transfer_library": {"fragment_types": ["b", "y"], "max_charge": 2}}


def _handler(config=CONFIG):
    reporter = SimpleNamespace(log_string=lambda *a, **k: None)
    return trq.HipTransferLibraryRequantificationHandler(config, None, None, None, None, reporter, G.aa_mass_table(),
                                                         G.MOD_MASS, G.MASS_PROTON, G.MASS_H2O, device=0)


def _psm(frame):
    n = len(frame)
    out = pd.DataFrame({c: np.arange(n, dtype=np.int64) for c in trq.REQUIRED_CANDIDATE_COLUMNS})
    for c in trq.OPTIONAL_CANDIDATE_COLUMNS:
        out[c] = frame[c].to_numpy() if c in frame.columns else np.zeros(n, dtype=np.float32)
    out["extra"] = 1.0
    return out


def test_handler_error_paths():
    psm = _psm(G.draw_precursors(12, seed=5, lengths=(7, 9, 12)))
    for drop in (["sequence"], ["mods", "charge"], ["mod_sites"]):
        with pytest.raises(KeyError) as e:
            _handler().requantify(None, psm.drop(columns=drop))
        assert all(c in str(e.value) for c in drop)
        assert not any(c in str(e.value) for c in set(trq.SEQUENCE_COLUMNS) - set(drop))
    bad = psm.copy()
    bad.loc[3, "mods"], bad.loc[3, "mod_sites"] = "Unobtainium@X", "2"
    with pytest.raises(KeyError, match="Unobtainium@X"):
        _handler().requantify(None, bad)
    with pytest.raises(KeyError, match="qval"):  # a column of the reference's list: pandas names it
        _handler().requantify(None, psm.drop(columns=["qval"]))
    with pytest.raises(ValueError, match="not supported"):
        _handler({"transfer_library": {"fragment_types": ["b", "z"], "max_charge": 2}}).requantify(None, psm)
    with pytest.raises(ValueError, match="128"):
        trq.HipTransferLibraryRequantificationHandler(CONFIG, None, None, None, None, None, np.zeros(26), {}, 1.0, 18.0)


def test_candidate_frame_and_tables():
    frame = G.draw_precursors(12, seed=5, lengths=(7, 9, 12))
    psm = _psm(frame)
    cand, tables, series = _handler().build_candidate_library(psm)
    assert list(cand.columns) == trq.REQUIRED_CANDIDATE_COLUMNS + trq.OPTIONAL_CANDIDATE_COLUMNS + ["nAA"]
    assert cand["nAA"].tolist() == [len(s) for s in frame["sequence"]]
    assert "nAA" not in psm.columns  # a copy: the caller's frame is left alone
    assert series[0] == ["b_z1", "b_z2", "y_z1", "y_z2"]
    assert tables.struct.n == 12 and tables.struct.n_series == 4
    assert trq.OPTIONAL_CANDIDATE_COLUMNS[:4] == ["proba", "score", "qval", "channel"] and len(trq.OPTIONAL_CANDIDATE_COLUMNS) == 17


def _reference_start_stop(psm_df, frag_df):
    """fragcomp/utils.py:38-45 as the reference writes it."""
    frag_df["frag_idx"] = np.arange(len(frag_df))
    index_df = frag_df.groupby("_candidate_idx", as_index=False).agg(
        _frag_start_idx=pd.NamedAgg("frag_idx", "min"), _frag_stop_idx=pd.NamedAgg("frag_idx", "max"))
    index_df["_frag_stop_idx"] += 1
    return psm_df.merge(index_df, "inner", on="_candidate_idx")


@pytest.mark.parametrize("grouped", [True, False])
def test_fragment_ranges_equal_the_reference(grouped):
    rng = np.random.default_rng(6)
    n = 50
    psm = pd.DataFrame({"precursor_idx": rng.permutation(200)[:n].astype(np.uint32), "rank": rng.integers(0, 3, n).astype(np.uint8),
                        "proba": rng.random(n).astype(np.float32), "sequence": np.full(n, "PEPTIDEK", dtype=object)},
                       index=np.arange(100, 100 + n))
    counts = rng.integers(0, 6, n)
    counts[[0, 17, n - 1]] = 0  # candidates that got no fragments
    owner = np.repeat(np.arange(n), counts)
    if not grouped:
        owner = rng.permutation(owner)
    frag = pd.DataFrame({"precursor_idx": psm["precursor_idx"].to_numpy()[owner], "rank": psm["rank"].to_numpy()[owner],
                         "mz": rng.random(len(owner)).astype(np.float32)})
    want_psm, want_frag = psm.copy(), frag.copy()
    want_psm["_candidate_idx"] = candidate_hash(want_psm["precursor_idx"].to_numpy(), want_psm["rank"].to_numpy())
    want_frag["_candidate_idx"] = candidate_hash(want_frag["precursor_idx"].to_numpy(), want_frag["rank"].to_numpy())
    want_psm = _reference_start_stop(want_psm, want_frag)
    got_psm, got_frag = trq.index_fragments(psm.copy(), frag.copy())
    assert len(got_psm) == n - (counts == 0).sum()
    pd.testing.assert_frame_equal(got_psm, want_psm, check_exact=True)
    pd.testing.assert_frame_equal(got_frag, want_frag, check_exact=True)
    # the key is the reference's: rank << 32 | precursor_idx as uint64
    want_key = (psm["precursor_idx"].to_numpy().astype(np.int64) + (psm["rank"].to_numpy().astype(np.int64) << 32)).astype(np.uint64)
    assert np.array_equal(candidate_hash(psm["precursor_idx"].to_numpy(), psm["rank"].to_numpy()), want_key)
    # frames that carry the columns already are left as they are
    again = trq.add_frag_start_stop_idx(got_psm, got_frag)
    assert again is got_psm
    # no fragments at all: every candidate leaves
    empty_psm, _ = trq.index_fragments(psm.copy(), frag.iloc[:0].copy())
    assert len(empty_psm) == 0 and {"_frag_start_idx", "_frag_stop_idx"} <= set(empty_psm.columns)
