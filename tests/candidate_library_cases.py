"""Inputs shared by tests/test_candidate_library.py and tests/test_candidate_library_gpu.py: the mass tables (written
here, alphabase is not imported), drawn precursors and the records packed from the NumPy restatement."""

from __future__ import annotations

import numpy as np
import pandas as pd

from alphadia_amd import _abi
from alphadia_amd import transfer_requantification as trq

# monoisotopic residue masses (Da)
RESIDUE_MASS = {
    "G": 57.02146372, "A": 71.03711379, "S": 87.03202841, "P": 97.05276385, "V": 99.06841391, "T": 101.04767847,
    "C": 103.00918496, "L": 113.08406398, "I": 113.08406398, "N": 114.04292744, "D": 115.02694303, "Q": 128.05857751,
    "K": 128.09496302, "E": 129.04259309, "M": 131.04048509, "H": 137.05891186, "F": 147.06841391, "R": 156.10111103,
    "Y": 163.06332853, "W": 186.07931295,
}
MASS_PROTON = 1.00727646688
MASS_H2O = 18.0105647
MOD_MASS = {"Carbamidomethyl@C": 57.021464, "Oxidation@M": 15.994915, "Acetyl@Protein_N-term": 42.010565,
            "Phospho@S": 79.966331, "Amidated@Any_C-term": -0.984016}
LETTERS = np.array(sorted(RESIDUE_MASS))
LENGTHS = (2, 3, 7, 31, 32, 33, 63, 64, 65, 128, 255)  # one row; either side of 32 and of 64 lanes; the uint8 edge


def aa_mass_table() -> np.ndarray:
    """128 float64: the mass of every ASCII code, 1e8 for the codes that are no residue."""
    table = np.full(128, 1e8, dtype=np.float64)
    for letter, mass in RESIDUE_MASS.items():
        table[ord(letter)] = mass
    return table


def draw_precursors(n: int, seed: int, lengths=LENGTHS) -> pd.DataFrame:
    """``sequence``, ``mods``, ``mod_sites``, ``charge`` of n precursors: lengths from ``lengths`` (every one of them
    occurs, the first and the last precursor have the shortest and the longest), charges 1-4, and in turn no
    modification, an N-terminal one (site 0), a C-terminal one (site -1), two on one residue, one of each."""
    rng = np.random.default_rng(seed)
    L = rng.choice(np.array(lengths), n)
    L[: len(lengths)] = lengths
    L[0], L[-1] = min(lengths), max(lengths)
    sequence = np.array(["".join(rng.choice(LETTERS, int(k))) for k in L], dtype=object)
    mods, sites = np.full(n, "", dtype=object), np.full(n, "", dtype=object)
    for p in range(n):
        kind = p % 5
        inner = int(rng.integers(1, L[p] + 1))
        if kind == 1:
            mods[p], sites[p] = "Acetyl@Protein_N-term", "0"
        elif kind == 2:
            mods[p], sites[p] = "Amidated@Any_C-term", "-1"
        elif kind == 3:
            mods[p], sites[p] = "Oxidation@M;Phospho@S", f"{inner};{inner}"
        elif kind == 4:
            mods[p], sites[p] = "Acetyl@Protein_N-term;Carbamidomethyl@C;Amidated@Any_C-term", f"0;{inner};-1"
    return pd.DataFrame({"sequence": sequence, "mods": mods, "mod_sites": sites,
                         "charge": rng.integers(1, 5, n).astype(np.uint8)})


def tables_of(frame: pd.DataFrame, fragment_types=("b", "y"), max_charge: int = 2):
    """``(arrays, series, host_args)``: the arrays of the precursors, the charged series and the positional arguments
    of ``host_candidate_library`` / ``_abi.pack_candidate_library``."""
    arrays = trq.candidate_library_tables(frame["sequence"].to_numpy(), frame["mods"].to_numpy(),
                                          frame["mod_sites"].to_numpy(), MOD_MASS)
    series = trq.charged_series(list(fragment_types), max_charge)
    args = (arrays["seq_offset"], arrays["residues"], arrays["mod_offset"], arrays["mod_site"], arrays["mod_mass"],
            aa_mass_table(), MASS_PROTON, MASS_H2O, *series[1:])
    return arrays, series, args


def records_of(columns: dict, mz=None) -> np.ndarray:
    """The 32-byte records of eight columns, ``mz`` (default: ``mz_library``) in the m/z field, every pad byte zero."""
    out = np.zeros(len(columns["mz_library"]), dtype=_abi.LIB_RECORD_DTYPE)
    for name in ("mz_library", "intensity", "type", "loss_type", "charge", "number", "position", "cardinality"):
        out[name] = columns[name]
    out["mz"] = columns["mz_library"] if mz is None else mz
    return out
