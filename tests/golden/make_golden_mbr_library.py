"""Golden vectors of the match-between-runs library, produced by RUNNING THE REFERENCE's ``MbrLibraryBuilder.forward``
and ``IndexBuilder`` (alphadia/libtransform/mbr.py) in the build container:

    python tests/golden/make_golden_mbr_library.py

TEST INFRASTRUCTURE, same rules as make_golden_transfer_library.py: the reference is imported from /root/reference
with stubs for the third-party modules that are not installed here (numba through ref_shim, alphabase), fed seeded
synthetic tables (tests/mbr_library_golden.py: ``cohort``), and inputs + outputs are stored in
``tests/golden/mbr_library.npz``.

alphabase's ``SpecLibBase`` is not installed.  ``DuckLibrary`` below stands in for it; its ``copy`` and
``remove_unused_fragments`` are written here, not taken from alphabase: ``remove_unused_fragments`` keeps the blocks of
the remaining precursors in the order of their old start, one block per precursor, renumbers them by a running sum of
their lengths, leaves the precursor frame's row order and index alone and gives the dense frames a fresh index.  For
the ``keep_decoys`` case ``DecoyGenerator`` and ``hash_precursor_df`` of the reference module are replaced by
``standin_decoy_generator`` and ``standin_rehash`` of tests/mbr_library_golden.py.

The FDR filter, the two group-bys (median, first), ``isin``, the two ``reindex`` lookups and the assignment are the
reference's own code, run by pandas.  Pinned to the stand-ins only: what happens to the dense rows of dropped
precursors, the index of the result, and everything about decoys.

Per case ``<c>``: ``<c>/meta`` (JSON: kind, parameters, ``raises``: the exception type's name or null).
kind "forward": ``psm``, ``library/precursor``, ``library/<dense>``, ``out/precursor``, ``out/<dense>`` as frames (a
column per entry, ``__columns__``, ``__index__``, ``<col>__null`` for object columns).
kind "index": the four key arrays, ``fallback`` / ``mask`` / ``specific`` (the reference's private indices), two
value arrays and ``applied``.
"""

from __future__ import annotations

import copy
import json
import os
import sys
import types
import zipfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

ref_shim.install()

import mbr_library_golden as G  # noqa: E402


def _stub(name: str, **attrs) -> types.ModuleType:
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, mod)
    return mod


_stub("alphabase")
_stub("alphabase.spectral_library")
_stub("alphabase.spectral_library.base", SpecLibBase=object, hash_precursor_df=None)
_stub("alphabase.spectral_library.decoy", decoy_lib_provider=None)

from alphadia.libtransform import mbr as REF  # noqa: E402


class DuckLibrary(G.Library):
    """Stands in for alphabase's SpecLibBase (see the module docstring)."""

    def copy(self):
        return copy.deepcopy(self)

    def remove_unused_fragments(self):
        df = self._precursor_df
        start, stop = df["frag_start_idx"].to_numpy().copy(), df["frag_stop_idx"].to_numpy().copy()
        rows, cursor = [], 0
        new_start, new_stop = start.copy(), stop.copy()
        for i in np.argsort(start, kind="stable"):
            rows.extend(range(int(start[i]), int(stop[i])))
            new_start[i], new_stop[i] = cursor, cursor + (stop[i] - start[i])
            cursor = int(new_stop[i])
        df["frag_start_idx"], df["frag_stop_idx"] = new_start, new_stop
        take = np.asarray(rows, dtype=np.int64)
        for name in self._dense:
            setattr(self, name, getattr(self, name).iloc[take].reset_index(drop=True))


class _StandInDecoys:
    def __init__(self, decoy_type="diann"):
        assert decoy_type == "diann"

    def __call__(self, lib):
        return G.standin_decoy_generator(lib)


REF.DecoyGenerator = _StandInDecoys
REF.hash_precursor_df = G.standin_rehash


def save_archive(path: str, arrays: dict) -> None:
    """``np.savez_compressed`` with a fixed time stamp on every member: the file is the same bytes on every run."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


def put_meta(out, case: str, **meta):
    out[f"{case}/meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)


def case_forward(out, case, seed, sizes, n_groups, fdr=0.01, keep_decoys=False, fail_fraction=0.1, **kw):
    rng = np.random.default_rng(seed)
    rows = np.concatenate([sizes, rng.integers(0, 21, n_groups - len(sizes))]).astype(np.int64)
    psm, lib = G.cohort(rng, n_groups, rows, fail_fraction=fail_fraction, exact_groups=range(4, len(sizes)), **kw)
    base = DuckLibrary(lib._precursor_df, {n: getattr(lib, n) for n in lib.available_dense_fragment_dfs()})
    G.put_frame(out, f"{case}/psm", psm)
    G.put_library(out, f"{case}/library", base)
    before = base._precursor_df.copy()
    raises = None
    try:
        got = REF.MbrLibraryBuilder(fdr=fdr, keep_decoys=keep_decoys)(psm, base)
        G.put_library(out, f"{case}/out", got)
    except Exception as e:  # noqa: BLE001  (the type is the golden)
        raises = type(e).__name__
    assert before.equals(base._precursor_df)
    passed = psm[psm["qval"] <= fdr]
    counts = sorted(set(passed.groupby("elution_group_idx").size().tolist()))
    put_meta(out, case, kind="forward", fdr=fdr, keep_decoys=keep_decoys, dense=list(G.DENSE), raises=raises,
             n_psm=len(psm), n_passed=len(passed), group_sizes=counts,
             n_out=None if raises else len(got._precursor_df))
    return raises or len(got._precursor_df)


def case_index(out, case, target_keys, target_fallback_keys, fallback_lookup_keys, specific_lookup_keys):
    for k, v in dict(target_keys=target_keys, target_fallback_keys=target_fallback_keys,
                     fallback_lookup_keys=fallback_lookup_keys, specific_lookup_keys=specific_lookup_keys).items():
        out[f"{case}/{k}"] = np.asarray(v)
    raises = None
    try:
        b = REF.IndexBuilder(target_keys, target_fallback_keys, fallback_lookup_keys, specific_lookup_keys)
        out[f"{case}/fallback"], out[f"{case}/mask"], out[f"{case}/specific"] = (b._fallback_indices, b._specific_index_mask,
                                                                                b._specific_indices)
        fv = np.arange(len(fallback_lookup_keys), dtype=np.float32) + np.float32(0.5)
        sv = -np.arange(len(specific_lookup_keys), dtype=np.float32) - np.float32(0.25)
        out[f"{case}/fallback_values"], out[f"{case}/specific_values"] = fv, sv
        out[f"{case}/applied"] = b.apply(fv, sv)
    except Exception as e:  # noqa: BLE001
        raises = type(e).__name__
    put_meta(out, case, kind="index", raises=raises)
    return raises


def main():
    out: dict[str, np.ndarray] = {}
    done = {}
    sizes = [3, 5, 4, 6, 1, 2, 3, 64, 65, 1100]  # (groups 1 to 3 are the planted ones of `cohort`)
    # more than one tile of the radix sort (its blocks take a few thousand keys), float32 RT, uint32 / int64 groups
    done["tiles_f32"] = case_forward(out, "tiles_f32", 41, sizes + [30] * 160, 400, rt_dtype=np.float32,
                                     group_dtype=np.uint32, library_group_dtype=np.int64)
    done["f64_signed"] = case_forward(out, "f64_signed", 42, sizes[:9], 60, rt_dtype=np.float64, group_dtype=np.int64,
                                      library_group_dtype=np.uint32, signed_hash=True, n_columns=3)
    done["keep_decoys"] = case_forward(out, "keep_decoys", 43, sizes[:7], 40, keep_decoys=True, rt_dtype=np.float32)
    done["none_pass"] = case_forward(out, "none_pass", 44, sizes[:7], 12, fdr=-1.0)
    rng = np.random.default_rng(45)
    look = G.hashes(rng.permutation(50), False)
    fb_keys = rng.permutation(20).astype(np.int64) * 3
    done["index_basic"] = case_index(out, "index_basic", G.hashes(rng.integers(0, 80, 200), False),
                                     fb_keys[rng.integers(0, 20, 200)], fb_keys, look)
    done["index_signed"] = case_index(out, "index_signed", G.hashes(rng.integers(0, 80, 70), True),
                                      fb_keys[rng.integers(0, 20, 70)].astype(np.uint32), fb_keys.astype(np.uint32),
                                      G.hashes(rng.permutation(50), True))
    done["index_empty_specific"] = case_index(out, "index_empty_specific", G.hashes(np.arange(30), False),
                                              fb_keys[rng.integers(0, 20, 30)], fb_keys, look[:0])
    done["index_duplicate"] = case_index(out, "index_duplicate", G.hashes(np.arange(30), False),
                                         fb_keys[rng.integers(0, 20, 30)], fb_keys, np.concatenate([look, look[:1]]))
    path = os.path.join(OUT_DIR, "mbr_library.npz")
    save_archive(path, out)
    print(path, done, f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
