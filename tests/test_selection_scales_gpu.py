"""Candidate selection end to end where the argument of its log is not small.

The smoothing kernel is the caller's, so a kernel scaled by a power of two scales every smoothed value exactly and
moves ``log(smooth + 1)`` (alphadia_amd/csrc/adh_log_f32.h) to exponents that the synthetic intensities of the other
selection tests (about 2e4) never reach: 2^12 and 2^33 bracket what Orbitrap intensities of 1e9 ... 1e10 give, 2^100
is the far end of the domain, and -2^-21 puts every ``smooth + 1`` into (0, 1], the out-of-line routine.  The
comparison is the one of test_selection's randomized tests: every column equal to the oracle's, which takes
``(float)std::log((double)(sm + 1.0f))``, the score to rtol 1e-6, no row left out.

What the scales must not do is asserted from the inputs and the oracle alone.  The largest cell of any tile comes
from the oracle's smoothing hook (it sees every tile before the convolution), so ``cell * sum|kernel| * |s|`` bounds
every smoothed value: below 2^127 nothing overflows, below 1 for the negative scale every log is finite and <= 0.
Scales that produce NaN or overflow are covered by test_log_f32_gpu's dispatch test only: nothing defines what
peak finding does on a NaN landscape.

An ion-mobility run smooths with the two factors of a kernel that has a positive centre; the product and the oracle
both refuse any other kernel, the negative scale among them, which is asserted instead.
"""

from __future__ import annotations

import numpy as np
import pytest

import synthetic as syn
import test_selection as TS
from alphadia_amd.scoring import fragment_columns
from alphadia_amd.selection import CANDIDATE_COLUMNS, CandidateSelectionConfig, gaussian_kernel

pytestmark = pytest.mark.gpu

SCALES = {"2^12": 2.0 ** 12, "2^33": 2.0 ** 33, "2^100": 2.0 ** 100, "-2^-21": -(2.0 ** -21)}
MIN_ROWS = 100  # rows with a candidate the oracle must return at every scale


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def _largest_cell(oracle_lib, select) -> float:
    """The largest cell of any tile the oracle smooths, recorded by its smoothing hook (the hook's answer, zeros,
    is thrown away with the call's result)."""
    seen = [0.0]

    def smooth_log(tile):
        seen[0] = max(seen[0], float(tile.max()))
        assert tile.min() >= 0
        return np.zeros_like(tile)

    oracle_lib.set_selection_hooks(smooth_log=smooth_log)
    try:
        select()
    finally:
        oracle_lib.set_selection_hooks()
    return seen[0]


def _scaled(kern: np.ndarray, s: float) -> np.ndarray:
    scaled = kern * np.float32(s)
    assert scaled.dtype == np.float32 and np.isfinite(scaled).all()
    # the scaling is exact wherever the product is a normal number
    normal = np.abs(scaled) >= np.finfo(np.float32).tiny
    assert np.array_equal(scaled[normal].astype(np.float64), kern[normal].astype(np.float64) * s)
    return scaled


def _assert_scale_is_in_range(cell: float, intensity_max: float, factors, s: float) -> None:
    """``factors``: the kernels whose absolute sums bound a smoothing pass (the whole kernel; for the separable form
    also the factor of the first pass, whose result is rounded to float32 as well)."""
    assert cell > 0 and intensity_max > 0
    for k in factors:
        reach = np.abs(k.astype(np.float64)).sum() * abs(s)
        assert intensity_max * reach < 2.0 ** 127 and cell * reach < 2.0 ** 127
        if s < 0:
            assert intensity_max * reach < 1.0 and cell * reach < 1.0


def _assert_equal(got, exp) -> None:
    for c in CANDIDATE_COLUMNS:
        if c == "score":
            assert np.allclose(got[c], exp[c], rtol=1e-6, atol=0), c
        else:
            assert np.array_equal(got[c], exp[c]), c


# ---------------------------------------------------------------- the generic path
@pytest.fixture(scope="module")
def generic(oracle_lib):
    case = syn.make_case(
        200, 100, config_id=761, per_precursor=1, n_ms2=8, ms1_peaks=500, ms2_peaks=220, mz_lo=400.0, mz_hi=480.0,
        frag_mz_lo=200, frag_mz_hi=450, ms1_mz_range=(395, 510), ms2_mz_range=(195, 470), few_fragment_fraction=0.0,
        planted_fraction=0.7, threads=1,
    )
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=45.0, candidate_count=3, top_k_precursors=3, precursor_mz_tolerance=15,
                    fragment_mz_tolerance=15, sigma_scale_rt=0.5))
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)
    pm = TS._pack(case.library.precursor_df)
    cell = _largest_cell(oracle_lib, lambda: oracle_lib.select(case.dia, cols, pm, cfg, kern, n_threads=1))
    return case, cfg, cols, kern, pm, cell


@pytest.mark.parametrize("scale", list(SCALES))
def test_hip_selection_with_a_scaled_kernel(ctx, oracle_lib, monkeypatch, generic, scale):
    case, cfg, cols, kern, pm, cell = generic
    s = SCALES[scale]
    k = _scaled(kern, s)
    _assert_scale_is_in_range(cell, float(case.dia.intensity_values.max()), [kern], s)
    exp = oracle_lib.select(case.dia, cols, pm, cfg, k, n_threads=4)
    assert np.isfinite(exp["score"]).all()
    assert (exp["score"] != 0).sum() >= MIN_ROWS, int((exp["score"] != 0).sum())

    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    got = ctx.select_candidates(pm, cfg, k)
    got = {c: np.array(got[c], copy=True) for c in CANDIDATE_COLUMNS}
    _assert_equal(got, exp)
    # the taps as scalar operands (default) and in LDS: the same bits
    monkeypatch.setenv("ADH_DEBUG_SELECT_LDS_TAPS", "1")
    again = ctx.select_candidates(pm, cfg, k)
    for c in CANDIDATE_COLUMNS:
        assert np.array_equal(again[c], got[c]), c


# ---------------------------------------------------------------- the ion-mobility path
@pytest.fixture(scope="module")
def mobility(oracle_lib):
    case = syn.make_timstof_case(n_precursors=120, n_cycles=70, config_id=861, per_precursor=1, n_ms2_frames=4,
                                 windows_per_frame=2, scan_max_index=96, events_per_push=40.0, planted_fraction=0.7)
    case.dia.has_mobility = True
    cfg = CandidateSelectionConfig()
    cfg.update(dict(rt_tolerance=2.5, mobility_tolerance=0.3, candidate_count=3, top_k_precursors=3, min_size_rt=2,
                    min_size_mobility=4, max_size_mobility=20, peak_len_rt=1.5, sigma_scale_rt=0.5,
                    peak_len_mobility=0.06, kernel_size=20))
    kern = gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size, cfg.peak_len_mobility,
                           cfg.sigma_scale_mobility)
    cols = fragment_columns(case.library.fragment_df, "mz_library")
    pm = TS._pack(case.library.precursor_df)
    cell = _largest_cell(oracle_lib, lambda: oracle_lib.select_timstof(case.dia, cols, pm, cfg, kern, n_threads=1))
    return case, cfg, cols, kern, pm, cell


@pytest.mark.parametrize("scale", [name for name, s in SCALES.items() if s > 0])
def test_hip_timstof_selection_with_a_scaled_kernel(ctx, oracle_lib, mobility, scale):
    case, cfg, cols, kern, pm, cell = mobility
    s = SCALES[scale]
    k = _scaled(kern, s)
    # the first pass runs along the cycles with the kernel's centre row, and is rounded to float32 too
    _assert_scale_is_in_range(cell, float(case.dia.intensity_values.max()), [kern, kern[kern.shape[0] // 2]], s)
    exp = oracle_lib.select_timstof(case.dia, cols, pm, cfg, k, n_threads=4)
    assert np.isfinite(exp["score"]).all()
    assert (exp["score"] != 0).sum() >= MIN_ROWS, int((exp["score"] != 0).sum())

    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    got = ctx.select_candidates(pm, cfg, k)
    _assert_equal(got, exp)


def test_hip_timstof_selection_refuses_the_negative_scale_as_the_oracle_does(ctx, oracle_lib, mobility):
    """The separable smoothing of an ion-mobility run is defined for kernels with a positive centre: the negative
    scale has no end-to-end answer there, on either side."""
    from alphadia_amd import runtime

    case, cfg, cols, kern, pm, _ = mobility
    k = _scaled(kern, SCALES["-2^-21"])
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        oracle_lib.select_timstof(case.dia, cols, pm, cfg, k, n_threads=1)
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*cols, force=True)
    with pytest.raises(runtime.HipBackendError, match="positive centre"):
        ctx.select_candidates(pm, cfg, k)
