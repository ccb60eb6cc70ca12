"""What candidate selection refuses from its inputs, on both run layouts: one bad row in an otherwise good precursor
table, and - on ion-mobility runs - a smoothing kernel the kernels cannot take.  Every refusal is decided before the
kernel that would read the offending data is launched (the slice and charge checks are the limits / plan kernel's,
which reads the precursor columns only; the kernel's shape is checked on the host), and the handle must select as
before afterwards: the table of the good inputs equals the oracle's before and after.  The Python wrapper passes
all of these on to the C call."""
import numpy as np
import pytest

import selection_limits as SL
import synthetic as syn
import test_selection as TS
from alphadia_amd.runtime import HipBackendError
from alphadia_amd.selection import gaussian_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


@pytest.fixture(scope="module")
def raw_case():
    case = syn.make_case(100, 61, config_id=143, **SL.RAW_RUN)
    cfg = SL.config(rt_tolerance=20.0, candidate_count=5, min_size_rt=2)
    return case, cfg, gaussian_kernel(case.dia, cfg.peak_len_rt, cfg.sigma_scale_rt, cfg.kernel_size)


@pytest.fixture(scope="module")
def im_case():
    case = SL.window_count_case()
    cfg = SL.config(candidate_count=3, top_k_precursors=4, exclude_shared_ions=True, **SL.IM_CFG)
    return case, cfg, SL.im_kernel(case.dia, cfg)


def _good(ctx, oracle_lib, layout, case, cfg, kern):
    pdf = case.library.precursor_df.sort_values("precursor_idx").reset_index(drop=True)
    fdf = case.library.fragment_df
    pm = TS._pack(pdf)
    cols = SL.staged(ctx, case.dia, fdf)
    select = oracle_lib.select if layout == "raw" else oracle_lib.select_timstof
    exp = select(case.dia, cols, pm, cfg, kern, n_threads=4)
    assert (exp["score"] > 0).sum() > 30
    SL.assert_tables_equal(ctx.select_candidates(pm, cfg, kern), exp, layout)
    return pdf, fdf, pm, exp


@pytest.mark.parametrize("layout", ["raw", "im"])
def test_one_bad_precursor_row_is_refused(ctx, oracle_lib, raw_case, im_case, layout):
    """A fragment slice that ends one past the staged library, one that ends before it starts, and a precursor of
    charge 0 - each in one row of a good table - are refused with their own words."""
    case, cfg, kern = raw_case if layout == "raw" else im_case
    pdf, fdf, pm, exp = _good(ctx, oracle_lib, layout, case, cfg, kern)
    i = len(pdf) // 2
    start, stop = pdf.flat_frag_start_idx.values.astype(np.int64), pdf.flat_frag_stop_idx.values.astype(np.int64)
    assert stop.max() <= len(fdf) and (pdf.charge.values > 0).all() and stop[i] > start[i] > 0
    for column, value, words in (("flat_frag_stop_idx", len(fdf) + 1, "fragment slice outside the staged library"),
                                 ("flat_frag_stop_idx", start[i] - 1, "fragment slice outside the staged library"),
                                 ("charge", 0, "precursor charge must be > 0")):
        bad = pdf.copy()
        values = bad[column].values.copy()
        values[i] = value
        bad[column] = values
        with pytest.raises(HipBackendError, match=words):
            ctx.select_candidates(TS._pack(bad), cfg, kern)
    SL.assert_tables_equal(ctx.select_candidates(pm, cfg, kern), exp, layout + ", after the refusals")


def test_im_smoothing_kernel_that_is_no_outer_product_is_refused(ctx, oracle_lib, im_case):
    """One entry of the Gaussian kernel off by 1 % (an entry beside the centre, large enough for 1 % of it to exceed
    the rounding allowance of 1e-5 of the centre), and a centre entry of 0."""
    case, cfg, kern = im_case
    _, _, pm, exp = _good(ctx, oracle_lib, "im", case, cfg, kern)
    a0, b0 = kern.shape[0] // 2, kern.shape[1] // 2
    assert kern.dtype == np.float32 and kern[a0, b0] > 0 and 0.01 * kern[a0 + 1, b0 + 1] > 1e-4 * kern[a0, b0]
    bent = kern.copy()
    bent[a0 + 1, b0 + 1] *= np.float32(1.01)
    with pytest.raises(HipBackendError, match=r"smoothing kernel is not separable \(not an outer product\)"):
        ctx.select_candidates(pm, cfg, bent)
    hollow = kern.copy()
    hollow[a0, b0] = 0.0
    with pytest.raises(HipBackendError, match="smoothing kernel without a positive centre"):
        ctx.select_candidates(pm, cfg, hollow)
    SL.assert_tables_equal(ctx.select_candidates(pm, cfg, kern), exp, "after the refusals")
