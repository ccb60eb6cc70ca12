// adh_select_rules.h - what candidate selection's host code (adh_select_host.hip) decides: which smoothing kernels
// and cycles it takes, how much scratch a call gets and where the batches are cut.  Plain functions without a HIP
// call or a handle (tools/probes/select_rules_probe.hip holds them without a GPU); a refusal carries the ABI's code.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/alphadia_hip.h"

namespace selrules {

struct Refusal {
    int code;         // ADH_OK: none
    const char *msg;
};
constexpr Refusal kFine{ADH_OK, nullptr};

// Rank-1 factors of the (k0, k1) smoothing kernel of an ion-mobility run: kernel[a][b] = ku[a] * kv[b] up to the
// float32 rounding of its entries, ku = 1 at the centre row.  Rows and columns are smoothed in turn: no other kernel.
inline Refusal rank1_factors(const float *kernel, int k0, int k1, std::vector<double> &ku, std::vector<double> &kv) {
    ku.assign((size_t)k0, 0.0);
    kv.assign((size_t)k1, 0.0);
    const int a0 = k0 / 2, b0 = k1 / 2;
    const double c = (double)kernel[a0 * k1 + b0];
    if (!(c > 0)) return Refusal{ADH_ERR_UNSUPPORTED, "smoothing kernel without a positive centre"};
    for (int a = 0; a < k0; ++a) ku[(size_t)a] = (double)kernel[a * k1 + b0] / c;
    for (int b = 0; b < k1; ++b) kv[(size_t)b] = (double)kernel[a0 * k1 + b];
    for (int a = 0; a < k0; ++a)
        for (int b = 0; b < k1; ++b)
            if (fabs(ku[(size_t)a] * kv[(size_t)b] - (double)kernel[a * k1 + b]) > 1e-5 * c + 1e-30)
                return Refusal{ADH_ERR_UNSUPPORTED, "smoothing kernel is not separable (not an outer product)"};
    return kFine;
}

// The non-zero columns of a two-row smoothing kernel as float64 scalar operands of the AlphaRaw kernel (Taps is
// sel::Taps).  cols = 0: another row count, or more columns than the table holds - the taps are read from LDS.
template <typename Taps>
Taps two_row_taps(const float *kernel, int k_rows, int k_cols) {
    constexpr int kCols = (int)(sizeof(Taps{}.v) / sizeof(double) / 2);
    Taps taps{};
    if (k_rows != 2) return taps;
    int lo = k_cols, hi = -1;
    for (int b = 0; b < k_cols; ++b)
        if (kernel[b] != 0.0f || kernel[k_cols + b] != 0.0f) lo = std::min(lo, b), hi = std::max(hi, b);
    if (hi < lo) lo = hi = 0;
    const int nb = hi - lo + 1;
    taps.cols = nb <= kCols ? kCols : 0;
    taps.col0 = lo;
    for (int a = 0; a < 2 && taps.cols; ++a)
        for (int b = 0; b < nb; ++b) taps.v[a * taps.cols + b] = (double)kernel[a * k_cols + lo + b];
    return taps;
}

// The AlphaRaw kernel keeps max_rows (sel::MAX_ROWS = 16) cycle rows per group (rows overlapping the isotope range,
// MS1 rows) and the reference sums every row: a cycle with more is refused before anything is launched, as scoring
// refuses more than ADH_MAX_OBS observations.  `cycle`: (lower, upper) m/z of the L rows.  Rows overlapping [a, b] =
// #(lower <= b) - #(upper < a) for rows with lower <= upper (an MS1 row (-1, -1) counts in both terms): two searches
// per precursor.
inline Refusal cycle_rows_refusal(const double *cycle, int L, int64_t n_ms1_obs, const float *mz, const uint8_t *charge,
                                  int64_t n, int n_iso, int max_rows) {
    if (n_ms1_obs > max_rows) return Refusal{ADH_ERR_UNSUPPORTED, "candidate selection: more than 16 cycle rows are MS1 rows"};
    std::vector<double> lower((size_t)L), upper((size_t)L);
    for (int row = 0; row < L; ++row) {
        lower[(size_t)row] = cycle[2 * (size_t)row];
        upper[(size_t)row] = cycle[2 * (size_t)row + 1];
        if (!(lower[(size_t)row] <= upper[(size_t)row])) return Refusal{ADH_ERR_INVALID_ARGUMENT, "cycle row with lower > upper m/z"};
    }
    std::sort(lower.begin(), lower.end());
    std::sort(upper.begin(), upper.end());
    // a bound first, from the cycle alone: no range as wide as the widest isotope range (charge 1) overlaps more
    // rows than the best one that starts at a row's upper edge.  Only a cycle that fails it is walked per precursor.
    const double widest = (double)std::max(n_iso - 1, 0) * 1.0033548350700006 + 0.01;
    int64_t bound = 0;
    for (int row = 0; row < L && L > max_rows; ++row) {
        const double a = upper[(size_t)row];
        bound = std::max<int64_t>(bound, (std::upper_bound(lower.begin(), lower.end(), a + widest) - lower.begin()) -
                                             (std::lower_bound(upper.begin(), upper.end(), a) - upper.begin()));
    }
    for (int64_t i = 0; i < n && n_iso > 0 && bound > max_rows; ++i) {
        if (charge[i] == 0) continue;  // (refused by the limits kernel)
        // the isotope range exactly as adh_select_kernel computes it (assemble_isotope_mz)
        const double a = (double)mz[i];
        const double b = (double)(float)((double)mz[i] + (double)(n_iso - 1) * 1.0033548350700006 / (double)charge[i]);
        const int64_t hit = (std::upper_bound(lower.begin(), lower.end(), b) - lower.begin()) -
                            (std::lower_bound(upper.begin(), upper.end(), a) - upper.begin());
        if (hit > max_rows)
            return Refusal{ADH_ERR_UNSUPPORTED, "candidate selection: a precursor's isotope range overlaps more than 16 cycle rows"};
    }
    return kFine;
}

// Scratch bytes one batch of an ion-mobility selection may take.  `all`: the blocks of every precursor, `biggest`:
// the largest of them, `held`: the scratch slab at hand, `by_hand`: ADH_SELECT_SCRATCH_MB in bytes, or NULL.  8 GiB
// unless set by hand, never more than the call needs, never less than one precursor needs.  A bigger slab at hand is
// used (fewer batches) - unless the budget was set by hand, which is how the tests reach the cutting of batches.
inline uint64_t selection_budget(uint64_t all, uint64_t biggest, uint64_t held, const uint64_t *by_hand) {
    uint64_t budget = by_hand ? *by_hand : (uint64_t)8 << 30;
    budget = std::max(std::min(budget, all), biggest);
    if (!by_hand) budget = std::max(budget, held);
    return budget;
}

// first = the first precursor of every batch, then n: a batch is the longest run of precursors whose blocks fit the
// budget together (cum: inclusive sums of their sizes).  selection_budget never goes below a block: the refusal guards.
inline Refusal cut_batches(const unsigned long long *cum, int64_t n, uint64_t budget, std::vector<int64_t> &first) {
    first.assign(1, 0);
    while (first.back() < n) {
        const int64_t f0 = first.back();
        const unsigned long long base = f0 > 0 ? cum[f0 - 1] : 0ull;
        const int64_t last = std::upper_bound(cum + f0, cum + n, base + budget) - cum;
        if (last == f0) return Refusal{ADH_ERR_UNSUPPORTED, "one precursor's tiles exceed the selection scratch budget"};
        first.push_back(last);
    }
    return kFine;
}

}  // namespace selrules
