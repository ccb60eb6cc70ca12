// adh_log_f32.h - table-driven float64 log of a float32 argument (candidate selection: one log per smoothed cell)
#pragma once
#include "adh_log_table.h"

// log of a finite float32 x >= 1 in float64: x = 2^e * m, the top 7 mantissa bits pick c = 1 + i / 128, and
// log(m) = -log(1 / c) + log1p(m / c - 1) with |m / c - 1| < 2^-7 and a degree-9 series.  All terms are
// >= 0 (no cancellation) and entry 0 is exact, so values next to 1 keep their relative accuracy.  The
// smoothing needs one log per non-zero output cell, 127 000 per precursor: this is about half the
// instructions of the general routine.
// Error: at most 2 ulp of float64 (the class of the library log), derived.  The result is
// fl(e ln2_hi + fl(fl(T + p) + fl(e ln2_lo))) with e ln2_hi exact (ln2_hi has 32 bits); the table entry T, T + p
// and the last sum are each within half an ulp of themselves, T and T + p lie below the result for e >= 1, and
// what is left - the series' remainder, the roundings of r, of p and of e ln2_lo, all far below the result - is
// under 2^-4 ulp there: 1.5 ulp + 2^-4.  At e = 0 nothing is added to T + p; the rounding of r counts against a
// smaller result, but T or r lies a binade below it: under 1.1 ulp.
// Measured on an MI355X against an 80-bit log (tests/test_log_f32_gpu.py): 1.023 ulp over all 2^23 mantissas of
// e = 0 (at 0x3F93F8E9), 1.202 ulp over every 128th mantissa and the table edges of e = 1 ... 127 (at 0x40DAB000,
// e = 2; under 0.6 ulp from e = 11 on), and (float) of the result equal to (float) of the 80-bit log on every one
// of them.  Over all 2^30 arguments it stays within 1 ulp of the device library's log, and no float32 rounding
// differs: what the selection depends on is that (float)adh_log_f32(x) == (float)log((double)x).
// (`tab`: the table as 256 doubles - adh_log_tab itself, or a copy of it in LDS: a table look-up per log is a global load
// in the middle of a dependent chain, and the smoothing kernel of the ion-mobility selection takes one log per cell)
__device__ __forceinline__ double adh_log_f32(float x, const double *tab = &adh_log_tab[0][0]) {
    const uint32_t bits = __float_as_uint(x);
    const int e = (int)(bits >> 23) - 127;
    const uint32_t mant = bits & 0x007FFFFFu;
    const int i = (int)(mant >> 16);
    const double m = (double)__uint_as_float(mant | 0x3F800000u);
    const double t_inv = tab[2 * i], t_log = tab[2 * i + 1];
    const double r = fma(m, t_inv, -1.0);
    double q = 1.0 / 9.0;
    q = fma(q, r, -1.0 / 8.0);
    q = fma(q, r, 1.0 / 7.0);
    q = fma(q, r, -1.0 / 6.0);
    q = fma(q, r, 1.0 / 5.0);
    q = fma(q, r, -1.0 / 4.0);
    q = fma(q, r, 1.0 / 3.0);
    q = fma(q, r, -1.0 / 2.0);
    const double p = fma(r * r, q, r);
    const double ed = (double)e;
    return ed * 6.93147180369123816490e-01 + ((t_log + p) + ed * 1.90821492927058770002e-10);
}

// float32-rounded log of an argument outside [1, inf) (a smoothed value that is negative, NaN or overflowed: only a
// caller's kernel with negative factors gets here).  Out of line on purpose: the library routine is ~200
// instructions and a dozen live float64 constants, which inlined into every log site of the smoothing kernel
// cost its hot paths their registers.
__device__ __attribute__((noinline)) float adh_log_f32_rare(float x) { return (float)log((double)x); }
