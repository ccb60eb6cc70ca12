"""Designed-edge runs for m/z window matching (pure NumPy): small runs whose peaks sit ON the float32 bounds of a
query's tolerance window, on the edges of the transposed run's m/z bins (float32 bits >> ADH_BIN_SHIFT), on powers of
two, on the run's smallest and largest m/z, and - for an ion-mobility run - on TOF bins and on the edges of the
``mz_lut`` buckets.  Every case states which designed peak belongs to which query (its *owner*); the builder then

* asserts every edge it claims (``peak == lo`` bit for bit, ``bits(lo) & 0x1FF == 0``, ``lo < 512 <= hi`` ...), so a
  case that drifts off its edge fails here instead of passing silently, and
* checks the stated owners against a predicate written from the reference's loop (AlphaRaw: first peak >= lo at or
  after the current one, consume while <= hi, never step back; ion mobility: the TOF bins
  ``[searchsorted_left(lo), searchsorted_left(hi))`` of every query on its own).

**Membership encoding.**  The designed peaks one query list can see in one spectrum carry distinct power-of-two
intensities (2^0 .. 2^23; uint16 runs: 2^0 .. 2^15), so a cell's float32 sum is exact in any order and decodes which
peaks were taken: ``expected`` is the intensity plane ``[K, F]`` (``[K, O, S, F]`` for the ion-mobility run).  The
intensity cases (E7) carry arbitrary intensities and ``expected is None``: they are compared with the reference's
output bit for bit only.

Bounds are computed as the reference's ``mass_range`` does under float32: ``t = tol * mz; q = t / 1e6; mz -+ q``.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

import synthetic as syn

F32 = np.float32
BIN_SHIFT = 9  # ADH_BIN_SHIFT (alphadia_amd/csrc/adh_device.h)
LOW = (1 << BIN_SHIFT) - 1
MS2_ROW = 3  # the window 420 .. 430 of make_cycle(8, 400, 480)
MS2_QUAD = (422.0, 425.0)
MS1_QUAD = (-1.0, -1.0)
INF = F32(np.inf)


class Case(NamedTuple):
    name: str
    frame_limits: np.ndarray  # uint64 (1, 3)
    mz_query: np.ndarray  # float32 [K]
    tol: np.float32
    quad: np.ndarray  # float64 (1, 2)
    expected: np.ndarray | None  # the intensity plane the designed peaks must give, None: no membership encoding
    family: str = ""
    labels: tuple = ()  # per designed peak of the case's group: what it sits on
    owners: tuple = ()  # per designed peak: tuple of the queries that take it (AlphaRaw: at most one)
    intensity: tuple = ()  # per designed peak
    scan_limits: np.ndarray | None = None  # ion-mobility cases only
    ascending: bool = True


# ------------------------------------------------------------------------------------------ float32 helpers
def bits(x) -> int:
    return int(np.asarray(x, dtype=F32).view(np.uint32))


def from_bits(b: int) -> np.float32:
    return np.uint32(b).view(F32)


def up(x, n: int = 1) -> np.float32:
    """n float32 patterns above a positive x (n = 1: np.nextafter(x, +inf))."""
    return from_bits(bits(x) + n)


def down(x, n: int = 1) -> np.float32:
    return from_bits(bits(x) - n)


def bin_of(x) -> int:
    return bits(x) >> BIN_SHIFT


def bounds(mz, tol):
    """mass_range of the reference, all float32."""
    mz = np.asarray(mz, dtype=F32)
    t = F32(tol) * mz
    q = t / F32(1e6)
    return (mz - q).astype(F32), (mz + q).astype(F32)


def find_query(start, tol, cond, span: int = 1 << 15) -> np.float32:
    """The first float32 at or above ``start`` (stepping like np.nextafter) whose bounds satisfy ``cond(m, lo, hi)``."""
    m = (np.uint32(bits(start)) + np.arange(span, dtype=np.uint32)).view(F32)
    assert np.nextafter(m[0], INF) == m[1]
    lo, hi = bounds(m, tol)
    ok = np.flatnonzero(cond(m, lo, hi))
    assert ok.size, f"no float32 within {span} patterns above {start} has the wanted bounds"
    return F32(m[ok[0]])


PRECURSOR_MZ, PRECURSOR_CHARGE = F32(425.37), 2  # inside the window of MS2_ROW with its whole isotope range +- 0.5
PRECURSOR_MZ_2OBS = F32(429.8)  # isotope range across the boundary at 430: the rows MS2_ROW and MS2_ROW + 1


def isotope_mz(mono_mz, charge, n):
    """The isotope m/z of a precursor as scoring computes them: float32(i * delta / charge) + float32 m/z."""
    return [F32(np.float64(i) * syn.ISOTOPE_DELTA / np.float64(charge)) + F32(mono_mz) for i in range(n)]


def take(spec_mz: np.ndarray, los, his) -> list:
    """The reference's AlphaRaw loop over one spectrum: per window the half-open range of peak positions it consumes.
    The first peak >= lo at or after the current position, then every peak <= hi; the position never goes back."""
    out, idx, n = [], 0, len(spec_mz)
    for lo, hi in zip(los, his):
        while idx < n and spec_mz[idx] < lo:
            idx += 1
        first = idx
        while idx < n and spec_mz[idx] <= hi:
            idx += 1
        out.append((first, idx))
    return out


# ------------------------------------------------------------------------------------------ AlphaRaw
class _Group:
    """Designed peaks that share a stretch of m/z (and the bits of the membership encoding)."""

    def __init__(self, name, peaks, intensity=None):
        self.name = name
        self.mz = np.array([p[0] for p in peaks], dtype=F32)
        self.labels = tuple(p[1] for p in peaks)
        assert len(peaks) <= 24, name
        self.encoded = intensity is None
        self.intensity = (np.array([2.0 ** i for i in range(len(peaks))], dtype=F32) if intensity is None
                          else np.asarray(intensity, dtype=F32))
        assert len(self.intensity) == len(self.mz)
        self.cases = []  # (family, name, queries, tol, owners, ascending)

    def case(self, family, name, queries, tol, owners, ascending=True):
        assert len(owners) == len(self.mz), name
        self.cases.append((family, name, np.asarray(queries, dtype=F32), F32(tol), tuple(owners), ascending))


def _e1(g, at, tol=15.0, family="E1", name="E1_bounds"):
    m = F32(at)
    lo, hi = bounds(m, tol)
    grp = _Group(name, [(down(lo), "one ulp below lo"), (lo, "on lo"), (up(lo), "one ulp above lo"),
                        (down(hi), "one ulp below hi"), (hi, "on hi"), (up(hi), "one ulp above hi")])
    assert grp.mz[1] == lo and grp.mz[4] == hi and np.nextafter(lo, -INF) == grp.mz[0] and np.nextafter(hi, INF) == grp.mz[5]
    grp.case(family, name, [m], tol, [-1, 0, 0, 0, 0, -1])
    g.append(grp)
    return grp


def _main_groups() -> list:
    g = []
    # ---- E5 (low end): the smallest m/z of the run is the lower bound of a query, bit for bit
    mA = F32(200.5)
    loA, hiA = bounds(mA, 15)
    low = _Group("E5_low", [(loA, "the run's smallest m/z"), (up(loA), "one ulp above the smallest m/z"), (hiA, "on hi of the query whose lo is the smallest m/z"),
                            (up(hiA), "one ulp above that hi")])
    low.case("E5", "E5_lo_is_mz_min", [mA], 15, [0, 0, 0, -1])
    loB, hiB = bounds(loA, 15)
    assert loB < loA <= hiB < hiA
    low.case("E5", "E5_mz_min_inside", [loA], 15, [0, 0, -1, -1])
    mC = find_query(loA * F32(1 - 16e-6), 15, lambda m, lo, hi: hi == loA)
    assert bounds(mC, 15)[1] == loA
    low.case("E5", "E5_hi_is_mz_min", [mC], 15, [0, -1, -1, -1])
    mD = F32(loA * F32(1 - 1e-4))
    assert bounds(mD, 15)[1] < loA
    low.case("E5", "E5_below_run", [mD], 15, [-1, -1, -1, -1])
    g.append(low)

    # ---- E1: the six patterns around the two bounds
    _e1(g, 231.1234)
    # ... and around the isotope windows of the precursor the scoring tests use (10 ppm, candidate.py:151-163)
    for i, mz in enumerate(isotope_mz(PRECURSOR_MZ, PRECURSOR_CHARGE, 4)):
        _e1(g, mz, tol=10.0, name=f"E1_isotope{i}")

    # ---- E2: windows that overlap
    m0 = F32(243.3)
    m1 = F32(m0 * F32(1 + 5e-6))
    (lo0, lo1), (hi0, hi1) = bounds([m0, m1], 15)
    assert lo0 < lo1 < hi0 < hi1
    grp = _Group("E2_pair", [(down(lo0), "one ulp below lo of window 0"), (lo1, "on lo of window 1, inside window 0"),
                             (hi0, "on hi of window 0, inside window 1"), (up(hi0), "one ulp above hi of window 0"),
                             (hi1, "on hi of window 1"), (up(hi1), "one ulp above hi of window 1")])
    grp.case("E2", "E2_overlap_pair", [m0, m1], 15, [-1, 0, 0, 1, 1, -1])
    g.append(grp)
    m = F32(247.7)
    lo, hi = bounds(m, 15)
    grp = _Group("E2_twin", [(lo, "on lo of both windows"), (m, "on the query of both windows"), (hi, "on hi of both windows")])
    grp.case("E2", "E2_identical_queries", [m, m], 15, [0, 0, 0])
    g.append(grp)
    q = np.array([251.9, 251.9 * (1 + 1e-4), 251.9 * (1 + 2e-4)], dtype=F32)
    lo, hi = bounds(q, 200)
    # window 2 reaches below the end of window 0: three windows deep.  (With ascending queries and one tolerance hi is
    # monotone, so the running maximum of the earlier upper bounds IS the previous window's: this case cannot tell the
    # two apart - only a list with a non-monotone hi could, and no caller builds one.)
    assert lo[2] < hi[0] < hi[1] < hi[2]
    grp = _Group("E2_triple", [(lo[2], "on lo of window 2, inside windows 0 and 1"), (hi[0], "on hi of window 0"),
                               (up(hi[0]), "one ulp above hi of window 0"), (hi[1], "on hi of window 1"),
                               (up(hi[1]), "one ulp above hi of window 1"), (hi[2], "on hi of window 2"), (up(hi[2]), "one ulp above hi of window 2")])
    grp.case("E2", "E2_three_deep", q, 200, [0, 0, 1, 1, 2, 2, -1])
    g.append(grp)
    q = np.array([266.0, 262.0, 270.0], dtype=F32)
    grp = _Group("E2_unsorted", [(q[1], "on query 1 (listed after a larger one)"), (q[0], "on query 0"), (q[2], "on query 2")])
    grp.case("E2", "E2_non_ascending", q, 15, [-1, 0, 2], ascending=False)
    g.append(grp)

    # ---- E3: bounds on the first / last pattern of a bin
    m = find_query(281.0, 15, lambda m, lo, hi: (lo.view(np.uint32) & LOW) == 0)
    lo, hi = bounds(m, 15)
    assert bits(lo) & LOW == 0 and bin_of(down(lo)) == bin_of(lo) - 1
    grp = _Group("E3_lo_first", [(down(lo), "last pattern of the bin below lo"), (lo, "on lo = first pattern of its bin"), (hi, "on hi"), (up(hi), "one ulp above hi")])
    grp.case("E3", "E3_lo_first_pattern", [m], 15, [-1, 0, 0, -1])
    g.append(grp)
    m = find_query(285.0, 15, lambda m, lo, hi: (lo.view(np.uint32) & LOW) == LOW)
    lo, hi = bounds(m, 15)
    assert bits(lo) & LOW == LOW and bin_of(up(lo)) == bin_of(lo) + 1
    grp = _Group("E3_lo_last", [(down(lo), "one ulp below lo"), (lo, "on lo = last pattern of its bin"), (up(lo), "first pattern of the bin above lo"), (up(hi), "one ulp above hi")])
    grp.case("E3", "E3_lo_last_pattern", [m], 15, [-1, 0, 0, -1])
    g.append(grp)
    m = find_query(289.0, 15, lambda m, lo, hi: (hi.view(np.uint32) & LOW) == 0)
    lo, hi = bounds(m, 15)
    assert bits(hi) & LOW == 0 and bin_of(down(hi)) == bin_of(hi) - 1
    grp = _Group("E3_hi_first", [(down(lo), "one ulp below lo"), (down(hi), "last pattern of the bin below hi"), (hi, "on hi = first pattern of its bin"), (up(hi), "one ulp above hi")])
    grp.case("E3", "E3_hi_first_pattern", [m], 15, [-1, 0, 0, -1])
    g.append(grp)
    m = find_query(293.0, 15, lambda m, lo, hi: (hi.view(np.uint32) & LOW) == LOW)
    lo, hi = bounds(m, 15)
    assert bits(hi) & LOW == LOW and bin_of(up(hi)) == bin_of(hi) + 1
    grp = _Group("E3_hi_last", [(lo, "on lo"), (down(hi), "one ulp below hi"), (hi, "on hi = last pattern of its bin"), (up(hi), "first pattern of the bin above hi")])
    grp.case("E3", "E3_hi_last_pattern", [m], 15, [0, 0, 0, -1])
    g.append(grp)
    m = find_query(297.0, 5, lambda m, lo, hi: ((lo.view(np.uint32) >> BIN_SHIFT) == (hi.view(np.uint32) >> BIN_SHIFT))
                   & ((lo.view(np.uint32) & LOW) > 1) & ((hi.view(np.uint32) & LOW) < LOW - 1))
    lo, hi = bounds(m, 5)
    b0 = bin_of(lo) << BIN_SHIFT
    assert bin_of(lo) == bin_of(hi)
    grp = _Group("E3_one_bin", [(from_bits(b0), "first pattern of the window's only bin"), (down(lo), "one ulp below lo"), (lo, "on lo"), (m, "on the query"),
                                (hi, "on hi"), (up(hi), "one ulp above hi"), (from_bits(b0 | LOW), "last pattern of the window's only bin")])
    grp.case("E3", "E3_inside_one_bin", [m], 5, [-1, -1, 0, 0, 0, -1, -1])
    g.append(grp)
    m = find_query(301.0, 60, lambda m, lo, hi: ((hi.view(np.uint32) >> BIN_SHIFT) - (lo.view(np.uint32) >> BIN_SHIFT) >= 2)
                   & ((lo.view(np.uint32) & LOW) < LOW) & ((hi.view(np.uint32) & LOW) > 0))
    lo, hi = bounds(m, 60)
    bl, bh = bin_of(lo), bin_of(hi)
    assert bh - bl >= 2
    grp = _Group("E3_bins", [(down(lo), "one ulp below lo"), (lo, "on lo"), (from_bits((bl << BIN_SHIFT) | LOW), "last pattern of the window's first bin"),
                             (from_bits((bl + 1) << BIN_SHIFT), "first pattern of the window's second bin"), (from_bits(((bl + 1) << BIN_SHIFT) | 200), "inside the window's second bin"),
                             (from_bits(((bl + 1) << BIN_SHIFT) | LOW), "last pattern of the window's second bin"), (from_bits(bh << BIN_SHIFT), "first pattern of the window's last bin"),
                             (hi, "on hi"), (up(hi), "one ulp above hi")])
    grp.case("E3", "E3_three_bins_one_cell", [m], 60, [-1, 0, 0, 0, 0, 0, 0, 0, -1])
    g.append(grp)

    # ---- E4: windows over a power of two, where the ulp doubles
    for P in (256.0, 512.0, 1024.0):
        P = F32(P)
        m = find_query(P * F32(1 + 2e-6), 15, lambda m, lo, hi: (lo < P) & (P <= hi))
        lo, hi = bounds(m, 15)
        assert lo < P <= hi and P - down(P) == (up(P) - P) / 2
        grp = _Group(f"E4_{int(P)}", [(down(lo), "one ulp below lo"), (lo, "on lo"), (down(P), f"one (half-size) ulp below {int(P)}"), (P, f"on {int(P)}"),
                                      (up(P), f"one ulp above {int(P)}"), (hi, "on hi"), (up(hi), "one ulp above hi")])
        grp.case("E4", f"E4_straddle_{int(P)}", [m], 15, [-1, 0, 0, 0, 0, 0, -1])
        mh = find_query(P * F32(1 - 16e-6), 15, lambda m, lo, hi: hi == P)
        lh, hh = bounds(mh, 15)
        assert hh == P and lh < down(lo)
        grp.case("E4", f"E4_hi_is_{int(P)}", [mh], 15, [0, 0, 0, 0, -1, -1, -1])
        ml = find_query(P * F32(1 + 14e-6), 15, lambda m, lo, hi: lo == P)
        ll, hl = bounds(ml, 15)
        assert ll == P and hl > up(hi)
        grp.case("E4", f"E4_lo_is_{int(P)}", [ml], 15, [-1, -1, -1, 0, 0, 0, 0])
        g.append(grp)

    # ---- E6: equal m/z in one spectrum (input order decides the running mean)
    m = F32(311.0)
    lo, hi = bounds(m, 15)
    grp = _Group("E6", [(down(lo), "below lo (first of two equal)"), (down(lo), "below lo (second of two equal)"), (lo, "on lo (first of two equal)"),
                        (lo, "on lo (second of two equal)"), (m, "on the query (first of three equal)"), (m, "on the query (second of three equal)"),
                        (m, "on the query (third of three equal)"), (hi, "on hi (first of two equal)"), (hi, "on hi (second of two equal)"), (up(hi), "one ulp above hi")])
    grp.case("E6", "E6_equal_mz", [m], 15, [-1, -1, 0, 0, 0, 0, 0, 0, 0, -1])
    g.append(grp)

    # ---- E7: intensities at the cuts of the running mean (no membership encoding; bit for bit against the reference)
    near = F32(1e-26)  # float32(1e-26) lies below 1e-26: it and its upper neighbour straddle the cut
    assert float(near) < 1e-26 < float(up(near))
    cells = [[0.0], [0.0, 37.5], [1e-40], [1e-30], [near], [up(near)], [1e-21], [1e-19], [3e9], [2.0 ** 24, 1.0, 1.0, 3.0], [1e-40, 2.5]]
    what = ["0", "0 then a normal peak", "1e-40 (denormal)", "1e-30", "the float32 just below 1e-26", "the float32 just above 1e-26", "1e-21", "1e-19", "3e9",
            "a sum that passes 2^24", "a denormal then a normal peak"]
    peaks, inten, owners, queries = [], [], [], []
    for j, cell in enumerate(cells):
        q = F32(321.0 + 2.0 * j)
        queries.append(q)
        for i, v in enumerate(cell):
            peaks.append((up(q, 3 * i), f"intensity {what[j]} (peak {i})"))
            inten.append(v)
            owners.append(j)
    grp = _Group("E7", peaks, intensity=inten)
    assert grp.intensity[3] > 0 and grp.intensity[3] < F32(1.2e-38)  # really a denormal
    grp.case("E7", "E7_intensities", queries, 15, owners)
    g.append(grp)

    # ---- E5 (high end)
    mD = F32(1100.5)
    loD, hiD = bounds(mD, 15)
    high = _Group("E5_high", [(down(loD), "one ulp below lo of the query whose hi is the largest m/z"), (loD, "on that lo"), (down(hiD), "one ulp below the largest m/z"),
                              (hiD, "the run's largest m/z")])
    high.case("E5", "E5_hi_is_mz_max", [mD], 15, [-1, 0, 0, 0])
    loE, hiE = bounds(hiD, 15)
    assert loD < loE <= hiD < hiE
    high.case("E5", "E5_mz_max_inside", [hiD], 15, [-1, -1, 0, 0])
    mF = find_query(hiD * F32(1 + 14e-6), 15, lambda m, lo, hi: lo == hiD)
    high.case("E5", "E5_lo_is_mz_max", [mF], 15, [-1, -1, -1, 0])
    mG = F32(hiD * F32(1 + 1e-4))
    assert bounds(mG, 15)[0] > hiD
    high.case("E5", "E5_above_run", [mG], 15, [-1, -1, -1, -1])
    g.append(high)
    return g


def _one_bin_groups() -> list:
    """Every peak of the run in one bin (n_bins == 1)."""
    b0 = bin_of(F32(300.0)) << BIN_SHIFT
    pats = [0, 1, 200, 255, 510, 511]
    grp = _Group("E5_one_bin", [(from_bits(b0 | p), f"pattern {p} of the run's only bin") for p in pats])
    grp.case("E5", "E5_one_bin_all", [from_bits(b0 | 255)], 60, [0] * 6)
    p200 = from_bits(b0 | 200)
    m = find_query(p200, 5, lambda m, lo, hi: lo == p200)
    lo, hi = bounds(m, 5)
    assert lo == p200 and from_bits(b0 | 255) <= hi < from_bits(b0 | 510)
    grp.case("E5", "E5_one_bin_inner", [m], 5, [-1, -1, 0, 0, -1, -1])
    first, last = from_bits(b0), from_bits(b0 | LOW)
    m = find_query(first * F32(1 - 16e-6), 15, lambda m, lo, hi: hi == first)
    grp.case("E5", "E5_one_bin_hi_is_mz_min", [m], 15, [0, -1, -1, -1, -1, -1])
    m = find_query(last * F32(1 + 14e-6), 15, lambda m, lo, hi: lo == last)
    grp.case("E5", "E5_one_bin_lo_is_mz_max", [m], 15, [-1, -1, -1, -1, -1, 0])
    grp.case("E5", "E5_one_bin_below", [F32(299.0)], 15, [-1] * 6)
    grp.case("E5", "E5_one_bin_above", [F32(301.0)], 15, [-1] * 6)
    return [grp]


def _wide_groups() -> list:
    """A run from 50 to 6000 Th: seven binades of bins."""
    g = []
    lo50 = _Group("E5_50", [(F32(50.0), "the run's smallest m/z, 50"), (up(F32(50.0)), "one ulp above 50")])
    lo50.case("E5", "E5_wide_mz_min_inside", [F32(50.0)], 15, [0, 0])
    lo50.case("E5", "E5_wide_below", [F32(49.9)], 15, [-1, -1])
    g.append(lo50)
    _e1(g, 51.3, family="E5", name="E5_wide_bounds_51")
    _e1(g, 3000.5, family="E5", name="E5_wide_bounds_3000")
    _e1(g, 5999.0, family="E5", name="E5_wide_bounds_5999")
    hi = _Group("E5_6000", [(down(F32(6000.0)), "one ulp below 6000"), (F32(6000.0), "the run's largest m/z, 6000")])
    hi.case("E5", "E5_wide_mz_max_inside", [F32(6000.0)], 15, [0, 0])
    hi.case("E5", "E5_wide_above", [F32(6001.0)], 15, [-1, -1])
    g.append(hi)
    return g


RUNS = {
    # name: (groups, cycles, designed cycles, the inner frame limits in cycles, noise peaks per spectrum)
    # (136 cycles: three groups of 64 cycles of the transposed run, so that the run can be staged in several slabs and
    # a box can cross a group)
    "main": (_main_groups, 136, (0, 5, 6, 70, 129, 130, 135), (6, 130), 3),
    "one_bin": (_one_bin_groups, 8, (0, 2, 3, 4, 5, 7), (3, 5), 0),
    "wide": (_wide_groups, 8, (0, 2, 3, 4, 5, 7), (3, 5), 6),
}


def build_alpharaw(seed: int = 0, run: str = "main"):
    """``(dia, cases)``: one MS1 row plus 8 touching 10 Th windows; the designed peaks stand in the MS1 row and in one
    MS2 row of the designed cycles (E8: the first and the last cycle of the run, the first and the last cycle inside
    the inner frame limits and the cycles just outside them), noise everywhere else.  Every case comes twice: as a
    fragment query (``*_ms2``) and as an MS1 / isotope query (``*_ms1``)."""
    make, n_cycles, designed, inner, n_noise = RUNS[run]
    groups = make()
    rng = np.random.default_rng([seed, 20261021, sorted(RUNS).index(run)])
    cycle = syn.make_cycle(n_ms2=8, mz_lo=400.0, mz_hi=480.0)
    L = cycle.shape[1]
    d_mz = np.concatenate([g.mz for g in groups])
    d_int = np.concatenate([g.intensity for g in groups])
    mz_min, mz_max = d_mz.min(), d_mz.max()
    # where noise must not fall: every group's peaks and windows, with room to spare
    guards = []
    for g in groups:
        los, his = zip(*[bounds(c[2], c[3]) for c in g.cases])
        a = min(float(g.mz.min()), min(float(x.min()) for x in los))
        b = max(float(g.mz.max()), max(float(x.max()) for x in his))
        guards.append((a - 0.1, b + 0.1))
    guards.sort()
    for (a0, b0), (a1, b1) in zip(guards[:-1], guards[1:]):
        assert b0 < a1, "two groups of designed peaks share a stretch of m/z"

    def noise(n):
        if n == 0:
            return np.zeros(0, F32), np.zeros(0, F32)
        m = rng.uniform(float(mz_min) + 1.0, float(mz_max) - 1.0, 4 * n).astype(F32)
        keep = np.ones(m.size, dtype=bool)
        for a, b in guards:
            keep &= ~((m >= a) & (m <= b))
        m = m[keep][:n]
        assert m.size == n
        return m, np.exp(rng.normal(3.0, 1.0, n)).astype(F32)

    mzs, ints, start, stop = [], [], [], []
    at = 0
    for c in range(n_cycles):
        for row in range(L):
            m, i = noise(n_noise)
            if c in designed and row in (0, MS2_ROW):
                m, i = np.concatenate([d_mz, m]), np.concatenate([d_int, i])
            o = np.argsort(m, kind="stable")  # equal m/z stay in input order
            mzs.append(m[o])
            ints.append(i[o])
            start.append(at)
            at += m.size
            stop.append(at)
    dia = syn.AlphaRawArrays(
        cycle=cycle, rt_values=(np.arange(n_cycles * L) * 0.5).astype(F32),
        peak_start_idx_list=np.asarray(start, dtype=np.int64), peak_stop_idx_list=np.asarray(stop, dtype=np.int64),
        mz_values=np.concatenate(mzs).astype(F32), intensity_values=np.concatenate(ints).astype(F32))
    assert dia.min_mz_value == mz_min and dia.max_mz_value == mz_max
    if run == "one_bin":
        assert bin_of(mz_min) == bin_of(mz_max)
    if run == "wide":
        assert mz_min == F32(50.0) and mz_max == F32(6000.0)
    if run == "main":
        assert bits(mz_min) == bits(bounds(F32(200.5), 15)[0]) and bits(mz_max) == bits(bounds(F32(1100.5), 15)[1])

    cases, n = [], 0
    for g in groups:
        for family, name, q, tol, owners, ascending in g.cases:
            for ms, row, quad in (("ms2", MS2_ROW, MS2_QUAD), ("ms1", 0, MS1_QUAD)):
                c0, c1 = (0, n_cycles) if n % 2 == 0 else inner
                n += 1
                cases.append(_case(dia, g, family, f"{name}_{ms}", q, tol, owners, ascending, row, quad, c0, c1, designed))
    if run == "main":  # E8: the limits around the designed cycles, on the E1 peaks
        g = next(x for x in groups if x.name == "E1_bounds")
        family, name, q, tol, owners, ascending = g.cases[0]
        for c0, c1 in ((0, 6), (5, 7), (6, 130), (130, 136), (135, 136), (0, 1), (1, 5), (0, 136), (60, 72)):
            for ms, row, quad in (("ms2", MS2_ROW, MS2_QUAD), ("ms1", 0, MS1_QUAD)):
                cases.append(_case(dia, g, "E8", f"E8_cycles_{c0}_{c1}_{ms}", q, tol, owners, ascending, row, quad, c0, c1, designed))
    return dia, cases


def _case(dia, g, family, name, q, tol, owners, ascending, row, quad, c0, c1, designed) -> Case:
    L = dia.cycle_len
    lo, hi = bounds(q, tol)
    assert ascending == bool(np.all(np.diff(q) >= 0)), name
    K, F = len(q), c1 - c0
    claimed = np.zeros((K, F), dtype=F32)
    for c in designed:
        if c0 <= c < c1:
            for own, v in zip(owners, g.intensity):
                if own >= 0:
                    claimed[own, c - c0] += v
    # the reference's loop over the spectra as built (designed peaks of the other groups and noise included)
    seen = np.zeros((K, F), dtype=F32)
    for f in range(F):
        sp = (c0 + f) * L + row
        a, b = dia.peak_start_idx_list[sp], dia.peak_stop_idx_list[sp]
        for k, (i0, i1) in enumerate(take(dia.mz_values[a:b], lo, hi)):
            for v in dia.intensity_values[a + i0:a + i1]:
                seen[k, f] += v
    if g.encoded:
        assert np.array_equal(claimed, seen), f"{name}: the stated owners are not what the reference's loop takes"
    return Case(name=name, frame_limits=np.array([[c0 * L, c1 * L, 1]], dtype=np.uint64), mz_query=q, tol=tol,
                quad=np.array([quad], dtype=np.float64), expected=claimed if g.encoded else None, family=family,
                labels=g.labels, owners=tuple((o,) if o >= 0 else () for o in owners), intensity=tuple(g.intensity.tolist()),
                ascending=ascending)


def describe_difference(case: Case, got_plane: np.ndarray) -> str:
    """Which designed peaks a differing intensity plane took or missed: for assertion messages."""
    if case.expected is None or np.array_equal(got_plane, case.expected):
        return ""
    lines = []
    for at in np.argwhere(got_plane != case.expected)[:4]:
        at = tuple(int(x) for x in at)
        g, e = float(got_plane[at]), float(case.expected[at])
        if g != int(g) or g < 0 or g >= 2 ** 24:
            lines.append(f"cell {at}: {g} is no sum of designed peaks (expected {e})")
            continue
        diff = int(g) ^ int(e)
        for j, label in enumerate(case.labels):
            if diff >> j & 1:
                lines.append(f"query {at[0]} ({case.mz_query[at[0]]!r}), cell {at}: the peak {label} was "
                             + ("taken but belongs to " if int(g) >> j & 1 else "missed; it belongs to ")
                             + (f"query {case.owners[j]}" if case.owners[j] else "no query"))
    return f"case {case.name}: " + "; ".join(lines)


def family_counts(cases) -> dict:
    """family -> (cases, designed peaks inside a window, designed peaks outside every window), as the tests print it."""
    out = {}
    for c in cases:
        n, i, o = out.get(c.family, (0, 0, 0))
        out[c.family] = (n + 1, i + sum(1 for w in c.owners if w), o + sum(1 for w in c.owners if not w))
    return out


SCORING_BOXES = ((0, 8), (3, 9), (4, 7), (60, 72), (124, 136), (104, 136), (129, 136))  # cycles; 3 ... 32 of them each


def query_lists(cases, at_most: int, at_least: int = 4) -> list:
    """The fragment queries of the cases (each case once, not per MS level) packed into lists of ``at_least`` ...
    ``at_most`` m/z, sorted as a library is; a list never splits a case."""
    lists, cur = [], []
    for c in cases:
        if not c.name.endswith("_ms2") or c.family == "E8":
            continue
        q = [float(x) for x in c.mz_query]
        if len(cur) + len(q) > at_most:
            lists.append(cur)
            cur = []
        cur = cur + q
    lists.append(cur)
    if len(lists[-1]) < at_least:  # (a precursor needs four fragments to be scored: filled up with queries of the first list)
        lists[-1] = lists[-1] + lists[0][:at_least - len(lists[-1])]
    assert all(at_least <= len(x) <= at_most for x in lists)
    return [np.sort(np.asarray(x, dtype=F32), kind="stable") for x in lists]


def tolerance_lists(cases) -> dict:
    """tolerance -> one fragment list of the queries designed at that tolerance (5, 60 and 200 ppm: the window inside
    one bin, the cell that continues over three bins, the windows three deep), filled up to four and more fragments
    with E1 and E4 queries, which are ordinary windows there."""
    by_name = {c.name: c for c in cases}
    fill = [float(by_name[n].mz_query[0]) for n in ("E1_bounds_ms2", "E4_straddle_256_ms2", "E4_straddle_512_ms2", "E4_straddle_1024_ms2")]
    out = {}
    for name in ("E3_inside_one_bin_ms2", "E3_three_bins_one_cell_ms2", "E2_three_deep_ms2"):
        c = by_name[name]
        out[float(c.tol)] = np.sort(np.asarray([float(x) for x in c.mz_query] + fill, dtype=F32), kind="stable")
    assert sorted(out) == [5.0, 60.0, 200.0]
    return out


def scoring_case(dia, cases, at_most: int = 12, at_least: int = 4, boxes=SCORING_BOXES, every_query: bool = False, lists=None):
    """The edge queries as a library on the run ``dia``: every list of ``query_lists`` is the fragment list of one
    precursor per box and per observation count (one: PRECURSOR_MZ, whose isotope windows carry the E1_isotope peaks
    in the MS1 row; two: PRECURSOR_MZ_2OBS), one candidate each.  Returns a ``syn.SyntheticCase``."""
    L = dia.cycle_len
    lists = list(lists) if lists is not None else query_lists(cases, at_most, at_least)
    if every_query:  # one more precursor with all of them
        lists += query_lists(cases, 64, at_least)
        assert len(lists[-1]) > 32
    rows = [(li, box, mz) for li in range(len(lists)) for box in boxes for mz in (PRECURSOR_MZ, PRECURSOR_MZ_2OBS)]
    c0 = np.array([b[0] for _, b, _ in rows], dtype=np.int64)
    c1 = np.array([b[1] for _, b, _ in rows], dtype=np.int64)
    n = len(rows)
    library = _library([lists[li] for li, _, _ in rows], [mz for _, _, mz in rows], PRECURSOR_CHARGE,
                       dia.rt_values[((c0 + c1) // 2) * L], np.zeros(n))
    candidates_df = _candidates(n, c0 * L, c1 * L, ((c0 + c1) // 2) * L, np.zeros(n), np.ones(n), np.zeros(n))
    return syn.SyntheticCase(dia, library, candidates_df, (c0 + c1) // 2)


def _library(fragment_lists, precursor_mz, charge, rt, mobility) -> syn.SyntheticLibrary:
    """One precursor per fragment list, an elution group each."""
    import pandas as pd

    n = len(fragment_lists)
    n_frag = np.array([len(x) for x in fragment_lists], dtype=np.int64)
    assert n_frag.max() < 67
    stop = np.cumsum(n_frag)
    start = stop - n_frag
    total = int(stop[-1])
    within = np.arange(total, dtype=np.int64) - np.repeat(start, n_frag)
    idx = np.arange(n, dtype=np.uint32)
    precursor_df = pd.DataFrame({
        "elution_group_idx": idx, "precursor_idx": idx, "channel": np.zeros(n, dtype=np.uint32), "decoy": np.zeros(n, dtype=np.uint8),
        "flat_frag_start_idx": start.astype(np.uint32), "flat_frag_stop_idx": stop.astype(np.uint32),
        "charge": np.full(n, charge, dtype=np.uint8), "rt_library": np.asarray(rt, dtype=F32),
        "mobility_library": np.asarray(mobility, dtype=F32), "mz_library": np.asarray(precursor_mz, dtype=F32),
        "proteins": np.full(n, "P", dtype=object), "genes": np.full(n, "G", dtype=object), "sequence": np.full(n, "PEPTIDEK", dtype=object),
        "mods": np.full(n, "", dtype=object), "mod_sites": np.full(n, "", dtype=object),
        "i_0": np.full(n, 0.4, dtype=F32), "i_1": np.full(n, 0.3, dtype=F32), "i_2": np.full(n, 0.2, dtype=F32), "i_3": np.full(n, 0.1, dtype=F32)})
    fragment_df = pd.DataFrame({
        "mz_library": np.concatenate(fragment_lists).astype(F32),
        # distinct library intensities, not ordered like the m/z: which fragments are kept and how they sort are two things
        "intensity": (0.05 + ((within * 7) % 67) / 80.0).astype(F32),  # (fewer than 67 fragments a precursor)
        "cardinality": np.ones(total, dtype=np.uint8), "type": np.where(within % 2 == 0, 98, 121).astype(np.uint8),
        "loss_type": np.zeros(total, dtype=np.uint8), "charge": np.ones(total, dtype=np.uint8),
        "number": (within + 1).astype(np.uint8), "position": within.astype(np.uint8)})
    return syn.SyntheticLibrary(precursor_df, fragment_df)


def _candidates(n, frame_start, frame_stop, frame_center, scan_start, scan_stop, scan_center):
    import pandas as pd

    idx = np.arange(n, dtype=np.uint32)
    i64 = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    return pd.DataFrame({
        "elution_group_idx": idx, "precursor_idx": idx, "rank": np.zeros(n, dtype=np.uint8), "scan_start": i64(scan_start),
        "scan_stop": i64(scan_stop), "scan_center": i64(scan_center), "frame_start": i64(frame_start), "frame_stop": i64(frame_stop),
        "frame_center": i64(frame_center), "score": np.linspace(10.0, 90.0, n).astype(F32)})


def scoring_case_timstof(dia, cases, at_most: int = 12, at_least: int = 4):
    """The same over the ion-mobility run: the queries of the T cases (the isotope cases aside: those windows are the
    precursor's own) in lists of ``at_most`` fragments, one precursor per list and box of T_BOXES."""
    L, S = dia.cycle_len, dia.scan_max_index
    lists = query_lists([c for c in cases if "isotope" not in c.name], at_most, at_least)
    rows = [(li, box) for li in range(len(lists)) for box in T_BOXES]
    n = len(rows)
    c0, c1 = (np.array([b[0][i] for _, b in rows], dtype=np.int64) for i in (0, 1))
    s0, s1 = (np.array([b[1][i] for _, b in rows], dtype=np.int64) for i in (0, 1))
    library = _library([lists[li] for li, _ in rows], [b[2] for _, b in rows], T_CHARGE, dia.rt_values[((c0 + c1) // 2) * L + 1],
                       dia.mobility_values[(s0 + s1) // 2])
    candidates_df = _candidates(n, c0 * L + 1, c1 * L + 1, ((c0 + c1) // 2) * L + 1, s0, s1, (s0 + s1) // 2)
    return syn.TimsTOFCase(dia, library, candidates_df)


# ------------------------------------------------------------------------------------------ ion mobility
T_SCANS, T_CYCLES, T_NTOF = 16, 12, 8192
T_DESIGNED_SCANS = (0, 3, 4, 9, 10, 15)
T_DESIGNED_CYCLES = (0, 2, 3, 8, 9, 11)
T_INNER = ((3, 9), (4, 10))  # cycles, scans: the designed cycles / scans lie on and just outside these limits
T_QUAD = (442.0, 445.0)
# precursors of the scoring tests: isolated at the scans 0 .. 6 (window 440 .. 460), at the scans 7 .. 13 (420 .. 440),
# and one whose isotope range lies across 440, seen in both frames by a box that spans both scan ranges
T_PRECURSOR_MZ, T_PRECURSOR_MZ_LOW, T_PRECURSOR_MZ_2OBS, T_PRECURSOR_TOL, T_CHARGE = F32(445.37), F32(425.37), F32(439.2), 20.0, 1
# (cycles, scans, precursor m/z) of the candidates
T_BOXES = (((3, 9), (4, 10), T_PRECURSOR_MZ), ((0, 12), (0, 16), T_PRECURSOR_MZ), ((2, 5), (2, 6), T_PRECURSOR_MZ), ((8, 12), (0, 5), T_PRECURSOR_MZ),
           ((0, 12), (7, 14), T_PRECURSOR_MZ_LOW), ((0, 12), (0, 16), T_PRECURSOR_MZ_2OBS), ((3, 9), (4, 10), T_PRECURSOR_MZ_2OBS))


def lut_layout(mz_values: np.ndarray):
    """How staging lays out the m/z lookup table (alphadia_amd/csrc/adh_api.hip): the smallest power of two of
    buckets >= 4 * n_tof between the first and the last TOF m/z; bucket b starts at ``lut_min + b * step``."""
    nb = 1
    while nb < 4 * len(mz_values):
        nb <<= 1
    lo, hi = float(mz_values[0]), float(mz_values[-1])
    return nb, lo, (hi - lo) / nb


def build_timstof(seed: int = 0):
    """``(dia, cases)`` for a small ion-mobility run: TOF bins whose float64 m/z stand on a query's float32 bounds and
    one float64 step on either side, windows of zero, one and many TOF bins, queries outside the TOF range and bounds
    on the edges of the m/z lookup buckets; events in the first and last scan and frame of the limits and just outside.
    ``expected[k, o, s, f]`` decodes the TOF bins taken (uint16 intensities 2^0 .. 2^15).  The reference takes the TOF
    bins ``lo <= mz < hi`` of every query on its own: hi is exclusive and overlapping windows share their bins."""
    rng = np.random.default_rng([seed, 20261021, 99])
    S, L = T_SCANS, 3
    cycle = syn.make_timstof_cycle(2, 2, S, 400.0, 480.0)
    assert cycle.shape[1] == L
    n_frames = T_CYCLES * L + 1
    t = np.arange(T_NTOF, dtype=np.float64)
    mz = (np.sqrt(100.0) + t * (np.sqrt(1124.0) - np.sqrt(100.0)) / (T_NTOF - 1)) ** 2
    mz[0], mz[-1] = 100.0, 1124.0
    nb, lut_min, step = lut_layout(mz)
    assert (nb, lut_min, step) == (32768, 100.0, 0.03125)  # bucket edges 100 + b / 32: exact in float32 and float64

    def edge(b):
        x = lut_min + b * step
        assert float(F32(x)) == x and (x - lut_min) * (1.0 / step) == b
        return F32(x)

    d64 = lambda x: np.nextafter(np.float64(x), -np.inf)  # noqa: E731
    u64 = lambda x: np.nextafter(np.float64(x), np.inf)  # noqa: E731
    groups = []  # (name, [(m/z, label)], [(case name, queries, tol, owners per bin)], first TOF bin or None)

    m = F32(250.77)
    lo, hi = bounds(m, 15)
    groups.append(("T1", [(d64(lo), "one float64 step below lo"), (np.float64(lo), "on lo"), (u64(lo), "one float64 step above lo"), (np.float64(m), "on the query"),
                          (d64(hi), "one float64 step below hi"), (np.float64(hi), "on hi (exclusive)"), (u64(hi), "one float64 step above hi")],
                   [("T_bounds_many_bins", [m], 15, [(), (0,), (0,), (0,), (0,), (), ()])], None))
    m = F32(300.3)
    lo, hi = bounds(m, 15)
    groups.append(("T2", [(d64(lo), "one float64 step below lo"), (np.float64(hi), "on hi (exclusive)")], [("T_zero_bins", [m], 15, [(), ()])], None))
    m = F32(350.9)
    lo, hi = bounds(m, 15)
    groups.append(("T3", [(d64(lo), "one float64 step below lo"), (np.float64(m), "on the query"), (np.float64(hi), "on hi (exclusive)")],
                   [("T_one_bin", [m], 15, [(), (0,), ()])], None))
    q = np.array([380.0, 380.0 * (1 + 5e-6)], dtype=F32)
    lo, hi = bounds(q, 15)
    assert lo[0] < lo[1] < hi[0] < hi[1]
    groups.append(("T4", [(np.float64(lo[0]), "on lo of window 0"), (np.float64(lo[1]), "on lo of window 1, inside window 0"), (np.float64(hi[0]), "on hi of window 0 (exclusive), inside window 1"),
                          (np.float64(hi[1]), "on hi of window 1 (exclusive)")], [("T_overlap_shares_bins", q, 15, [(0,), (0, 1), (1,), ()])], None))
    # the isotope windows of the precursor the scoring tests use (20 ppm there)
    for i, m in enumerate(isotope_mz(T_PRECURSOR_MZ, T_CHARGE, 3)):
        lo, hi = bounds(m, T_PRECURSOR_TOL)
        groups.append((f"T_iso{i}", [(d64(lo), "one float64 step below lo"), (np.float64(lo), "on lo"), (np.float64(m), "on the isotope m/z"), (d64(hi), "one float64 step below hi"),
                                     (np.float64(hi), "on hi (exclusive)")], [(f"T_isotope{i}_bounds", [m], T_PRECURSOR_TOL, [(), (0,), (0,), (0,), ()])], None))
    # bucket edges of the lookup table
    x = edge(12868)
    ml = find_query(x * F32(1 + 14e-6), 15, lambda m, lo, hi: lo == x)
    xh = edge(13204)
    mh = find_query(xh * F32(1 - 16e-6), 15, lambda m, lo, hi: hi == xh)
    assert bounds(ml, 15)[0] == x and bounds(mh, 15)[1] == xh
    groups.append(("T5", [(d64(x), "one float64 step below lo = an interior bucket edge"), (np.float64(x), "on lo = an interior bucket edge"), (u64(x), "one float64 step above that edge")],
                   [("T_lo_on_bucket_edge", [ml], 15, [(), (0,), (0,)])], None))
    groups.append(("T6", [(d64(xh), "one float64 step below hi = an interior bucket edge"), (np.float64(xh), "on hi = an interior bucket edge (exclusive)")],
                   [("T_hi_on_bucket_edge", [mh], 15, [(0,), ()])], None))
    first, last = edge(0), edge(nb)
    m0 = find_query(first * F32(1 + 14e-6), 15, lambda m, lo, hi: lo == first)
    m1 = find_query(first * F32(1 - 16e-6), 15, lambda m, lo, hi: hi == first)
    groups.append(("T7", [(np.float64(first), "the first TOF m/z = the first bucket edge"), (u64(first), "one float64 step above the first TOF m/z")],
                   [("T_lo_on_first_bucket", [m0], 15, [(0,), (0,)]), ("T_hi_on_first_tof", [m1], 15, [(), ()]), ("T_first_tof_inside", [first], 15, [(0,), (0,)]),
                    ("T_below_first_tof", [F32(99.0)], 15, [(), ()])], 0))
    m0 = find_query(last * F32(1 - 16e-6), 15, lambda m, lo, hi: hi == last)
    m1 = find_query(last * F32(1 + 14e-6), 15, lambda m, lo, hi: lo == last)
    groups.append(("T8", [(d64(last), "one float64 step below the last TOF m/z"), (np.float64(last), "the last TOF m/z = the last bucket edge")],
                   [("T_hi_on_last_bucket", [m0], 15, [(0,), ()]), ("T_lo_on_last_tof", [m1], 15, [(), (0,)]), ("T_last_tof_inside", [last], 15, [(0,), (0,)]),
                    ("T_above_last_tof", [F32(1130.0)], 15, [(), ()])], T_NTOF - 2))

    # place the designed bins into the TOF axis
    designed_bins, taken = {}, np.zeros(T_NTOF, dtype=bool)
    for name, pk, _, t0 in groups:
        vals = np.array([p[0] for p in pk], dtype=np.float64)
        assert np.all(np.diff(vals) > 0) and len(vals) <= 16, name
        if t0 is None:
            t0 = int(np.searchsorted(mz, vals[0])) - len(vals) // 2
        sl = slice(t0, t0 + len(vals))
        assert not taken[max(t0 - 1, 0):t0 + len(vals) + 1].any(), name
        taken[sl] = True
        mz[sl] = vals
        designed_bins[name] = t0
    assert np.all(np.diff(mz) > 0) and mz[0] == 100.0 and mz[-1] == 1124.0

    # events: every designed bin at every designed (cycle, frame of the cycle, scan); noise on the other bins
    ev_tof, ev_push, ev_int = [], [], []
    for name, pk, _, _ in groups:
        for j in range(len(pk)):
            for c in T_DESIGNED_CYCLES:
                for fr in range(L):
                    for s in T_DESIGNED_SCANS:
                        ev_tof.append(designed_bins[name] + j)
                        ev_push.append((1 + c * L + fr) * S + s)
                        ev_int.append(1 << j)
    n_noise = 3000
    free = np.flatnonzero(~taken)
    key = np.unique(rng.choice(free, n_noise).astype(np.int64) * (n_frames * S) + rng.integers(S, n_frames * S, n_noise))
    ev_tof = np.concatenate([np.asarray(ev_tof, np.int64), key // (n_frames * S)])
    ev_push = np.concatenate([np.asarray(ev_push, np.int64), key % (n_frames * S)])
    ev_int = np.concatenate([np.asarray(ev_int, np.int64), np.clip(rng.lognormal(3.0, 1.0, key.size), 1, 60000).astype(np.int64)])
    o = np.lexsort((ev_push, ev_tof))
    ev_tof, ev_push, ev_int = ev_tof[o], ev_push[o], ev_int[o]
    dia = syn.TimsTOFArrays(
        cycle=cycle, dia_precursor_cycle=np.repeat(np.arange(L, dtype=np.int64), S), rt_values=np.arange(n_frames, dtype=np.float64) * 0.1,
        mobility_values=np.linspace(1.6, 0.6, S).astype(np.float64), mz_values=mz,
        tof_indptr=np.concatenate([[0], np.cumsum(np.bincount(ev_tof, minlength=T_NTOF))]).astype(np.int64),
        push_indices=ev_push.astype(np.uint32), intensity_values=ev_int.astype(np.uint16), scan_max_index=S)

    cases, n = [], 0
    for name, pk, cs, _ in groups:
        t0 = designed_bins[name]
        for cname, q, tol, owners in cs:
            q = np.asarray(q, dtype=F32)
            for ms, quad in (("ms2", T_QUAD), ("ms1", MS1_QUAD)):
                (c0, c1), (s0, s1) = ((0, T_CYCLES), (0, S)) if n % 2 == 0 else T_INNER
                n += 1
                cases.append(_tims_case(dia, f"{cname}_{ms}", q, F32(tol), quad, c0, c1, s0, s1, t0, pk, owners))
    return dia, cases


def _tims_case(dia, name, q, tol, quad, c0, c1, s0, s1, t0, pk, owners) -> Case:
    L, S = dia.cycle_len, dia.scan_max_index
    lo, hi = bounds(q, tol)
    flat = dia.cycle.reshape(-1, 2)
    # the pushes of the query and their observation (bruker_jit.py: the quadrupole test per (frame of the cycle, scan))
    obs_of = {}
    for fr in range(c0 * L + 1, c1 * L + 1):
        for s in range(s0, s1):
            at = ((fr - 1) * S + s) % (L * S)
            if quad[0] <= flat[at, 1] and quad[1] >= flat[at, 0]:
                obs_of[fr * S + s] = int(dia.dia_precursor_cycle[at])
    obs = sorted(set(obs_of.values()))
    K, F = len(q), c1 - c0
    claimed = np.zeros((K, len(obs), s1 - s0, F), dtype=F32)
    seen = np.zeros_like(claimed)
    for push, ob in obs_of.items():
        fr, s = divmod(push, S)
        c = (fr - 1) // L
        if c in T_DESIGNED_CYCLES and s in T_DESIGNED_SCANS:
            for j, own in enumerate(owners):
                for k in own:
                    claimed[k, obs.index(ob), s - s0, c - c0] += F32(1 << j)
    for k in range(K):
        for tof in range(int(np.searchsorted(dia.mz_values, lo[k], "left")), int(np.searchsorted(dia.mz_values, hi[k], "left"))):
            for e in range(dia.tof_indptr[tof], dia.tof_indptr[tof + 1]):
                push = int(dia.push_indices[e])
                if push in obs_of:
                    fr, s = divmod(push, S)
                    seen[k, obs.index(obs_of[push]), s - s0, (fr - 1) // L - c0] += F32(dia.intensity_values[e])
    assert np.array_equal(claimed, seen), f"{name}: the stated owners are not what the reference's search takes"
    assert len(obs) > 0
    return Case(name=name, frame_limits=np.array([[c0 * L + 1, c1 * L + 1, 1]], dtype=np.uint64), mz_query=q, tol=tol,
                quad=np.array([quad], dtype=np.float64), expected=claimed, family="T", labels=tuple(p[1] for p in pk), owners=tuple(owners),
                intensity=tuple(float(1 << j) for j in range(len(pk))), scan_limits=np.array([[s0, s1, 1]], dtype=np.uint64))


# ------------------------------------------------------------------------------------------ candidate selection
SELECT_CYCLES, SELECT_PRECURSORS, SELECT_FRAGMENTS = 100, 6, 6


def selection_case(seed: int = 0, flip: bool = False) -> syn.SyntheticCase:
    """A run for candidate selection: six precursors, one per isolation window, whose six fragment windows (15 ppm) and
    three isotope windows (10 ppm) each carry four peaks with a Gaussian profile over the cycles around the precursor's
    apex - on lo and on hi with the fragment's amplitude, one ulp below lo and one ulp above hi with ten times that
    amplitude, so that a peak taken on the wrong side of a bound moves the score.  ``flip``: the peak below lo of the
    first fragment of the first precursor stands ON lo instead (the run a wrong ``>=`` would see)."""
    rng = np.random.default_rng([seed, 20261021, 7])
    cycle = syn.make_cycle(n_ms2=8, mz_lo=400.0, mz_hi=480.0)
    L = cycle.shape[1]
    apex = 15 + 12 * np.arange(SELECT_PRECURSORS)
    prec_mz = (405.0 + 10.0 * np.arange(SELECT_PRECURSORS)).astype(F32)
    frag_lists = [np.array([210.1234 + 20.0 * p + 2.5 * j for j in range(SELECT_FRAGMENTS)], dtype=F32) for p in range(SELECT_PRECURSORS)]
    per_spectrum = {}  # (cycle, row) -> list of (m/z, intensity)
    guards = []

    def plant(p, row, m, tol, amplitude, flipped):
        lo, hi = (x[0] for x in bounds([m], tol))
        guards.append((float(lo) - 0.1, float(hi) + 0.1))
        below = lo if flipped else down(lo)
        for c in range(apex[p] - 5, apex[p] + 6):
            g = float(np.exp(-0.5 * ((c - apex[p]) / 2.0) ** 2))
            per_spectrum.setdefault((c, row), []).extend([(below, 10 * amplitude * g), (lo, amplitude * g), (hi, amplitude * g), (up(hi), 10 * amplitude * g)])

    for p in range(SELECT_PRECURSORS):
        for j, m in enumerate(frag_lists[p]):
            plant(p, p + 1, m, 15.0, 1000.0 * (1 + j), flip and p == 0 and j == 0)
        for i, m in enumerate(isotope_mz(prec_mz[p], PRECURSOR_CHARGE, 3)):
            plant(p, 0, m, 10.0, 5000.0 / (1 + i), False)
    mzs, ints, start, stop, at = [], [], [], [], 0
    for c in range(SELECT_CYCLES):
        for row in range(L):
            m = rng.uniform(200.0, 500.0, 12).astype(F32)
            keep = np.ones(m.size, dtype=bool)
            for a, b in guards:
                keep &= ~((m >= a) & (m <= b))
            m = m[keep][:3]
            i = np.exp(rng.normal(3.0, 1.0, m.size)).astype(F32)
            d = per_spectrum.get((c, row), [])
            m = np.concatenate([np.array([x[0] for x in d], dtype=F32), m])
            i = np.concatenate([np.array([x[1] for x in d], dtype=F32), i])
            o = np.argsort(m, kind="stable")
            mzs.append(m[o])
            ints.append(i[o])
            start.append(at)
            at += m.size
            stop.append(at)
    rt = (np.arange(SELECT_CYCLES * L) * (1.5 / L)).astype(F32)
    dia = syn.AlphaRawArrays(cycle=cycle, rt_values=rt, peak_start_idx_list=np.asarray(start, dtype=np.int64),
                             peak_stop_idx_list=np.asarray(stop, dtype=np.int64), mz_values=np.concatenate(mzs).astype(F32),
                             intensity_values=np.concatenate(ints).astype(F32))
    library = _library(frag_lists, prec_mz, PRECURSOR_CHARGE, rt[apex * L], np.zeros(SELECT_PRECURSORS))
    return syn.SyntheticCase(dia, library, None, apex)


TS_SCANS, TS_CYCLES, TS_NTOF, TS_CHARGE = 96, 40, 6000, 1
TS_FRAGMENT_TOL, TS_PRECURSOR_TOL = 15.0, 20.0
# (precursor m/z, apex cycle, apex scan): one per isolation window of two frames and both scan ranges of the cycle
TS_PRECURSORS = ((445.0, 10, 20), (460.0, 17, 30), (420.0, 24, 65), (405.0, 31, 75))


def selection_case_timstof(seed: int = 0, flip: bool = False) -> syn.TimsTOFCase:
    """The ion-mobility counterpart of ``selection_case``: four precursors whose six fragment windows and three isotope
    windows each hold four TOF bins - on lo and one float64 step below hi (inside; hi is exclusive) with the window's
    amplitude, one float64 step below lo and on hi (outside) with ten times that amplitude - with events on a Gaussian
    profile over the cycles and scans around the precursor's apex.  The second fragment of the first precursor has its
    lo on an edge of the m/z lookup buckets.  ``flip``: the events below lo of the first fragment
    window of the first precursor fall into the bin on lo instead."""
    rng = np.random.default_rng([seed, 20261021, 8])
    S, L = TS_SCANS, 4
    cycle = syn.make_timstof_cycle(3, 2, S, 400.0, 480.0)
    assert cycle.shape[1] == L
    n_frames = TS_CYCLES * L + 1
    t = np.arange(TS_NTOF, dtype=np.float64)
    mz = (np.sqrt(195.0) + t * (np.sqrt(490.0) - np.sqrt(195.0)) / (TS_NTOF - 1)) ** 2
    mz[0], mz[-1] = 195.0, 490.0
    nb, lut_min, step = lut_layout(mz)
    assert (nb, lut_min, step) == (32768, 195.0, 295.0 / 32768)  # (bucket edges 195 + b * 295 / 2^15: exact)
    taken = np.zeros(TS_NTOF, dtype=bool)
    ev_tof, ev_push, ev_int = [], [], []
    frag_lists = []

    def plant(m, tol, frame_in_cycle, apex_c, apex_s, amplitude, flipped):
        lo, hi = (np.float64(x[0]) for x in bounds([m], tol))
        vals = np.array([np.nextafter(lo, -np.inf), lo, np.nextafter(hi, -np.inf), hi])
        t0 = int(np.searchsorted(mz, vals[0])) - 2
        assert not taken[t0 - 1:t0 + 5].any(), m
        taken[t0:t0 + 4] = True
        mz[t0:t0 + 4] = vals
        for j, a in enumerate((10 * amplitude, amplitude, amplitude, 10 * amplitude)):
            for c in range(apex_c - 4, apex_c + 5):
                for s in range(apex_s - 6, apex_s + 7):
                    v = int(round(a * np.exp(-0.5 * ((c - apex_c) / 2.0) ** 2) * np.exp(-0.5 * ((s - apex_s) / 3.0) ** 2)))
                    if v > 0:
                        ev_tof.append(t0 + (1 if flipped and j == 0 else j))
                        ev_push.append((1 + c * L + frame_in_cycle) * S + s)
                        ev_int.append(v)

    for p, (pmz, apex_c, apex_s) in enumerate(TS_PRECURSORS):
        frames = [fr for fr in range(L) if cycle[0, fr, apex_s, 0] <= pmz <= cycle[0, fr, apex_s, 1]]
        assert len(frames) == 1 and all(cycle[0, frames[0], s, 0] <= pmz <= cycle[0, frames[0], s, 1] for s in range(apex_s - 6, apex_s + 7))
        q = np.array([210.1234 + 25.0 * p + 3.0 * j for j in range(6)], dtype=F32)
        if p == 0:
            x = lut_min + np.ceil((float(q[1]) - lut_min) / step) * step
            assert float(F32(x)) == x and ((x - lut_min) * (1.0 / step)).is_integer()
            q[1] = find_query(F32(x) * F32(1 + 14e-6), TS_FRAGMENT_TOL, lambda m, lo, hi: lo == F32(x))
            assert bounds(q[1:2], TS_FRAGMENT_TOL)[0][0] == F32(x) and q[0] < q[1] < q[2]
        frag_lists.append(q)
        for j, m in enumerate(q):
            plant(m, TS_FRAGMENT_TOL, frames[0], apex_c, apex_s, 300.0 * (1 + j), flip and p == 0 and j == 0)
        for i, m in enumerate(isotope_mz(F32(pmz), TS_CHARGE, 3)):
            plant(m, TS_PRECURSOR_TOL, 0, apex_c, apex_s, 1500.0 / (1 + i), False)
    assert np.all(np.diff(mz) > 0) and max(ev_int) < 65536
    n_push = n_frames * S
    free = np.flatnonzero(~taken)
    key = np.unique(rng.choice(free, 20000).astype(np.int64) * n_push + rng.integers(S, n_push, 20000))
    ev_tof = np.concatenate([np.asarray(ev_tof, np.int64), key // n_push])
    ev_push = np.concatenate([np.asarray(ev_push, np.int64), key % n_push])
    ev_int = np.concatenate([np.asarray(ev_int, np.int64), np.clip(rng.lognormal(3.0, 1.0, key.size), 1, 60000).astype(np.int64)])
    o = np.lexsort((ev_push, ev_tof))
    ev_tof, ev_push, ev_int = ev_tof[o], ev_push[o], ev_int[o]
    rt = np.arange(n_frames, dtype=np.float64) * 0.1
    mobility = np.linspace(1.6, 0.6, S).astype(np.float64)
    dia = syn.TimsTOFArrays(
        cycle=cycle, dia_precursor_cycle=np.repeat(np.arange(L, dtype=np.int64), S), rt_values=rt, mobility_values=mobility, mz_values=mz,
        tof_indptr=np.concatenate([[0], np.cumsum(np.bincount(ev_tof, minlength=TS_NTOF))]).astype(np.int64),
        push_indices=ev_push.astype(np.uint32), intensity_values=ev_int.astype(np.uint16), scan_max_index=S)
    apex_c = np.array([x[1] for x in TS_PRECURSORS])
    apex_s = np.array([x[2] for x in TS_PRECURSORS])
    library = _library(frag_lists, [x[0] for x in TS_PRECURSORS], TS_CHARGE, rt[1 + apex_c * L], mobility[apex_s])
    return syn.TimsTOFCase(dia, library, None)
