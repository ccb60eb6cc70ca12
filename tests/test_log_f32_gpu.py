"""The selection's table-driven log (alphadia_amd/csrc/adh_log_f32.h) on the device, over its whole domain.

Candidate selection takes one log per smoothed cell through ``adh_log_f32``: a float64 log of a float32 argument
in [1, inf), which the two smoothing kernels round to float32, and ``adh_log_f32_rare`` for everything else.  The
test entries ``adh_debug_log_f32`` / ``adh_debug_log_f32_sweep`` evaluate that code as the library's build compiles
it, with the table read from global memory and from a copy in LDS (the two forms the kernels use):

* every mantissa at exponent 0 and a dense sample of every other exponent against ``np.log`` on ``np.longdouble``
  (63 mantissa bits): the float64 error, and the float32 value the kernels store;
* every float32 in [1, inf), 1 073 741 824 arguments, against the device library's own log, in one launch;
* the three-way dispatch of the call sites and the out-of-line routine: 1, +inf, NaN, negatives, zeros, subnormals,
  (0, 1).

The float64 bound, 2 ulp, is derived (see ``adh_log_f32.h``): the result is fl(e ln2_hi + fl(fl(T + p) + fl(e ln2_lo)))
with e ln2_hi exact; the table entry T, T + p and the final sum are each within half an ulp of themselves, T and
T + p lie below the result for e >= 1, and the degree-9 series on |r| < 2^-7 adds less than 2^-4 ulp: at most 1.5 ulp
+ 2^-4.  "ulp" is ``np.spacing(abs(float64(ref)))`` throughout.  Every measured figure is printed and appended to
log_f32.jsonl, beside test_gpu_parity's parity_masks.jsonl.
"""

from __future__ import annotations

import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

from test_calibration_gpu import f32_knife_edge

pytestmark = pytest.mark.gpu

LD = np.longdouble
FIRST, LAST = 0x3F800000, 0x7F7FFFFF  # 1.0f, the largest finite float32
ULP_BOUND = 2.0       # adh_log_f32 against the 80-bit log (derived, see above)
SWEEP_BOUND = 3.0     # against the device library's log: 2 ulp + the library's 1 ulp
KNIFE_ULPS = 2.0      # a float32 knife-edge: the reference within 2 float64 ulp of a float32 rounding midpoint
KNIFE_CAP = 4         # knife-edge arguments allowed in one set
SWEEP_CAPACITY = 4096


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def test_the_reference_is_an_80_bit_log():
    assert np.finfo(LD).nmant >= 63


def _log(record: dict) -> None:
    """One line per measurement in log_f32.jsonl, printed and kept before anything is asserted; the file lies beside
    the suite's other comparison log, parity_masks.jsonl of test_gpu_parity (which runs first)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    record = dict(test=os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], **record)
    print("[log_f32]", json.dumps(record))
    for beside in sorted(glob.glob(os.path.join(root, "*", "parity_masks.jsonl")))[:1]:
        try:
            with open(os.path.join(os.path.dirname(beside), "log_f32.jsonl"), "a") as f:
                f.write(json.dumps(record) + "\n")
        except OSError:
            pass


def _floats(bits) -> np.ndarray:
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def _ulp(ref: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(ref.astype(np.float64)))


def _knife(ref: np.ndarray) -> np.ndarray:
    """Judged from the reference alone: ref within KNIFE_ULPS float64 ulp of the midpoint of two float32 neighbours."""
    return f32_knife_edge(ref, KNIFE_ULPS * _ulp(ref))


def _check_domain(ctx, bits: np.ndarray, what: str) -> dict:
    """The three assertions on arguments inside [1, inf); returns the per-exponent maxima of the float64 error."""
    x = _floats(bits)
    ref = np.log(x.astype(LD))
    ulp = _ulp(ref)
    want32 = ref.astype(np.float32)
    knife = _knife(ref)
    out64, out32 = ctx.debug_log_f32(x, lds_table=False)
    lds64, lds32 = ctx.debug_log_f32(x, lds_table=True)
    err = (np.abs(out64.astype(LD) - ref) / ulp).astype(np.float64)  # (x == 1: 0 / the smallest subnormal)
    exps = (bits >> 23).astype(np.int64) - 127
    order = np.argsort(exps, kind="stable")
    starts = np.flatnonzero(np.diff(exps[order], prepend=-1))
    per_exp = {int(exps[order[s]]): float(v) for s, v in zip(starts, np.maximum.reduceat(err[order], starts))}
    worst = int(np.argmax(err))
    wrong32 = np.flatnonzero((out32 != want32) & ~knife)
    _log(dict(what=what, n=int(x.size), max_ulp=float(err[worst]), max_ulp_exponent=int(exps[worst]),
              max_ulp_bits=f"0x{int(bits[worst]):08X}", bound=ULP_BOUND, knife_edges=int(knife.sum()),
              float32_mismatches_off_the_knife_edges=int(wrong32.size),
              lds_out64_differs=int((out64.view(np.uint64) != lds64.view(np.uint64)).sum()),
              max_ulp_per_exponent={str(k): round(v, 4) for k, v in per_exp.items()}))
    assert np.array_equal(out64.view(np.uint64), lds64.view(np.uint64))
    assert np.array_equal(out32.view(np.uint32), lds32.view(np.uint32))
    assert err.max() <= ULP_BOUND, (float(err[worst]), hex(int(bits[worst])))
    assert wrong32.size == 0, [hex(int(b)) for b in bits[wrong32[:8]]]
    assert knife.sum() <= KNIFE_CAP, int(knife.sum())
    return dict(bits=bits, out64=out64, out32=out32, ref=ref, err=err)


def test_every_mantissa_at_exponent_0(ctx):
    """2(a): the 2^23 arguments of [1, 2), both table forms: out64 the same bits, within 2 ulp of the 80-bit log,
    out32 == float32(reference) off the knife-edges (at most 4 of them); log(1) is exactly 0 and the neighbour of 1
    is within 1 ulp (table entry 0 is exact: values next to 1 keep their relative accuracy)."""
    bits = np.arange(0x3F800000, 0x40000000, dtype=np.uint32)
    r = _check_domain(ctx, bits, "exponent 0, every mantissa")
    assert r["out64"][0] == 0.0 and not np.signbit(r["out64"][0])
    assert r["out32"][0] == 0.0 and not np.signbit(r["out32"][0])
    assert _floats(bits[1:2])[0] == np.nextafter(np.float32(1), np.float32(2))
    assert r["err"][1] <= 1.0, float(r["err"][1])
    assert r["err"].max() <= 1.1  # the bound at e = 0, where nothing is added to T + p


def test_every_other_exponent_sampled_and_at_the_table_edges(ctx):
    """2(b): exponents 1 ... 127, every 128th mantissa and the table-interval edges (mant = i << 16 and its two
    neighbours, inside the exponent): the three assertions of 2(a)."""
    edges = np.arange(129, dtype=np.int64) << 16
    mant = np.concatenate([np.arange(0, 1 << 23, 128, dtype=np.int64), edges - 1, edges, edges + 1])
    mant = np.unique(mant[(mant >= 0) & (mant < (1 << 23))])
    assert mant.size == 65536 + 2 * 128  # (i << 16 is on the grid of 128; -1 and 2^23 fall outside)
    bits = (((np.arange(1, 128, dtype=np.int64) + 127) << 23)[:, None] | mant[None, :]).reshape(-1)
    bits = bits[bits < 0x7F800000].astype(np.uint32)
    assert bits.size == 127 * mant.size and bits[-1] == LAST
    _check_domain(ctx, bits, "exponents 1 ... 127, every 128th mantissa and the table edges")


def test_every_float32_of_the_domain_against_the_device_library(ctx):
    """2(c): one launch per table form over all 1 073 741 824 arguments of [1, inf).  Two logs within 2 ulp and 1 ulp
    of the truth round to different float32 values only where the truth lies within 2 ulp of a float32 midpoint
    (2^-27 of the arguments: about 8), so the list of 4096 must not fill up, every listed argument must be such a
    knife-edge by the host's 80-bit log, and the largest float64 difference is at most 3 ulp."""
    runs = {lds: ctx.debug_log_f32_sweep(FIRST, LAST, lds_table=lds, capacity=SWEEP_CAPACITY) for lds in (False, True)}
    plain, lds = runs[False], runs[True]
    listed = plain["bits"]
    ref = np.log(_floats(listed).astype(LD))
    knife = _knife(ref)
    _log(dict(what="sweep of [1, inf) against the device library's log", n=LAST - FIRST + 1,
              mismatches=plain["count"], mismatch_bits=[f"0x{int(b):08X}" for b in listed[:64]],
              mismatches_off_the_knife_edges=int((~knife).sum()), max_ulps=plain["max_ulps"],
              max_ulps_bits=f"0x{plain['max_bits']:08X}", bound=SWEEP_BOUND, lds_mismatches=lds["count"],
              lds_max_ulps=lds["max_ulps"], lds_max_ulps_bits=f"0x{lds['max_bits']:08X}"))
    assert LAST - FIRST + 1 == 1 << 30  # 128 exponents of 2^23 mantissas
    assert plain["count"] <= SWEEP_CAPACITY and listed.size == plain["count"], plain["count"]
    assert lds["count"] == plain["count"] and np.array_equal(lds["bits"], listed)
    assert (lds["max_ulps"], lds["max_bits"]) == (plain["max_ulps"], plain["max_bits"])
    assert knife.all(), [hex(int(b)) for b in listed[~knife][:8]]
    assert 0.0 < plain["max_ulps"] <= SWEEP_BOUND, (plain["max_ulps"], hex(plain["max_bits"]))
    assert FIRST <= plain["max_bits"] <= LAST


def test_sweep_bookkeeping_on_parts_of_a_range(ctx):
    """The sweep's own bookkeeping (count, list order, per-workgroup maximum and its argument), which needs no
    reference: a range of 2^24 arguments across an exponent boundary gives the sum, the concatenation and the maximum
    of its three uneven parts (the smallest argument on a tie); a part shorter than a workgroup and the single
    argument 1 work; and the maximum over a short range agrees with |out64 - log| recomputed on the host from the
    element entry, up to the 2 ulp two library logs may lie apart."""
    first, last = 0x47FEFED3, 0x48FEFED2
    cuts = [first, first + 100, first + 100 + 5_000_001, last + 1]
    whole = ctx.debug_log_f32_sweep(first, last, lds_table=True)
    parts = [ctx.debug_log_f32_sweep(a, b - 1, lds_table=True) for a, b in zip(cuts[:-1], cuts[1:])]
    assert whole["count"] == sum(p["count"] for p in parts) <= SWEEP_CAPACITY
    assert np.array_equal(whole["bits"], np.concatenate([p["bits"] for p in parts]))
    assert np.all(np.diff(whole["bits"].astype(np.int64)) > 0)
    best = max(parts, key=lambda p: (p["max_ulps"], -p["max_bits"]))
    assert (whole["max_ulps"], whole["max_bits"]) == (best["max_ulps"], best["max_bits"]) and whole["max_ulps"] > 0
    for p, a, b in zip(parts, cuts[:-1], cuts[1:]):
        assert a <= p["max_bits"] < b and np.all((p["bits"] >= a) & (p["bits"] < b))

    one = ctx.debug_log_f32_sweep(FIRST, FIRST, capacity=0)
    assert (one["count"], one["bits"].size, one["max_ulps"], one["max_bits"]) == (0, 0, 0.0, FIRST)

    bits = np.arange(first, first + 70_001, dtype=np.uint32)
    short = ctx.debug_log_f32_sweep(int(bits[0]), int(bits[-1]))
    out64, _ = ctx.debug_log_f32(_floats(bits))
    host = np.log(_floats(bits).astype(np.float64))
    assert abs(short["max_ulps"] - (np.abs(out64 - host) / np.spacing(host)).max()) <= 2.0


def _rare_arguments() -> dict:
    rng = np.random.default_rng(20)
    f = np.float32
    # (0, 1): half of them uniform in the bit pattern (every exponent), half uniform in the value
    unit = np.concatenate([rng.integers(0x00800000, 0x3F800000, 2048, dtype=np.uint32).view(f),
                           np.maximum(rng.random(2047, dtype=np.float32), f(2.0 ** -24))])
    sub = np.concatenate([np.array([1, 2, 0x007FFFFF, 0x00400000], np.uint32),
                          rng.integers(1, 0x00800000, 60, dtype=np.uint32)]).view(np.float32)
    neg = np.concatenate([np.array([-np.inf, -1.0, -0.5, -2.0, -np.finfo(f).max, -np.finfo(f).tiny], f),
                          np.array([0x80000001, 0x807FFFFF], np.uint32).view(f),
                          -(rng.random(56, dtype=np.float32) + f(1e-3)) * f(10) ** rng.integers(-30, 30, 56).astype(f)])
    return {
        "one": np.array([1.0], f),
        "inf": np.array([np.inf], f),
        "nan": np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001], np.uint32).view(f),
        "negative": neg,
        "zero": np.array([0.0, -0.0], f),
        "subnormal": sub,
        "unit": np.concatenate([unit, np.array([np.nextafter(f(1), f(0))], f)]),
    }


def test_dispatch_and_the_out_of_line_routine(ctx):
    """2(d): out32 on 1 (+0.0), +inf (+inf), NaN and every negative value (NaN), the zeros (-inf), subnormals and
    4 096 values of (0, 1), nextafter(1, 0) among them, against float32(np.log(float64(x))), both table forms.
    NaN, -inf and +inf are compared bit for bit, the NaNs passed through from NaN arguments included; the default NaN
    that a negative argument produces is the same but for its sign bit, which no rule defines (x86: 0xFFC00000, the
    device: 0x7FC00000; both sides' patterns are logged).  Finite values are equal off the knife-edges of 2(a),
    judged from the 80-bit log."""
    args = _rare_arguments()
    assert args["unit"].size == 4096 and np.all((args["unit"] > 0) & (args["unit"] < 1))
    assert np.all(args["negative"] < 0) and np.all((args["subnormal"] > 0) & (args["subnormal"] < np.finfo(np.float32).tiny))
    x = np.concatenate(list(args.values()))
    with np.errstate(all="ignore"):
        want = np.log(x.astype(np.float64)).astype(np.float32)
        ref = np.log(x.astype(LD))
    out64, out32 = ctx.debug_log_f32(x, lds_table=False)
    lds64, lds32 = ctx.debug_log_f32(x, lds_table=True)
    finite = np.isfinite(want)
    knife = np.zeros(x.size, bool)
    knife[finite] = _knife(ref[finite])
    _log(dict(what="dispatch and rare path", n=int(x.size), finite=int(finite.sum()), knife_edges=int(knife.sum()),
              float32_mismatches_off_the_knife_edges=int(((out32 != want) & finite & ~knife).sum()),
              device_nan_bits=sorted({f"0x{int(b):08X}" for b in out32.view(np.uint32)[np.isnan(out32)]}),
              host_nan_bits=sorted({f"0x{int(b):08X}" for b in want.view(np.uint32)[np.isnan(want)]})))
    assert np.array_equal(out32.view(np.uint32), lds32.view(np.uint32))
    assert np.array_equal(out64.view(np.uint64), lds64.view(np.uint64))
    at, got = 0, {}
    for name, v in args.items():
        got[name] = out32[at:at + v.size]
        at += v.size
    assert got["one"].view(np.uint32)[0] == 0  # +0.0
    assert got["inf"].view(np.uint32)[0] == 0x7F800000
    assert np.isnan(got["nan"]).all() and np.isnan(got["negative"]).all()
    assert np.all(got["zero"].view(np.uint32) == 0xFF800000)
    assert np.isfinite(got["subnormal"]).all() and np.isfinite(got["unit"]).all() and np.all(got["unit"] < 0)
    # ... and all of them against the reference
    assert np.array_equal(np.isnan(out32), np.isnan(want))
    # NaN, -inf, +inf: bit for bit - but for the sign of a NaN that the log MAKES (negative arguments: an invalid
    # operation), which IEEE 754 leaves to the platform: x86 makes 0xFFC00000, the device 0x7FC00000 (measured)
    special, made = ~finite, x < 0
    got_bits, want_bits = out32.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got_bits[special & ~made], want_bits[special & ~made])
    assert np.array_equal(got_bits[made] & 0x7FFFFFFF, want_bits[made] & 0x7FFFFFFF)
    assert np.all(got_bits[made] & 0x7FFFFFFF == 0x7FC00000)
    assert np.isfinite(out32[finite]).all()
    assert np.all((out32 == want) | knife | ~finite)
    assert knife.sum() <= KNIFE_CAP
    # out64 is defined inside [1, inf) only: the log there, NaN elsewhere
    inside = (x >= 1) & (x < np.inf)
    assert np.isnan(out64[~inside]).all() and out64[x == 1][0] == 0.0


def test_no_values_and_the_refusals(ctx):
    """n = 0 returns without touching the outputs; NULL pointers, n < 0 and first_bits > last_bits are refused with
    ADH_ERR_INVALID_ARGUMENT, as is a sweep that leaves [1, inf), where the float64 log is not defined."""
    from alphadia_amd import runtime

    lib, h = runtime.lib, ctx._h
    o64, o32 = ctx.debug_log_f32(np.zeros(0, np.float32), lds_table=True)
    assert o64.shape == (0,) and o64.dtype == np.float64 and o32.shape == (0,) and o32.dtype == np.float32
    x, out64, out32 = np.full(4, 2.0, np.float32), np.full(4, -7.0), np.full(4, -7.0, np.float32)
    px, p64, p32 = (x.ctypes.data_as(C.POINTER(C.c_float)), out64.ctypes.data_as(C.POINTER(C.c_double)),
                    out32.ctypes.data_as(C.POINTER(C.c_float)))
    assert lib.adh_debug_log_f32(h, px, 0, 0, p64, p32) == 0
    assert np.all(out64 == -7.0) and np.all(out32 == -7.0)
    invalid = -1  # ADH_ERR_INVALID_ARGUMENT
    assert lib.adh_debug_log_f32(None, px, 4, 0, p64, p32) == invalid
    assert lib.adh_debug_log_f32(h, None, 4, 0, p64, p32) == invalid
    assert lib.adh_debug_log_f32(h, px, 4, 0, None, p32) == invalid
    assert lib.adh_debug_log_f32(h, px, 4, 1, p64, None) == invalid
    assert lib.adh_debug_log_f32(h, px, -1, 0, p64, p32) == invalid
    assert np.all(out64 == -7.0) and np.all(out32 == -7.0)
    assert lib.adh_debug_log_f32(h, px, 4, 0, p64, p32) == 0 and np.all(out32 == np.float32(np.log(2.0)))

    bits = np.zeros(8, np.uint32)
    pb = bits.ctypes.data_as(C.POINTER(C.c_uint32))
    n, ulps, at = C.c_int64(-5), C.c_double(-5.0), C.c_uint32(5)
    good = (h, FIRST, FIRST + 1000, 0, C.byref(n), pb, 8, C.byref(ulps), C.byref(at))
    for pos, bad in ((0, None), (4, None), (5, None), (7, None), (8, None), (6, -1)):
        a = list(good)
        a[pos] = bad
        assert lib.adh_debug_log_f32_sweep(*a) == invalid, pos
    for first, last in ((FIRST + 1, FIRST), (FIRST - 1, FIRST), (0, LAST), (FIRST, LAST + 1), (LAST + 1, 0xFFFFFFFF)):
        a = list(good)
        a[1], a[2] = first, last
        assert lib.adh_debug_log_f32_sweep(*a) == invalid, (first, last)
    assert (n.value, ulps.value, at.value) == (-5, -5.0, 5) and not bits.any()
    assert lib.adh_debug_log_f32_sweep(*good) == 0 and n.value >= 0
    with pytest.raises(runtime.HipBackendError, match="first_bits > last_bits"):
        ctx.debug_log_f32_sweep(FIRST + 1, FIRST)
    with pytest.raises(runtime.HipBackendError, match="negative count"):
        runtime._check(lib.adh_debug_log_f32(h, px, -1, 0, p64, p32), "adh_debug_log_f32")
