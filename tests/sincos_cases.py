"""Arguments for include/pdmpc_math.h's pdmpc_sincos, aimed at each stage of its Cody-Waite reduction, all inside the documented range
|x| < 2^20 * pi/2.  Shared by tests/test_math.py (host compile against a 200-bit reference) and tests/test_gpu_edge_check_limits.py
(device compile against host compile, bit for bit)."""
import numpy as np

N_MAX = 1 << 20
PIO2 = np.longdouble("1.57079632679489661923132169163975144209858")


def libm_set():
    """the arguments of tests/test_math.py::test_sincos_within_one_ulp_of_libm"""
    rng = np.random.default_rng(0)
    return np.concatenate([
        rng.uniform(-np.pi, np.pi, 200000),
        rng.uniform(-100, 100, 200000),
        rng.uniform(-1e5, 1e5, 100000),
        np.linspace(-7, 7, 20001),
        np.array([0.0, -0.0, np.pi / 4, np.pi / 2, np.pi, 1e-300, 1e-10, 2.0**-27, 2.0**-28]),
    ])


def nearest_multiples(n):
    """the double nearest to n * pi/2 (n an integer array below 2^20: the extended-precision product is good to far below a double's
    rounding step; the rare tie it could misjudge is covered by the neighbours near_multiples adds)"""
    return (np.asarray(n).astype(np.longdouble) * PIO2).astype(np.float64)


def near_multiples():
    """every double nearest to n * pi/2, 0 < n < 2^20, its two neighbours, and the negatives of all three: these cancel all of the
    argument's leading bits and take the reduction's third stage"""
    x = nearest_multiples(np.arange(1, N_MAX))
    x = np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])
    return np.concatenate([x, -x])


def second_stage(rng, count):
    """arguments that leave between 17 and 49 bits cancelled, n * pi/2 * (1 +- 2^-k): candidates for exactly two stages (reduction_stage
    says which of them are)"""
    n = rng.integers(1, N_MAX, count)
    k = rng.integers(18, 48, count)
    x = nearest_multiples(n) * (1.0 + rng.choice([-1.0, 1.0], count) * 2.0 ** (-k.astype(np.float64)))
    return x * rng.choice([-1.0, 1.0], count)


def specials():
    tiny = np.array([0.0, 5e-324, 2.5e-320, 2.2250738585072014e-308 / 2, 2.2250738585072014e-308, 1e-300, 2.0**-28, np.nextafter(2.0**-27, 0), 2.0**-27, np.nextafter(2.0**-27, 1),
                     2.0**-26, np.nextafter(np.pi / 4, 0), np.pi / 4, np.nextafter(np.pi / 4, 1)])
    return np.concatenate([tiny, -tiny, [np.inf, -np.inf, np.nan]])


def _exponent(v):
    return ((v.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)


def reduction_stage(x):
    """How many stages of pdmpc_rem_pio2 an argument takes (0: |x| <= pi/4, no reduction), from the header's own criterion — the exponent
    lost between the argument and the reduced value, more than 16 bits after one stage, more than 49 after two — in numpy doubles.  It
    sorts arguments; it checks nothing."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    t = np.abs(x)
    hi = (t.view(np.uint64) >> np.uint64(32)).astype(np.int64)
    fn = np.floor(t * 6.36619772367581382433e-01 + 0.5)
    r = t - fn * 1.57079632673412561417e+00
    w = fn * 6.07710050650619224932e-11
    j = hi >> 20
    i1 = j - _exponent(r - w)
    t2 = r
    w2 = fn * 6.07710050630396597660e-11
    r2 = t2 - w2
    w2 = fn * 2.02226624879595063154e-21 - ((t2 - r2) - w2)
    i2 = j - _exponent(r2 - w2)
    stage = np.where(i1 > 16, np.where(i2 > 49, 3, 2), 1)
    return np.where(hi <= 0x3FE921FB, 0, stage)


def ulps_from_exact(got, exact_mpf, mp):
    """|got - exact| in units of the exact value's last place as a double (2^-52 of its binade; a denormal's place is 2^-1074)"""
    if exact_mpf == 0:
        return 0.0 if got == 0 else float("inf")
    e = max(int(mp.floor(mp.log(abs(exact_mpf), 2))) - 52, -1074)
    return float(abs(mp.mpf(float(got)) - exact_mpf) / mp.mpf(2) ** e)
