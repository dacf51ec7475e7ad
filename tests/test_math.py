"""include/pdmpc_math.h (the sin/cos shared by oracle and kernel) against libm."""
import numpy as np

from oracle import oracle


def ulp_diff(a, b):
    a = np.asarray(a, dtype=np.float64).view(np.int64)
    b = np.asarray(b, dtype=np.float64).view(np.int64)
    a = np.where(a < 0, np.int64(-(2**63)) - a, a)
    b = np.where(b < 0, np.int64(-(2**63)) - b, b)
    return np.abs(a - b)


def test_sincos_within_one_ulp_of_libm():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.uniform(-np.pi, np.pi, 200000),
        rng.uniform(-100, 100, 200000),
        rng.uniform(-1e5, 1e5, 100000),
        np.linspace(-7, 7, 20001),
        np.array([0.0, -0.0, np.pi / 4, np.pi / 2, np.pi, 1e-300, 1e-10, 2.0**-27, 2.0**-28]),
    ])
    s, c = oracle.sincos(x)
    assert ulp_diff(s, np.sin(x)).max() <= 1
    assert ulp_diff(c, np.cos(x)).max() <= 1
    assert np.abs(s * s + c * c - 1).max() < 4e-16


def test_sincos_special_values():
    s, c = oracle.sincos(np.array([0.0, -0.0, np.inf, -np.inf, np.nan]))
    assert s[0] == 0 and c[0] == 1 and np.signbit(s[1]) and c[1] == 1
    assert np.isnan(s[2:]).all() and np.isnan(c[2:]).all()


def test_sincos_symmetry():
    x = np.random.default_rng(1).uniform(-50, 50, 10000)
    s1, c1 = oracle.sincos(x)
    s2, c2 = oracle.sincos(-x)
    assert np.array_equal(s1, -s2) and np.array_equal(c1, c2)


def test_the_sets_reach_every_stage_of_the_reduction():
    """what the tests below and the device comparison (tests/test_gpu_edge_check_limits.py) are aimed at: the doubles nearest a multiple
    of pi/2 take all three stages, their perturbed copies exactly two, and the set of the libm test the first and none"""
    import sincos_cases as S

    near = S.near_multiples()
    assert near.size == 6 * (S.N_MAX - 1) and np.abs(near).max() < S.N_MAX * np.pi / 2
    assert (S.reduction_stage(S.nearest_multiples(np.arange(1, S.N_MAX))) == 3).all()
    assert (S.reduction_stage(near) == 3).mean() > 0.99
    two = S.second_stage(np.random.default_rng(5), 200000)
    assert (S.reduction_stage(two) == 2).sum() > 150000 and np.abs(two).max() < S.N_MAX * np.pi / 2
    assert set(np.unique(S.reduction_stage(S.libm_set()))) >= {0, 1}
    assert (S.reduction_stage(S.specials()[:-3]) == 0).all()  # up to pi/4 (by the high word: a little beyond it too) nothing is reduced


def test_sincos_within_one_ulp_of_a_200_bit_reference():
    """The header's own claim, error < 1 ulp, against mpmath at 200 bits (libm is itself only good to an ulp): on a seeded sample of the
    libm test's set, of the arguments of exactly two reduction stages and of the doubles nearest a multiple of pi/2 with their neighbours,
    and on the members of the last with the smallest |sin| and the smallest |cos|, where the reduction has the least to spare.  The worst
    seen is 0.73 ulp (the libm set; 0.66 on two stages, 0.50 on the near-multiples); only |x| < 2^20 * pi/2 is promised (include/pdmpc_math.h)."""
    import mpmath as mp

    import sincos_cases as S

    mp.mp.prec = 240
    rng = np.random.default_rng(6)
    near = S.near_multiples()
    two = S.second_stage(rng, 20000)
    two = two[S.reduction_stage(two) == 2]
    s_near, c_near = oracle.sincos(near)
    smallest = np.concatenate([near[np.argsort(np.abs(s_near), kind="stable")[:300]], near[np.argsort(np.abs(c_near), kind="stable")[:300]]])
    x = np.concatenate([rng.choice(S.libm_set(), 1500), rng.choice(two, 1500), rng.choice(near, 3000), smallest, S.specials()[:-3]])
    s, c = oracle.sincos(x)
    worst = 0.0
    for xi, si, ci in zip(x.tolist(), s.tolist(), c.tolist()):
        exact = mp.mpf(xi)
        worst = max(worst, S.ulps_from_exact(si, mp.sin(exact), mp), S.ulps_from_exact(ci, mp.cos(exact), mp))
    print("worst error of pdmpc_sincos: %.4f ulp over %d arguments" % (worst, x.size))
    assert worst < 1.0
