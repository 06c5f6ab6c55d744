"""The argument sets of tests/_math_cases.py hold what they promise, and the host compilation of include/okenv_math.h and of
ok_learn_adam (okenv_debug_math / okenv_debug_adam_device with OKENV_DEBUG_ON_HOST) already meets, on those very sets, every bar
tests/test_gpu_math.py applies to the device: so a failure there is the device's.  No GPU needed.

The shares of not correctly rounded results printed here (run with -s) are the ones tests/test_gpu_math.py doubles; docs/HISTORY.md
records them."""
import numpy as np
import pytest

import _math_cases as M

f32 = np.float32
HOST = M.ON_HOST


def has(a, values):
    return np.isin(np.asarray(values, dtype=np.float64).astype(f32).view(np.uint32), M.bits(a)).all()


def binades(a):
    """the (sign, biased exponent) pairs present"""
    u = M.bits(a)
    return set(np.unique(u >> np.uint32(23)).tolist())


def test_strided_floats_cover_every_binade_of_both_signs():
    a = M.all_floats_strided()
    assert a.size == 1 << 24 and np.unique(M.bits(a)).size == a.size and ((M.bits(a) & 0xFF) == 0x5B).all()
    assert binades(a) == set(range(512))  # exponents 0 (subnormals) .. 255 (NaNs) of both signs
    assert np.isnan(a).sum() == 2 * (1 << 15) and not np.isinf(a).any()
    assert a is M.all_floats_strided() and not a.flags.writeable
    b = M.all_floats_strided(16)
    assert b.size == 1 << 16 and binades(b) == set(range(512))
    s = M.specials()
    assert has(s, [0.0, np.inf, -np.inf, float(M.FLT_MAX), float(M.SUB_MIN)]) and (M.bits(s) == 0x80000000).any() and np.isnan(s).sum() == 4


def test_around_holds_both_sides_of_both_signs():
    a = M.around([1.0, 0.0, float(M.FLT_MAX)], ulps=4096)
    for centre in (1.0, -1.0, 0.0):
        k = M.keys(np.array([centre], dtype=f32))[0]
        assert np.isin(M.from_keys(k + np.arange(-4096, 4097)).view(np.uint32), M.bits(a)).all()
    assert (M.bits(a) == 0x80000000).any() and (M.bits(a) == 0).any()                  # both zeros
    assert np.isinf(a).sum() == 2 and not np.isnan(a).any()                           # clipped at the infinities, never beyond
    assert a.size == 2 * 8193 + 8194 + 2 * 4098 and np.unique(M.bits(a)).size == a.size
    assert M.around([3.0], ulps=1).tolist() == [-3.000000238418579, -3.0, -2.999999761581421, 2.999999761581421, 3.0, 3.000000238418579]


def required_neighbours(points, reach):
    """every float within `reach` ulps of +-v for each v, written out point by point: sorted keys, each once"""
    inf_key = 0x7F800000
    step = np.arange(-reach, reach + 1, dtype=np.int64)
    parts = []
    for v in np.asarray(points, dtype=np.float64).astype(f32):
        for s in (v, -v):
            parts.append(np.clip(M.keys(np.array([s], dtype=f32))[0] + step, -inf_key, inf_key))
    return np.unique(np.concatenate(parts))


@pytest.mark.parametrize("fn", ["tanh", "exp", "log", "sincos", "normalize_angle", "expert_normalize_angle"])
def test_unary_sets_hold_their_branch_points(fn):
    a = M.unary_set(fn)
    normaliser = "normalize" in fn
    reach = 64 if normaliser else 4096
    points = {"tanh": M.tanh_points, "exp": M.exp_points, "log": M.log_points, "sincos": M.sincos_points, "normalize_angle": M.normalize_points,
              "expert_normalize_angle": M.normalize_points}[fn]()
    # the set is the strided floats, then the neighbourhoods, then the special values
    strided = M.all_floats_strided(16 if normaliser else 8)
    special = M.specials()
    assert np.array_equal(M.bits(a[: strided.size]), M.bits(strided)) and np.array_equal(M.bits(a[-special.size:]), M.bits(special))
    assert binades(strided) == set(range(512))
    near = a[strided.size: a.size - special.size]
    want = required_neighbours(points, reach)
    have = np.unique(M.keys(near))
    assert np.isin(want, have, assume_unique=True).all() if fn == "sincos" else np.array_equal(want, have)
    assert want.size >= points.size * reach  # the neighbourhoods overlap only where the points are close
    if fn == "tanh":
        assert points.size == 61 and has(near, [2.0 ** -12, 20.0, -20.0])
        # a half-integer of -2|x| / ln 2 lies strictly inside the reach of every tie point
        for k in (0, 29, 58):
            close = M.around([points[2 + k]]).astype(np.float64)
            q = 2.0 * close[close > 0] / M.LN2
            assert q.min() < k + 0.5 < q.max()
    if fn == "exp":
        assert points.size == 6 + 280
        # each landmark's neighbourhood holds results on both sides of it: 0 | subnormal, the smallest subnormal | the next,
        # subnormal | normal, finite | infinite
        def results(x):
            with np.errstate(all="ignore"):
                return np.exp(M.around([x]).astype(np.float64)[: 2 * 4096 + 1] if x < 0 else M.around([x]).astype(np.float64)[-(2 * 4096 + 1):]).astype(f32)
        r = results(-103.98)
        assert (r == 0).any() and (r == M.SUB_MIN).any()
        r = results(-103.28)
        assert (r == M.SUB_MIN).all()  # exp(-103.28) is the smallest subnormal itself
        r = results(-87.34)
        assert ((r > 0) & (r < M.FLT_MIN)).any() and (r >= M.FLT_MIN).any()
        r = results(88.72)
        assert np.isinf(r).any() and np.isfinite(r).any()
    if fn == "log":
        assert points.size == 5 + 2 * 277
    if fn == "sincos":
        c = M.half_pi_convergents()
        assert c.size > 400 and (c > 0).sum() == (c < 0).sum() and np.isin(required_neighbours(c[c > 0], 2), have, assume_unique=True).all()
        assert np.abs(c).max() < 2.0 ** 31 and (np.abs(c) > 2.0e6).any()
        # how close they get to a multiple of pi/2, in exact arithmetic
        from fractions import Fraction
        rmin = min(abs(Fraction(float(v)) - round(Fraction(float(v)) / (M.PI / 2)) * (M.PI / 2)) for v in c[c > 0])
        assert rmin < Fraction(1, 10 ** 8)
        assert (np.abs(a) >= f32(2.0 ** 31)).sum() > 1 << 20  # the fmod path
    if normaliser:
        assert has(near, 360.0 * np.array([1, -1, 4095, 4096, 4097, -4096, 65535, 65536, 65537, -65536])) and has(near, [2.0 ** 24, 2.0 ** 30, 2.0 ** 34])
        big = f32(2.0 ** 34)
        assert big + f32(360.0) == big and f32(2.0 ** 30) + f32(360.0) == f32(2.0 ** 30 + 384.0) and f32(2.0 ** 24) + f32(360.0) == f32(2.0 ** 24 + 360.0)


def test_convergents_equal_the_high_precision_set_of_test_math():
    """The same floats as tests/test_math.py builds with 60 digits, where mpmath is installed."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    xs = set()
    for e in range(-30, 8):
        a, k0, k1 = mp.mpf(2) ** e / (mp.pi / 2), 1, 0
        for _ in range(40):
            ai = int(mp.floor(a))
            k0, k1 = k1, ai * k1 + k0
            if k1 >= (1 << 24):
                break
            if k1 > 0 and 0 < float(k1) * 2.0 ** e < 2147483648.0:
                xs.add(f32(float(k1) * 2.0 ** e))
            if a - ai == 0:
                break
            a = 1 / (a - ai)
    c = M.half_pi_convergents()
    assert sorted(xs) == c[c > 0].tolist()


def test_atan2_pairs_are_the_cross_product():
    v = M.atan2_floats()
    y, x = M.atan2_pairs()
    assert 2000 < v.size < 3500 and y.size == x.size == v.size ** 2 and np.unique(M.bits(v)).size == v.size
    assert has(v, [0.0, np.inf, -np.inf, float(M.SUB_MIN), -float(M.SUB_MIN), float(M.FLT_MIN), float(M.FLT_MAX), -float(M.FLT_MAX)])
    assert (M.bits(v) == 0x80000000).any() and np.isnan(v).sum() == 1
    assert has(v, 2.0 ** np.arange(-140, 128, 10).astype(np.float64))
    assert np.array_equal(M.bits(y.reshape(v.size, v.size)[:, 3]), M.bits(v)) and np.array_equal(M.bits(x[: v.size]), M.bits(v))
    # the fold threshold is crossed, the diagonal met, in every octant
    ok_ = ~(np.isnan(y) | np.isnan(x) | np.isinf(y) | np.isinf(x)) & (x != 0) & (y != 0)
    ay, ax = np.abs(y[ok_]).astype(np.float64), np.abs(x[ok_]).astype(np.float64)
    q = np.minimum(ay, ax) / np.maximum(ay, ax)
    just = np.abs(q - M.TAN_PI_8) < 4e-6
    assert (q[just] > M.TAN_PI_8).sum() > 1000 and (q[just] <= M.TAN_PI_8).sum() > 1000 and (ay == ax).sum() > 4000
    for centre in (1.0, M.TAN_PI_8, -3.0):
        k = M.keys(np.array([centre], dtype=np.float64).astype(f32))[0]
        assert np.isin(M.from_keys(k + np.arange(-8, 9)).view(np.uint32), M.bits(v)).all()


def test_adam_cases_are_the_product():
    p, m, v, g = M.adam_cases()
    assert p.size == 5 * 5 * 6 * 17 and all(a.size == p.size and a.dtype == f32 for a in (m, v, g))
    assert len(set(zip(M.bits(p).tolist(), M.bits(m).tolist(), M.bits(v).tolist(), M.bits(g).tolist()))) == p.size
    assert np.isnan(g).any() and np.isinf(g).any() and (g == M.SUB_MIN).any() and (g == -M.SUB_MIN).any()
    g32 = g[np.isfinite(g)]
    with np.errstate(all="ignore"):
        sq = g32 * g32
    assert np.isinf(sq).any() and ((sq > 0) & (sq < M.FLT_MIN)).any() and (sq[g32 != 0] == 0).any()
    assert (v == M.SUB_MIN).any() and (np.abs(m) == f32(1e-40)).any() and (np.abs(p) == f32(3e38)).any()
    assert M.ADAM_STEPS == (1, 2, 1000, 10 ** 6) and [hp["eps"] for hp in M.ADAM_PARAMS] == [1e-8, 0.0]


# ---- the host evaluation meets the device's bars ----------------------------------------------------------------------------

@pytest.mark.parametrize("fn", ["sincos", "tanh", "exp", "log", "atan2"])
def test_host_is_within_one_ulp_of_fp64(ok, fn):
    for share in M.rounding_shares(ok, fn, HOST):
        assert share <= M.HOST_SHARE_BAR[fn], (fn, share)


@pytest.mark.parametrize("fn", ["normalize_angle", "expert_normalize_angle"])
def test_host_normalisers_equal_the_restated_loops(ok, fn):
    M.check_normaliser(ok, fn, HOST)


def test_host_entry_equals_the_older_host_entries(ok):
    """okenv_debug_math on the host is the function the older, per-function debug entries evaluate."""
    for fn, old in (("exp", ok.debug_expf), ("log", ok.debug_logf), ("expert_normalize_angle", ok.debug_expert_normalize_angle)):
        a = M.unary_set(fn)[::64]
        M.assert_same_bits(fn, ok.debug_math(fn, a, device=HOST), old(a), a)
    y, x = M.atan2_pairs()
    M.assert_same_bits("atan2", ok.debug_math("atan2", y[::64], x[::64], device=HOST), ok.debug_atan2f(y[::64], x[::64]), y[::64], x[::64])


def test_host_tanh_and_sincos_equal_the_oracle(ok, oracle):
    """The oracle compiles the header a second time, on its own: a second witness for the two functions it exports."""
    a = M.unary_set("tanh")[::16]
    t = np.zeros_like(a)
    oracle.lib().oracle_tanhf(np.ascontiguousarray(a), t, a.size)
    M.assert_same_bits("tanh", ok.debug_math("tanh", a, device=HOST), t, a)
    a = M.unary_set("sincos")[::16]
    s, c = np.zeros_like(a), np.zeros_like(a)
    oracle.lib().oracle_sincosf(np.ascontiguousarray(a), s, c, a.size)
    hs, hc = ok.debug_math("sincos", a, device=HOST)
    M.assert_same_bits("sin", hs, s, a)
    M.assert_same_bits("cos", hc, c, a)


def test_host_atan2_table(ok):
    M.check_atan2_table(ok, HOST)


def test_host_symmetry(ok):
    M.check_symmetry(ok, HOST)


def test_host_error_codes(ok):
    M.check_error_codes(ok, HOST)


def test_host_adam(ok):
    M.check_adam_fp64(ok, HOST)
    p, m, v, g = M.adam_cases()
    for t in M.ADAM_STEPS:  # with the examples' eps it is okenv_debug_adam's evaluation
        got = M.run_adam(ok, M.ADAM_PARAMS[0], t, HOST)
        want = ok.debug_adam(ok.capi.learner_params(**M.ADAM_PARAMS[0]), t, p, m, v, g)
        for name, a, b in zip("pmv", got, want):
            M.assert_same_bits("Adam " + name, a, b, p, m, v, g)
