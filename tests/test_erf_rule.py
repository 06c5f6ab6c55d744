"""ok_erff (include/okenv_math.h) on the host entry: within one ulp of math.erf rounded to fp32 on every 256th float and around 0, the
first subnormal, every branch point and the first argument whose result is 1 -- the bound that an fp64 evaluation rounded once has;
odd in the bits; the special values.  No GPU needed."""
import numpy as np

import _erf_cases as E
import _math_cases as M

f32 = np.float32


def test_erf_is_within_one_ulp_of_fp64(ok):
    a, want = E.erf_set(), E.reference()
    got = E.evaluate(ok, M.ON_HOST)
    finite = a == a
    assert np.isnan(got[~finite]).all() and not np.isnan(got[finite]).any()
    dist = M.ulp_distance(got[finite], want[finite])
    unequal = int((dist != 0).sum())
    # recorded, not asserted: what this printed when it was written is in the comment of ok_erff's test in DESIGN.md section 30
    print("ok_erff: %d of %d arguments not equal to the rounded math.erf; largest distance %d ulp" % (unequal, int(finite.sum()), int(dist.max())))
    worst = int(np.argmax(dist))
    assert int(dist.max()) <= 1, "erf(%r) = %r, math.erf rounds to %r" % (float(a[finite][worst]), float(got[finite][worst]), float(want[finite][worst]))
    assert E.first_one() > 3.8 and float(ok.debug_math("erf", np.array([E.first_one()], f32), device=M.ON_HOST)[0]) == 1.0


def test_erf_is_odd_in_the_bits(ok):
    a = E.erf_set()[::16]
    neg = (M.bits(a) ^ np.uint32(0x80000000)).view(f32)
    plus, minus = ok.debug_math("erf", a, device=M.ON_HOST), ok.debug_math("erf", neg, device=M.ON_HOST)
    finite = a == a
    M.assert_same_bits("erf(-x) against -erf(x)", minus[finite], (M.bits(plus[finite]) ^ np.uint32(0x80000000)).view(f32), a[finite])


def test_erf_special_values(ok):
    a = np.array([0.0, -0.0, np.inf, -np.inf, 4.0, -4.0, 1e30, -1e30], f32)
    got = ok.debug_math("erf", a, device=M.ON_HOST)
    M.assert_same_bits("erf at the zeros, the infinities and beyond the last branch point", got, np.array([0.0, -0.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0], f32), a)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32).view(f32)
    out = ok.debug_math("erf", nan, device=M.ON_HOST)
    assert np.isnan(out).all()
    sub = np.array([M.SUB_MIN, -M.SUB_MIN, M.SUB_MAX, M.FLT_MIN], f32)  # erf x = 2 x / sqrt(pi) there, rounded once
    M.assert_same_bits("erf of subnormals", ok.debug_math("erf", sub, device=M.ON_HOST), (sub.astype(np.float64) * 1.1283791670955126).astype(f32), sub)
