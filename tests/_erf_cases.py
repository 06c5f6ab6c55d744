"""The argument set and the reference of ok_erff's tests (include/okenv_math.h): every 256th float, the neighbourhoods of 0, of the
first subnormal, of the branch points 1, 2, 3 and 4 and of the first argument whose result is 1, the specials; math.erf, which is
within an ulp of fp64, rounded to fp32."""
import functools
import math

import numpy as np

import _math_cases as M

f32 = np.float32
BRANCH_POINTS = (1.0, 2.0, 3.0, 4.0)


@functools.lru_cache(maxsize=None)
def first_one():
    """The smallest fp32 argument whose erf rounds to 1.0f: bisection over the floats of [3, 4] (erf is monotone)."""
    lo, hi = (int(k) for k in M.keys(np.array([3.0, 4.0], f32)))
    assert f32(math.erf(3.0)) < 1 and f32(math.erf(4.0)) == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f32(math.erf(float(M.from_keys(np.array([mid]))[0]))) == 1:
            hi = mid
        else:
            lo = mid
    return float(M.from_keys(np.array([hi]))[0])


@functools.lru_cache(maxsize=None)
def erf_set():
    points = (0.0, float(M.SUB_MIN)) + BRANCH_POINTS + (first_one(),)
    return M._frozen(np.concatenate([M.all_floats_strided(), M.around(points), M.specials()]))


@functools.lru_cache(maxsize=None)
def reference():
    """math.erf of every argument, rounded once to fp32 (NaN for NaN).  math.erf is called where it has something to say, 2^-28 <=
    |x| < 4 (an eighth of the set).  Below, erf x = 2 x / sqrt(pi) (1 - x^2 / 3 + ...) is the fp64 product 2 x / sqrt(pi) to the last
    place; from first_one() on it rounds to +-1 because erf is monotone."""
    with np.errstate(invalid="ignore", under="ignore"):
        a = erf_set().astype(np.float64)
        out = np.full(a.shape, np.nan)
        mag = np.abs(a)
        small, large = mag < 2.0 ** -28, mag >= 4.0
        mid = ~small & ~large & (a == a)
        out[small] = a[small] * (2.0 / math.sqrt(math.pi))
        out[large] = np.sign(a[large])
        out[mid] = np.frompyfunc(math.erf, 1, 1)(a[mid]).astype(np.float64)
        return M._frozen(out.astype(f32))


def evaluate(okmod, device):
    return okmod.debug_math("erf", erf_set(), device=device)
