"""include/okenv_math.h and ok_learn_adam compiled for the device, over their whole argument range (the sets of tests/_math_cases.py):
the same bits as the host compilation, within one ulp of float64, odd and even where the function is.  Every learner, actor, expert
and controller test compares a device kernel with a host entry built from these functions; this is the floor they stand on.
tests/test_math_cases.py applies the same checks to the host evaluation without a GPU."""
import numpy as np
import pytest

import _math_cases as M

pytestmark = pytest.mark.gpu
HOST = M.ON_HOST


def both(gpu, fn):
    dev, host = M.evaluate(gpu, fn, 0), M.evaluate(gpu, fn, HOST)
    args = M.atan2_pairs() if fn == "atan2" else (M.unary_set(fn),)
    return dev, host, args


@pytest.mark.parametrize("fn", ["tanh", "exp", "log", "atan2", "normalize_angle", "expert_normalize_angle"])
def test_device_equals_host(gpu, fn):
    dev, host, args = both(gpu, fn)
    M.assert_same_bits("%s, device against host" % fn, dev, host, *args)


def test_device_equals_host_sincos(gpu):
    dev, host, args = both(gpu, "sincos")
    M.assert_same_bits("sine, device against host", dev[0], host[0], *args)
    M.assert_same_bits("cosine, device against host", dev[1], host[1], *args)


@pytest.mark.parametrize("fn", ["sincos", "tanh", "exp", "log", "atan2"])
def test_device_is_within_one_ulp_of_fp64(gpu, fn):
    """Never more than one ulp from the rounded fp64 value, and not that value on at most twice the share of the set on which the
    host evaluation is not (measured here, on the same set; tests/test_math_cases.py holds the host's share under its bar)."""
    host = M.rounding_shares(gpu, fn, HOST)
    dev = M.rounding_shares(gpu, fn, 0)
    for h, d in zip(host, dev):
        assert d <= 2.0 * h, (fn, d, h)


@pytest.mark.parametrize("fn", ["normalize_angle", "expert_normalize_angle"])
def test_device_normalisers_equal_the_restated_loops(gpu, fn):
    M.check_normaliser(gpu, fn, 0)


def test_device_atan2_table(gpu):
    M.check_atan2_table(gpu, 0)


def test_device_symmetry(gpu):
    M.check_symmetry(gpu, 0)


def test_device_error_codes(gpu):
    M.check_error_codes(gpu, 0)


def test_device_adam_equals_host(gpu):
    p, m, v, g = M.adam_cases()
    for hp in M.ADAM_PARAMS:
        for t in M.ADAM_STEPS:
            dev, host = M.run_adam(gpu, hp, t, 0), M.run_adam(gpu, hp, t, HOST)
            for name, a, b in zip("pmv", dev, host):
                M.assert_same_bits("Adam %s, t = %d, eps = %g, device against host" % (name, t, hp["eps"]), a, b, p, m, v, g)
            finite = np.isfinite(p) & np.isfinite(m) & np.isfinite(v) & np.isfinite(g)
            for a, b in zip(dev, host):  # no NaN from finite inputs unless the host gives one
                assert not (np.isnan(a) & ~np.isnan(b) & finite).any()


def test_device_adam_against_fp64(gpu):
    M.check_adam_fp64(gpu, 0)
