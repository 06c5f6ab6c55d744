"""ok_sincosf_pair (include/okenv_math.h) is, by definition, two calls of ok_sincosf: the same 32 bits in all four results, for every
pair of arguments, on the host and on the device.  The step kernels evaluate the agent's heading and the lane's ray angle through it
in every step, so every position, hit point and crash flag stands on this.

Both sides of each comparison come from the same place (okenv_debug_math on the host, or on the device), so nothing is excused: no
tolerance, NaN payloads included, the share of differing elements is 0.  The sets:
  self, partner_second, partner_first   every 256th float bit pattern (tests/_math_cases.py: 2^24 values, every binade of both signs,
                  subnormals, NaNs) paired with itself, and with a fixed ordinary partner in either slot;
  half_pi         every float within 4 ulps of k * pi/2, k = 1 .. 64, and of the floats below 2^31 that lie unusually close to a
                  multiple of pi/2 (the convergents tests/test_math.py uses), paired with itself and with the partner in either slot;
  special         the cross product of +-0, the ends of the subnormal range, +-Inf, NaN, 2^31 and its two neighbours of both signs,
                  larger values and ordinary ones.  The second argument runs fastest, so neighbouring lanes of a wave differ in whether
                  their pair needs the rare branch."""
import functools

import numpy as np
import pytest

import _math_cases as M

f32 = np.float32
PARTNER = f32(1.2345)  # finite, far below 2^31: never takes the rare branch itself
CASES = ("self", "partner_second", "partner_first", "half_pi", "special")


@functools.lru_cache(maxsize=None)
def special_values():
    two31 = np.array([0x4EFFFFFF, 0x4F000000, 0x4F000001], dtype=np.uint32).view(f32)  # 2^31 - 128, 2^31, 2^31 + 256
    pos = np.concatenate([[0.0, float(M.SUB_MIN), float(M.SUB_MAX), float(M.FLT_MIN), np.inf], two31,
                          [3.0e9, 1.0e30, float(M.FLT_MAX)], [0.5, 1.5707964, 2.5, 100.0, 12345.678]]).astype(f32)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001], dtype=np.uint32).view(f32)
    return np.concatenate([pos, -pos, nan])


@functools.lru_cache(maxsize=None)
def pairs(case):
    """(a, b) of one case, read-only"""
    if case in ("self", "partner_second", "partner_first"):
        s = M.all_floats_strided()
        p = np.full(s.shape, PARTNER, dtype=f32)
        a, b = {"self": (s, s), "partner_second": (s, p), "partner_first": (p, s)}[case]
    elif case == "half_pi":
        n = M.around(np.concatenate([np.arange(1, 65) * (np.pi / 2), M.half_pi_convergents().astype(np.float64)]), ulps=4)
        p = np.full(n.shape, PARTNER, dtype=f32)
        a, b = np.concatenate([n, n, p]), np.concatenate([n, p, n])
    else:
        v = special_values()
        a, b = np.repeat(v, v.size), np.tile(v, v.size)
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


_single = {}


def two_calls(ok, x, device):
    """ok_sincosf over x as [n, 2] (sine, cosine); the strided set and the partner are evaluated once per process and device"""
    if x is M.all_floats_strided():
        sn, cs = M.evaluate(ok, "sincos", device)  # (the sincos set of tests/_math_cases.py begins with the strided floats)
        assert np.array_equal(M.bits(M.unary_set("sincos")[:x.size]), M.bits(x))
        return np.stack([sn[:x.size], cs[:x.size]], axis=1)
    if x.size and (M.bits(x) == M.bits(x[:1])).all():  # the partner, n times
        if device not in _single:
            _single[device] = ok.debug_math("sincos", x[:1], device=device)
        sn, cs = _single[device]
        return np.stack([np.repeat(sn, x.size), np.repeat(cs, x.size)], axis=1)
    sn, cs = ok.debug_math("sincos", x, device=device)
    return np.stack([sn, cs], axis=1)


def check(ok, case, device):
    a, b = pairs(case)
    got_a, got_b = ok.debug_math("sincos_pair", a, b, device=device)
    rare = ~((np.abs(a) < f32(2147483648.0)) & (np.abs(b) < f32(2147483648.0)))
    print("%s on %s: %d pairs, %d of them through the rare branch" % (case, "the host" if device == M.ON_HOST else "device %d" % device, a.size, int(rare.sum())))
    for what, got, x in (("first", got_a, a), ("second", got_b, b)):
        want = two_calls(ok, x, device)
        bad = np.flatnonzero((M.bits(got).reshape(-1, 2) != M.bits(want).reshape(-1, 2)).any(axis=1))
        lines = ["  (0x%08X, 0x%08X): pair 0x%08X 0x%08X, two calls 0x%08X 0x%08X" % (int(M.bits(a)[i]), int(M.bits(b)[i]), *(int(w) for w in M.bits(got[i])),
                                                                                       *(int(w) for w in M.bits(want[i]))) for i in bad[:5]]
        assert bad.size == 0, "%s, %s argument: %d of %d pairs differ\n%s" % (case, what, bad.size, a.size, "\n".join(lines))


def test_sets_hold_what_they_promise():
    v = special_values()
    assert np.isin(np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x4EFFFFFF, 0x4F000000, 0x4F000001, 0xCF000000],
                            dtype=np.uint32), M.bits(v)).all() and np.isnan(v).any()
    a, b = pairs("special")
    need = ~((np.abs(a) < f32(2147483648.0)) & (np.abs(b) < f32(2147483648.0)))
    assert (need[1:] != need[:-1]).sum() > v.size  # lanes next to each other on both sides of the rare branch, many times over
    a, b = pairs("half_pi")
    for k in (1, 2, 3, 64):
        centre = M.keys(np.array([k * np.pi / 2], dtype=np.float64).astype(f32))[0]
        assert np.isin(M.from_keys(centre + np.arange(-4, 5)).view(np.uint32), M.bits(a)).all()
    assert pairs("self")[0].size == 1 << 24


@pytest.mark.parametrize("case", CASES)
def test_pair_equals_two_calls_on_the_host(ok, case):
    check(ok, case, M.ON_HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_pair_equals_two_calls_on_the_device(gpu, case):
    check(gpu, case, 0)
