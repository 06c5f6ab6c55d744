"""Argument sets for the leaf functions of include/okenv_math.h and for ok_learn_adam (include/okenv_learn.h), and the comparisons
tests/test_math_cases.py (host, no GPU) and tests/test_gpu_math.py (device) apply to them.  Every set is deterministic (fixed seeds, no
clock), built once per process and returned read-only.

What a set costs decides its size.  The transcendental functions take about 30 ns per element on the host, so they get every 256th
float (2^24 values) plus every float within 4096 ulps of each branch point their source names.  The two angle normalisers are
loops: a float beyond 360 * 65536 costs ok_normalize_angle_deg its full 65536 dependent additions (about 100 us on the host), and
two fifths of all floats are such.  They therefore get every 65536th float (2^16 values, all binades of both signs still present)
and 64 ulps around their branch points: about 30 000 full-length loops, a few seconds on the host, instead of 7 million."""
import functools
from fractions import Fraction

import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(f32).max
FLT_MIN = np.finfo(f32).tiny
SUB_MIN = f32(1.401298464324817e-45)               # the smallest subnormal, bits 0x00000001
SUB_MAX = np.array([0x007FFFFF], np.uint32).view(f32)[0]  # the largest subnormal
TAN_PI_8 = 0.41421356237309503                     # ok_atan2f's fold threshold, 0x1.a827999fcef32p-2
LN2 = 0.6931471805599453
# pi to 50 digits: exact rational arithmetic for the convergents below needs more than a double
PI = Fraction("3.14159265358979323846264338327950288419716939937510")

FNS = ("sincos", "tanh", "exp", "log", "atan2", "normalize_angle", "expert_normalize_angle")


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def keys(a):
    """fp32 -> int64, monotone in the value: adjacent floats have adjacent keys; +0 and -0 share key 0."""
    i = np.ascontiguousarray(a, dtype=f32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def from_keys(k):
    k = np.asarray(k, dtype=np.int64)
    u = np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32)
    return u.view(f32)


def ulp_distance(a, b):
    return np.abs(keys(a) - keys(b))


@functools.lru_cache(maxsize=None)
def all_floats_strided(low_bits=8):
    """Every fp32 bit pattern whose low `low_bits` bits are those of 0x5B5B (0x5B for the default 8): 2^(32 - low_bits) values, both
    signs, every binade, subnormals and NaNs.  The zeros and the infinities end in zero bits and are not among them: specials()."""
    low = 0x5B5B & ((1 << low_bits) - 1)
    u = (np.arange(1 << (32 - low_bits), dtype=np.uint64) << np.uint64(low_bits)) | np.uint64(low)
    return _frozen(u.astype(np.uint32).view(f32))


def specials():
    """What no stride reaches: the zeros, the infinities, the ends of the subnormal and normal ranges, quiet and signalling-pattern NaNs."""
    pos = np.array([0.0, SUB_MIN, SUB_MAX, FLT_MIN, 1.0, FLT_MAX, np.inf], dtype=f32)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFBFFFFF], dtype=np.uint32).view(f32)
    return np.concatenate([pos, -pos, nan])


def around(values, ulps=4096):
    """Every float within `ulps` ulps of each listed value and of its negative (clipped at the infinities), sorted, each once; -0 is
    added wherever +0 is in reach."""
    v = np.asarray(values, dtype=np.float64).astype(f32)
    v = v[v == v]
    centre = keys(np.concatenate([v, -v]))
    inf_key = 0x7F800000
    k = np.unique(np.clip(centre[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :], -inf_key, inf_key))
    out = from_keys(k)
    if (k == 0).any():
        out = np.concatenate([out, np.array([-0.0], dtype=f32)])
    return out


# ---- the branch points each function's source names ---------------------------------------------------------------------------

def tanh_points():
    """|x| = 2^-12 (the identity exit), 20 (the clamp), and (k + 1/2) ln 2 / 2 for k = 0 .. 58, where -2|x| / ln 2 is a half-integer:
    the ties of rint for n = 0 .. -58."""
    return np.concatenate([[2.0 ** -12, 20.0], (np.arange(0, 59) + 0.5) * LN2 / 2.0])


def exp_points():
    """0, the clamps +-200, the results' landmarks (-103.98: the last 0; -103.28: the smallest subnormal; -87.34: the largest
    subnormal; 88.72: the first infinity) and the ties (k + 1/2) ln 2 of rint for k = -151 .. 128."""
    return np.concatenate([[0.0, 200.0, -103.98, -103.28, -87.34, 88.72], (np.arange(-151, 129) + 0.5) * LN2])


def log_points():
    """1, 2^k and sqrt 2 * 2^k for k = -149 .. 127 (the binade edges and the mantissa's halving), 1e-8 (the clamp of the probability),
    the ends of the subnormal range and FLT_MAX."""
    k = np.arange(-149, 128).astype(np.float64)
    return np.concatenate([[1.0, 1e-8, float(SUB_MIN), float(SUB_MAX), float(FLT_MAX)], 2.0 ** k, np.sqrt(2.0) * 2.0 ** k])


def sincos_points():
    """2^31 (the fmod path begins there) and k * pi/2 for k = 1 .. 64."""
    return np.concatenate([[2147483648.0], np.arange(1, 65) * (np.pi / 2)])


def normalize_points():
    """0, 360, 360 k for k next to the two caps (4096 and 65536 turns), 2^24 (the last binade in which x + 360 is exact), 2^30 (x + 360
    is x + 384 there) and 2^34 (x + 360 is x)."""
    return np.concatenate([[0.0, 360.0, 2.0 ** 24, 2.0 ** 30, 2.0 ** 34], 360.0 * np.array([1, 4095, 4096, 4097, 65535, 65536, 65537])])


@functools.lru_cache(maxsize=None)
def half_pi_convergents():
    """The floats x = q * 2^e (q < 2^24) below 2^31 that lie unusually close to a multiple of pi/2: q runs over the denominators of
    the continued-fraction convergents of 2^e / (pi/2), e = -30 .. 7 (the set of tests/test_math.py, here in exact rational
    arithmetic from 50 digits of pi, which is ample: the convergents with q < 2^24 depend on about 2^-48 of the quotient).  Both signs."""
    xs = set()
    for e in range(-30, 8):
        a = Fraction(2) ** e / (PI / 2)
        k0, k1 = 1, 0
        for _ in range(40):
            ai = a.numerator // a.denominator
            k0, k1 = k1, ai * k1 + k0
            if k1 >= (1 << 24):
                break
            if k1 > 0:
                x = float(k1) * 2.0 ** e
                if 0 < x < 2147483648.0:
                    xs.add(f32(x))
            frac = a - ai
            if frac == 0:
                break
            a = 1 / frac
    x = np.array(sorted(xs), dtype=f32)
    return _frozen(np.concatenate([x, -x]))


@functools.lru_cache(maxsize=None)
def unary_set(fn):
    """The whole argument set of one unary function."""
    if fn == "tanh":
        parts = [all_floats_strided(), around(tanh_points())]
    elif fn == "exp":
        parts = [all_floats_strided(), around(exp_points())]
    elif fn == "log":
        parts = [all_floats_strided(), around(log_points())]
    elif fn == "sincos":
        parts = [all_floats_strided(), around(sincos_points()), around(half_pi_convergents(), ulps=2)]
    elif fn in ("normalize_angle", "expert_normalize_angle"):
        parts = [all_floats_strided(16), around(normalize_points(), ulps=64)]
    else:
        raise KeyError(fn)
    return _frozen(np.concatenate(parts + [specials()]))


@functools.lru_cache(maxsize=None)
def atan2_floats():
    """The floats whose full cross product atan2_pairs() is: the zeros, the infinities, a NaN, the ends of the subnormal and normal
    ranges, 2^k for every tenth k, 64 random mantissas (in random binades), and for 32 base values v the floats v +- 0 .. 8 ulps and
    v tan(pi/8) +- 0 .. 8 ulps, which put the quotient on both sides of the fold threshold and on the diagonal; all of both signs."""
    rng = np.random.default_rng(20250)
    edge = np.array([0.0, np.inf, float(SUB_MIN), float(FLT_MIN), float(FLT_MAX)], dtype=f32)
    pow2 = (2.0 ** np.arange(-140, 128, 10).astype(np.float64)).astype(f32)
    rand = (rng.integers(1, 254, 64).astype(np.uint32) << np.uint32(23) | rng.integers(0, 1 << 23, 64).astype(np.uint32)).view(f32)
    # bases: binades from deep in the subnormal quotient's reach to near overflow, with random mantissas; 1 and 3 for round numbers
    base = np.concatenate([[1.0, 3.0], 2.0 ** rng.integers(-120, 120, 30) * rng.uniform(1.0, 2.0, 30)]).astype(f32)
    step = np.arange(-8, 9, dtype=np.int64)
    near_v = from_keys(keys(base)[:, None] + step[None, :]).ravel()
    near_t = from_keys(keys((base.astype(np.float64) * TAN_PI_8).astype(f32))[:, None] + step[None, :]).ravel()
    pos = np.unique(np.concatenate([edge, pow2, rand, near_v, near_t]))
    return _frozen(np.concatenate([pos, -pos, np.array([np.nan], dtype=f32)]))


@functools.lru_cache(maxsize=None)
def atan2_pairs():
    """(y, x): the cross product of atan2_floats() with itself."""
    v = atan2_floats()
    return _frozen(np.repeat(v, v.size)), _frozen(np.tile(v, v.size))


ADAM_STEPS = (1, 2, 1000, 10 ** 6)
# the examples' hyper-parameters (examples/ppo_racer.py and the others: lr 3e-4 with torch.optim.Adam's defaults) and the same with eps = 0
ADAM_PARAMS = (dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8), dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=0.0))


@functools.lru_cache(maxsize=None)
def adam_cases():
    """(p, m, v, g): the product of the four lists, flattened.  g * g is subnormal at 1e-20 and below, overflows at 1.9e19."""
    mag = np.array([1e-45, 1e-30, 1e-20, 1e-19, 1.0, 1e19, 1.9e19])
    g = np.concatenate([[0.0], mag, -mag, [np.inf, np.nan]]).astype(f32)
    v = np.array([0.0, 1e-45, 1e-38, 1e-20, 1.0, 3e38], dtype=f32)
    m = np.array([0.0, 1e-40, -1e-40, 1.0, -1.0], dtype=f32)
    p = np.array([0.0, 1.0, -1.0, 3e38, -3e38], dtype=f32)
    P, M, V, G = np.meshgrid(p, m, v, g, indexing="ij")
    return tuple(_frozen(a.ravel()) for a in (P, M, V, G))


# ---- comparisons ---------------------------------------------------------------------------------------------------------------

def same_bits(got, want):
    """True where the two fp32 arrays hold the same 32 bits, or both hold a NaN (payloads are not compared: x + y propagates them
    differently on x86-64 and on gfx950, and the rule does not define them)."""
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def assert_same_bits(what, got, want, *args):
    """No element differs; otherwise the count and the first five arguments with both results in hex."""
    bad = np.flatnonzero(~same_bits(got, want))
    if bad.size:
        lines = ["%s: %d of %d elements differ" % (what, bad.size, np.size(got))]
        for i in bad[:5]:
            shown = ", ".join("%r (0x%08X)" % (float(a[i]), int(bits(a)[i])) for a in args)
            lines.append("  at %s: 0x%08X against 0x%08X" % (shown, int(bits(got)[i]), int(bits(want)[i])))
        raise AssertionError("\n".join(lines))


def rounding_report(what, got, want):
    """Against an fp64 reference rounded once to fp32: (largest distance in ulps, share of elements that differ).  NaN where the
    reference is NaN counts as equal, NaN on one side only as infinitely far."""
    g, w = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    both_nan = np.isnan(g) & np.isnan(w)
    one_nan = np.isnan(g) != np.isnan(w)
    d = np.where(both_nan, 0, np.where(one_nan, 1 << 40, ulp_distance(g, w)))
    worst = int(d.max()) if d.size else 0
    differing = int((d != 0).sum())
    share = differing / d.size if d.size else 0.0
    print("%s: %d elements, %d not the rounded fp64 value (share %.3g), largest distance %d ulp" % (what, d.size, differing, share, worst))
    if worst > 1:
        i = int(np.argmax(d))
        print("  worst at element %d of the selection: got 0x%08X, want 0x%08X" % (i, int(bits(g)[i]), int(bits(w)[i])))
    return worst, share


def normalize_restated(x, turns, expert):
    """The two capped loops of ok_normalize_angle_deg (turns = 65536) / ok_expert_normalize_angle_deg (turns = 4096, and 0 for what
    does not end in [0, 360)), one np.float32 addition per turn.  An element that a turn leaves unchanged (x + 360 == x, a NaN, or
    the loop's condition false) can never change in that loop again, so it leaves the working set: what remains are the few
    thousand floats between 2^25 and 2^33 that really take every turn."""
    a = np.array(x, dtype=f32, copy=True)
    for sign, cond in ((f32(360.0), lambda v: v < f32(360.0)), (f32(-360.0), lambda v: v >= f32(360.0))):
        live = np.flatnonzero(cond(a))
        for _ in range(turns):
            if live.size == 0:
                break
            with np.errstate(all="ignore"):
                nxt = a[live] + sign
            moved = nxt != a[live]
            a[live] = nxt
            live = live[moved & cond(nxt)]
    if expert:
        a = np.where((a >= f32(0.0)) & (a < f32(360.0)), a, f32(0.0)).astype(f32)
    return a


# ---- the checks, for a host or a device evaluation alike ------------------------------------------------------------------------

ON_HOST = -1
_results = {}


def evaluate(ok, fn, device):
    """fn over its whole set through okenv_debug_math, once per process and device: the result, or (sine, cosine)."""
    key = (fn, device)
    if key not in _results:
        if fn == "atan2":
            y, x = atan2_pairs()
            _results[key] = ok.debug_math(fn, y, x, device=device)
        else:
            _results[key] = ok.debug_math(fn, unary_set(fn), device=device)
    return _results[key]


# the largest share of not correctly rounded results the host evaluation may show: the bars tests/test_math.py (sine, cosine, tanh),
# tests/test_actor_rule.py (exp) and tests/test_reinforce_rule.py (log) already apply to random samples.  ok_atan2f had none: its
# polynomial is good to 2^-52.7 and the fp64 operations around it add a few 2^-53, so the fp64 value is within about 2^-50 of the
# truth and rounds differently only where the truth lies within 2^-50 of a rounding boundary of fp32 (2^-24 apart): one argument in
# 2^25 or so.  1e-5 leaves two orders of magnitude for arguments that are not spread evenly.
HOST_SHARE_BAR = {"sincos": 1e-5, "tanh": 1e-4, "exp": 1e-5, "log": 1e-5, "atan2": 1e-5}


def fp64_reference(fn):
    """(indices of the elements an fp64 reference is valid for, the fp64 references of those elements, one per output); once per process."""
    if fn not in _references:
        with np.errstate(all="ignore"):
            if fn == "atan2":
                y, x = atan2_pairs()
                sel = np.flatnonzero(~(np.isnan(y) | np.isnan(x)))
                refs = [np.arctan2(y[sel].astype(np.float64), x[sel].astype(np.float64))]
            else:
                a = unary_set(fn)
                if fn == "tanh":
                    sel = np.flatnonzero(np.isfinite(a))
                elif fn == "exp":
                    sel = np.flatnonzero((a >= f32(-200.0)) & (a <= f32(88.7)))
                elif fn == "log":
                    sel = np.flatnonzero((a > 0) & np.isfinite(a))
                else:
                    # numpy's fp64 sine is trusted up to 2e6 and away from the multiples of pi/2 the convergents sit on (tests/test_math.py)
                    sel = np.flatnonzero((np.abs(a) <= f32(2.0e6)) & ~np.isin(a, around(half_pi_convergents(), ulps=2)))
                a64 = a[sel].astype(np.float64)
                refs = {"tanh": lambda: [np.tanh(a64)], "exp": lambda: [np.exp(a64)], "log": lambda: [np.log(a64)],
                        "sincos": lambda: [np.sin(a64), np.cos(a64)]}[fn]()
            # rounded ONCE to fp32, subnormal results included
            _references[fn] = (sel, [r.astype(f32) for r in refs])
    return _references[fn]


_references = {}


def rounding_shares(ok, fn, device):
    """Check 2 for one transcendental function: never more than one ulp from the rounded fp64 value.  Returns the shares of elements
    that are not that value, one per output."""
    got = evaluate(ok, fn, device)
    got = list(got) if isinstance(got, tuple) else [got]
    sel, refs = fp64_reference(fn)
    shares = []
    for k, (g, r) in enumerate(zip(got, refs)):
        worst, share = rounding_report("%s[%d] on %s" % (fn, k, "the host" if device == ON_HOST else "device %d" % device), g[sel], r)
        assert worst <= 1, (fn, k, worst)
        shares.append(share)
    return shares


def check_normaliser(ok, fn, device):
    """Check 2 for the two normalisers: the bits of the restated loops."""
    a = unary_set(fn)
    expert = fn == "expert_normalize_angle"
    want = normalize_restated(a, 4096 if expert else 65536, expert)
    assert_same_bits(fn + " against the restated loops", evaluate(ok, fn, device), want, a)


def atan2_table():
    """C99 F.9.1.4, every row, as (y, x, result); y > 0 and x finite stand for 1, FLT_MAX and the smallest subnormal."""
    pi = np.pi
    rows = []
    for s in (1.0, -1.0):  # the sign of y, and of the result
        z = s * 0.0
        rows += [(z, -0.0, s * pi), (z, 0.0, z), (s * np.inf, -np.inf, s * 3 * pi / 4), (s * np.inf, np.inf, s * pi / 4)]
        for w in (1.0, float(FLT_MAX), float(SUB_MIN)):
            rows += [(z, -w, s * pi), (z, w, z), (s * w, 0.0, s * pi / 2), (s * w, -0.0, s * pi / 2), (s * w, -np.inf, s * pi), (s * w, np.inf, z),
                     (s * np.inf, w, s * pi / 2), (s * np.inf, -w, s * pi / 2)]
        rows += [(s * np.inf, 0.0, s * pi / 2), (s * np.inf, -0.0, s * pi / 2)]
    t = np.array(rows, dtype=np.float64)
    return t[:, 0].astype(f32), t[:, 1].astype(f32), t[:, 2].astype(f32)


def check_atan2_table(ok, device):
    y, x, want = atan2_table()
    assert_same_bits("atan2 at the zeros and infinities (C99 F.9.1.4)", ok.debug_math("atan2", y, x, device=device), want, y, x)


def check_symmetry(ok, device):
    """Check 3: tanh and sine are odd, cosine is even, atan2 is odd in y -- in the bits, the sign of zero included."""
    neg = lambda v: (bits(v) ^ np.uint32(0x80000000)).view(f32)  # flips the sign bit and nothing else, of zeros and NaNs too
    for fn in ("tanh", "sincos"):
        a = unary_set(fn)[::16]
        plus, minus = ok.debug_math(fn, a, device=device), ok.debug_math(fn, neg(a), device=device)
        if fn == "tanh":
            assert_same_bits("tanh(-x) against -tanh(x)", minus, neg(plus), a)
        else:
            assert_same_bits("sin(-x) against -sin(x)", minus[0], neg(plus[0]), a)
            assert_same_bits("cos(-x) against cos(x)", minus[1], plus[1], a)
    y, x = atan2_pairs()
    y, x = y[::7], x[::7]  # 7 and the set's size are coprime: every y meets a seventh of the x
    assert_same_bits("atan2(-y, x) against -atan2(y, x)", ok.debug_math("atan2", neg(y), x, device=device), neg(ok.debug_math("atan2", y, x, device=device)), y, x)


def check_error_codes(ok, device):
    """Check 4: what both entries refuse, and that an empty call is fine.  No call here reaches a kernel."""
    L, ptr = ok.capi.load(), ok.capi.ptr
    a, o0, o1 = np.zeros(4, f32), np.zeros(4, f32), np.zeros(4, f32)
    INVALID = -1
    nfn = len(ok.capi.DEBUG_FNS)
    assert L.okenv_debug_math(device, -1, ptr(a), ptr(a), ptr(o0), ptr(o1), 4) == INVALID
    assert L.okenv_debug_math(device, nfn, ptr(a), ptr(a), ptr(o0), ptr(o1), 4) == INVALID
    assert L.okenv_debug_math(device, FNS.index("atan2"), ptr(a), None, ptr(o0), None, 4) == INVALID
    assert L.okenv_debug_math(device, FNS.index("sincos"), ptr(a), None, ptr(o0), None, 4) == INVALID
    for fn in range(nfn):
        assert L.okenv_debug_math(device, fn, None, ptr(a), ptr(o0), ptr(o1), 4) == INVALID
        assert L.okenv_debug_math(device, fn, ptr(a), ptr(a), None, ptr(o1), 4) == INVALID
        assert L.okenv_debug_math(device, fn, ptr(a), ptr(a), ptr(o0), ptr(o1), -1) == INVALID
        assert L.okenv_debug_math(device, fn, ptr(a), ptr(a), ptr(o0), ptr(o1), 0) == 0
    assert b"okenv_debug_math" in L.okenv_last_error(None)
    # b and out1 are not needed by the other functions
    assert L.okenv_debug_math(device, FNS.index("tanh"), ptr(a), None, ptr(o0), None, 0) == 0
    import ctypes as C
    hp = ok.capi.learner_params()
    p, m, v, g = (np.zeros(4, f32) for _ in range(4))
    adam = L.okenv_debug_adam_device
    assert adam(device, C.byref(hp), 0, ptr(p), ptr(m), ptr(v), ptr(g), 4) == INVALID
    assert adam(device, C.byref(hp), -5, ptr(p), ptr(m), ptr(v), ptr(g), 4) == INVALID
    assert adam(device, None, 1, ptr(p), ptr(m), ptr(v), ptr(g), 4) == INVALID
    for hole in range(4):
        args = [ptr(p), ptr(m), ptr(v), ptr(g)]
        args[hole] = None
        assert adam(device, C.byref(hp), 1, *args, 4) == INVALID
    assert adam(device, C.byref(hp), 1, ptr(p), ptr(m), ptr(v), ptr(g), -1) == INVALID
    assert adam(device, C.byref(ok.capi.learner_params(eps=-1.0)), 1, ptr(p), ptr(m), ptr(v), ptr(g), 4) == INVALID
    assert b"okenv_debug_adam_device" in L.okenv_last_error(None)
    assert adam(device, C.byref(hp), 1, ptr(p), ptr(m), ptr(v), ptr(g), 0) == 0
    assert adam(device, C.byref(ok.capi.learner_params(eps=0.0)), 1, ptr(p), ptr(m), ptr(v), ptr(g), 0) == 0
    assert not p.any() and not o0.any()


# ---- Adam ----------------------------------------------------------------------------------------------------------------------

def adam_consts(hp, t):
    """ok_learn_adam_consts as okLearnAdamConsts makes them: fp64 from the fp32 hyper-parameters, the power by repeated squaring, each
    rounded once."""
    def powi(b, n):
        r = 1.0
        while n > 0:
            if n & 1:
                r = r * b
            b = b * b
            n >>= 1
        return r
    b1, b2, lr, eps = (float(f32(hp[k])) for k in ("beta1", "beta2", "lr", "eps"))
    return dict(beta1=b1, beta2=b2, eps=eps, omb1=float(f32(1.0 - b1)), omb2=float(f32(1.0 - b2)),
                step=float(f32(lr / (1.0 - powi(b1, t)))), bc2=float(f32(np.sqrt(1.0 - powi(b2, t)))))


def adam_fp64(hp, t):
    """The formula of include/okenv_learn.h in float64 from the fp32 inputs, with a bound on what the fp32 evaluation may differ by.
    Returns (p, m, v, bound_p, bound_m, bound_v, valid).  u = 2^-24 is the relative error of one fp32 operation, to first order:
      m:   two products and a sum                      |dm| <= u (|beta1 m| + |omb1 g| + |m'|)
      v:   three products and a sum of terms >= 0      |dv| <= 4 u v'
      root = sqrt(v'): 2u from v', u of its own; den = root / bc2 + eps, terms >= 0: 5u
      q = m' / den:    |dq| <= |dm| / den + 6u |q|;   upd = step q: |dupd| <= step |dq| + u |upd|;   p' = p - upd: + u |p'|
    and 2 % on top for the second-order terms.  `valid`: every intermediate finite and, unless exactly zero, normal in fp32."""
    c = adam_consts(hp, t)
    p, m, v, g = (a.astype(np.float64) for a in adam_cases())
    u = 2.0 ** -24
    with np.errstate(all="ignore"):
        m1, m2 = c["beta1"] * m, c["omb1"] * g
        mn = m1 + m2
        v1, w, = c["beta2"] * v, c["omb2"] * g
        v2 = w * g
        vn = v1 + v2
        root = np.sqrt(vn)
        scaled = root / c["bc2"]
        den = scaled + c["eps"]
        q = mn / den
        upd = c["step"] * q
        pn = p - upd
        dm = u * (np.abs(m1) + np.abs(m2) + np.abs(mn))
        dv = 4 * u * vn
        dq = dm / den + 6 * u * np.abs(q)
        dp = c["step"] * dq + u * np.abs(upd) + u * np.abs(pn)
        valid = np.ones(p.shape, dtype=bool)
        for x in (m1, m2, mn, v1, w, v2, vn, root, scaled, den, q, upd, pn):
            ax = np.abs(x)
            valid &= np.isfinite(x) & ((x == 0) | ((ax >= 2 * float(FLT_MIN)) & (ax <= 0.5 * float(FLT_MAX))))
        valid &= den > 0
    return pn, mn, vn, 1.02 * dp, 1.02 * dm, 1.02 * dv, valid


def run_adam(ok, hp, t, device):
    p, m, v, g = adam_cases()
    return ok.debug_adam_device(ok.capi.learner_params(**hp), t, p, m, v, g, device=device)


def check_adam_fp64(ok, device):
    p0, m0, v0, g0 = adam_cases()
    seen = 0
    for hp in ADAM_PARAMS:
        for t in ADAM_STEPS:
            got = run_adam(ok, hp, t, device)
            pn, mn, vn, dp, dm, dv, valid = adam_fp64(hp, t)
            seen += int(valid.sum())
            for name, g_, w_, d_ in (("p", got[0], pn, dp), ("m", got[1], mn, dm), ("v", got[2], vn, dv)):
                with np.errstate(invalid="ignore"):  # inf - inf where the case is not a valid one
                    err = np.abs(g_.astype(np.float64) - w_)
                bad = np.flatnonzero(valid & ~(err <= d_))
                assert bad.size == 0, "Adam %s, t = %d, eps = %g: %d elements beyond the bound, first (p, m, v, g) = %r: got %r, fp64 %r, bound %r" % (
                    name, t, hp["eps"], bad.size, tuple(float(a[bad[0]]) for a in (p0, m0, v0, g0)), float(g_[bad[0]]), float(w_[bad[0]]), float(d_[bad[0]]))
    assert seen > 1000  # the well-scaled part of the set is not empty
