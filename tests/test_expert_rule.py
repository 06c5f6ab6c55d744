"""The expert drivers' rule on the CPU (include/okenv_math.h through okenv_expert_act_host and the host-only debug entries):
against an independent numpy restatement (tests/_expert_numpy.py), against actions recorded from the reference's own
PotFieldAgent / VFHAgent (tests/golden/ref_field_agents.npz), in a closed loop with the oracle's Environment::step, and the
two dataset writers."""
import ctypes
import os

import numpy as np
import pytest

import _expert_numpy as E

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
FANS = {5: np.array([-70, -30, 0, 30, 70], f32), 7: np.linspace(-90, 90, 7).astype(f32), 15: np.linspace(-70, 70, 15).astype(f32),
        19: np.linspace(-90, 90, 19).astype(f32), 64: np.linspace(-90, 90, 64).astype(f32)}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def ulps(a, b):
    ai, bi = bits(a).view(np.int32).astype(np.int64), bits(b).view(np.int32).astype(np.int64)
    ai, bi = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai), np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=f32))).astype(np.float64)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "ref_field_agents.npz"))
    out = {}
    for k in ("pf", "vfh19", "vfh23", "vfh41"):
        pos = z[k + "_pos"].astype(f32)
        out[k] = dict(pos=pos, rot=z[k + "_rot"], goal=(pos + z[k + "_goal_off"].astype(f32)).astype(f32), dist=z[k + "_dist"].astype(f32),
                      fan=z[k + "_fan"], action=z[k + "_action"])
    assert "PotentialFieldAgent.hpp:52-84" in str(z["provenance"]) and "glibc 2.35" in str(z["provenance"])
    assert sorted(z.files) == sorted([k + s for k in out for s in ("_pos", "_rot", "_goal_off", "_dist", "_fan", "_action")] + ["provenance"])
    return out


def ok_atan2_scalar(ok):
    return lambda y, x: ok.debug_atan2f([y], [x])[0]


def host_actions(ok, kind, c, **params):
    ep = ok.capi.expert_params(kind, **params)
    return ok.expert_act_host(ep, c["fan"], c["pos"][:, 0], c["pos"][:, 1], c["rot"], c["dist"], goals=(c["goal"][:, 0], c["goal"][:, 1]))


# ---- ok_atan2f -----------------------------------------------------------------------------------------------------------------

def atan2_inputs():
    rng = np.random.default_rng(7)
    n = 400000
    y = rng.standard_normal(n).astype(f32)
    x = rng.standard_normal(n).astype(f32)
    # tiny and huge ratios, all four quadrants
    ys = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(f32)
    xs = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(f32)
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38, 1.1754944e-38], f32)
    gy, gx = np.meshgrid(sp, sp)
    return np.concatenate([y, ys, gy.ravel()]), np.concatenate([x, xs, gx.ravel()])


def test_atan2f_against_fp64_and_glibc(ok):
    y, x = atan2_inputs()
    got = ok.debug_atan2f(y, x)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(f32)
    u = ulps(got, want)
    print("ok_atan2f vs rounded fp64 arctan2: max %d ulp, share differing %.3g of %d" % (u.max(), (u > 0).mean(), u.size))
    assert u.max() <= 1
    assert np.array_equal(np.signbit(got), np.signbit(want))  # signed zeros
    assert np.isnan(ok.debug_atan2f([np.nan, 1.0], [1.0, np.nan])).all()
    libm = ctypes.CDLL("libm.so.6")
    libm.atan2f.restype = ctypes.c_float
    libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
    m = 100000
    sel = np.concatenate([np.arange(m), np.arange(400000, 400000 + m), np.arange(800000, y.size)])
    g = np.array([libm.atan2f(float(y[i]), float(x[i])) for i in sel], f32)
    ug = ulps(got[sel], g)
    print("ok_atan2f vs glibc atan2f: max %d ulp, share differing %.3g" % (ug.max(), (ug > 0).mean()))
    assert ug.max() <= 1


# ---- bounded normalizeAngleDeg -------------------------------------------------------------------------------------------------

def test_bounded_normalize_angle(ok):
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(-1e5, 1e5, 3000), rng.uniform(-800, 800, 2000), [0.0, 360.0, -360.0, 359.99997, 720.0, 1e5, -1e5]]).astype(f32)
    got = ok.debug_expert_normalize_angle(a)
    want = np.array([E.normalize_angle_deg(v) for v in a], f32)
    assert np.array_equal(bits(got), bits(want))
    # beyond the cap, and where the reference would spin for ever or answer NaN: defined as 0
    odd = np.array([np.inf, -np.inf, np.nan, 1e9, -1e9, 3e38], f32)
    assert np.array_equal(bits(ok.debug_expert_normalize_angle(odd)), bits(np.zeros(odd.size, f32)))
    # the numpy restatement's capped form is the same rule
    assert all(E.normalize_angle_deg(v, cap=4096) == 0 for v in odd)
    # a non-finite rot_ through the whole rule: finite, defined steering
    ep = ok.capi.expert_params("potfield")
    thr, steer = ok.expert_act_host(ep, FANS[7], [0, 0, 0], [0, 0, 0], [np.inf, -np.inf, np.nan], np.full((3, 7), 50, f32), goals=([1, 1, 1], [1, 1, 1]))
    assert np.array_equal(steer, np.zeros(3, f32)) and np.isfinite(thr).all()


# ---- host function == numpy restatement, bit for bit ---------------------------------------------------------------------------

def test_host_equals_numpy_on_golden_inputs(ok, golden):
    at = ok_atan2_scalar(ok)
    c = golden["pf"]
    thr, steer = host_actions(ok, "potfield", c)
    tb = E.ray_tables(c["fan"])
    want = np.array([E.potfield(c["pos"][i], c["rot"][i], c["goal"][i], c["dist"][i], c["fan"], at, tables=tb, norm_cap=4096)
                     for i in range(len(thr))], f32)
    assert np.array_equal(bits(thr), bits(want[:, 0])) and np.array_equal(bits(steer), bits(want[:, 1]))
    for k in ("vfh19", "vfh23", "vfh41"):
        c = golden[k]
        thr, steer = host_actions(ok, "vfh", c)
        want = np.array([E.vfh(c["pos"][i], c["rot"][i], c["goal"][i], c["dist"][i], c["fan"], at) for i in range(len(thr))], f32)
        assert np.array_equal(bits(thr), bits(want[:, 0])) and np.array_equal(bits(steer), bits(want[:, 1])), k


@pytest.mark.parametrize("R", [5, 7, 15, 19, 64])
@pytest.mark.parametrize("kind", ["potfield", "vfh"])
def test_host_equals_numpy_on_fresh_inputs(ok, kind, R):
    """Goal points from the centre line, both goal modes; steering clamp on and off; VFH thresholds 0 and 1; goal angles all
    round the agent (a negative goal_sector takes the non-negative remainder on both sides)."""
    at = ok_atan2_scalar(ok)
    t = ok.Track("Silverstone")
    fan = FANS[R]
    rng = np.random.default_rng(100 * R + len(kind))
    n = 240
    idx = rng.integers(0, t.P, n)
    idx[:20] = t.P - 1 - np.arange(20) % 3  # the end of the centre line: wrap and clamp differ there
    px = (t.x[idx] + rng.uniform(-6, 6, n)).astype(f32)
    py = (t.y[idx] + rng.uniform(-6, 6, n)).astype(f32)
    rot = np.where(rng.random(n) < 0.5, rng.uniform(-180, 180, n), rng.uniform(-7200, 7200, n)).astype(f32)
    dist = np.where(rng.random((n, R)) < 0.5, rng.uniform(0.2, 8, (n, R)), rng.uniform(8, 400, (n, R))).astype(f32)
    tb = E.ray_tables(fan)
    for wrap in (False, True):
        for variant in (0, 1):
            if kind == "potfield":
                params = dict(lookahead=2, goal_wrap=wrap, clamp_deg=10.0 if variant else 0.0)
            else:
                params = dict(lookahead=3, goal_wrap=wrap, vfh_threshold=variant, vfh_throttle=80.0 + variant)
            ep = ok.capi.expert_params(kind, **params)
            thr, steer = ok.expert_act_host(ep, fan, px, py, rot, dist, centerline=(t.x, t.y))
            for i in range(n):
                gi = E.goal_index(E.nearest_index(t.x, t.y, px[i], py[i]), params["lookahead"], t.P, wrap)
                goal = (t.x[gi], t.y[gi])
                if kind == "potfield":
                    w = E.potfield((px[i], py[i]), rot[i], goal, dist[i], fan, at, clamp_deg=params["clamp_deg"], tables=tb, norm_cap=4096)
                else:
                    w = E.vfh((px[i], py[i]), rot[i], goal, dist[i], fan, at, threshold=variant, throttle=params["vfh_throttle"])
                assert bits(thr[i]) == bits(w[0]) and bits(steer[i]) == bits(w[1]), (wrap, variant, i, thr[i], steer[i], w)


def test_numpy_restatement_reproduces_the_reference_with_glibc_atan2f(golden):
    """The restatement itself is pinned: with glibc's atan2f (what the recording used) it gives the recorded bits."""
    libm = ctypes.CDLL("libm.so.6")
    libm.atan2f.restype = ctypes.c_float
    libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
    at = lambda y, x: f32(libm.atan2f(float(y), float(x)))  # noqa: E731
    c = golden["pf"]
    tb = E.ray_tables(c["fan"])
    for i in range(0, 20000, 7):
        w = E.potfield(c["pos"][i], c["rot"][i], c["goal"][i], c["dist"][i], c["fan"], at, tables=tb)
        assert bits(w[0]) == bits(c["action"][i, 0]) and bits(w[1]) == bits(c["action"][i, 1]), i
    for k in ("vfh19", "vfh23", "vfh41"):
        c = golden[k]
        for i in range(0, len(c["rot"]), 5):
            w = E.vfh(c["pos"][i], c["rot"][i], c["goal"][i], c["dist"][i], c["fan"], at)
            assert bits(w[1]) == bits(c["action"][i, 1]), (k, i)


# ---- host function against the recorded reference --------------------------------------------------------------------------------

def test_potfield_against_the_reference(ok, golden):
    """The only licensed difference is the last bit of atan2f.  What one ulp of it can do to steering_delta, step by step
    (PotentialFieldAgent.hpp:78-84, Utils.h:3-14):
      * atan2f in (-pi, pi]: one ulp is at most 2^-22 rad; `* 180.F` in fp32 maps neighbours 4.3e-5 apart before its own
        rounding at magnitudes below 1024 (ulp 6.1e-5): at most two ulps, 1.22e-4; `/ M_PI` in fp64: d = 3.9e-5 degrees;
      * `goal_rotation - rot_` narrowed to fp32 at magnitude M <= |rot_| + 180: rounding is monotone, so the two results
        differ by at most d + ulp(M);
      * normalizeAngleDeg: adding or subtracting 360 = 2^3 * 45 is exact whenever the magnitude does not grow and the ulp is
        below 8 (|angle| < 2^26); only the additions that cross zero into [0, 720) round, at most two of them, each moving
        the difference by at most ulp(512) = 6.1e-5; the final `-= 360` from (180, 360) is exact.
    tol = 3.9e-5 + ulp32(|rot_| + 180) + 2 * 6.1e-5 degrees per case; throttle does not pass through atan2f: bit-equal.
    Measured (docs/HISTORY.md section 16): printed below."""
    c = golden["pf"]
    thr, steer = host_actions(ok, "potfield", c)
    assert np.array_equal(bits(thr), bits(c["action"][:, 0]))
    dev = np.abs(steer.astype(np.float64) - c["action"][:, 1].astype(np.float64))
    tol = 3.9e-5 + ulp32(np.abs(c["rot"]) + f32(180.0)) + 2 * 6.1e-5
    equal = (bits(steer) == bits(c["action"][:, 1])).mean()
    worst = int(np.argmax(dev / tol))
    print("potfield vs reference: bit-equal steering %.4f of %d, largest deviation %.3g deg (tolerance there %.3g, |rot| %.1f)"
          % (equal, dev.size, dev.max(), tol[int(np.argmax(dev))], abs(c["rot"][int(np.argmax(dev))])))
    assert (dev <= tol).all(), (worst, dev[worst], tol[worst])


def test_vfh_against_the_reference(ok, golden):
    """VFH is discrete: the steering is one of R sector angles, chosen by goal_sector = trunc((a - first) / fov * R) of the goal
    angle a in the robot frame (VFHAgent.hpp:97-110, 76).  The last bit of atan2f moves a by at most
      tol_a = 3.1e-5 (one ulp of atan2f through `/ M_PI * 180.f` and the narrowing at <= 180) + ulp32(|rot_| + 180) (the fp32
              subtraction of rot_) + ulp32(360) (the wrap)  degrees,
    and the three fp32 operations of the sector index add at most 4 ulp32(R) sectors = 4 ulp32(R) * fov / R degrees.  A case
    whose action differs is excused only if its a (recomputed here) lies within that of a sector boundary
    first + k * fov / R; at most 0.01 % of the cases may be excused.  Every other case is bit-equal."""
    at = ok_atan2_scalar(ok)
    total = excused = 0
    for k in ("vfh19", "vfh23", "vfh41"):
        c = golden[k]
        thr, steer = host_actions(ok, "vfh", c)
        assert np.array_equal(bits(thr), bits(c["action"][:, 0]))
        diff = np.nonzero(bits(steer) != bits(c["action"][:, 1]))[0]
        total += len(thr)
        R, first = len(c["fan"]), float(c["fan"][0])
        fov = abs(float(c["fan"][-1]) - first)
        for i in diff:
            a = float(E.vfh_goal_angle(c["pos"][i], c["rot"][i], c["goal"][i], at))
            tol_a = 3.1e-5 + float(ulp32(abs(c["rot"][i]) + f32(180.0))) + float(ulp32(360.0)) + 4 * float(ulp32(R)) * fov / R
            s = (a - first) / fov * R
            assert abs(s - round(s)) * fov / R <= tol_a, (k, i, a, steer[i], c["action"][i, 1])
            excused += 1
    print("vfh vs reference: %d of %d cases differ (all within the tolerance of a sector boundary)" % (excused, total))
    assert excused <= total * 1e-4


# ---- closed loop on the CPU ------------------------------------------------------------------------------------------------------

COLLECTOR = dict(lookahead=2, goal_wrap=False, clamp_deg=10.0)  # collect_data_random.cpp:45,111-112


def cpu_loop(ok, oracle, track, N, steps, seed, kind="potfield", fan=None, auto_reset=False, params=COLLECTOR, record=False):
    """collect_data_random.cpp:163-183 with the oracle's Environment::step and okenv_expert_act_host."""
    fan = FANS[7] if fan is None else fan
    t = oracle.Track(track)
    env = oracle.OracleEnv(t.segments, N, fan.size, fan, (t.x, t.y, t.heading))
    env.set_lane_bounds(t.li, t.ri)
    flags = 1 | 2 | 4
    env.set_auto_reset(auto_reset, flags, seed, 0)
    env.reset_random(None, flags, seed, 0, 0)
    env.step(1)
    ep = ok.capi.expert_params(kind, **params)
    progress = np.zeros(N, np.int64)
    prev = None
    rec = []
    for _ in range(steps):
        px, py = env.get(oracle.F_POS_X), env.get(oracle.F_POS_Y)
        dist = env.get(oracle.F_DIST)
        thr, steer = ok.expert_act_host(ep, fan, px, py, env.get(oracle.F_ROT), dist, centerline=(t.x, t.y))
        if record:
            rec.append(dict(action=np.stack([thr, steer], 1), dist=dist.copy(), rel_x=env.get(oracle.F_REL_X), rel_y=env.get(oracle.F_REL_Y),
                            alive=(env.get(oracle.F_CRASHED) == 0).astype(np.uint8)))
        env.set(oracle.F_THR, thr)
        env.set(oracle.F_STEER, steer)
        env.step(1)
        if not record:
            d2 = (px[:, None] - t.x[None, :]) ** 2 + (py[:, None] - t.y[None, :]) ** 2
            idx = d2.argmin(1)
            if prev is not None:
                delta = (idx - prev + t.P // 2) % t.P - t.P // 2
                progress += delta
            prev = idx
    return env, progress, rec


@pytest.mark.parametrize("track", ["Silverstone", "Monza"])
def test_closed_loop_potfield_on_the_cpu(ok, oracle, track):
    """The collectors' settings: 7-ray fan -90..90, clamp 10 degrees, lane and heading randomised; 256 agents, 2000 steps.
    Reproducible, and every agent still alive has made positive progress along the centre line.  How many survive is a
    property of the reference's algorithm, recorded in docs/HISTORY.md section 16, not a bar."""
    N, steps = 256, 2000
    e1, p1, _ = cpu_loop(ok, oracle, track, N, steps, seed=11)
    e2, p2, _ = cpu_loop(ok, oracle, track, N, steps, seed=11)
    s1, s2 = e1.snapshot(), e2.snapshot()
    for k in s1:
        assert np.array_equal(np.ascontiguousarray(s1[k]).view(np.uint8), np.ascontiguousarray(s2[k]).view(np.uint8)), k
    assert np.array_equal(p1, p2)
    alive = s1["crashed"] == 0
    print("%s: %d of %d agents alive after %d steps; progress of the living: min %d, median %d centre-line points"
          % (track, alive.sum(), N, steps, p1[alive].min() if alive.any() else 0, np.median(p1[alive]) if alive.any() else 0))
    assert (p1[alive] > 0).all()


# ---- writers ---------------------------------------------------------------------------------------------------------------------

def test_birdseye_writer_round_trip(tmp_path):
    from openkitchen_amd.dataset import BirdseyeWriter, decode_png
    import struct
    import zlib
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, (2, 3, 12, 16, 4)).astype(np.uint8)
    actions = np.array([[[100, -10], [37.25, 0.5], [1e-3, 10]], [[99.5, 3.14159], [0, 0], [100, -0.015625]]], f32)
    alive = np.array([[1, 0, 1], [1, 1, 0]], np.uint8)
    w = BirdseyeWriter(str(tmp_path / "Track_random"), "Track")
    assert w.save_recorded(actions, frames, alive) == 4
    assert sorted(os.listdir(tmp_path / "Track_random")) == sorted("birdseye_Track_%d%s" % (i, e) for i in range(4) for e in (".txt", ".png"))
    kept = [(0, 0), (0, 2), (1, 0), (1, 1)]
    for ctr, (t, a) in enumerate(kept):
        text = open(w.path(ctr)).read()
        assert text == "%g %g" % (actions[t, a, 0], actions[t, a, 1]) and not text.endswith("\n")
        data = open(w.path(ctr, ".png"), "rb").read()
        assert np.array_equal(decode_png(data), frames[t, a])
        # the PNG by hand: signature, IHDR, the IDAT stream inflated with zlib = rows of filter byte 0 + pixels
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
        assert struct.unpack(">IIBBBBB", data[16:29]) == (16, 12, 8, 6, 0, 0, 0)
        n = struct.unpack(">I", data[33:37])[0]
        assert data[37:41] == b"IDAT"
        rows = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(12, 1 + 16 * 4)
        assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(12, 16, 4), frames[t, a])
    assert open(w.path(0)).read() == "100 -10"
    # class frames are greyscale PNGs
    w2 = BirdseyeWriter(str(tmp_path / "cls"), "T")
    w2.write_sample(frames[0, 0, :, :, 0], 1.0, 2.0)
    assert np.array_equal(decode_png(open(w2.path(0, ".png"), "rb").read())[:, :, 0], frames[0, 0, :, :, 0])


def test_laser_save_recorded_skips_dead_entries(tmp_path):
    from openkitchen_amd.dataset import Laser2dWriter, read_sample
    rng = np.random.default_rng(4)
    rel = rng.uniform(-200, 200, (3, 4, 7, 2)).astype(f32)
    actions = rng.uniform(-10, 100, (3, 4, 2)).astype(f32)
    alive = (rng.random((3, 4)) < 0.6).astype(np.uint8)
    alive[0, 0], alive[0, 1] = 1, 0
    w = Laser2dWriter(str(tmp_path / "d"), "Monza")
    assert w.save_recorded(actions, rel, alive) == int(alive.sum())
    assert len(os.listdir(tmp_path / "d")) == int(alive.sum())
    kept = [(t, a) for t in range(3) for a in range(4) if alive[t, a]]
    for ctr, (t, a) in enumerate(kept):
        hits, thr, steer = read_sample(w.path(ctr))
        assert os.path.basename(w.path(ctr)) == "laser2d_Monza_%d.txt" % ctr
        assert np.allclose(hits, rel[t, a], rtol=1e-5, atol=1e-4) and np.isclose(thr, actions[t, a, 0], rtol=1e-5, atol=1e-4)
        text = open(w.path(ctr)).read()
        assert text.count("\n") == 7 and not text.endswith("\n")
        assert text.split("\n")[-1] == "%g %g" % (actions[t, a, 0], actions[t, a, 1])
