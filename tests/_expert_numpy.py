"""The two expert drivers of the reference's FieldNavigators/, restated in numpy scalars for the tests.

Written from the reference's lines (PotentialFieldAgent.hpp:52-84, collect_data/collect_data_random.cpp:59-65 and 108-120,
VFHAgent.hpp:40-44 and 53-123, main.cpp:20-25, Environment/Utils.h:3-14), not from include/okenv_math.h: every fp32 operation is
an np.float32 operation, every fp64 one an np.float64 (or Python float) one, in the order the C++ conversions give.  The one
function that is not pinned, atan2f, is passed in: the library's ok_atan2f to compare with the library bit for bit, glibc's to
compare with the recorded reference."""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
PI = f64(math.pi)
SENSOR_RANGE = f32(200.0)


def normalize_angle_deg(angle, cap=None):
    """Utils.h:3-14.  cap=None: the reference's unbounded loops; cap=k: at most k turns per loop, 0 where that does not reach
    [0, 360) (the library's bounded form)."""
    angle = f32(angle)
    n = 0
    while angle < f32(360.0) and (cap is None or n < cap):
        angle = f32(angle + f32(360.0))
        n += 1
    n = 0
    while angle >= f32(360.0) and (cap is None or n < cap):
        angle = f32(angle - f32(360.0))
        n += 1
    if cap is not None and not (angle >= f32(0.0) and angle < f32(360.0)):
        return f32(0.0)
    return angle


def ray_tables(ray_deg):
    """cos / sin (angle * M_PI / 180.f) as the C++ evaluates them: float * double, / double, libm's fp64 cos / sin."""
    c = [math.cos(float(f64(f32(a)) * PI / f64(180.0))) for a in ray_deg]
    s = [math.sin(float(f64(f32(a)) * PI / f64(180.0))) for a in ray_deg]
    return c, s


def potfield(pos, rot, goal, dist, ray_deg, atan2f, k_att=100.0, k_rep=10.0, effect_range=5.0, clamp_deg=0.0, norm_cap=None,
             tables=None):
    k_att, k_rep, effect_range, clamp_deg = f32(k_att), f32(k_rep), f32(effect_range), f32(clamp_deg)
    cs, sn = tables if tables is not None else ray_tables(ray_deg)
    ax = f32(f32(goal[0]) - f32(pos[0]))
    ay = f32(f32(goal[1]) - f32(pos[1]))
    with np.errstate(all="ignore"):
        length = f32(np.sqrt(f32(f32(ax * ax) + f32(ay * ay))))
        ax = f32(f32(ax / length) * k_att)
        ay = f32(f32(ay / length) * k_att)
        rx = f32(0.0)
        ry = f32(0.0)
        for i in range(len(ray_deg)):
            n = f32(dist[i])
            if n < effect_range:
                mag = f32(k_rep * f32(f32(f32(1.0) / n) - f32(f32(1.0) / effect_range)))
                rx = f32(f64(rx) + f64(cs[i]) * f64(mag))
                ry = f32(f64(ry) + f64(sn[i]) * f64(mag))
        tx = f32(ax - rx)
        ty = f32(ay - ry)
        goal_rotation = f64(f32(f32(atan2f(ty, tx)) * f32(180.0))) / PI
        tl = f32(np.sqrt(f32(f32(tx * tx) + f32(ty * ty))))
        throttle = tl if tl < f32(100.0) else f32(100.0)
        steer = f32(goal_rotation - f64(f32(rot)))
    steer = normalize_angle_deg(steer, norm_cap)
    if steer > f32(180.0):
        steer = f32(steer - f32(360.0))
    if clamp_deg > 0:
        steer = -clamp_deg if steer < -clamp_deg else (clamp_deg if clamp_deg < steer else steer)
    return throttle, steer


def vfh_goal_angle(pos, rot, goal, atan2f):
    world = f32(f64(f32(atan2f(f32(f32(goal[1]) - f32(pos[1])), f32(f32(goal[0]) - f32(pos[0]))))) / PI * f64(f32(180.0)))
    a = f32(world - f32(rot))
    a = f32(math.fmod(float(a), 360.0))
    if a > f32(180.0):
        a = f32(a - f32(360.0))
    elif a <= f32(-180.0):
        a = f32(a + f32(360.0))
    return a


def vfh(pos, rot, goal, dist, ray_deg, atan2f, threshold=1, throttle=100.0, goal_angle=None):
    R = len(ray_deg)
    ns = R
    first, last = f32(ray_deg[0]), f32(ray_deg[-1])
    fov = f32(abs(f32(last - first)))
    width = f32(fov / f32(ns))
    hist = [0] * ns
    for i in range(R):
        if f32(dist[i]) < SENSOR_RANGE:
            hist[int(f32(f32(f32(i) / f32(R)) * f32(ns)))] += 1
    occ = [h > threshold for h in hist]
    a = vfh_goal_angle(pos, rot, goal, atan2f) if goal_angle is None else f32(goal_angle)
    goal_sector = int(f32(f32(f32(a - first) / fov) * f32(ns)))  # int() truncates, like the cast
    best = goal_sector
    for i in range(ns):
        s = (goal_sector + i) % ns  # Python's remainder is the non-negative one
        if not occ[s]:
            best = s
            break
        s = (goal_sector - i + ns) % ns
        if not occ[s]:
            best = s
            break
    return f32(throttle), f32(f32(width * f32(best)) + first)


def nearest_index(cx, cy, x, y):
    """RaceTrack::findNearestTrackIndexBruteForce: first minimum of the fp32 squared distance."""
    dx = f32(x) - cx
    dy = f32(y) - cy
    return int(np.argmin(dx * dx + dy * dy))


def goal_index(nearest, lookahead, P, wrap):
    return (nearest + lookahead) % P if wrap else min(nearest + lookahead, P - 1)
