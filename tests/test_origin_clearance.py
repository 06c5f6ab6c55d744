"""The square the origin test clears and the walk's start at the origin, on the CPU (tests/cpp/origin_clearance_check.cpp drives the
product's headers: ok_raycast.h's okOriginClearScalar, okOriginMoved and ok_cast_poly_interval).

The kernels repeat the origin test when the origin has moved, along either axis, by the half-width the last test reported.  That
is sound when the open square of that half-width holds no point of an F segment (an inner boundary, the only place chi flips).
So, for the four tracks at cell edges 20, 24 and 28 px and for origins on the centre line and up to 3 px beside it (where the
bench recipe's agents drive):
  * half-width <= the float64 brute-force Chebyshev distance to the nearest F segment (the square is empty),
  * hence also <= the Euclidean distance to it,
  * half-width >= the value of the formula it replaces (written out in the driver), and >= what the cell's border and the
    segments' boxes give in float64, less the slack: the arithmetic has not been made more timid.
Origins in cells that are not certifiable have no square and are skipped; their share is printed and capped at 10 %.
(A clearance table per cell -- a lower bound of the distance to the F segments NOT registered in a cell, to let the half-width
grow past the cell's border -- was built and measured first: the neighbours' F segments run right behind the border of the cells
the track crosses, the half-width grew by 1 to 5 % and the reruns fell by 8 %; it was dropped, docs/HISTORY.md section 47.)

The start at the origin (the set-up without the slab clip, ok_cast_poly_interval<.., .., true>) must report what the generic
set-up reports: min_t bit for bit, `conclusive`, and t_reached where the walk is not conclusive."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
TRACKS = ["Austin", "Monza", "Silverstone", "Spa"]
CELLS = [20.0, 24.0, 28.0]
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def clearcheck():
    src = os.path.join(HERE, "cpp", "origin_clearance_check.cpp")
    out_dir = os.path.join(HERE, "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libclearcheck_san.so" if O.SANITIZE else "libclearcheck.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + (O.SAN_FLAGS if O.SANITIZE else []) + ["-o", so, src],
                   check=True)
    G = C.CDLL(so)
    G.clearcheck_split.argtypes = [O.f32p, C.c_int, C.c_float, O.f32p, O.i32p, u8p]
    G.clearcheck_radii.argtypes = [O.f32p, C.c_int, C.c_float, O.f32p, O.f32p, C.c_int, u8p, O.f32p, O.f32p, u8p]
    G.clearcheck_walk.argtypes = [O.f32p, C.c_int, C.c_float, O.f32p, O.f32p, O.f32p, O.f32p, C.c_int, C.c_float, O.f32p, O.f32p, u8p, u8p]
    return G


_tracks = {}


def track(oracle, name):
    if name not in _tracks:
        _tracks[name] = oracle.Track(name)
    return _tracks[name]


def split(G, t, cell):
    geom, d, is_f = np.zeros(5, np.float32), np.zeros(2, np.int32), np.zeros(t.S, np.uint8)
    assert G.clearcheck_split(np.ascontiguousarray(t.segments.reshape(-1)), t.S, cell, geom, d, is_f) == 0
    return geom, d, is_f.astype(bool)


def point_seg_dist(px, py, seg):
    """float64 distances of the points (n) from the segments (m, 4): an (n, m) array"""
    ax, ay = seg[:, 0][None, :], seg[:, 1][None, :]
    dx, dy = seg[:, 2][None, :] - ax, seg[:, 3][None, :] - ay
    l2 = dx * dx + dy * dy
    ex, ey = px[:, None] - ax, py[:, None] - ay
    u = np.clip((ex * dx + ey * dy) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
    return np.hypot(ex - u * dx, ey - u * dy)


def origins(t):
    """every centre-line point, and the same points displaced by up to 3 px (fixed seed)"""
    rng = np.random.default_rng(20240607)
    r, phi = rng.uniform(0, 3, t.P), rng.uniform(0, 2 * np.pi, t.P)
    ox = np.concatenate([t.x, (t.x + r * np.cos(phi)).astype(np.float32)]).astype(np.float32)
    oy = np.concatenate([t.y, (t.y + r * np.sin(phi)).astype(np.float32)]).astype(np.float32)
    return ox, oy


def point_seg_cheb(px, py, seg):
    """float64 Chebyshev distances max(|x - px|, |y - py|) of the points (n) from the segments (m, 4): an (n, m) array.  Along a
    segment both differences are linear in the parameter, so the maximum of their magnitudes is convex and piecewise linear: its
    minimum over [0, 1] is at an end or where two of the four lines +-u, +-v meet."""
    ax, ay = seg[:, 0][None, :], seg[:, 1][None, :]
    dx, dy = seg[:, 2][None, :] - ax, seg[:, 3][None, :] - ay
    ux, uy = ax - px[:, None], ay - py[:, None]
    best = np.minimum(np.maximum(np.abs(ux), np.abs(uy)), np.maximum(np.abs(ux + dx), np.abs(uy + dy)))
    with np.errstate(all="ignore"):
        for num, den in ((uy - ux, dx - dy), (-(ux + uy), dx + dy), (-ux, dx), (-uy, dy)):  # u = v, u = -v, u = 0, v = 0
            tt = np.clip(np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0), 0.0, 1.0)
            best = np.minimum(best, np.maximum(np.abs(ux + tt * dx), np.abs(uy + tt * dy)))
    return best


_nearest_f = {}


def nearest_f(G, t, name, ox, oy):
    """brute force, once per track: the F segments are the same at every cell edge"""
    if name not in _nearest_f:
        is_f = split(G, t, 24.0)[2]
        segf = t.segments[is_f].astype(np.float64)
        x, y = ox.astype(np.float64), oy.astype(np.float64)
        _nearest_f[name] = (is_f, point_seg_dist(x, y, segf).min(axis=1), point_seg_cheb(x, y, segf).min(axis=1))
    return _nearest_f[name]


def square_in_float64(t, is_f, geom, ox, oy):
    """What the border and the boxes give: the cell of each origin in float64 from the grid's fp32 geometry, the Chebyshev distance
    to its border, and to the bounding box of every F segment that comes within the cell inflated by 1 px (a superset of the
    registered ones: the margin is 1/8 px), less the slack and 1e-3 px for the fp32 arithmetic."""
    x0, y0, ce = float(geom[0]), float(geom[1]), float(geom[4])
    x, y = ox.astype(np.float64), oy.astype(np.float64)
    ix, iy = np.floor((x - x0) / ce), np.floor((y - y0) / ce)
    lx, ly = x0 + ix * ce, y0 + iy * ce
    near = np.minimum(np.minimum(x - lx, lx + ce - x), np.minimum(y - ly, ly + ce - y))
    seg = t.segments[is_f].astype(np.float64)
    bx0, bx1 = np.minimum(seg[:, 0], seg[:, 2])[None, :], np.maximum(seg[:, 0], seg[:, 2])[None, :]
    by0, by1 = np.minimum(seg[:, 1], seg[:, 3])[None, :], np.maximum(seg[:, 1], seg[:, 3])[None, :]
    close = (bx1 >= lx[:, None] - 1) & (bx0 <= lx[:, None] + ce + 1) & (by1 >= ly[:, None] - 1) & (by0 <= ly[:, None] + ce + 1)
    gx = np.maximum(np.maximum(bx0 - x[:, None], x[:, None] - bx1), 0.0)
    gy = np.maximum(np.maximum(by0 - y[:, None], y[:, None] - by1), 0.0)
    box = np.where(close, np.maximum(gx, gy), np.inf).min(axis=1)
    return 0.99 * np.minimum(near, box) - 1.0e-3 - 1.0e-3


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", TRACKS)
def test_cleared_square_is_empty_and_as_wide_as_the_boxes_allow(clearcheck, oracle, name, cell):
    t = track(oracle, name)
    ox, oy = origins(t)
    is_f, dist, cheb = nearest_f(clearcheck, t, name, ox, oy)
    geom, _, is_f_here = split(clearcheck, t, cell)
    assert np.array_equal(is_f, is_f_here)
    n = ox.size
    usable, rad, rad_was, cert = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    assert clearcheck.clearcheck_radii(np.ascontiguousarray(t.segments.reshape(-1)), t.S, cell, ox, oy, n, usable, rad, rad_was, cert) == 0
    use = usable.astype(bool)
    skipped = 1.0 - use.mean()
    print("%s cell %.0f: %d origins, skipped %.3f, mean half-width %.2f px, certified %.3f" % (name, cell, n, skipped, rad[use].mean(), cert[use].mean()))
    assert skipped <= 0.10
    assert (rad[use] <= cheb[use]).all(), (ox[use][rad[use] > cheb[use]][:4], oy[use][rad[use] > cheb[use]][:4])
    assert (rad[use] <= dist[use]).all()
    assert (rad[use] >= rad_was[use]).all()  # never smaller than the formula it replaces, written out in the driver
    assert (rad[use] >= square_in_float64(t, is_f, geom, ox[use], oy[use])).all()
    assert (rad[~use] <= 0).all()  # (inside the box, not certifiable: 0; these origins are never outside the box)


def walk(G, t, cell, ox, oy, dx, dy, t_b):
    n = ox.size
    mt, tr, co, am = np.zeros(2 * n, np.float32), np.zeros(2 * n, np.float32), np.zeros(2 * n, np.uint8), np.zeros(2 * n, np.uint8)
    rc = G.clearcheck_walk(np.ascontiguousarray(t.segments.reshape(-1)), t.S, cell, ox, oy, dx, dy, n, t_b, mt, tr, co, am)
    assert rc == 0, rc
    return (mt[:n], tr[:n], co[:n]), (mt[n:], tr[n:], co[n:])


@pytest.mark.parametrize("name,cell", [("Silverstone", 28.0), ("Silverstone", 20.0), ("Austin", 24.0), ("Monza", 28.0), ("Spa", 24.0)])
def test_start_at_the_origin_equals_the_generic_set_up(clearcheck, oracle, name, cell):
    t = track(oracle, name)
    geom = split(clearcheck, t, cell)[0]
    x0, y0, x1, y1 = (np.float32(v) for v in geom[:4])
    rng = np.random.default_rng(7 + int(cell))
    f = np.float32
    k = 4000
    # origins: beside the centre line; anywhere in the box; within 40 px of the box's border; exactly on the border and its corners
    idx = rng.integers(0, t.P, k)
    ax, ay = (t.x[idx] + rng.normal(0, 4, k)).astype(f), (t.y[idx] + rng.normal(0, 4, k)).astype(f)
    bx, by = rng.uniform(x0, x1, k).astype(f), rng.uniform(y0, y1, k).astype(f)
    cx, cy = rng.uniform(x0, x1, k).astype(f), rng.uniform(y0, y1, k).astype(f)
    side = rng.integers(0, 4, k)
    off = rng.uniform(0, 40, k).astype(f)
    cx = np.where(side == 0, x0 + off, np.where(side == 1, x1 - off, cx)).astype(f)
    cy = np.where(side == 2, y0 + off, np.where(side == 3, y1 - off, cy)).astype(f)
    ex, ey = rng.uniform(x0, x1, k).astype(f), rng.uniform(y0, y1, k).astype(f)
    side = rng.integers(0, 4, k)
    ex = np.where(side == 0, x0, np.where(side == 1, x1, ex)).astype(f)
    ey = np.where(side == 2, y0, np.where(side == 3, y1, ey)).astype(f)
    ex[:8] = [x0, x0, x1, x1, x0, x1, x0, x1]
    ey[:8] = [y0, y1, y0, y1, y0, y1, y1, y0]
    ox = np.clip(np.concatenate([ax, bx, cx, ex]), x0, x1).astype(f)
    oy = np.clip(np.concatenate([ay, by, cy, ey]), y0, y1).astype(f)
    n = ox.size
    ang = rng.uniform(-np.pi, np.pi, n)
    dx, dy = np.cos(ang).astype(f), np.sin(ang).astype(f)
    # axis-parallel directions, exact; and, for the origins near and on the border, directions that leave the grid
    axis = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], f)
    pick = rng.integers(0, 4, n)
    every = np.arange(n) % 5 == 0
    dx[every], dy[every] = axis[pick[every], 0], axis[pick[every], 1]
    out_ang = np.arctan2(oy - (y0 + y1) / 2, ox - (x0 + x1) / 2) + rng.normal(0, 0.5, n)
    outward = (np.arange(n) >= 2 * k) & (np.arange(n) % 5 != 0) & (np.arange(n) % 2 == 0)
    dx[outward], dy[outward] = np.cos(out_ang[outward]).astype(f), np.sin(out_ang[outward]).astype(f)
    left_grid = 0
    for t_b in (48.0, float("inf")):
        (m0, r0, c0), (m1, r1, c1) = walk(clearcheck, t, cell, ox, oy, dx, dy, t_b)
        assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32))
        assert np.array_equal(c0, c1)
        open_ = c0 == 0
        assert np.array_equal(r0[open_].view(np.uint32), r1[open_].view(np.uint32))
        if t_b == 48.0:
            # rays that leave the grid within 48 px without a hit are there in numbers, and both set-ups call them conclusive
            tx = np.where(dx > 0, (x1 - ox) / np.where(dx != 0, dx, 1), np.where(dx < 0, (x0 - ox) / np.where(dx != 0, dx, 1), np.inf))
            ty = np.where(dy > 0, (y1 - oy) / np.where(dy != 0, dy, 1), np.where(dy < 0, (y0 - oy) / np.where(dy != 0, dy, 1), np.inf))
            leaves = (np.minimum(tx, ty) < 47.0) & (m0 == f(200.0))
            left_grid = int(leaves.sum())
            assert left_grid > 300 and (c0[leaves] == 1).all()
            assert (open_ & (m0 == f(200.0))).sum() > 1000  # and walks that phase 2 would continue
        else:
            assert (c0 == 1).all()
