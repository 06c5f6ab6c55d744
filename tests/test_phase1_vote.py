"""The wave's vote that ends phase 1 of the raycast, on the CPU (tests/cpp/phase1_vote_check.cpp drives the product's header:
ok_raycast.h's ok_cast_poly_interval<.., .., .., kVote>).

On the GPU the lanes of a wave count themselves; on the host the count is the caller's, so here the walk that starts a ray is cut
after k = 1, 2, 3, ... cells, every k up to the walk's own length (range "none": the whole ray), whatever a wave would have voted.
Every cut that is not conclusive is continued from its t_reached with 1, 5 and 8 equal parameter intervals, cut as
okStepCoopKernel's coop_pass cuts them (dt = (range - t_reached) * rcp(m), last interval open-ended, first-hit bound = range) and
with skip_unowned_start as the kernel sets it (j > 0 || t_reached > 0).  Then, on the front image of Silverstone, Monza, Spa and
Austin at cell edges 20 / 24 / 28 px, for 16 000 rays each --
  origins: beside the centre line; anywhere in the grid box; within 40 px of its border; on the border and its corners,
  directions: random; every fifth axis-parallel, exactly; for the origins near and on the border, half aimed out of the grid --
  * the minimum over the pieces equals ok_cast_ray_poly's single walk in every bit,
  * a cut the walk calls conclusive reports that minimum by itself,
  * the pieces' ambiguity flags together are set whenever the whole walk's is,
  * a walk told to end after k cells has looked at exactly k,
  * no ray is skipped (the count is printed and asserted),
  * cuts with a t_reached of a fraction of a pixel, and of 0, are among them in numbers (origins at a cell's border)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
TRACKS = ["Silverstone", "Monza", "Spa", "Austin"]
CELLS = [20.0, 24.0, 28.0]
RAYS = 16000
SPLITS = np.array([1, 5, 8], np.int32)
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def votecheck():
    src = os.path.join(HERE, "cpp", "phase1_vote_check.cpp")
    out_dir = os.path.join(HERE, "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libvotecheck_san.so" if O.SANITIZE else "libvotecheck.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + (O.SAN_FLAGS if O.SANITIZE else []) + ["-o", so, src],
                   check=True)
    G = C.CDLL(so)
    G.votecheck_geom.argtypes = [O.f32p, C.c_int, C.c_float, O.f32p]
    G.votecheck_run.argtypes = [O.f32p, C.c_int, C.c_float, O.f32p, O.f32p, O.f32p, O.f32p, C.c_int, C.c_float, O.i32p, C.c_int, i64p, O.i32p, C.c_int]
    return G


def rays(t, geom, seed):
    """RAYS rays in four families of origins, with the three kinds of directions mixed in"""
    x0, y0, x1, y1 = (np.float32(v) for v in geom[:4])
    cell = np.float32(geom[4])
    rng = np.random.default_rng(seed)
    f = np.float32
    k = RAYS // 4
    idx = rng.integers(0, t.P, k)
    ax, ay = (t.x[idx] + rng.normal(0, 4, k)).astype(f), (t.y[idx] + rng.normal(0, 4, k)).astype(f)
    # (a tenth of them right at a border of their cell, along x, along y or both: the walk leaves the start cell after a
    # fraction of a pixel, or at 0)
    snap = np.arange(k) % 10 == 0
    sx = (x0 + np.round((ax - x0) / cell) * cell).astype(f)
    sy = (y0 + np.round((ay - y0) / cell) * cell).astype(f)
    kind = rng.integers(0, 3, k)
    ax = np.where(snap & (kind != 1), sx, ax).astype(f)
    ay = np.where(snap & (kind != 0), sy, ay).astype(f)
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
    axis = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], f)
    pick = rng.integers(0, 4, n)
    every = np.arange(n) % 5 == 0
    dx[every], dy[every] = axis[pick[every], 0], axis[pick[every], 1]
    out_ang = np.arctan2(oy - (y0 + y1) / 2, ox - (x0 + x1) / 2) + rng.normal(0, 0.5, n)
    outward = (np.arange(n) >= 2 * k) & (np.arange(n) % 5 != 0) & (np.arange(n) % 2 == 0)
    dx[outward], dy[outward] = np.cos(out_ang[outward]).astype(f), np.sin(out_ang[outward]).astype(f)
    return ox, oy, dx, dy


@pytest.mark.parametrize("vote_only", [0, 1])  # (the walk's two forms: the vote beside an interval's end, the vote alone)
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", TRACKS)
def test_a_walk_cut_after_any_cell_and_continued_gives_the_whole_walks_bits(votecheck, oracle, name, cell, vote_only):
    t = oracle.Track(name)
    segs = np.ascontiguousarray(t.segments.reshape(-1))
    geom = np.zeros(5, np.float32)
    assert votecheck.votecheck_geom(segs, t.S, cell, geom) == 0
    ox, oy, dx, dy = rays(t, geom, 11 + int(cell) + 100 * TRACKS.index(name))
    assert ox.size == RAYS
    counts, first_bad = np.zeros(12, np.int64), np.zeros(1, np.int32)
    rc = votecheck.votecheck_run(segs, t.S, cell, ox, oy, dx, dy, RAYS, float("inf"), SPLITS, SPLITS.size, counts, first_bad, vote_only)
    assert rc == 0, rc
    c = counts
    print("%s cell %.0f: %d rays walked, %d skipped; %d starting walks (longest %d cells), %d ended by the vote; %d continuations; "
          "t_reached below half a pixel %d, zero %d" % (name, cell, c[0], c[1], c[2], c[11], c[3], c[4], c[8], c[9]))
    i = int(first_bad[0])
    where = "" if i < 0 else "first at ray %d: origin (%r, %r) direction (%r, %r)" % (i, ox[i], oy[i], dx[i], dy[i])
    assert c[0] == RAYS and c[1] == 0
    assert c[7] == 0, where    # a walk told to end after k cells looked at k
    assert c[10] == 0, where   # a conclusive cut is the whole walk's minimum
    assert c[5] == 0, where    # the pieces' minimum is, in every bit
    assert c[6] == 0, where    # the ambiguity flag is not lost
    # the cases are there: walks ended by the vote, continuations in all three splits, tiny and zero t_reached
    assert c[3] > RAYS and c[4] > 3 * RAYS and c[4] % 3 == 0  # (more than one cut and one continued cut per ray, on average)
    assert c[8] > 100 and c[9] > 0
