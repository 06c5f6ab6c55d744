"""The start of the walks and the origin test on the GPU (openkitchen_amd/csrc/ok_raycast.h: the set-up of ok_cast_poly_interval with
its start at the origin, the header that travels as "the next cell's"; okenv_kernels.h: okOriginChiGroup and the square it clears):
snapshots equal the oracle's on every field, bit for bit, where the new paths are taken and where they are not --
  * 40 agents x 64 rays for 130 steps of the bench driver in launches of 1, 20 and 109 (one agent per wave: an action block is
    crossed, the run ends inside one, the last workgroup is partly filled),
  * 40 x 16 (four agents per wave: the origins differ inside a wave),
  * 8 x 64 with three agents outside the grid box and two in cells on its border, so that one launch holds waves that start at
    the origin and waves that take the generic set-up,
  * a 32-ray MLP episode of 64 agents in the cooperative policy form, and one of 8 agents in listed tail launches: both share
    okOriginChiGroup and the walks with the ray-only kernels."""
import numpy as np
import pytest

from test_gpu_episode import make_ga, oracle_ga_loop
from test_gpu_parity import assert_same_state, make_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,R", [(40, 64), (40, 16)])
def test_bench_driver_in_launches_of_1_20_and_109(gpu, oracle, monkeypatch, N, R):
    # (so small a population would be widened to 64 lanes per agent and lose phase 1: the handle is held to its natural width)
    monkeypatch.setenv("OKENV_LANES_PER_AGENT", str(R))
    t, dev, orc = make_pair(gpu, oracle, "Silverstone", N, R)
    dev.init_bench_state(0, 0)
    orc.init_bench_state(0, 0)
    done = 0
    for n in (1, 20, 109):
        dev.rollout_random(n, 1234, 0, done)
        orc.rollout_random(n, 1234, 0, done, threads=8)
        done += n
        assert_same_state(dev.snapshot(), orc.snapshot(), "%d x %d after %d steps" % (N, R, done))
    assert dev.info()["lanes_per_agent"] == R
    dev.close()


def test_origins_outside_the_box_and_in_border_cells(gpu, oracle, monkeypatch):
    monkeypatch.delenv("OKENV_LANES_PER_AGENT", raising=False)
    N, R = 8, 64
    t, dev, orc = make_pair(gpu, oracle, "Silverstone", N, R)
    seg = t.segments
    lo_x, hi_x = float(seg[:, [0, 2]].min()), float(seg[:, [0, 2]].max())
    lo_y, hi_y = float(seg[:, [1, 3]].min()), float(seg[:, [1, 3]].max())
    mid_x, mid_y = 0.5 * (lo_x + hi_x), 0.5 * (lo_y + hi_y)
    info = dev.info()
    assert info["lanes_per_agent"] == 64 and info["front_back_bytes"] > 0
    cell = info["grid_cell"]
    # three outside the box (the box is the segments' bounding box and a quarter pixel): near it and looking in, near it and
    # looking away, far from it; two in the first and the last column of cells; three on the centre line
    x = np.array([lo_x - 30.0, hi_x + 5.0, mid_x, lo_x + 0.3 * cell, hi_x - 0.3 * cell, t.x[10], t.x[400], t.x[900]], np.float32)
    y = np.array([mid_y, mid_y, hi_y + 400.0, mid_y, mid_y, t.y[10], t.y[400], t.y[900]], np.float32)
    rot = np.array([0.0, 0.0, -90.0, 180.0, 0.0, t.heading[10], t.heading[400], t.heading[900]], np.float32)
    idx = np.arange(N, dtype=np.int32)
    for e in (dev, orc):
        e.reset_agents(idx, x, y, rot)
    rng = np.random.default_rng(3)
    for step in range(10):
        thr = rng.uniform(0, 60, N).astype(np.float32)
        steer = rng.uniform(-3, 3, N).astype(np.float32)
        dev.set_actions(thr, steer)
        orc.set(oracle.F_THR, thr)
        orc.set(oracle.F_STEER, steer)
        dev.step(1)
        orc.step(1)
        assert_same_state(dev.snapshot(), orc.snapshot(), "step %d" % step)
    dev.step(20)
    orc.step(20)
    o = orc.snapshot()
    assert_same_state(dev.snapshot(), o, "after the launch of 20")
    # the placement is what it was meant to be: the far agent sees nothing, the ones on the centre line see the track
    # (a ray without a hit reports the length of its 200 px, to rounding)
    assert (o["dist"][2] > np.float32(199.9)).all() and (o["dist"][5:] < np.float32(199.0)).any()
    dev.close()


@pytest.mark.parametrize("N,tail_max,form", [(64, "0", "coop_mlp32"), (8, None, "tail_mlp32")])
def test_mlp_episode_in_the_cooperative_form_and_in_listed_tail_launches(gpu, oracle, monkeypatch, N, tail_max, form):
    monkeypatch.delenv("OKENV_TAIL_MAX_AGENTS", raising=False)
    monkeypatch.delenv("OKENV_LANES_PER_AGENT", raising=False)
    if tail_max is not None:  # (the cooperative form, in the handle's natural 32-lane groups: phase 1 and the dealt phase 2)
        monkeypatch.setenv("OKENV_TAIL_MAX_AGENTS", tail_max)
        monkeypatch.setenv("OKENV_LANES_PER_AGENT", "32")
    t, dev, orc, ga = make_ga(gpu, oracle, "Monza", N, 32)
    start = (float(t.x[3]), float(t.y[3]), float(t.heading[0]))
    dev.reset_all(*start)
    ga.reset_all(*start)
    dev.step(1)
    orc.step(1)
    dev.step_forms(clear=True)
    cap = 400
    want = oracle_ga_loop(orc, ga, cap)
    dev.episode_begin()
    taken = 0
    while taken < cap:
        n = min(25, cap - taken)
        dev.rollout_policy(n)
        taken += n
        alive, listed = dev.episode_compact()
        if alive == 0:
            break
    assert dev.episode_end() == want
    assert_same_state(dev.snapshot(), orc.snapshot(), "%s episode" % form)
    assert np.array_equal(dev.ga_scores(), ga.scores())
    forms = dev.step_forms(clear=True)["forms"]
    assert form in forms, forms
    dev.close()
