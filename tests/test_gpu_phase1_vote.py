"""The wave's vote that ends phase 1 of the raycast, on the GPU (ok_raycast.h: ok_cast_poly_interval<.., .., .., kVote>;
okenv_kernels.h: every okStepCoopKernel form with a phase 1 passes OKENV_VOTE).  Where phase 1 ends moves cells between the two
phases and nothing else, so snapshots equal the oracle's on every field, bit for bit --
  * 40 agents x 64 rays and 40 x 16 for 130 steps of the bench driver in launches of 1, 20 and 109, the handle held to the fan's
    width so that phase 1 exists: one agent per wave (one origin per vote) and four (the vote runs across agents; crashed agents'
    lanes never enter it),
  * 8 x 64 with origins outside the grid box and in cells on its border: waves that take the generic set-up, and rays that leave
    the grid inside phase 1 while others are cut by the vote,
  * a 32-ray MLP episode of 64 agents in the cooperative policy form (two agents per wave),
  * a 16-ray Q-learning episode of 64 agents in the cooperative Q form (four agents per wave, 32 px phase 1)."""
import numpy as np
import pytest

from test_gpu_episode import make_ga, make_q, oracle_ga_loop
from test_gpu_parity import assert_same_state, bits, make_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,R", [(40, 64), (40, 16)])
def test_bench_driver_one_and_four_agents_per_wave(gpu, oracle, monkeypatch, N, R):
    # (so small a population would be widened to 64 lanes per agent and lose phase 1)
    monkeypatch.setenv("OKENV_LANES_PER_AGENT", str(R))
    t, dev, orc = make_pair(gpu, oracle, "Silverstone", N, R)
    info = dev.info()
    assert info["lanes_per_agent"] == R  # (the natural width: okPlanLanes keeps phase 1)
    dev.init_bench_state(0, 0)
    orc.init_bench_state(0, 0)
    done = 0
    for n in (1, 20, 109):
        dev.rollout_random(n, 1234, 0, done)
        orc.rollout_random(n, 1234, 0, done, threads=8)
        done += n
        assert_same_state(dev.snapshot(), orc.snapshot(), "%d x %d after %d steps" % (N, R, done))
    dev.close()


def test_origins_outside_the_box_and_in_border_cells(gpu, oracle, monkeypatch):
    monkeypatch.setenv("OKENV_LANES_PER_AGENT", "64")
    N, R = 8, 64
    t, dev, orc = make_pair(gpu, oracle, "Silverstone", N, R)
    seg = t.segments
    lo_x, hi_x = float(seg[:, [0, 2]].min()), float(seg[:, [0, 2]].max())
    lo_y, hi_y = float(seg[:, [1, 3]].min()), float(seg[:, [1, 3]].max())
    mid_x, mid_y = 0.5 * (lo_x + hi_x), 0.5 * (lo_y + hi_y)
    info = dev.info()
    assert info["lanes_per_agent"] == 64 and info["front_back_bytes"] > 0
    cell = info["grid_cell"]
    # two outside the box (looking in, looking away), one far from it; two in the first and the last column of cells, one of them
    # right on the box's border; two on the centre line
    x = np.array([lo_x - 30.0, hi_x + 5.0, mid_x, lo_x + 0.3 * cell, hi_x - 0.3 * cell, lo_x, t.x[400], t.x[900]], np.float32)
    y = np.array([mid_y, mid_y, hi_y + 400.0, mid_y, mid_y, mid_y + 7.0, t.y[400], t.y[900]], np.float32)
    rot = np.array([0.0, 0.0, -90.0, 180.0, 0.0, 135.0, t.heading[400], t.heading[900]], np.float32)
    idx = np.arange(N, dtype=np.int32)
    for e in (dev, orc):
        e.reset_agents(idx, x, y, rot)
    rng = np.random.default_rng(5)
    for step in range(8):
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
    assert (o["dist"][2] > np.float32(199.9)).all() and (o["dist"][6:] < np.float32(199.0)).any()
    dev.close()


def test_mlp_episode_two_agents_per_wave(gpu, oracle, monkeypatch):
    monkeypatch.setenv("OKENV_TAIL_MAX_AGENTS", "0")
    monkeypatch.setenv("OKENV_LANES_PER_AGENT", "32")
    t, dev, orc, ga = make_ga(gpu, oracle, "Spa", 64, 32)
    assert dev.info()["lanes_per_agent"] == 32
    start = (float(t.x[7]), float(t.y[7]), float(t.heading[7]))
    dev.reset_all(*start)
    ga.reset_all(*start)
    dev.step(1)
    orc.step(1)
    dev.step_forms(clear=True)
    cap = 300
    want = oracle_ga_loop(orc, ga, cap)
    dev.episode_begin()
    taken = 0
    while taken < cap:
        n = min(30, cap - taken)
        dev.rollout_policy(n)
        taken += n
        alive, listed = dev.episode_compact()
        if alive == 0:
            break
    assert dev.episode_end() == want
    assert_same_state(dev.snapshot(), orc.snapshot(), "coop_mlp32 episode")
    assert np.array_equal(dev.ga_scores(), ga.scores())
    forms = dev.step_forms(clear=True)["forms"]
    assert "coop_mlp32" in forms, forms
    dev.close()


def test_q_learning_episode_four_agents_per_wave(gpu, oracle, monkeypatch):
    monkeypatch.setenv("OKENV_TAIL_MAX_AGENTS", "0")
    monkeypatch.setenv("OKENV_LANES_PER_AGENT", "16")
    t, dev, orc, oq = make_q(gpu, oracle, "Monza", 64, 16)
    info = dev.info()
    assert info["lanes_per_agent"] == 16
    dev.q_begin_episode(3)
    oq.begin_episode(3)
    dev.step_forms(clear=True)
    for chunk, n in enumerate((1, 40, 60, 60, 60)):
        base = sum((1, 40, 60, 60, 60)[:chunk])
        dev.rollout_q(n, 0.9, 77, 0, base)
        oq.rollout(n, 0.9, 77, 0, base)
        assert_same_state(dev.snapshot(), orc.snapshot(), "chunk %d" % chunk)
        for got, want in zip(dev.q_state(), oq.state()):
            assert np.array_equal(got, want), chunk
        assert np.array_equal(bits(dev.q_table()), bits(oq.table())), chunk
    forms = dev.step_forms(clear=True)["forms"]
    assert "coop_q" in forms, forms
    dev.close()
