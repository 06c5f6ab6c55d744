"""Every step-kernel form the launcher can pick, forced by a row of tests/_step_forms.py and compared with the oracle bit for bit.

Each row asserts (1) that okenv_debug_step_forms saw the row's form run, with the row's attributes, and nothing outside the row's
set of forms, and (2) that the state after the run -- and, for the policy rows, the Q tables, the MLP weights after ga_select_mate,
the tracker's bookkeeping, the episode's step count and live agent-steps -- equals the oracle's.  Populations are derived from the
device's compute units, so that a row forces its form in any partition mode (tests/test_step_form_table.py checks that on the CPU
for 32, 128 and 256 CUs)."""
import numpy as np
import pytest

import _step_forms as T
from test_gpu_episode import make_ga, make_q, oracle_ga_loop
from test_gpu_parity import assert_same_state, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(gpu):
    t = gpu.Track("Austin")
    probe = gpu.BatchedEnvironment(t.segments, 1, gpu.default_ray_fan(5))
    c = probe.info()["compute_units"]
    probe.close()
    assert c > 0
    return c


class Tally:
    """step_forms() of the calls under test, summed: the set-up's own steps (the initial observation of the policy rollouts,
    okenv_step) are read and dropped by skip()"""

    def __init__(self):
        self.forms, self.attrs = {}, {}

    def take(self, dev):
        sf = dev.step_forms(clear=True)
        for f, n in sf["forms"].items():
            self.forms[f] = self.forms.get(f, 0) + n
            a = self.attrs.setdefault(f, dict.fromkeys(sf["attrs"][f], 0))
            for k, v in sf["attrs"][f].items():
                a[k] += v

    def skip(self, dev):
        dev.step_forms(clear=True)

    def result(self):
        return {"forms": self.forms, "attrs": self.attrs}


def window(snapshot, lo, n):
    return {k: v[lo:lo + n] for k, v in snapshot.items()}


# ---- drivers: one call sequence each, every one compared with the oracle ---------------------------------------------------

def d_step(gpu, oracle, row, N, R, attach, tally):
    """Environment::step with host actions, one launch per step: crashes (and their stale rays) and, from the agents that never
    move, standstill timeouts after 200 steps."""
    from test_gpu_parity import make_pair
    t, dev, orc = make_pair(gpu, oracle, row["track"], N, R, flags=row["flags"])
    rng = np.random.default_rng(N + R)
    idx = rng.integers(0, t.P, N)
    for e in (dev, orc):
        e.reset_agents(np.arange(N), t.x[idx], t.y[idx], t.heading[idx])
    mode = (np.arange(N) % 2).astype(np.uint8)
    dev.set(gpu.capi.F_MODE, mode)
    orc.set(oracle.F_MODE, mode)
    timed_out = crashed = False
    for s in range(215):
        thr = rng.uniform(0, 60, N).astype(np.float32)
        thr[:3] = 0.0
        steer = rng.uniform(-3, 3, N).astype(np.float32)
        dev.set_actions(thr, steer)
        orc.set(oracle.F_THR, thr)
        orc.set(oracle.F_STEER, steer)
        dev.step(1)
        orc.step(1)
        if s % 43 == 0 or s == 214:
            o = orc.snapshot()
            assert_same_state(dev.snapshot(), o, "%s step %d" % (row["id"], s))
            timed_out |= bool(o["timed_out"].any())
            crashed |= bool(o["crashed"].any())
    assert timed_out and crashed
    return dev, {}


def d_random(gpu, oracle, row, N, R, attach, tally):
    from test_gpu_parity import make_pair
    t, dev, orc = make_pair(gpu, oracle, row["track"], N, R, flags=row["flags"])
    dev.init_bench_state(0, 0)
    orc.init_bench_state(0, 0)
    done, crashed = 0, False
    for n in (1, 60, 90, 80):
        dev.rollout_random(n, 1234, 0, done)
        orc.rollout_random(n, 1234, 0, done, threads=8)
        done += n
        o = orc.snapshot()
        assert_same_state(dev.snapshot(), o, "%s after %d steps" % (row["id"], done))
        crashed |= bool(o["crashed"].any())
    assert crashed
    return dev, {}


def d_random_window(gpu, oracle, row, N, R, attach, tally):
    """A population of several rounds of workgroups: windows of it (its start, its middle, its ragged end) against the oracle
    stepping those windows' global agent ids."""
    W = 40
    t = gpu.Track(row["track"])
    fan = gpu.default_ray_fan(R)
    dev = gpu.BatchedEnvironment.from_track(t, N, num_rays=R)
    bases = [0, N // 2 - W // 2, N - W]
    orcs = [oracle.OracleEnv(t.segments, W, R, fan, (t.x, t.y, t.heading)) for _ in bases]
    dev.init_bench_state(0, 0)
    for o, b in zip(orcs, bases):
        o.init_bench_state(b, 0)
    done = 0
    for n in (1, 40, 60):
        dev.rollout_random(n, 4321, 0, done)
        for o, b in zip(orcs, bases):
            o.rollout_random(n, 4321, b, done, threads=8)
        done += n
        snap = dev.snapshot()
        for o, b in zip(orcs, bases):
            assert_same_state(window(snap, b, W), o.snapshot(), "%s window %d after %d steps" % (row["id"], b, done))
    assert (snap["crashed"] == 1).any()
    return dev, {}


def d_packed(gpu, oracle, row, N, R, attach, tally, steps=220):
    from test_gpu_resident import Run, make
    run = Run(gpu, oracle, *make(gpu, oracle, N, R, track=row["track"], seed=N))
    run.steps(steps)
    assert run.dev.step_count == steps
    assert run.check() == steps
    return run.dev, {}


def d_resident(gpu, oracle, row, N, R, attach, tally):
    dev, info = d_packed(gpu, oracle, row, N, R, attach, tally, steps=300)
    assert dev.info()["packed_resident_steps"] == 300
    return dev, info


def _attach_others(dev, kind):
    """the policies a single-policy handle of `kind` does not have"""
    if kind != "mlp":
        dev.policy_mlp_create(16, 99, 0)
    if kind != "q":
        dev.q_create()
    if kind != "ctrl":
        dev.controller_create(16)
        dev.tracker_create(1)


def d_ga_episode(gpu, oracle, row, N, R, attach, tally):
    t, dev, orc, ga = make_ga(gpu, oracle, row["track"], N, R, flags=row["flags"])
    if attach:
        _attach_others(dev, "mlp")
    start = (float(t.x[3]), float(t.y[3]), float(t.heading[0]))
    trace = []
    for generation in range(2):
        tally.take(dev)
        dev.reset_all(*start)
        ga.reset_all(*start)
        dev.step(1)
        orc.step(1)
        tally.skip(dev)   # (the initial observation)
        want = oracle_ga_loop(orc, ga, 1500)
        dev.episode_begin()
        taken, listed_trace = 0, []
        while taken < 1500:
            n = min(25, 1500 - taken)
            dev.rollout_policy(n)
            if taken == 0:
                trace.append(dev.episode_tail_limit())
            taken += n
            alive, listed = dev.episode_compact()
            listed_trace.append(listed)
            if alive == 0:
                break
        steps, live = dev.episode_end()
        trace.append(listed_trace)
        assert (steps, live) == want, (row["id"], generation, steps, live, want)
        assert_same_state(dev.snapshot(), orc.snapshot(), "%s generation %d" % (row["id"], generation))
        assert np.array_equal(dev.ga_scores(), ga.scores())
        assert np.array_equal(dev.ga_select_mate(5, generation), ga.select_mate(5, generation))
        assert np.array_equal(bits(dev.policy_weights()), bits(ga.weights()))
    return dev, {"trace": trace}


def d_ga_plain(gpu, oracle, row, N, R, attach, tally):
    t, dev, orc, ga = make_ga(gpu, oracle, row["track"], N, R, flags=row["flags"])
    rng = np.random.default_rng(N)
    idx = rng.integers(0, t.P, N)
    for e in (dev, orc):
        e.reset_agents(np.arange(N), t.x[idx], t.y[idx], t.heading[idx])
    dev.step(1)
    orc.step(1)
    tally.skip(dev)
    for n in (1, 60, 160):
        dev.rollout_policy(n)
        ga.rollout_policy(n)
        assert_same_state(dev.snapshot(), orc.snapshot(), row["id"])
    assert orc.snapshot()["crashed"].any()
    assert np.array_equal(dev.ga_scores(), ga.scores())
    assert np.array_equal(dev.ga_select_mate(5, 0), ga.select_mate(5, 0))
    assert np.array_equal(bits(dev.policy_weights()), bits(ga.weights()))
    return dev, {}


def d_ga_window(gpu, oracle, row, N, R, attach, tally):
    W, seed, hidden = 48, 1234, 30
    BASE = N - W   # the last, partly filled workgroup
    t = gpu.Track(row["track"])
    dev = gpu.BatchedEnvironment.from_track(t, N, num_rays=R)
    dev.set(gpu.capi.F_MODE, np.ones(N, dtype=np.uint8))
    dev.policy_mlp_create(hidden, seed, 0)
    fan = gpu.default_ray_fan(R)
    orc = oracle.OracleEnv(t.segments, W, R, fan, (t.x, t.y, t.heading))
    orc.set(oracle.F_MODE, np.ones(W, dtype=np.uint8))
    ga = oracle.OracleGA(orc, hidden, seed, BASE)
    rng = np.random.default_rng(3)
    idx = rng.integers(0, t.P, N)
    dev.reset_agents(np.arange(N), t.x[idx], t.y[idx], t.heading[idx])
    orc.reset_agents(np.arange(W), t.x[idx[BASE:]], t.y[idx[BASE:]], t.heading[idx[BASE:]])
    dev.step(1)
    orc.step(1)
    tally.skip(dev)
    for n in (1, 40, 80):
        dev.rollout_policy(n)
        ga.rollout_policy(n)
        assert_same_state(window(dev.snapshot(), BASE, W), orc.snapshot(), row["id"])
    assert orc.snapshot()["crashed"].any()
    assert np.array_equal(bits(dev.policy_weights()[BASE:BASE + W]), bits(ga.weights()))
    assert np.array_equal(dev.ga_scores()[BASE:BASE + W], ga.scores())
    return dev, {}


def d_q_episode(gpu, oracle, row, N, R, attach, tally):
    t, dev, orc, oq = make_q(gpu, oracle, row["track"], N, R)
    if attach:
        _attach_others(dev, "q")
    seed, eps, total, trace = 31, np.float32(0.9), 0, []
    for episode, reset_idx in enumerate((3, 700)):
        tally.take(dev)
        dev.q_begin_episode(reset_idx)
        oq.begin_episode(reset_idx)
        tally.skip(dev)   # (its initial observation)
        want_steps, want_live = 0, 0
        while want_steps < 1000:
            want_live += oracle.lib().oracle_env_alive_count(orc.h)
            oq.rollout(1, float(eps), seed, 0, total + want_steps)
            want_steps += 1
            if oracle.lib().oracle_env_alive_count(orc.h) == 0:
                break
        dev.episode_begin()
        taken, listed_trace = 0, []
        while taken < 1000:
            n = min(25, 1000 - taken)
            dev.rollout_q(n, float(eps), seed, 0, total + taken)
            if taken == 0:
                trace.append(dev.episode_tail_limit())
            taken += n
            alive, listed = dev.episode_compact()
            listed_trace.append(listed)
            if alive == 0:
                break
        trace.append(listed_trace)
        steps, live = dev.episode_end()
        assert (steps, live) == (want_steps, want_live), (row["id"], episode)
        total += steps
        assert_same_state(dev.snapshot(), orc.snapshot(), "%s episode %d" % (row["id"], episode))
        assert np.array_equal(bits(dev.q_table()), bits(oq.table()))
        for got, want in zip(dev.q_state(), oq.state()):
            assert np.array_equal(got, want)
        eps = eps - np.float32(0.05)
    return dev, {"trace": trace}


def d_q_plain(gpu, oracle, row, N, R, attach, tally):
    t, dev, orc, oq = make_q(gpu, oracle, row["track"], N, R)
    seed, eps = 77, 0.9
    dev.q_begin_episode(3)
    oq.begin_episode(3)
    tally.skip(dev)
    done = 0
    for n in (1, 40, 170):
        dev.rollout_q(n, eps, seed, 0, done)
        oq.rollout(n, eps, seed, 0, done)
        done += n
        assert_same_state(dev.snapshot(), orc.snapshot(), "%s after %d steps" % (row["id"], done))
        assert np.array_equal(bits(dev.q_table()), bits(oq.table()))
        for got, want in zip(dev.q_state(), oq.state()):
            assert np.array_equal(got, want)
    assert orc.snapshot()["crashed"].any()
    return dev, {}


def _ctrl_make(gpu, oracle, row, N, R, kind):
    from test_gpu_rollout_controller import RAYS, make
    fan = RAYS if R == 5 else gpu.default_ray_fan(R)
    return make(gpu, oracle, row["track"], N, fan, row["hidden"], kind, seed=row["hidden"] + R)


def d_ctrl(gpu, oracle, row, N, R, attach, tally):
    from test_gpu_rollout_controller import oracle_iteration, same_everything
    t, dev, orc, params, rng = _ctrl_make(gpu, oracle, row, N, R, 1)
    tally.skip(dev)
    done = 0
    for n in (1, 30, 110, 70):   # standstill timeouts at step 201
        dev.rollout_controller(n, 100.0, 5.0)
        for _ in range(n):
            oracle_iteration(oracle, orc, params, row["hidden"])
        done += n
        same_everything(gpu, oracle, dev, orc, "%s after %d steps" % (row["id"], done))
    assert dev.get(gpu.capi.F_CRASHED).any()
    return dev, {}


def d_ctrl_episode(gpu, oracle, row, N, R, attach, tally):
    from test_gpu_rollout_controller import oracle_iteration, same_everything
    t, dev, orc, params, rng = _ctrl_make(gpu, oracle, row, N, R, 1)
    tally.skip(dev)
    if attach:
        _attach_others(dev, "ctrl")
    T_ = 0
    while T_ < 1500:
        oracle_iteration(oracle, orc, params, row["hidden"])
        T_ += 1
        if orc.get(oracle.F_CRASHED).all():
            break
    dev.episode_begin()
    taken, listed_trace, trace = 0, [], []
    while taken < 1500:
        n = min(16, 1500 - taken)
        dev.rollout_controller(n, 100.0, 5.0)
        if taken == 0:
            trace.append(dev.episode_tail_limit())
        taken += n
        alive, listed = dev.episode_compact()
        listed_trace.append(listed)
        if alive == 0:
            break
    steps, live = dev.episode_end()
    trace.append(listed_trace)
    assert steps == T_ and N <= live <= N * T_
    same_everything(gpu, oracle, dev, orc, "%s episode of %d steps" % (row["id"], T_))
    return dev, {"trace": trace}


DRIVERS = {"step": d_step, "random": d_random, "random_window": d_random_window, "packed": d_packed, "resident": d_resident,
           "ga_episode": d_ga_episode, "ga_plain": d_ga_plain, "ga_window": d_ga_window, "q_episode": d_q_episode, "q_plain": d_q_plain,
           "ctrl": d_ctrl, "ctrl_episode": d_ctrl_episode}


def run_row(gpu, oracle, monkeypatch, row, C, attach=False):
    for k in ("OKENV_FRONT_BACK", "OKENV_TAIL_MAX_AGENTS", "OKENV_LANES_PER_AGENT", "OKENV_COOP", "OKENV_RESIDENT", "OKENV_BLOCK_THREADS",
              "OKENV_AGENTS_PER_BLOCK", "OKENV_PHASE1_RANGE", "OKENV_RESIDENT_STALL_US"):
        monkeypatch.delenv(k, raising=False)
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    N, R = T.population(row, C), row["R"]
    tally = Tally()
    dev, extra = DRIVERS[row["driver"]](gpu, oracle, row, N, R, attach, tally)
    shape = T.handle_shape(N, R, C, row["env"], row["flags"])
    info = dev.info()
    assert info["compute_units"] == C
    assert (info["lanes_per_agent"], info["block_threads"], info["agents_per_block"]) == (shape["G"], shape["block_threads"], shape["agents_per_block"])
    tally.take(dev)
    dev.close()
    return tally.result(), extra


def check_forms(sf, row):
    forms, attrs = sf["forms"], sf["attrs"]
    f = row["form"]
    assert f in forms, "%s: %s did not run (ran: %s)" % (row["id"], f, forms)
    assert set(forms) <= set(row["forms"]), "%s: forms outside the row's set ran: %s" % (row["id"], forms)
    total = forms[f]
    for a, want in row["attrs"].items():
        n = attrs[f][a]
        ok = {"all": n == total, "none": n == 0, "some": 0 < n < total}[want]
        assert ok, "%s: attribute %s on %d of %d launches of %s, expected %s" % (row["id"], a, n, total, f, want)


@pytest.mark.parametrize("row", T.ROWS, ids=[r["id"] for r in T.ROWS])
def test_step_form_equals_oracle(gpu, oracle, monkeypatch, cus, row):
    sf, _ = run_row(gpu, oracle, monkeypatch, row, cus)
    check_forms(sf, row)
    print("%s (C=%d): %s" % (row["id"], cus, sf["forms"]))


@pytest.mark.parametrize("mrow", T.MULTI_ROWS, ids=[r["id"] for r in T.MULTI_ROWS])
def test_handle_with_every_policy_runs_the_single_policy_forms(gpu, oracle, monkeypatch, cus, mrow):
    """A handle with the MLP, Q-learning and controller policies attached picks, for each kind of episode, the forms, lists and
    tail limit of the single-policy handle of the same shape (okenv_episode_begin used to list the population by the policies
    attached, not by the rollout that follows), and equals the oracle."""
    row = next(r for r in T.ROWS if r["id"] == mrow["like"])
    single, s_extra = run_row(gpu, oracle, monkeypatch, row, cus)
    multi, m_extra = run_row(gpu, oracle, monkeypatch, row, cus, attach=True)
    check_forms(multi, row)
    assert multi == single
    assert m_extra["trace"] == s_extra["trace"]
