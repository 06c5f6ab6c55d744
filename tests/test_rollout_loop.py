"""The episode loop of rollout.py's four collectors, driven on the CPU with a stub environment that logs every call: the stopping rule,
the number of synchronising alive_count() calls, the order act -> step -> push, the draw-offset word of a captured chunk and the caches
of captured chunks.  The GPU tests compare eager and chunked episodes bit for bit but only sample these mechanics; nothing here needs
libokenv.so or a GPU."""
import itertools

import pytest
import torch

from openkitchen_amd import _capi as capi
from openkitchen_amd import rollout

N, R = 3, 2
LAST = (1, 5, 8, 9)            # the step in which the last agent crashes: alive_count() is 0 from then on
CHECK_EVERY = (1, 4, 8)
MAX_STEPS = (None, 6, 16)
CHUNK = (0, 1, 4)


class _Graph:
    """What a captured graph is to the caller: replay() runs the body with the draw-offset word the launches were captured with; the
    host's step count does not move."""

    def __init__(self, venv, body, word):
        self.venv, self.body, self.word = venv, body, word

    def replay(self):
        env = self.venv.env
        count, env.replaying = env.count, self
        try:
            self.body()
        finally:
            env.count, env.replaying = count, None


class _StubEnv:
    """venv.env: the host step count (a uint32, as in the C ABI), alive_count and the two draw-offset setters."""

    def __init__(self, venv, count):
        self.venv, self.count, self.draw_offset, self.replaying = venv, count % 2 ** 32, None, None

    @property
    def step_count(self):
        return self.count

    @step_count.setter
    def step_count(self, value):
        self.venv.log.append(("set_step_count", int(value) % 2 ** 32))
        self.count = int(value) % 2 ** 32

    def alive_count(self):
        self.venv.log.append(("alive_count",))
        return 0 if self.venv.t >= self.venv.last else 1

    def _set_draw_offset(self, name, word):
        self.venv.log.append((name, word))
        self.draw_offset = word

    def actor_set_draw_offset(self, word=None):
        self._set_draw_offset("actor_set_draw_offset", word)

    def ddpg_set_draw_offset(self, word=None):
        self._set_draw_offset("ddpg_set_draw_offset", word)


class _StubVenv:
    """The attributes and methods of VectorEnvironment that the collectors use, with tensors on the CPU.  `t` counts the steps since
    reset(); the act methods write it into the record, so that the rows of an episode and the pushes can be told apart."""

    def __init__(self, auto_reset=False, count=100):
        self.device = torch.device("cpu")
        self.num_envs, self.num_rays = N, R
        self.reward_kind, self.auto_reset = capi.REWARD_STEP, auto_reset
        self.actor_has_value = False
        self._actor_nets = self._ddpg_nets = object()
        self.replay_push_all = self.ddpg_push_all = False
        self._actor_graphs, self._ddpg_graphs = {}, {}
        self.reward = torch.zeros(N)
        self.done = torch.zeros(N, dtype=torch.bool)
        self.distances = torch.zeros(N, R)
        self.log, self.t, self.last, self.fail_capture = [], 0, 1, False
        self.base = {}  # (collector, K) -> the host's count at the capture, as the test reckons it
        self.env = _StubEnv(self, count)

    def reset(self):
        self.log.append(("reset",))
        self.t = 0
        self.env.count = (self.env.count + 1) % 2 ** 32  # the step for the initial observation
        self.done.fill_(False)
        self.reward.zero_()

    def observation(self):
        return self.distances / 200.0

    def step(self, actions=None):
        self.log.append(("step",))
        self.t += 1
        self.env.count = (self.env.count + 1) % 2 ** 32
        self.reward.fill_(float(self.t))
        self.done.fill_(self.t >= self.last)
        self.distances.fill_(float(self.t))

    def _act(self, name, record):
        # the word a launch adds to its draw index: the one it was captured with, none for an eager call
        graph = self.env.replaying
        word = self.env.draw_offset if graph is None else graph.word
        self.log.append((name, self.t, None if word is None else int(word.item()), graph is not None, record["state"].data_ptr()))
        record["state"].fill_(float(self.t))
        record["action"].fill_(self.t)
        record["alive"].fill_(1 if self.t < self.last else 0)
        if "prob" in record:
            record["prob"].fill_(1.0 / (self.t + 2))

    def actor_act(self, record=None):
        self._act("actor_act", record)

    def ddpg_act(self, record=None):
        self._act("ddpg_act", record)

    def _push(self, name, record, reward):
        assert set(record) >= {"state", "action", "alive"}
        self.log.append((name, int(record["state"].reshape(-1)[0]), reward))

    def replay_push(self, record, reward=None):
        self._push("replay_push", record, reward)

    def ddpg_replay_push(self, record, reward=None):
        self._push("ddpg_replay_push", record, reward)

    def capture(self, body, warmup=3):
        assert warmup == 0, "warm-up iterations would move the count the launches are captured with"
        self.log.append(("capture",))
        if self.fail_capture:
            raise RuntimeError("capture failed")
        return _Graph(self, body, self.env.draw_offset)

    def names(self, *wanted):
        return [e for e in self.log if e[0] in wanted]


def _policy(state):
    return torch.full((state.shape[0], 3), 1.0 / 3.0)


# name -> (collector(venv, **kw), act, push, draw-offset setter, the cache of captured chunks)
COLLECTORS = {
    "host": (lambda venv, **kw: rollout.collect_episode(venv, _policy, **kw), None, None, None, None),
    "device": (rollout.collect_episode_device, "actor_act", None, "actor_set_draw_offset", "_actor_graphs"),
    "dqn": (rollout.collect_episode_dqn, "actor_act", "replay_push", "actor_set_draw_offset", "_actor_graphs"),
    "ddpg": (rollout.collect_episode_ddpg, "ddpg_act", "ddpg_replay_push", "ddpg_set_draw_offset", "_ddpg_graphs"),
}


def _expected_steps(last, check_every, max_steps, K):
    """The stopping rule as the collectors document it: after each iteration (each chunk of K with a graph) stop if this is a step at
    which the agents are counted (a multiple of check_every; every chunk) and nobody is alive, else if max_steps is reached."""
    steps = 0
    while True:
        steps += K if K else 1
        counted = True if K else steps % check_every == 0
        if counted and steps >= last:
            return steps
        if max_steps is not None and steps >= max_steps:
            return steps


def _int32(x):
    return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31


def _run(venv, name, last, check_every, max_steps, K):
    """One episode on `venv` with everything the issue of the loop can be asked for asserted; returns (start, steps)."""
    collect, act, push, setter, _ = COLLECTORS[name]
    case = "%s L=%d check_every=%d max_steps=%s K=%d auto_reset=%s" % (name, last, check_every, max_steps, K, venv.auto_reset)
    venv.last, venv.log = last, []
    before = venv.env.count
    kw = {"graph_chunk": K} if name != "host" else {}
    res = collect(venv, max_steps=max_steps, check_every=check_every, **kw)
    start = (before + 1) % 2 ** 32
    want = _expected_steps(last, check_every, max_steps, K)
    steps = res["steps"] if "steps" in res else venv.t
    assert steps == want and venv.t == want, case
    assert venv.log[0] == ("reset",) and len(venv.names("reset")) == 1, case
    assert len(venv.names("alive_count")) == (want // K if K else want // check_every), case
    # act, step and push in order, the push seeing the record of its own iteration
    trace = venv.names(*[n for n in (act, "step", push) if n])
    per = 1 + (act is not None) + (push is not None)
    assert len(trace) == per * want, case
    for i in range(want):
        it = trace[per * i:per * (i + 1)]
        assert [e[0] for e in it] == [n for n in (act, "step", push) if n], case
        if act:
            assert it[0][1] == i and it[0][3] == (K > 0), case
        if push:
            assert it[-1][1] == i, case
    # the draw-offset word: none for eager launches; for replayed ones start - base at the episode's first iteration, K more per chunk
    words = [e[2] for e in venv.names(act)] if act else []
    if K == 0 or venv.auto_reset:
        assert all(w is None for w in words), case
    else:
        base = venv.base[name, K] = venv.base.get((name, K), start)  # captured in the first episode with this K, right after its reset
        assert words == [_int32(start - base + K * (i // K)) for i in range(want)], case
    # the host's count: replays do not advance it, so the collector moves it once; eager steps have advanced it already
    assert venv.names("set_step_count") == ([("set_step_count", (start + want) % 2 ** 32)] if K and not venv.auto_reset else []), case
    assert venv.env.step_count == (start if K and venv.auto_reset else (start + want) % 2 ** 32), case
    assert venv.env.draw_offset is None, case
    if setter:
        assert all(e[0] == setter for e in venv.log if e[0].endswith("_set_draw_offset")), case
    # what the first two collectors return
    if name in ("host", "device"):
        T = want
        if name == "device":
            T = want if venv.auto_reset else min(last, want)
            T = T if max_steps is None else min(T, max_steps)
            assert torch.equal(res["states"][:, 0, 0], torch.arange(T, dtype=torch.float32)), case
            assert torch.equal(res["actions"][:, 1], torch.arange(T)), case
            assert torch.equal(res["log_probs"][:, 2], torch.log(1.0 / (torch.arange(T, dtype=torch.float32) + 2))), case
            assert venv._episode_probs[0] is res["log_probs"] and torch.equal(torch.log(venv._episode_probs[1]), res["log_probs"]), case
            assert venv._episode_draw_first[0] is res["log_probs"] and venv._episode_draw_first[1] == start, case
        assert res["states"].shape == (T, N, R) and res["actions"].shape == (T, N) and res["alive"].shape == (T, N), case
        assert torch.equal(res["rewards"][:, 0], torch.arange(1, T + 1, dtype=torch.float32)), case
        assert torch.equal(res["alive"][:, 0], torch.arange(T) < last), case
    return start, want


def _cases(auto_reset):
    return [c for c in itertools.product(LAST, CHECK_EVERY, MAX_STEPS) if c[2] is not None or not auto_reset]


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("name,K", [("host", 0)] + [(n, K) for n in ("device", "dqn", "ddpg") for K in CHUNK])
def test_stopping_rule_sync_calls_and_draw_offset(name, K, auto_reset):
    """The whole grid of (last living step, check_every, max_steps) as successive episodes on one environment: every episode after the
    first finds its chunk in the cache, and its offset word is the distance of its start from the capture's."""
    venv = _StubVenv(auto_reset=auto_reset)
    captures = 0
    for last, check_every, max_steps in _cases(auto_reset):
        _run(venv, name, last, check_every, max_steps, K)
        captured = venv.names("capture")
        captures += len(captured)
        if captured:  # the offset is set for the capture alone
            setter = COLLECTORS[name][3]
            events = [e for e in venv.log if e[0] in ("capture", setter)]
            assert [e[0] for e in events] == [setter, "capture", setter] and events[2][1] is None
            assert (events[0][1] is None) == auto_reset
    assert captures == (1 if K else 0)
    if K:
        assert len(getattr(venv, COLLECTORS[name][4])) == 1


@pytest.mark.parametrize("name", ["device", "dqn", "ddpg"])
def test_offset_word_wraps_with_the_step_count(name):
    """The host's count is a uint32 and the word an int32 that the kernel adds to it: an episode that starts past the wrap, or below
    the count of the capture, still gets start - base modulo 2^32."""
    venv = _StubVenv(count=2 ** 32 - 4)
    start, steps = _run(venv, name, 9, 8, None, 4)
    assert start == 2 ** 32 - 3 and (start + steps) % 2 ** 32 == 9
    assert _run(venv, name, 5, 8, None, 4)[0] == 10  # start - base = 13 - 2^32: read as +13
    venv.env.count = 2 ** 32 - 40
    assert _run(venv, name, 5, 8, None, 4)[0] == 2 ** 32 - 39  # below the capture's count: a negative word
    assert len(venv.names("capture")) == 0


@pytest.mark.parametrize("name", ["device", "dqn", "ddpg"])
def test_draw_offset_is_removed_when_capture_raises(name):
    collect, _, _, setter, cache = COLLECTORS[name]
    venv = _StubVenv()
    venv.fail_capture = True
    with pytest.raises(RuntimeError, match="capture failed"):
        collect(venv, graph_chunk=4)
    events = [e for e in venv.log if e[0] == setter]
    assert len(events) == 2 and events[0][1] is not None and events[1][1] is None and venv.env.draw_offset is None
    assert not getattr(venv, cache)
    venv.fail_capture = False
    _run(venv, name, 5, 8, None, 4)  # the next episode captures and runs
    assert len(venv.names("capture")) == 1 and len(getattr(venv, cache)) == 1


def test_caches_of_captured_chunks():
    """One graph per (collector, K, reward tensor); the device collector and the Deep-Q collector share _actor_graphs under distinct keys;
    an emptied cache (what set_actor_epsilon, set_actor_dropout and enable_replay do) makes the next episode capture again."""
    venv = _StubVenv()
    count = lambda: len(venv.names("capture"))  # noqa: E731
    _run(venv, "device", 5, 8, None, 4)
    assert count() == 1 and len(venv._actor_graphs) == 1
    _run(venv, "dqn", 5, 8, None, 4)
    assert count() == 1 and len(venv._actor_graphs) == 2
    for name in ("device", "dqn"):
        _run(venv, name, 8, 8, None, 4)
        assert count() == 0 and len(venv._actor_graphs) == 2
    _run(venv, "dqn", 5, 8, None, 1)  # another K: another graph
    assert count() == 1 and len(venv._actor_graphs) == 3
    _run(venv, "ddpg", 5, 8, None, 4)
    assert count() == 1 and len(venv._ddpg_graphs) == 1 and len(venv._actor_graphs) == 3
    venv._actor_graphs, venv._ddpg_graphs, venv.base = {}, {}, {}
    for name in ("device", "dqn", "ddpg"):
        _run(venv, name, 5, 8, None, 4)
        assert count() == 1
    assert len(venv._actor_graphs) == 2 and len(venv._ddpg_graphs) == 1


@pytest.mark.parametrize("name", ["dqn", "ddpg"])
@pytest.mark.parametrize("K", [0, 4])
def test_reward_argument_reaches_the_push(name, K):
    """reward=None, "tracker" (the environment's own tensor) or a tensor of the caller's: handed to every push as it is, and a chunk
    captured with one reward tensor is not replayed for another."""
    collect, _, push, _, cache = COLLECTORS[name]
    venv = _StubVenv()
    mine = torch.zeros(N)
    venv.last = 5
    for reward, want in ((None, None), ("tracker", venv.reward), (mine, mine)):
        first = len(venv.log)
        assert collect(venv, graph_chunk=K, reward=reward) == {"steps": 8}
        pushes = [e for e in venv.log[first:] if e[0] == push]
        assert len(pushes) == 8 and all(e[2] is want for e in pushes)
        assert len([e for e in venv.log[first:] if e[0] == "capture"]) == (1 if K else 0)
    assert len(getattr(venv, cache)) == (3 if K else 0)
    if K == 0:  # the eager record is made once per environment
        collect(venv)
        assert len({e[4] for e in venv.log if e[0].endswith("_act")}) == 1
