"""The Deep-Q image racers' rule (include/okenv_qcnn.h) without a GPU: the host entry okenv_qcnn_act_host against the float64 mirror,
the parameter layout and the flatten index against the PyTorch module, the grey against dqn_cnn.gray, the padding against a
zero-extended plane, the choice against the shared-network actor's, the frame ring's push and batch against the mirror, the limits of
the shape, the plan functions, every refusal, and the host side under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _population_cases as P
import _qcnn_numpy as mirror

f32 = np.float32
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3)

# The bound on |host entry - float64 mirror| of the Q-values, from the same frames (two of random bytes a seed) and fp32 parameters
# (mirror.draw_params): the largest deviation measured here on the CPU per shape over seeds 0 .. 3, times 4, the project's margin for an
# fp32 chain against float64 (DESIGN.md sections 25, 26 and 29).  Per seed the deviations were
#   tiny        7.75e-8, 1.94e-8, 1.06e-7, 4.14e-8        nopad       6.93e-8, 1.36e-8, 5.78e-8, 6.17e-8
#   odd         9.62e-8, 7.11e-8, 1.12e-7, 6.26e-8        wide        1.05e-7, 1.81e-7, 1.32e-7, 1.13e-7
#   deep_pad    1.07e-7, 6.14e-8, 1.08e-7, 5.93e-8        reference   1.22e-7, 8.10e-8, 1.19e-7, 8.67e-8
#   two_tiles   1.52e-7, 7.61e-8, 8.75e-8, 8.16e-8        three_tiles 1.23e-7, 1.02e-7, 1.06e-7, 6.57e-8
# with the largest |q| of a run between 0.078 (reference, seed 0) and 0.61 (the test holds it inside 0.01 .. 3, and a frame's Q-values
# apart, so that a wrong term shows).
MEASURED_DEVIATION = {"tiny": 1.07e-7, "nopad": 6.94e-8, "odd": 1.12e-7, "wide": 1.82e-7, "deep_pad": 1.09e-7, "reference": 1.22e-7,
                      "two_tiles": 1.52e-7, "three_tiles": 1.24e-7}
TOL = {name: 4 * v for name, v in MEASURED_DEVIATION.items()}


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def config(capi, name_or_members, **more):
    members = mirror.SHAPES[name_or_members] if isinstance(name_or_members, str) else name_or_members
    return capi.qcnn_config(**dict(members, **more))


@pytest.fixture(scope="module")
def host_runs(capi):
    """Per shape and seed: (deviation of the host entry's Q-values from the mirror's, the mirror's Q-values)."""
    runs = {}
    for name, cfg in mirror.SHAPES.items():
        assert mirror.sides(cfg) == mirror.SIDES[name] == capi.qcnn_sides(config(capi, name)) and mirror.features(cfg) == mirror.FEATURES[name]
        for seed in SEEDS:
            params, frames = mirror.draw_params(cfg, seed), mirror.draw_frames(cfg["image_size"], seed)
            want = mirror.forward(cfg, params, frames)
            got = capi.qcnn_act_host(config(capi, name), params, frames)
            assert got["q"].dtype == f32 and got["q"].shape == want.shape and np.isfinite(got["q"]).all()
            assert np.array_equal(got["action"], got["q"].argmax(1)) and np.array_equal(got["value"], got["q"].max(1))  # greedy
            table = np.array(capi.QCNN_ACTION_MAP, f32)
            if cfg["num_actions"] <= len(table):
                assert np.array_equal(got["throttle"], table[got["action"], 0]) and np.array_equal(got["steer"], table[got["action"], 1])
            assert np.array_equal(got["alive"], np.ones(2, np.uint8))
            runs[name, seed] = (float(np.abs(got["q"].astype(np.float64) - want).max()), want)
    return runs


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_host_entry_against_mirror(host_runs, name):
    for seed in SEEDS:
        dev, q = host_runs[name, seed]
        print("%s seed %d: deviation %.3e, largest |q| %.3f" % (name, seed, dev, float(np.abs(q).max())))
        assert 0.01 < np.abs(q).max() < 3, "the draw gives nothing or too much: a wrong term would not show"
        assert (q.max(1) - q.min(1) > 1e-4).all(), "a frame's Q-values must not all be equal"
    worst = max(host_runs[name, seed][0] for seed in SEEDS)
    assert worst <= TOL[name], (worst, TOL[name])


@pytest.mark.parametrize("S, sides, F", [(96, (24, 12, 12), 9216), (48, (12, 6, 6), 2304)])
def test_layout_equals_the_pytorch_module(capi, S, sides, F):
    from openkitchen_amd import dqn_cnn
    model = dqn_cnn.QCNN(S)
    sd = model.state_dict()
    cfg = dqn_cnn.qcnn_config_from_state_dict(sd, image_size=S)
    assert (cfg.image_size, tuple(cfg.kernel), tuple(cfg.stride), tuple(cfg.padding), tuple(cfg.channels), cfg.hidden, cfg.num_actions) == (
        S, (8, 4, 3), (4, 2, 1), (2, 1, 1), (32, 64, 64), 512, 5)
    assert capi.qcnn_sides(cfg) == sides and model.fc1.in_features == F
    assert [tuple(row) for row in cfg.action_table][:5] == [(60.0, 0.0), (30.0, 5.0), (30.0, -5.0), (30.0, 2.5), (30.0, -2.5)]
    members = dict(mirror.SHAPES["reference"], image_size=S)
    want = [(name, tuple(p.shape)) for name, p in model.named_parameters()]
    assert [(n, tuple(s)) for n, a, s in capi.qcnn_layout(cfg)] == want == [(n, tuple(s)) for n, a, s in mirror.layout(members)]
    assert [a for n, a, s in capi.qcnn_layout(cfg)] == [a for n, a, s in mirror.layout(members)]
    total = sum(p.numel() for p in model.parameters())
    assert capi.qcnn_num_params(cfg) == mirror.num_params(members) == total
    if S == 96:
        assert total == 4793509
    params = dqn_cnn.qcnn_params_from_state_dict(sd, image_size=S)
    assert torch.equal(params, torch.cat([p.detach().reshape(-1) for p in model.parameters()]))
    # the flatten index: fp32 torch against the fp32 host entry on the module's own weights, fc1 enlarged so that a wrong index shows
    # (a permutation of fc1's columns moves q by more than 1e-2; chains of up to 9216 terms agree to 1e-4)
    torch.manual_seed(S)
    with torch.no_grad():
        model.fc1.weight.mul_(4.0)
    frames = torch.from_numpy(mirror.draw_frames(S, 7, n=2))
    with torch.no_grad():
        want_q = model(dqn_cnn.gray(frames)).numpy()
        shuffled = model.fc2(torch.relu(model.fc1(torch.relu(model.conv3(torch.relu(model.conv2(torch.relu(model.conv1(
            dqn_cnn.gray(frames)[:, None])))))).permute(0, 2, 3, 1).flatten(1)))).numpy()
    got = capi.qcnn_act_host(cfg, dqn_cnn.qcnn_params_from_state_dict(model.state_dict(), image_size=S).numpy(), frames.numpy())["q"]
    print("torch vs host: %.3e; channels-last flatten moves q by %.3e" % (np.abs(got - want_q).max(), np.abs(shuffled - want_q).max()))
    assert np.abs(shuffled - want_q).max() > 1e-2 and np.abs(got - want_q).max() <= 1e-4


def test_grey_equals_torch_bit_for_bit(capi):
    """The rule's grey (okenv_debug_qcnn_grey_host) against dqn_cnn.gray on the CPU in fp32, and against the mirror's: every byte value in
    every channel occurs."""
    from openkitchen_amd import dqn_cnn
    frames = mirror.draw_frames(37, 11, n=3)
    frames[0, :16, :16, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    frames[1, :16, :16, 1] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    frames[2, :16, :16, 2] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    got = capi.qcnn_grey_host(frames)
    want = dqn_cnn.gray(torch.from_numpy(frames)).numpy()
    assert got.dtype == want.dtype == f32 and got.shape == want.shape == (3, 37, 37)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), mirror.grey32(frames).view(np.uint32))
    altered = frames.copy()
    altered[..., 3] ^= 0xFF  # alpha is not an input
    assert np.array_equal(capi.qcnn_grey_host(altered), got)
    assert 0.0 <= got.min() and got.max() <= 1.0 and np.abs(got.astype(np.float64) - mirror.grey64(frames)).max() < 2e-7


@pytest.mark.parametrize("name", ["tiny", "odd", "deep_pad", "reference"])
def test_padding_equals_a_zero_extended_plane(capi, name):
    """Layer 0's padding p against the same network with p = 0 on the grey plane extended by p zeros on every side: the same Q-values
    bit for bit (the extended forward evaluates the border's fmaf(+0.0f, w, acc) terms the padded one leaves out)."""
    shape = mirror.SHAPES[name]
    S, p = shape["image_size"], shape["padding"][0]
    assert p > 0
    params, frames = mirror.draw_params(shape, 5), mirror.draw_frames(S, 5, n=2)
    planes = capi.qcnn_grey_host(frames)
    padded = capi.qcnn_forward_planes_host(config(capi, name), params, planes)
    assert np.array_equal(padded.view(np.uint32), capi.qcnn_act_host(config(capi, name), params, frames)["q"].view(np.uint32))
    extended = np.zeros((2, S + 2 * p, S + 2 * p), f32)
    extended[:, p:p + S, p:p + S] = planes
    other = dict(shape, image_size=S + 2 * p, padding=(0,) + tuple(shape["padding"][1:]))
    assert mirror.sides(other) == mirror.sides(shape)
    by_hand = capi.qcnn_forward_planes_host(config(capi, other), params, extended)
    assert np.array_equal(padded.view(np.uint32), by_hand.view(np.uint32))
    assert np.abs(by_hand - capi.qcnn_forward_planes_host(config(capi, other), params, np.roll(extended, 1, axis=2))).max() > 0


EPS_SEED = 4  # with it, of 33 agents at epsilon 0.5 and draw 9 some explore and some do not (asserted below)


def test_choice_is_the_shared_network_actors(ok, capi):
    shape = mirror.SHAPES["odd"]
    A, N, S = shape["num_actions"], 33, shape["image_size"]
    params, frames = mirror.draw_params(shape, 1), mirror.draw_frames(S, 1, n=N)
    greedy = capi.qcnn_act_host(config(capi, "odd"), params, frames)
    # epsilon = 1: the indices of okenv_actor_act_host in OKENV_ACTOR_EPS_GREEDY for the same seed, agent_base, draw and A
    rng = np.random.default_rng(0)
    actor = capi.actor_params(4, capi.QCNN_ACTION_MAP, mode="eps_greedy", epsilon=1.0, seed=77, agent_base=1000)
    lidar = ok.actor_act_host(actor, rng.normal(size=4 * 3 + 4 + A * 4 + A).astype(f32), None, rng.uniform(1, 200, (N, 3)).astype(f32), draw_index=9)
    image = capi.qcnn_act_host(config(capi, "odd", mode="eps_greedy", epsilon=1.0, seed=77, agent_base=1000), params, frames, draw_index=9)
    assert np.array_equal(image["action"], lidar["action"]) and len(set(image["action"].tolist())) == A
    assert np.array_equal(image["q"], greedy["q"]) and np.array_equal(image["value"], image["q"][np.arange(N), image["action"]])
    assert np.array_equal(image["throttle"], lidar["throttle"]) and np.array_equal(image["steer"], lidar["steer"])
    other = capi.qcnn_act_host(config(capi, "odd", mode="eps_greedy", epsilon=1.0, seed=77, agent_base=1000), params, frames, draw_index=10)
    assert not np.array_equal(other["action"], image["action"])
    # epsilon = 0.5: explored and greedy agents both occur; the explored ones take the index of the epsilon = 1 run
    half = capi.qcnn_act_host(config(capi, "odd", mode="eps_greedy", epsilon=0.5, seed=EPS_SEED), params, frames, draw_index=9)
    full = capi.qcnn_act_host(config(capi, "odd", mode="eps_greedy", epsilon=1.0, seed=EPS_SEED), params, frames, draw_index=9)
    took_greedy = half["action"] == greedy["action"]
    explored = ~took_greedy
    assert 5 <= int(explored.sum()) <= 28 and np.array_equal(half["action"][explored], full["action"][explored])
    assert int((took_greedy & (full["action"] != greedy["action"])).sum()) >= 5  # agents that did not explore although their draw differs
    # epsilon = 0 and the greedy mode agree; ties go to the lowest index; a NaN never wins
    zero = capi.qcnn_act_host(config(capi, "odd", mode="eps_greedy", epsilon=0.0, seed=3), params, frames, draw_index=9)
    assert np.array_equal(zero["action"], greedy["action"])
    tie = params.copy()
    lay = {n: (a, s) for n, a, s in mirror.layout(shape)}
    w_at, w_shape = lay["fc2.weight"]
    b_at, _ = lay["fc2.bias"]
    tie[w_at:w_at + A * shape["hidden"]] = 0.0
    tie[b_at:b_at + A] = [0.25, 0.5, 0.5, 0.125, 0.5]
    assert np.array_equal(capi.qcnn_act_host(config(capi, "odd"), tie, frames[:2])["action"], [1, 1])
    tie[b_at:b_at + A] = [np.nan, 0.25, np.nan, 0.5, 0.5]
    got = capi.qcnn_act_host(config(capi, "odd"), tie, frames[:2])
    # (ok_actor_argmax starts from q_0: a NaN there stays, since no comparison with it is true -- the shared-network actor's behaviour)
    assert np.array_equal(got["action"], [0, 0]) and np.isnan(got["value"]).all()
    tie[b_at:b_at + A] = [0.25, np.nan, 0.5, np.nan, 0.5]
    assert np.array_equal(capi.qcnn_act_host(config(capi, "odd"), tie, frames[:2])["action"], [2, 2])


def push_inputs(S, n, seed):
    rng = np.random.default_rng(seed)
    return dict(action=rng.integers(0, 5, n).astype(np.int64), alive=(rng.random(n) < 0.7).astype(np.uint8),
                frames=rng.integers(0, 256, (n, S, S, 4), dtype=np.uint8), next_frames=rng.integers(0, 256, (n, S, S, 4), dtype=np.uint8),
                crashed=(rng.random(n) < 0.3).astype(np.uint8), dist=rng.uniform(0.5, 250.0, (n, 3)).astype(f32),
                reward=rng.normal(size=n).astype(f32))


def rings_equal(a, b):
    return a["pushed"] == b["pushed"] and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("state", "next_state", "action", "reward", "done"))


@pytest.mark.parametrize("capacity, push_all, with_reward", [(40, False, False), (8, False, False), (40, True, False), (40, False, True), (8, True, True)])
def test_push_host_equals_the_mirror(capi, capacity, push_all, with_reward):
    """C = 40 over several pushes of 33 with a wrap, C = 8 < n, PUSH_ALL and a reward array, field by field; slots no transition
    reached keep their sentinel."""
    S, n = 16, 33
    got, want = capi.qcnn_ring(capacity, S), mirror.ring(capacity, S)
    for r in (got, want):
        for k in ("state", "next_state", "reward", "done"):
            r[k].fill(-7.0)
        r["action"].fill(-7)
    for round_ in range(3):
        x = push_inputs(S, n, 10 * capacity + round_)
        if round_ == 0 and not push_all:
            x["alive"][:] = 0
            x["alive"][[2, 5, 30]] = 1  # three transitions: most slots stay untouched after the first push
        kw = dict(reward=x["reward"] if with_reward else None, dist=x["dist"], push_all=push_all)
        capi.qcnn_push_host(got, x["action"], None if push_all else x["alive"], x["frames"], x["next_frames"], x["crashed"], **kw)
        mirror.push(want, x["action"], x["alive"], x["frames"], x["next_frames"], x["crashed"], **kw)
        assert rings_equal(got, want), round_
        if round_ == 0 and not push_all and capacity == 40:
            assert got["pushed"] == 3 and (got["state"][3:] == -7.0).all() and (got["action"][3:] == -7).all() and (got["reward"][3:] == -7.0).all()
    assert got["pushed"] > capacity  # it wrapped
    if not with_reward:
        assert set(np.unique(got["reward"][got["done"] == 1.0])) <= {f32(-200.0)} and -200.0 < got["reward"][got["done"] == 0.0].min()
        assert got["reward"].max() <= 200.0


@pytest.mark.parametrize("case", range(len(P.RING_CASES)), ids=["%s-%d-%s-%d" % c for c in P.RING_CASES])
def test_push_host_equals_the_mirror_at_the_population_cases(capi, case):
    """The (N, selection, capacity) cases tests/test_gpu_image_populations.py holds the device to (tests/_population_cases.py), three
    pushes each, field by field and `pushed`.  The mirror pushes the transitions one by one, which is the rule's "as if": of n > C
    selected agents the last C survive because the earlier ones are overwritten."""
    name, N, selection, capacity = P.RING_CASES[case]
    shape = mirror.SHAPES[name]
    S, A = shape["image_size"], shape["num_actions"]
    got, want = capi.qcnn_ring(capacity, S), mirror.ring(capacity, S)
    for r in (got, want):
        for k in ("state", "next_state", "reward", "done"):
            r[k].fill(-7.0)
        r["action"].fill(-7)
    expected = 0
    for push in range(P.RING_PUSHES):
        x = P.ring_inputs(S, A, N, selection, push, 3)
        push_all = x["alive"] is None
        expected += N if push_all else int(x["alive"].sum())
        kw = dict(reward=x["reward"] if case % 2 else None, dist=x["dist"], push_all=push_all)
        capi.qcnn_push_host(got, x["action"], x["alive"], x["frames"], x["next_frames"], x["crashed"], **kw)
        mirror.push(want, x["action"], x["alive"], x["frames"], x["next_frames"], x["crashed"], **kw)
        assert got["pushed"] == want["pushed"] == expected
        for k in ("state", "next_state", "action", "reward", "done"):
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (push, k)
    if expected < capacity:  # slots no transition reached keep their sentinel
        assert (got["state"][expected:] == -7.0).all() and (got["action"][expected:] == -7).all()
    assert (expected == 0) == (selection == "nobody")


def test_population_constants_are_the_kernels(capi):
    assert P.HEAD_AGENTS == capi.QCNN_AGENTS == capi.CNN_AGENTS == mirror.AGENTS
    assert P.LIST_THREADS == P.REPLAY_THREADS == 4 * P.WAVE and P.LIST_THREADS % P.HEAD_AGENTS == 0 and P.HEAD_AGENTS % P.HEAD_SLOTS == 0


@pytest.mark.parametrize("B", [1, 32, 50])
def test_batch_host_equals_the_mirror(capi, B):
    """Both modes on the empty ring, a ring that is not full yet and one that has wrapped; UNIFORM's index is ok_dqn_sample."""
    S, n, capacity = 16, 33, 40
    got, want = capi.qcnn_ring(capacity, S), mirror.ring(capacity, S)
    for pushes in range(4):  # sizes 0, < C, C (wrapped), C (wrapped twice)
        if pushes:
            x = push_inputs(S, n, pushes)
            x["alive"][:] = 1
            x["alive"][::3] = 0
            capi.qcnn_push_host(got, x["action"], x["alive"], x["frames"], x["next_frames"], x["crashed"], dist=x["dist"])
            mirror.push(want, x["action"], x["alive"], x["frames"], x["next_frames"], x["crashed"], dist=x["dist"])
        size = min(got["pushed"], capacity)
        assert (size == 0) == (pushes == 0) and (size < capacity) == (pushes < 2)
        for mode, start in (("sequential", 0), ("sequential", 17), ("sequential", 1000003), ("uniform", 0), ("uniform", 5)):
            a, b = capi.qcnn_batch_host(got, B, mode, start, seed=21), mirror.batch(want, B, mode, start, seed=21)
            for k in b:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (pushes, mode, start, k)
            if size == 0:
                assert not any(np.any(v) for v in a.values())
            elif mode == "uniform":
                assert np.array_equal(a["index"], [mirror.sample(21, q, start, size) for q in range(B)])
            else:  # the walk is in push order: the oldest transition first, wrapping at the newest
                first = got["pushed"] - size
                assert np.array_equal(a["index"], [(first + (start + q) % size) % capacity for q in range(B)])
    L = capi.load()
    ring, out = capi._qcnn_ring_struct(got), capi.OkenvQcnnBatchOut()
    assert L.okenv_qcnn_batch_host(C.byref(ring), capacity, S, got["pushed"], 0, 4, 1, 0, C.byref(out)) == 0  # every output may be NULL
    for args in ((None, capacity, S, 0, 0, 4, 1, 0, C.byref(out)), (C.byref(ring), 0, S, 0, 0, 4, 1, 0, C.byref(out)), (C.byref(ring), capacity, S, 0, 0, 0, 1, 0, C.byref(out)),
                 (C.byref(ring), capacity, S, 0, 0, 4, 2, 0, C.byref(out)), (C.byref(ring), capacity, S, 0, 0, 4, 1, -1, C.byref(out)),
                 (C.byref(ring), capacity, S, 0, 0, 4, 1, 0, None), (C.byref(ring), capacity, 8, 0, 0, 4, 1, 0, C.byref(out))):
        assert L.okenv_qcnn_batch_host(*args) == INVALID and b"okenv_qcnn_batch_host: bad argument" in L.okenv_last_error(None)


BAD_SHAPES = [dict(image_size=15), dict(image_size=129), dict(kernel=(0, 4, 3)), dict(kernel=(8, 9, 3)), dict(stride=(0, 2, 1)),
              dict(stride=(4, 5, 1), kernel=(8, 8, 3)), dict(stride=(4, 2, 4)), dict(padding=(-1, 1, 1)), dict(padding=(4, 1, 1)),
              dict(padding=(2, 1, 3)), dict(kernel=(8, 4, 1), padding=(2, 1, 1)), dict(channels=(8, 64, 64)), dict(channels=(32, 64, 144)),
              dict(channels=(32, 24, 64)), dict(image_size=128, channels=(32, 64, 128)), dict(hidden=8), dict(hidden=520), dict(hidden=24),
              dict(num_actions=1), dict(num_actions=9),
              dict(image_size=16, kernel=(8, 8, 8), stride=(4, 4, 4), padding=(0, 0, 0))]


def test_shape_limits_and_refusals(capi):
    L = capi.load()
    ref = mirror.SHAPES["reference"]
    params, frames = np.zeros(mirror.num_params(ref), f32), np.zeros((1, 96, 96, 4), np.uint8)
    q = np.empty((1, 8), f32)
    plan = (C.c_int32 * 3)()

    def act_host(cfg):
        return L.okenv_qcnn_act_host(C.byref(cfg), capi.ptr(params), 1, capi.ptr(frames), None, 0, None, None, capi.ptr(q), None, None, None)

    for bad in BAD_SHAPES:
        cfg = config(capi, ref, **bad)
        assert capi.qcnn_lds_bytes(cfg) == 0, bad
        assert L.okenv_qcnn_plan(C.byref(cfg), plan) == INVALID, bad
        assert b"okenv_qcnn_plan: shape outside the limits" in L.okenv_last_error(None)
        assert act_host(cfg) == INVALID and b"okenv_qcnn_act_host: shape outside the limits" in L.okenv_last_error(None), bad
    # F = 128 x 16 x 16 = 32768 > 16384 is what refuses 128 channels on the frame of 128: with 64 (F = 16384, the limit itself) it passes
    assert capi.qcnn_lds_bytes(config(capi, ref, image_size=128)) > 0
    for bad, why in ((dict(mode="sample"), b"unknown mode"), (dict(mode=7), b"unknown mode"), (dict(mode="eps_greedy", epsilon=1.5), b"epsilon outside [0, 1]"),
                     (dict(epsilon=-0.1), b"epsilon outside [0, 1]"), (dict(epsilon=float("nan")), b"epsilon outside [0, 1]"),
                     (dict(action_table=((1.0, float("inf")),)), b"the action table must be finite"),
                     (dict(action_table=((0.0, 0.0),) * 7 + ((float("nan"), 0.0),)), b"the action table must be finite")):
        assert act_host(config(capi, ref, **bad)) == INVALID and why in L.okenv_last_error(None), bad
    assert act_host(config(capi, ref)) == 0
    # the corners of the limits are inside
    for good in (dict(image_size=16, kernel=(1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), channels=(16, 16, 16), hidden=16, num_actions=2),
                 dict(image_size=128, kernel=(8, 8, 6), stride=(4, 4, 4), padding=(3, 3, 3), channels=(128, 128, 128), hidden=512, num_actions=8),
                 dict(image_size=16, kernel=(4, 4, 4), stride=(1, 1, 1), padding=(3, 3, 3), channels=(16, 16, 16), hidden=16, num_actions=2)):
        assert capi.qcnn_lds_bytes(config(capi, good)) > 0, good
    c = config(capi, "tiny")
    tp, tf = mirror.draw_params(mirror.SHAPES["tiny"], 0), mirror.draw_frames(16, 0)
    assert L.okenv_qcnn_act_host(C.byref(c), capi.ptr(tp), 2, capi.ptr(tf), None, 0, None, None, None, None, None, None) == 0  # every output may be NULL
    assert L.okenv_qcnn_act_host(C.byref(c), None, 2, capi.ptr(tf), None, 0, None, None, None, None, None, None) == INVALID
    assert L.okenv_qcnn_act_host(C.byref(c), capi.ptr(tp), 2, None, None, 0, None, None, None, None, None, None) == INVALID
    assert L.okenv_qcnn_act_host(C.byref(c), capi.ptr(tp), -1, capi.ptr(tf), None, 0, None, None, None, None, None, None) == INVALID
    assert L.okenv_qcnn_act_host(None, capi.ptr(tp), 2, capi.ptr(tf), None, 0, None, None, None, None, None, None) == INVALID
    crashed = np.array([0, 3], np.uint8)
    assert np.array_equal(capi.qcnn_act_host(c, tp, tf, crashed)["alive"], [1, 0])
    # the push's refusals
    ring = capi.qcnn_ring(4, 16)
    x = push_inputs(16, 2, 0)
    rs, pushed = capi._qcnn_ring_struct(ring), C.c_uint64(0)
    good = [C.byref(rs), 4, 16, C.byref(pushed), 0, 2, capi.ptr(x["action"]), capi.ptr(x["alive"]), capi.ptr(x["frames"]), capi.ptr(x["next_frames"]),
            capi.ptr(x["crashed"]), None, capi.ptr(x["dist"]), 3]
    assert L.okenv_qcnn_push_host(*good) == 0 and pushed.value == int(x["alive"].astype(bool).sum())
    incomplete = capi.OkenvQcnnRing()
    for at, value in ((0, None), (0, C.byref(incomplete)), (1, 0), (2, 8), (2, 130), (3, None), (4, 2), (5, -1), (6, None), (7, None), (8, None), (9, None),
                      (10, None), (12, None), (13, 0)):
        args = list(good)
        args[at] = value
        assert L.okenv_qcnn_push_host(*args) == INVALID and b"okenv_qcnn_push_host: " in L.okenv_last_error(None), at
    args = list(good)
    args[4], args[7] = capi.REPLAY_PUSH_ALL, None  # alive may be NULL with PUSH_ALL; dist may be NULL with a reward array
    args[11], args[12], args[13] = capi.ptr(x["reward"]), None, 0
    assert L.okenv_qcnn_push_host(*args) == 0
    assert L.okenv_debug_qcnn_grey_host(16, 1, None, capi.ptr(q)) == INVALID and L.okenv_debug_qcnn_forward_planes_host(C.byref(c), capi.ptr(tp), 1, None, capi.ptr(q)) == INVALID


def test_plan_functions_equal_the_mirror(capi):
    L = capi.load()
    for name, cfg in mirror.SHAPES.items():
        assert capi.qcnn_lds_bytes(config(capi, name)) == mirror.lds_bytes(cfg) <= capi.QCNN_LDS_BUDGET == mirror.LDS_BUDGET, name
        assert capi.qcnn_plan(config(capi, name)) == mirror.plan(cfg) == mirror.PATHS[name], name
    # every value the plan can return is selected by some row
    assert [{p[i] for p in mirror.PATHS.values()} for i in range(3)] == [{1, 2, 3, 4}, {0, 1}, {0, 1}]
    assert (mirror.WAVES, mirror.AGENTS) == (8, capi.QCNN_AGENTS)
    assert mirror.lds_bytes(mirror.SHAPES["reference"]) == 4 * (14 * 14 * 65 + 26 * 26 * 33) == 140192
    # inside the shape's limits and outside the LDS: 128 x 128 pixels of 128 channels do not fit a workgroup
    big = dict(image_size=128, kernel=(1, 8, 8), stride=(1, 4, 4), padding=(0, 0, 0), channels=(128, 16, 16), hidden=16, num_actions=2)
    assert capi.qcnn_lds_bytes(config(capi, big)) == mirror.lds_bytes(big) > capi.QCNN_LDS_BUDGET
    plan = (C.c_int32 * 3)()
    assert L.okenv_qcnn_plan(C.byref(config(capi, big)), plan) == INVALID and b"does not fit 160 KB" in L.okenv_last_error(None)
    assert L.okenv_qcnn_plan(None, plan) == INVALID and L.okenv_qcnn_plan(C.byref(config(capi, "tiny")), None) == INVALID
    assert L.okenv_qcnn_lds_bytes(None) == 0


def test_update_is_the_references_step():
    """dqn_cnn.update against the step written out: q' without a gradient, the target equal to q but at the action, Adam."""
    from openkitchen_amd import dqn_cnn
    torch.manual_seed(0)
    S, B = 48, 6
    models = [dqn_cnn.QCNN(S) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    opts = [torch.optim.Adam(m.parameters(), lr=dqn_cnn.LEARNING_RATE) for m in models]
    batch = dict(state=torch.rand(B, S, S), next_state=torch.rand(B, S, S), action=torch.randint(0, 5, (B,)), reward=torch.randn(B),
                 done=(torch.rand(B) < 0.5).float())
    for mask_done in (False, True):
        loss = dqn_cnn.update(models[0], opts[0], batch, mask_done=mask_done)
        q = models[1](batch["state"][:, None])
        nq = models[1](batch["next_state"][:, None]).detach()
        g = (1 - batch["done"][:, None]) * 0.99 if mask_done else 0.99
        y = batch["reward"][:, None] + g * torch.amax(nq, 1, True)
        target = q.clone().detach()
        for b in range(B):
            target[b, batch["action"][b]] = y[b, 0]
        want = torch.nn.functional.mse_loss(q, target)
        opts[1].zero_grad()
        want.backward()
        opts[1].step()
        assert torch.allclose(loss, want.detach(), rtol=1e-6, atol=0) and float(loss) > 0
        for a, b in zip(models[0].parameters(), models[1].parameters()):
            assert torch.allclose(a, b, rtol=0, atol=1e-7)


def test_host_side_stays_inside_its_arrays(tmp_path):
    """The host forward, push and batch as a stand-alone program under AddressSanitizer and UBSan (tests/cpp/qcnn_host_check.cpp), on
    frames, parameter vectors, work spaces, rings and batches of exactly their sizes: every shape of the mirror and the corners of the
    limits."""
    exe = str(tmp_path / "qcnn_host_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "qcnn_host_check.cpp")], check=True)
    keys = ("kernel", "stride", "padding", "channels")
    shapes = [(s["image_size"],) + sum((tuple(s[k]) for k in keys), ()) + (s["hidden"], s["num_actions"]) for s in mirror.SHAPES.values()]
    shapes += [(16, 1, 1, 1, 1, 1, 1, 0, 0, 0, 16, 16, 16, 16, 2),           # the smallest frame, pointwise layers: F = 4096
               (16, 4, 4, 4, 1, 1, 1, 3, 3, 3, 16, 16, 16, 16, 8),           # p = k - 1 throughout: sides 19 / 22 / 25
               (16, 8, 8, 1, 1, 1, 1, 0, 0, 0, 16, 16, 16, 512, 2),          # sides 9 / 2 / 2, the widest hidden layer
               (128, 8, 8, 6, 4, 4, 4, 3, 3, 3, 128, 128, 128, 16, 8),       # the largest frame, strides, paddings and channels
               (29, 8, 3, 2, 3, 2, 2, 1, 0, 1, 16, 16, 128, 16, 3),          # rows left over on every layer
               (32, 2, 2, 2, 1, 1, 1, 2, 0, 0, 16, 16, 16, 16, 2)]           # a padding as wide as its kernel: p < k refuses it
    args = [str(v) for shape in shapes[:-1] for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(shapes) - 1)], r.stdout[-1000:] + r.stderr[-4000:]
    r = subprocess.run([exe] + [str(v) for v in shapes[-1]], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2  # the program refuses a shape outside the limits
