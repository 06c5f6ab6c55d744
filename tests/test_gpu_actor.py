"""The shared-network actors on the device (okenv_actor_*, openkitchen_amd/csrc/ok_actor.h): bit-equal to the host entry that shares
their rule, sharding, closed loops against the oracle's Environment::step, HIP-graph replay, collect_episode_device, parameter
hand-over, validation and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_actor_rule import PPO_ACTIONS, PPO_FAN, TABLE8, cpu_loop, loop_networks, make_case

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ["pos_x", "pos_y", "rot", "speed", "acc", "thr", "steer", "mode", "crashed", "timed_out", "disp_ctr", "disp_x", "disp_y", "disp_to",
         "hit_x", "hit_y", "rel_x", "rel_y", "dist"]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def record_tensors(N, R, lead=()):
    rec = {"state": torch.full(lead + (N, R), -7.0, device="cuda"), "action": torch.full(lead + (N,), -7, dtype=torch.int64, device="cuda"),
           "prob": torch.full(lead + (N,), -7.0, device="cuda"), "value": torch.full(lead + (N,), -7.0, device="cuda"),
           "alive": torch.full(lead + (N,), 9, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    return rec


def make_env(gpu, track, N, fan, seed):
    t = gpu.Track(track)
    dev = gpu.BatchedEnvironment.from_track(t, N, ray_angles_deg=fan)
    dev.reset_random(None, 1, seed, 0, 0)
    dev.step(4)
    return t, dev


@pytest.mark.parametrize("track,R,H,A,Hv,N", [
    ("Austin", 5, 128, 3, 128, 4096), ("Silverstone", 1, 1, 2, 0, 257), ("Monza", 15, 16, 5, 256, 4096), ("Austin", 64, 256, 8, 256, 257),
    ("Silverstone", 64, 128, 8, 1, 1), ("Monza", 5, 256, 2, 16, 257), ("Silverstone", 15, 1, 3, 128, 4096), ("Austin", 1, 16, 5, 0, 1),
    ("Monza", 6, 9, 4, 13, 257)])
def test_device_equals_host(gpu, track, R, H, A, Hv, N):
    """Every record slot and the two action fields, all modes, crashed agents among them, agent_base != 0, each record pointer
    NULL in turn.  The row (6, 9, 4, 13) is the first in okActorKernel whose first layers (54 and 78 floats) end inside a 16-byte
    load of okActorStage while everything behind them is shifted (R even, so the LDS row stride is R + 1; the other even fan, 64
    at widths 128 and 256, ends on a load), with widths that leave a lane a partial last round of hidden units."""
    fan = gpu.default_ray_fan(R) if R > 1 else np.zeros(1, dtype=f32)
    t, dev = make_env(gpu, track, N, fan, seed=R + N)
    rng = np.random.default_rng(N * 7 + R + H)
    crashed = dev.get(gpu.capi.F_CRASHED)
    crashed[rng.random(N) < 0.2] = 1
    dev.set(gpu.capi.F_CRASHED, crashed)
    dist = dev.get(gpu.capi.F_DIST)
    dist[rng.random(N) < 0.05] = 0.0
    dist[rng.random(N) < 0.05] = 200.0
    dev.set(gpu.capi.F_DIST, dist)
    count = dev.step_count
    base = 1_000_000
    for i, (mode, eps, scale) in enumerate([("sample", 0.0, 0.1), ("sample", 0.0, 30.0), ("greedy", 0.0, 1.0), ("eps_greedy", 0.0, 1.0),
                                            ("eps_greedy", 0.3, 1.0), ("eps_greedy", 1.0, 0.1)]):
        policy, value, _ = make_case(rng, R, H, A, Hv, scale, 1, tied=(i == 2 and H > 1))
        dev.actor_create(H, TABLE8[:A], Hv, mode, eps, seed=11 + i, agent_base=base)
        dev.actor_set_params(policy, value)
        ap = gpu.capi.actor_params(H, TABLE8[:A], Hv, mode, eps, 11 + i, base)
        want = gpu.actor_act_host(ap, policy, value, dist, crashed=crashed, draw_index=count)
        rec = record_tensors(N, R)
        dev.actor_act(rec)
        dev.sync()
        assert same(dev.get(gpu.capi.F_THROTTLE), want["throttle"]) and same(dev.get(gpu.capi.F_STEER), want["steer"]), (mode, eps)
        for k in rec:
            if k == "value" and Hv == 0:
                assert (rec[k].cpu().numpy() == -7.0).all()  # left alone without a value network
            else:
                assert same(rec[k].cpu().numpy(), want[k]), (k, mode, eps)
        if i in (0, 3):  # each record pointer NULL in turn: the others and the action fields are unchanged
            for skip in rec:
                part = record_tensors(N, R)
                dev.actor_act({k: (None if k == skip else v) for k, v in part.items()})
                dev.sync()
                for k in part:
                    if k == skip or (k == "value" and Hv == 0):
                        assert (part[k].cpu().numpy() == (9 if k == "alive" else -7)).all(), (skip, k)
                    else:
                        assert same(part[k].cpu().numpy(), want[k]), (skip, k)
                assert same(dev.get(gpu.capi.F_THROTTLE), want["throttle"])
            dev.actor_act(None)
            dev.sync()
            assert same(dev.get(gpu.capi.F_STEER), want["steer"])
    assert dev.step_count == count  # read, not advanced
    dev.close()


def test_sharded_handles_act_like_the_unsharded_one(gpu):
    N, R, H = 512, 5, 128
    t = gpu.Track("Silverstone")
    policy, value = loop_networks()
    whole = gpu.BatchedEnvironment.from_track(t, N, ray_angles_deg=PPO_FAN)
    whole.reset_random(None, 1, 3, 0, 0)
    whole.step(2)
    whole.actor_create(H, PPO_ACTIONS, 128, "sample", 0.0, seed=3, agent_base=0)
    whole.actor_set_params(policy, value)
    rec = record_tensors(N, R)
    whole.actor_act(rec)
    whole.sync()
    for lo in (0, N // 2):
        part = gpu.BatchedEnvironment.from_track(t, N // 2, ray_angles_deg=PPO_FAN)
        part.reset_random(None, 1, 3, 0, lo)
        part.step(2)
        assert same(part.get(gpu.capi.F_DIST), whole.get(gpu.capi.F_DIST)[lo:lo + N // 2])
        part.actor_create(H, PPO_ACTIONS, 128, "sample", 0.0, seed=3, agent_base=lo)
        part.actor_set_params(policy, value)
        prec = record_tensors(N // 2, R)
        part.actor_act(prec)
        part.sync()
        for k in rec:
            assert same(prec[k].cpu().numpy(), rec[k][lo:lo + N // 2].cpu().numpy()), k
        part.close()
    whole.close()


@pytest.mark.parametrize("track,mode,eps,auto_reset", [("Silverstone", "sample", 0.0, False), ("Monza", "sample", 0.0, True),
                                                       ("Austin", "eps_greedy", 0.3, True)])
def test_closed_loop_against_the_cpu_loop(gpu, oracle, track, mode, eps, auto_reset):
    """600 steps of actor_act -> step -> tracker_update against the oracle's step + the host entry: every state field, every slot."""
    N, steps, seed = 96, 600, 29
    orc, want = cpu_loop(gpu, oracle, track, N, steps, seed, mode=mode, eps=eps, auto_reset=auto_reset)
    t = gpu.Track(track)
    dev = gpu.BatchedEnvironment.from_track(t, N, ray_angles_deg=PPO_FAN)
    dev.set_lane_bounds(t.li, t.ri)
    dev.tracker_create(gpu.capi.REWARD_STEP)
    dev.set_auto_reset(auto_reset, 1, seed, 0)
    dev.reset_random(None, 1, seed, 0, 0)
    dev.step(1)
    dev.tracker_begin()
    policy, value = loop_networks()
    dev.actor_create(128, PPO_ACTIONS, 128, mode, eps, seed=seed, agent_base=0)
    dev.actor_set_params(policy, value)
    rec = record_tensors(N, 5, lead=(steps,))
    for s in range(steps):
        dev.actor_act({k: v[s] for k, v in rec.items()})
        dev.step(1)
        dev.tracker_update()
    dev.sync()
    d, o = dev.snapshot(), orc.snapshot()
    for k in STATE:
        assert same(d[k], o[k]), k
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    for s in range(steps):
        for k in got:
            assert same(got[k][s], want[s][k]), (k, s)
    print("%s %s auto_reset=%d: %d of %d alive after %d steps" % (track, mode, auto_reset, int((d["crashed"] == 0).sum()), N, steps))
    dev.close()


def ppo_networks(seed=0, R=5, H=128):
    torch.manual_seed(seed)
    actor = torch.nn.Sequential(torch.nn.Linear(R, H), torch.nn.ReLU(), torch.nn.Linear(H, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(R, H), torch.nn.ReLU(), torch.nn.Linear(H, 1)).cuda()
    return actor, critic


def make_venv(gpu, N, auto_reset, seed=5, track="Silverstone"):
    from openkitchen_amd.torch_env import VectorEnvironment
    return VectorEnvironment(track, N, ray_angles_deg=PPO_FAN, auto_reset=auto_reset, seed=seed, reward="step")


def test_graph_replay_equals_eager_and_draws_afresh(gpu):
    """actor_act + step + tracker_update captured once, replayed 256 times: the eager sequence's bits, the device step count
    advancing, the draws differing from replay to replay."""
    N, replays = 300, 256
    results = []
    for use_graph in (False, True):
        venv = make_venv(gpu, N, auto_reset=True)
        actor, critic = ppo_networks()
        venv.enable_actor(actor, critic)
        slot = record_tensors(N, 5)
        log = {k: [] for k in ("action", "prob", "value")}

        def body():
            venv.actor_act(slot)
            venv.step()

        graph = venv.capture(body) if use_graph else None
        start = venv.env.step_count
        for _ in range(replays):
            graph.replay() if use_graph else body()
            for k in log:
                log[k].append(slot[k].clone())
        torch.cuda.synchronize()
        assert venv.env.step_count == start + replays
        results.append(({k: torch.stack(v).cpu().numpy() for k, v in log.items()}, {n: t.cpu().numpy() for n, t in venv._state_tensors().items()}))
        venv.close()
    (eager, e_state), (graph, g_state) = results
    for k in eager:
        assert same(eager[k], graph[k]), k
    for k in e_state:
        assert same(e_state[k], g_state[k]), k
    changes = (graph["action"][1:] != graph["action"][:-1]).mean()
    assert changes > 0.05, "the replays repeat their draws"


def test_collect_episode_device(gpu, oracle):
    from openkitchen_amd.rollout import collect_episode, collect_episode_device
    N = 200
    out = {}
    for chunk in (0, 32):
        venv = make_venv(gpu, N, auto_reset=False, seed=8)
        actor, critic = ppo_networks(1)
        venv.enable_actor(actor, critic)
        # two episodes: the second reuses the captured graph.  Both forms test for the end every 32 steps, so that the environment
        # has taken the same number of steps (the second episode's reset epoch and draw indices) when the second one starts.
        episodes = [collect_episode_device(venv, max_steps=3000, check_every=32, graph_chunk=chunk) for _ in range(2)]
        out[chunk] = [{k: v.cpu().numpy() for k, v in ep.items()} for ep in episodes]
        if chunk == 0:
            before, dist = venv.observation().clone(), venv.distances.clone()
            slot = record_tensors(N, 5)
            venv.actor_act(slot)
            torch.cuda.synchronize()
            state = slot["state"].cpu().numpy()
            # the recorded state is the IEEE division of what the step left ...
            assert same(state, dist.cpu().numpy() / f32(200.0))
            # ... and observation() on the device, which multiplies by the rounded reciprocal of 200 (relative error up to 3 units
            # roundoff against the division's 1), is never more than two places away
            assert np.abs(state.view(np.int32).astype(np.int64) - before.cpu().numpy().view(np.int32)).max() <= 2
        policy = torch.cat([p.detach().reshape(-1) for p in actor.parameters()]).cpu().numpy()
        value = torch.cat([p.detach().reshape(-1) for p in critic.parameters()]).cpu().numpy()
        venv.close()
    for a, b in zip(out[0], out[32]):
        assert sorted(a) == ["actions", "alive", "log_probs", "rewards", "states", "values"]
        for k in a:
            assert a[k].shape == b[k].shape and same(a[k], b[k]), k
    ep = out[0][0]
    T = ep["states"].shape[0]
    assert 0 < T < 3000
    assert (np.diff(ep["alive"].astype(np.int8), axis=0) <= 0).all()  # monotone per agent
    assert ep["alive"][T - 1].any()
    # the reference loop on the oracle with the host entry: the same length, the same rows
    t = oracle.Track("Silverstone")
    env = oracle.OracleEnv(t.segments, N, 5, PPO_FAN, (t.x, t.y, t.heading))
    env.set_auto_reset(False, 1, 8, 0)
    # VectorEnvironment's constructor: reset at epoch 0xFFFFFFFF without a step; collect's reset(): epoch = step count (0), then a step
    env.reset_random(None, 1, 8, 0, 0)
    env.step(1)
    ap = gpu.capi.actor_params(128, PPO_ACTIONS, 128, "sample", 0.0, 8, 0)
    steps = 0
    while (env.get(oracle.F_CRASHED) == 0).any():
        o = gpu.actor_act_host(ap, policy, value, env.get(oracle.F_DIST), crashed=env.get(oracle.F_CRASHED), draw_index=1 + steps)
        assert steps < T, "the device loop ended early"
        assert same(ep["states"][steps], o["state"]) and same(ep["actions"][steps], o["action"]), steps
        assert np.allclose(ep["log_probs"][steps], np.log(o["prob"]), rtol=1e-6, atol=1e-7)  # (two logarithms, each good to an ulp or two)
        assert same(ep["alive"][steps], o["alive"].astype(bool)) and same(ep["values"][steps], o["value"]), steps
        env.set(oracle.F_THR, o["throttle"])
        env.set(oracle.F_STEER, o["steer"])
        env.step(1)
        steps += 1
    assert steps == T
    # keys, shapes and dtypes of collect_episode for the same environment
    venv = make_venv(gpu, N, auto_reset=False, seed=8)
    actor, critic = ppo_networks(1)
    venv.enable_actor(actor, critic)
    ref = collect_episode(venv, actor, max_steps=16)
    new = collect_episode_device(venv, max_steps=16)
    for k in ref:
        assert new[k].shape == ref[k].shape and new[k].dtype == ref[k].dtype and new[k].device == ref[k].device, k
    assert set(new) == set(ref) | {"values"}
    venv.close()


def test_parameter_hand_over(gpu):
    N = 256
    venv = make_venv(gpu, N, auto_reset=False, seed=2)
    actor, critic = ppo_networks(4)
    venv.enable_actor(actor, critic, mode="greedy")
    venv.reset()
    slot = record_tensors(N, 5)
    venv.actor_act(slot)
    first = slot["action"].cpu().numpy().copy()
    opt = torch.optim.SGD(actor.parameters(), lr=5.0)
    rare = int(np.bincount(first, minlength=3).argmin())
    loss = actor(venv.observation())[:, rare].log().mean()  # push towards the action chosen least
    opt.zero_grad()
    (-loss).backward()
    opt.step()
    venv.actor_act(slot)
    torch.cuda.synchronize()
    assert same(slot["action"].cpu().numpy(), first)  # not handed over yet
    venv.sync_actor()
    venv.actor_act(slot)
    torch.cuda.synchronize()
    flat = lambda net: torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()  # noqa: E731
    ap = gpu.capi.actor_params(128, PPO_ACTIONS, 128, "greedy", 0.0, 2, 0)
    want = gpu.actor_act_host(ap, flat(actor), flat(critic), venv.distances.cpu().numpy(), draw_index=venv.env.step_count)
    for k in ("action", "prob", "value"):
        assert same(slot[k].cpu().numpy(), want[k]), k
    assert not same(want["action"], first)
    venv.close()


def test_validation_on_a_handle(gpu):
    t = gpu.Track("Austin")
    dev = gpu.BatchedEnvironment.from_track(t, 8, ray_angles_deg=PPO_FAN)
    E = gpu.capi.OkenvError
    with pytest.raises(E) as e:
        dev.actor_act()
    assert e.value.code == -5
    with pytest.raises(E) as e:
        dev.actor_num_params()
    assert e.value.code == -5
    for kwargs in (dict(hidden=0), dict(hidden=257), dict(value_hidden=300), dict(mode=7), dict(epsilon=2.0)):
        args = dict(hidden=8, actions=PPO_ACTIONS, value_hidden=0, mode="sample", epsilon=0.0)
        args.update(kwargs)
        with pytest.raises(E) as e:
            dev.actor_create(**args)
        assert e.value.code == -1, kwargs
    assert dev.actor_create(8, PPO_ACTIONS, 4) == (5 * 8 + 8 + 3 * 8 + 3, 5 * 4 + 4 + 4 + 1)
    with pytest.raises(E) as e:
        dev.actor_act()  # no parameters yet
    assert e.value.code == -5
    dev.actor_set_params(np.zeros(75, f32), None)
    with pytest.raises(E) as e:
        dev.actor_act()  # the value network has none yet
    assert e.value.code == -5
    dev.actor_set_params(None, np.zeros(29, f32))
    dev.actor_act()
    with pytest.raises(E) as e:
        dev.actor_set_epsilon(-1.0)
    assert e.value.code == -1
    dev.sync()
    dev.close()
    wide = gpu.BatchedEnvironment.from_track(t, 4, 65)
    with pytest.raises(E) as e:
        wide.actor_create(8, PPO_ACTIONS)
    assert e.value.code == -1
    wide.close()
    venv = make_venv(gpu, 16, auto_reset=False)
    with pytest.raises(ValueError):
        venv.enable_actor(torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 3)).cuda())
    with pytest.raises(ValueError):
        venv.enable_actor(torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.Tanh(), torch.nn.Linear(8, 3)).cuda())
    venv.close()


def test_example_runs_with_the_device_actor(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_racer.py"), "--device-actor", "--agents", "256", "--episodes", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum(line.startswith("episode") for line in r.stdout.splitlines()) == 2, r.stdout
