"""Deep-Q learning on the device (okenv_replay_push, okenv_dqn_update, openkitchen_amd/csrc/ok_dqn.h): the push and the update
bit-equal to the host entries that share their rule; NULL outputs; continuation across calls; acting with the new parameters without
sync_actor; a captured graph of act + step + push; collect_episode_dqn eager and chunked against a per-step replay through the host
entries, with dqn_update behind it; a new ring between two chunked episodes; the target network switched on a second time;
validation on a handle; the example on both update paths."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _learn_numpy as L_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HP = dict(lr=1e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8)
# (6, 9, 4) and (10, 13, 5): even fans with R = 2 mod 4 and odd widths, so okActorStage's first layer (54 / 130 floats) ends inside a
# 16-byte load while everything behind it is shifted by H floats; the other even fan, 64 x 256, ends on a load
SHAPES = [(5, 128, 5), (7, 9, 4), (64, 256, 8), (1, 1, 2), (6, 9, 4), (10, 13, 5)]
TABLE8 = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(8))
RING_FIELDS = ("state", "next_state", "action", "reward", "done")
DQN_FAN = np.array([-70, -30, 0, 30, 70], dtype=f32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


def record_tensors(N, R):
    rec = {"state": torch.full((N, R), -7.0, device="cuda"), "action": torch.full((N,), -7, dtype=torch.int64, device="cuda"),
           "alive": torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    return rec


def make_env(gpu, N, R, H, A, seed, policy=None, eps=0.5):
    fan = gpu.default_ray_fan(R) if R > 1 else np.zeros(1, dtype=f32)
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan)
    dev.reset_random(None, 1, seed, 0, 0)
    dev.step(4)
    rng = np.random.default_rng(seed)
    policy = (rng.standard_normal(L_.n_params(R, H, A)) * 0.3).astype(f32) if policy is None else policy
    dev.actor_create(H, TABLE8[:A], 0, "eps_greedy", eps, seed=seed, agent_base=0)
    dev.actor_set_params(policy, None)
    return dev, policy


def same_ring(dev, want, what):
    got = dev.replay_get()
    assert dev.replay_size() == (min(want["pushed"], want["state"].shape[0]), want["pushed"]), what
    for k in RING_FIELDS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)
    return got


def act_step_push(gpu, dev, rec, host_ring, reward=None, push_all=False):
    """One act + step + push on the device, and the same push through the host entry from what the device left."""
    dev.actor_act(rec)
    dev.step(1)
    dev.replay_push(rec, reward)
    dev.sync()
    gpu.replay_push_host(host_ring, rec["state"].cpu().numpy(), rec["action"].cpu().numpy(), rec["alive"].cpu().numpy(), dev.get(gpu.capi.F_DIST),
                         dev.get(gpu.capi.F_CRASHED), None if reward is None else reward.cpu().numpy(), push_all)


@pytest.mark.parametrize("N", [1, 65, 256, 257, 512, 1025])
def test_push_equals_host_entry(gpu, N):
    """Every ring field and the counter after each of ten consecutive pushes' worth of act + step + push: capacities below one call's
    transitions (1, 7), below ten calls' (100) and above (5000: no wrap unless N = 1025), every mask (set through crashed_ before the
    act, so that `alive` is the actor's own byte and some agents crash during the step as well), push-all and a caller's reward in
    turn.  N = 257 and 1025 span two and five workgroups of the push kernels; N = 256 and 512 are exact workgroup edges (no thread
    of the last workgroup fails `a < p.N` in okReplaySelected)."""
    R, H, A = 5, 16, 5
    dev, _ = make_env(gpu, N, R, H, A, seed=N)
    rng = np.random.default_rng(N)
    rec = record_tensors(N, R)
    case = 0
    for capacity in (1, 7, 100, 5000):
        for mask in ("all", "none", "alternating", "random"):
            push_all, own_reward = case % 3 == 1, case % 3 == 2
            case += 1
            dev.replay_create(capacity, push_all)
            host = gpu.replay_ring(capacity, R)
            reward = torch.from_numpy(rng.standard_normal(N).astype(f32)).cuda() if own_reward else None
            for push in range(10):
                crashed = {"all": np.zeros(N, np.uint8), "none": np.ones(N, np.uint8), "alternating": (np.arange(N) % 2).astype(np.uint8),
                           "random": (rng.random(N) < 0.4).astype(np.uint8)}[mask]
                if push % 3 == 0:  # (otherwise the flags are what the last step left: crashed agents stay crashed)
                    dev.set(gpu.capi.F_CRASHED, crashed)
                act_step_push(gpu, dev, rec, host, reward, push_all)
            got = same_ring(dev, host, (N, capacity, mask, push_all, own_reward))
            if mask == "all" and not own_reward and capacity >= 100:
                live = got["done"][:min(host["pushed"], capacity)] == 0
                assert (got["reward"][:len(live)][live] <= 200.0).all() and (got["reward"][:len(live)][~live] == -200.0).all()
    # reset: the counter returns to 0, the next push starts at slot 0
    dev.replay_reset()
    assert dev.replay_size() == (0, 0)
    dev.close()


def ring_on_device(gpu, dev, N, R, size, rng):
    """A ring of `size` transitions from real steps (push-all, four pushes of N agents), and its host copy."""
    dev.replay_create(size, True)
    rec = record_tensors(N, R)
    for _ in range(4):
        dev.actor_act(rec)
        dev.step(1)
        dev.replay_push(rec)
    host = dev.replay_get()
    n, pushed = dev.replay_size()
    assert pushed == 4 * N and n == min(size, pushed)
    host["pushed"] = pushed
    return host


def device_state(dev):
    st = dev.learner_state()
    st["policy"] = dev.actor_get_params()[0]
    return st


def device_update(dev, shape, B, iterations, resample, draw_base, want=("loss", "grad_policy", "index")):
    R, H, A = shape
    sizes = {"loss": (iterations, torch.float32), "grad_policy": (L_.n_params(R, H, A), torch.float32), "index": (B, torch.int32)}
    out = {k: torch.full((sizes[k][0],), 77, dtype=sizes[k][1], device="cuda") for k in want}
    torch.cuda.synchronize()
    dev.dqn_update(B, iterations, resample, draw_base, out)
    dev.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_update_equal(dev, got, want_state, want, what):
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)
    st = device_state(dev)
    assert st["t"] == want_state["t"], what
    for k in ("policy", "policy_m", "policy_v"):
        assert np.array_equal(bits(st[k]), bits(want_state[k])), (k,) + tuple(what)


@pytest.mark.parametrize("shape", SHAPES)
def test_update_equals_host_entry(gpu, shape):
    """Parameters, both moments, losses, the last gradient and the drawn slots: size in {1, 33, 1000} x B in {1, 33, 100} (a single
    position, a chunk edge plus one, four chunks with a padded tree) with iterations, resample, mask-done and the target network
    rotating through the cases; then each output NULL in turn, a continuation across two calls, and acting with the new parameters
    without sync_actor."""
    R, H, A = shape
    N = 257
    rng = np.random.default_rng(sum(shape) + 3)
    dev, _ = make_env(gpu, N, R, H, A, seed=R + H)
    lp = gpu.capi.learner_params(**HP)
    case = 0
    for size in (1, 33, 1000):
        ring = ring_on_device(gpu, dev, N, R, size, rng)
        for B in (1, 33, 100):
            iterations, resample, mask_done, target_on = (1, 3)[case % 2], case % 2 == 1, case % 3 == 1, case % 4 >= 2
            case += 1
            policy = (rng.standard_normal(L_.n_params(R, H, A)) * 0.3).astype(f32)
            target = (policy + rng.standard_normal(policy.size).astype(f32) * f32(0.05)) if target_on else None
            st = {"policy": policy, "policy_m": np.zeros_like(policy), "policy_v": np.zeros_like(policy), "t": 0}
            if target_on:  # the target network is a copy of what the actor holds at sync time
                dev.actor_set_params(target, None)
                dev.dqn_params(0.99, mask_done, True, seed=R)
                dev.dqn_sync_target()
            else:
                dev.dqn_params(0.99, mask_done, False, seed=R)
            dev.actor_set_params(policy, None)
            dev.learner_create(**HP)
            cfg = gpu.capi.dqn_config(0.99, mask_done, target_on, R)
            got = device_update(dev, shape, B, iterations, resample, 5)
            want_state, want = gpu.dqn_update_host(lp, cfg, shape, st, ring, B, iterations, resample, 5, target)
            assert_update_equal(dev, got, want_state, want, (shape, size, B, iterations, resample, mask_done, target_on))
    # (the ring of 1000 and the last case's configuration from here on)
    st = device_state(dev)
    for skip in ("loss", "grad_policy", "index", None):
        names = tuple(k for k in ("loss", "grad_policy", "index") if k != skip)
        got = device_update(dev, shape, 33, 2, True, 9, names)
        st, want = gpu.dqn_update_host(lp, cfg, shape, st, ring, 33, 2, True, 9, target)
        assert_update_equal(dev, got, st, want, (shape, "without", skip))
    dev.dqn_update(33, 2, True, 11, None)  # a NULL output struct
    st, _ = gpu.dqn_update_host(lp, cfg, shape, st, ring, 33, 2, True, 11, target)
    assert_update_equal(dev, {}, st, {}, (shape, "no outputs"))
    # acting with the new parameters, no sync_actor in between
    rec = record_tensors(N, R)
    dist, crashed, count = dev.get(gpu.capi.F_DIST), dev.get(gpu.capi.F_CRASHED), dev.step_count
    dev.actor_act(rec)
    dev.sync()
    ap = gpu.capi.actor_params(H, TABLE8[:A], 0, "eps_greedy", 0.5, R + H, 0)
    want = gpu.actor_act_host(ap, st["policy"], None, dist, crashed=crashed, draw_index=count)
    assert np.array_equal(rec["action"].cpu().numpy(), want["action"]) and np.array_equal(bits(rec["state"].cpu().numpy()), bits(want["state"]))
    dev.close()


def test_an_empty_ring_leaves_the_parameters_alone(gpu):
    shape = (5, 128, 5)
    dev, policy = make_env(gpu, 8, *shape, seed=2)
    dev.learner_create(**HP)
    dev.replay_create(64)
    got = device_update(dev, shape, 33, 3, False, 0)
    st = device_state(dev)
    assert st["t"] == 3 and np.array_equal(bits(st["policy"]), bits(policy)) and not st["policy_m"].any() and not st["policy_v"].any()
    assert not got["loss"].any() and not got["grad_policy"].any()
    dev.close()


def make_venv(gpu, N, auto_reset, seed=5):
    from openkitchen_amd.rollout import DQN_ACTIONS
    from openkitchen_amd.torch_env import VectorEnvironment
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=DQN_FAN, auto_reset=auto_reset, seed=seed)
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 5)).cuda()
    venv.enable_actor(net, mode="eps_greedy", actions=DQN_ACTIONS, epsilon=0.3)
    return venv, net


def test_graph_of_act_step_push_equals_the_eager_loop(gpu):
    """actor_act + step + replay_push captured once and replayed 64 times: the eager loop's ring (it wraps: 64 x 300 transitions
    into 5000 slots), counter and environment state."""
    N, replays = 300, 64
    results = []
    for use_graph in (False, True):
        venv, _ = make_venv(gpu, N, auto_reset=True)
        venv.enable_replay(5000)
        rec = record_tensors(N, 5)

        def body():
            venv.actor_act(rec)
            venv.step()
            venv.replay_push(rec)

        graph = venv.capture(body, warmup=0) if use_graph else None
        for _ in range(replays):
            graph.replay() if use_graph else body()
        torch.cuda.synchronize()
        results.append((venv.env.replay_get(), venv.env.replay_size(), {n: t.cpu().numpy() for n, t in venv._state_tensors().items()}))
        venv.close()
    (e_ring, e_size, e_state), (g_ring, g_size, g_state) = results
    assert e_size == g_size and e_size[0] == 5000 and 5000 < e_size[1] <= N * replays
    for k in RING_FIELDS:
        assert np.array_equal(bits(e_ring[k]), bits(g_ring[k])), k
    for k in e_state:
        assert np.array_equal(e_state[k], g_state[k]), k


def test_collect_episode_dqn_and_dqn_update(gpu):
    """Two episodes of 64 agents, eager and in chunks of 32: the same ring; the first episode's ring equals a per-step replay through
    okenv_replay_push_host; rollout.dqn_update behind them equals okenv_dqn_update_host chained the same way (two calls, the draw
    counter advancing), and pull_actor hands the module those parameters."""
    from openkitchen_amd.rollout import collect_episode_dqn, dqn_update
    N, capacity = 64, 4096
    rings = {}
    for chunk in (0, 32):
        venv, net = make_venv(gpu, N, auto_reset=False, seed=8)
        venv.enable_learner(lr=1e-4)
        venv.enable_replay(capacity, seed=21)
        policy0 = venv.env.actor_get_params()[0]
        first = collect_episode_dqn(venv, max_steps=320, check_every=32, graph_chunk=chunk)
        ring1 = venv.env.replay_get()
        ring1["pushed"] = venv.env.replay_size()[1]
        second = collect_episode_dqn(venv, max_steps=320, check_every=32, graph_chunk=chunk)
        ring2 = venv.env.replay_get()
        ring2["pushed"] = venv.env.replay_size()[1]
        rings[chunk] = (first["steps"], ring1, second["steps"], ring2)
        assert ring2["pushed"] > ring1["pushed"] > 0
        if chunk == 0:  # the per-step replay of the first episode through the host entries, on a fresh environment
            twin, _ = make_venv(gpu, N, auto_reset=False, seed=8)
            twin.reset()
            host = gpu.replay_ring(capacity, 5)
            rec = record_tensors(N, 5)
            for _ in range(first["steps"]):
                act_step_push_venv(gpu, twin, rec, host)
            twin.close()
            assert host["pushed"] == ring1["pushed"]
            for k in RING_FIELDS:
                assert np.array_equal(bits(host[k]), bits(ring1[k])), k
        else:
            # the update behind the chunked episodes: two calls of three iterations
            losses = [dqn_update(venv, batch=100, iterations=3), dqn_update(venv, batch=100, iterations=3, resample=True)]
            venv.pull_actor()
            torch.cuda.synchronize()
            lp, cfg = gpu.capi.learner_params(**HP), gpu.capi.dqn_config(0.99, False, False, 21)
            st = {"policy": policy0, "policy_m": np.zeros_like(policy0), "policy_v": np.zeros_like(policy0), "t": 0}
            st, out_a = gpu.dqn_update_host(lp, cfg, (5, 128, 5), st, ring2, 100, 3, False, 0)
            st, out_b = gpu.dqn_update_host(lp, cfg, (5, 128, 5), st, ring2, 100, 3, True, 1)
            assert np.array_equal(bits(losses[0].cpu().numpy()), bits(out_a["loss"])) and np.array_equal(bits(losses[1].cpu().numpy()), bits(out_b["loss"]))
            dst = device_state(venv.env)
            assert dst["t"] == 6
            for k in ("policy", "policy_m", "policy_v"):
                assert np.array_equal(bits(dst[k]), bits(st[k])), k
            module = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()
            assert np.array_equal(bits(module), bits(st["policy"]))
        venv.close()
    assert rings[0][0] == rings[32][0] and rings[0][2] == rings[32][2]
    for which in (1, 3):
        assert rings[0][which]["pushed"] == rings[32][which]["pushed"]
        for k in RING_FIELDS:
            assert np.array_equal(bits(rings[0][which][k]), bits(rings[32][which][k])), (which, k)


def test_a_new_ring_between_two_chunked_episodes(gpu):
    """enable_replay again between two episodes of the same chunk size, with the epsilon left alone: the captured chunk of the first
    episode carries the first ring's pointers, capacity and flags, so it must not be replayed.  The second episode fills the NEW
    ring (another capacity, push-all) exactly as the eager loop does."""
    from openkitchen_amd.rollout import collect_episode_dqn
    N, results = 64, {}
    for chunk in (0, 32):
        venv, _ = make_venv(gpu, N, auto_reset=False, seed=8)
        venv.enable_replay(4096)
        collect_episode_dqn(venv, max_steps=64, check_every=32, graph_chunk=chunk)
        assert venv.env.replay_size()[1] > 0
        venv.enable_replay(512, push_all=True)
        assert venv.env.replay_size() == (0, 0)
        second = collect_episode_dqn(venv, max_steps=64, check_every=32, graph_chunk=chunk)
        results[chunk] = (second["steps"], venv.env.replay_size(), venv.env.replay_get())
        venv.close()
    assert results[0][0] == results[32][0] == 64
    assert results[0][1] == results[32][1] == (512, 64 * N)  # push-all: every agent of every step, into the new capacity
    for k in RING_FIELDS:
        assert np.array_equal(bits(results[0][2][k]), bits(results[32][2][k])), k


def test_turning_the_target_network_on_again_refills_its_copy(gpu):
    """On, off, new parameters, on: q' comes from the parameters of the second switch, not from the first copy."""
    shape = (5, 16, 5)
    R, H, A = shape
    dev, first = make_env(gpu, 65, R, H, A, seed=4)
    rng = np.random.default_rng(4)
    ring = ring_on_device(gpu, dev, 65, R, 100, rng)
    dev.dqn_params(0.99, False, True, seed=1)   # copies `first`
    dev.dqn_params(0.99, False, False, seed=1)
    second = (first + rng.standard_normal(first.size).astype(f32) * f32(0.1)).astype(f32)
    dev.actor_set_params(second, None)
    dev.dqn_params(0.99, False, True, seed=1)   # must copy `second`
    online = (rng.standard_normal(first.size) * 0.3).astype(f32)
    dev.actor_set_params(online, None)
    dev.learner_create(**HP)
    got = device_update(dev, shape, 33, 2, False, 0)
    st = {"policy": online, "policy_m": np.zeros_like(online), "policy_v": np.zeros_like(online), "t": 0}
    want_state, want = gpu.dqn_update_host(gpu.capi.learner_params(**HP), gpu.capi.dqn_config(0.99, False, True, 1), shape, st, ring, 33, 2, False, 0, second)
    assert_update_equal(dev, got, want_state, want, "second copy")
    stale = gpu.dqn_update_host(gpu.capi.learner_params(**HP), gpu.capi.dqn_config(0.99, False, True, 1), shape, st, ring, 33, 2, False, 0, first)[1]
    assert not np.array_equal(bits(stale["loss"]), bits(want["loss"]))  # (the case can tell the two copies apart)
    dev.close()


def act_step_push_venv(gpu, venv, rec, host):
    venv.actor_act(rec)
    venv.step()
    torch.cuda.synchronize()
    gpu.replay_push_host(host, rec["state"].cpu().numpy(), rec["action"].cpu().numpy(), rec["alive"].cpu().numpy(), venv.distances.cpu().numpy(),
                         venv.crashed.cpu().numpy())


def test_validation_on_a_handle(gpu):
    L = gpu.capi.load()
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=DQN_FAN)
    h = dev._h
    rec = record_tensors(8, 5)
    full = gpu.capi.fill_pointers(gpu.capi.OkenvActorRecord(), rec, "record")
    err = lambda: L.okenv_last_error(h).decode()
    assert L.okenv_replay_push(h, C.byref(full), None) == -5 and "okenv_replay_create" in err()  # a push before the ring
    assert L.okenv_replay_reset(h) == -5 and L.okenv_replay_size(h, None, None) == -5
    assert L.okenv_replay_create(h, 0, 0) == -1 and "capacity" in err()
    assert L.okenv_replay_create(h, 16, 2) == -1 and "unknown flags" in err()
    assert L.okenv_replay_create(h, 16, 0) == 0
    assert L.okenv_replay_push(h, None, None) == -1
    for missing in ("state", "action", "alive"):
        part = gpu.capi.fill_pointers(gpu.capi.OkenvActorRecord(), {k: v for k, v in rec.items() if k != missing}, "record")
        assert L.okenv_replay_push(h, C.byref(part), None) == -1 and missing in err(), missing
    assert L.okenv_replay_get(h, None) == -1
    cfg = gpu.capi.dqn_config()
    assert L.okenv_dqn_params(h, None) == -1
    for gamma in (float("nan"), -0.5, 1.5):
        assert L.okenv_dqn_params(h, C.byref(gpu.capi.dqn_config(gamma=gamma))) == -1 and "gamma" in err()
    cfg.flags = 4
    assert L.okenv_dqn_params(h, C.byref(cfg)) == -1 and "unknown flags" in err()
    assert L.okenv_dqn_sync_target(h) == -5
    assert L.okenv_dqn_update(h, 4, 1, 0, 0, None) == -5 and "okenv_learner_create" in err()  # an update before the learner
    dev.actor_create(16, TABLE8[:5], 0, "eps_greedy", 0.1, 1, 0)
    dev.actor_set_params(np.zeros(L_.n_params(5, 16, 5), f32), None)
    dev.learner_create(**HP)
    assert L.okenv_dqn_update(h, 0, 1, 0, 0, None) == -1 and L.okenv_dqn_update(h, 4, 0, 0, 0, None) == -1 and "at least 1" in err()
    assert L.okenv_dqn_update(h, 2 ** 30, 1, 0, 0, None) == -1 and "2^31" in err()
    assert L.okenv_dqn_update(h, 4, 1, 0, 0, None) == 0
    assert L.okenv_debug_dqn_timing(h, None) == -1
    ms = (C.c_double * 2)()
    assert L.okenv_debug_dqn_timing(h, C.cast(ms, C.c_void_p)) == -5  # it ran untimed
    dev.set_timing(True)
    dev.dqn_update(33, 2)
    t = dev.dqn_timing()
    assert set(t) == {"grad", "step"} and all(v > 0 for v in t.values())
    dev.set_timing(False)
    # a push-all ring takes a record without alive
    dev.replay_create(16, True)
    part = gpu.capi.fill_pointers(gpu.capi.OkenvActorRecord(), {k: v for k, v in rec.items() if k != "alive"}, "record")
    assert L.okenv_replay_push(h, C.byref(part), None) == 0
    dev.sync()
    assert dev.replay_size() == (8, 8)
    # a new actor drops the learner: the update asks for it again
    dev.actor_create(16, TABLE8[:5], 0, "eps_greedy", 0.1, 1, 0)
    assert L.okenv_dqn_update(h, 4, 1, 0, 0, None) == -5
    dev.close()


@pytest.mark.parametrize("path", ["--device-update", "--torch-update"])
def test_dqn_racer_example_runs(gpu, path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dqn_racer.py"), "--agents", "64", "--episodes", "2", "--max-steps", "192",
                          "--iterations", "20", "--capacity", "20000", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-2000:]
    lines = [ln for ln in text.splitlines() if ln.startswith("episode")]
    assert len(lines) == 2
    stored = [int(ln.split("stored")[1].split()[0]) for ln in lines]
    assert 0 < stored[0] < stored[1]
