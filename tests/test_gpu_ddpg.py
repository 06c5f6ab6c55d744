"""DDPG on the device (okenv_ddpg_act, okenv_ddpg_replay_push, okenv_ddpg_update, openkitchen_amd/csrc/ok_ddpg.h): the action, the push
and the update bit-equal to the host entries that share their rule; NULL outputs; continuation across calls; acting with the new
parameters without a sync call; a captured graph of act + step + push; collect_episode_ddpg eager and chunked against a per-step
replay through the host entries; a shared-network actor and its ring on the same handle left alone; validation on a handle; the
example on both update paths."""
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
RING_FIELDS = ("state", "next_state", "action", "reward", "done")
VECTORS = ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v")
FAN = np.array([-70, -30, 0, 30, 70], dtype=f32)
CFG = dict(scale=(50.0, 5.0), bias=(50.0, 0.0), noise=(0.0, 0.0), seed=0, agent_base=0, gamma=0.99, tau=0.005, lr_actor=1e-4, lr_critic=1e-3,
           beta1=0.9, beta2=0.999, eps=1e-8, sample_seed=0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


def n_actor(R, H):
    return L_.n_params(R, H, 2)


def n_critic(R, Hc):
    return L_.n_params(R + 2, Hc, 1)


def record_tensors(N, R):
    rec = {"state": torch.full((N, R), -7.0, device="cuda"), "action": torch.full((N, 2), -7.0, device="cuda"),
           "alive": torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    return rec


def make_env(gpu, N, R, H, Hc, env_seed, **cfg):
    fan = gpu.default_ray_fan(R) if R > 1 else np.zeros(1, dtype=f32)
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan)
    dev.reset_random(None, 1, env_seed, 0, 0)
    dev.step(4)
    rng = np.random.default_rng(env_seed)
    scale = 0.3 if R < 62 else 0.05
    actor, critic = (rng.standard_normal(n_actor(R, H)) * scale).astype(f32), (rng.standard_normal(n_critic(R, Hc)) * scale).astype(f32)
    assert dev.ddpg_create(H, Hc, **dict(CFG, **cfg)) == (actor.size, critic.size)
    dev.ddpg_set_params(actor, critic)
    return dev, actor, critic


# ---- acting --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 257, 1025])
def test_act_equals_host_entry(gpu, N):
    """A partial workgroup, a partial wave and several workgroups; four shapes; noise off and on (one component only, too); a sharded
    agent_base; crashed agents; each record pointer NULL in turn.  (6, 9) is the first even fan of okDdpgActKernel whose first
    layer (54 floats) ends inside a 16-byte load of okActorStage while everything behind it is shifted (by 9 floats); (7, 9) is
    the same width with the identity copy, and both leave lane 0 of a group a second, partial round of hidden units (j = 8)."""
    for R, H in ((5, 128), (62, 256), (6, 9), (7, 9)):
        for noise, base in (((0.0, 0.0), 0), ((20.0, 2.0), 4000), ((0.0, 3.0), 7)):
            cfg = dict(CFG, noise=noise, seed=31, agent_base=base)
            dev, actor, _ = make_env(gpu, N, R, H, 8, env_seed=N + R, **cfg)
            crashed = (np.arange(N) % 3 == 1).astype(np.uint8)
            dev.set(gpu.capi.F_CRASHED, crashed)
            dist, count = dev.get(gpu.capi.F_DIST), dev.step_count
            want = gpu.ddpg_act_host(gpu.capi.ddpg_config(H, 8, **cfg), actor, dist, crashed, count)
            for skip in (None, "state", "action", "alive"):
                rec = record_tensors(N, R)
                dev.ddpg_act({k: v for k, v in rec.items() if k != skip})
                dev.sync()
                what = (N, R, H, noise, skip)
                for k in rec:
                    got = rec[k].cpu().numpy()
                    if k == skip:
                        assert (got == (9 if k == "alive" else -7.0)).all(), what
                    else:
                        assert np.array_equal(bits(got), bits(want[k])), (k,) + what
                assert np.array_equal(bits(dev.get(gpu.capi.F_THROTTLE)), bits(want["throttle"])), what
                assert np.array_equal(bits(dev.get(gpu.capi.F_STEER)), bits(want["steer"])), what
            dev.ddpg_act(None)  # a NULL record
            dev.sync()
            assert np.array_equal(bits(dev.get(gpu.capi.F_THROTTLE)), bits(want["throttle"]))
            dev.close()


# ---- the push ------------------------------------------------------------------------------------------------------------------------

def same_ring(dev, want, what):
    got = dev.ddpg_replay_get()
    assert dev.ddpg_replay_size() == (min(want["pushed"], want["state"].shape[0]), want["pushed"]), what
    for k in RING_FIELDS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)
    return got


def act_step_push(gpu, dev, rec, host_ring, reward=None, push_all=False):
    dev.ddpg_act(rec)
    dev.step(1)
    dev.ddpg_replay_push(rec, reward)
    dev.sync()
    gpu.ddpg_replay_push_host(host_ring, rec["state"].cpu().numpy(), rec["action"].cpu().numpy(), rec["alive"].cpu().numpy(), dev.get(gpu.capi.F_DIST),
                              dev.get(gpu.capi.F_CRASHED), None if reward is None else reward.cpu().numpy(), push_all)


@pytest.mark.parametrize("N", [1, 65, 256, 257, 512, 1025])
def test_push_equals_host_entry(gpu, N):
    """Every ring field and the counter after ten consecutive act + step + push: capacities below one call's transitions (1, 7), below
    ten calls' (100) and above (5000), every mask, push-all and a caller's reward in turn.  N = 256 and 512 are exact workgroup
    edges of the push kernels: no thread of the last workgroup fails `a < p.N` in okReplaySelected."""
    R, H = 5, 16
    dev, _, _ = make_env(gpu, N, R, H, 8, env_seed=N, noise=(10.0, 1.0))
    rng = np.random.default_rng(N)
    rec = record_tensors(N, R)
    case = 0
    for capacity in (1, 7, 100, 5000):
        for mask in ("all", "none", "alternating", "random"):
            push_all, own_reward = case % 3 == 1, case % 3 == 2
            case += 1
            dev.ddpg_replay_create(capacity, push_all)
            host = gpu.ddpg_ring(capacity, R)
            reward = torch.from_numpy(rng.standard_normal(N).astype(f32)).cuda() if own_reward else None
            for push in range(10):
                crashed = {"all": np.zeros(N, np.uint8), "none": np.ones(N, np.uint8), "alternating": (np.arange(N) % 2).astype(np.uint8),
                           "random": (rng.random(N) < 0.4).astype(np.uint8)}[mask]
                if push % 3 == 0:  # (otherwise the flags are what the last step left: crashed agents stay crashed)
                    dev.set(gpu.capi.F_CRASHED, crashed)
                act_step_push(gpu, dev, rec, host, reward, push_all)
            got = same_ring(dev, host, (N, capacity, mask, push_all, own_reward))
            if not own_reward and host["pushed"]:
                assert (got["reward"][:min(host["pushed"], capacity)] == 1.0).all()
    dev.ddpg_replay_reset()
    assert dev.ddpg_replay_size() == (0, 0)
    dev.close()


# ---- the update ----------------------------------------------------------------------------------------------------------------------

def ring_on_device(dev, N, R, size):
    """A ring of `size` transitions from real steps (push-all, four pushes of N agents), and its host copy."""
    dev.ddpg_replay_create(size, True)
    rec = record_tensors(N, R)
    for _ in range(4):
        dev.ddpg_act(rec)
        dev.step(1)
        dev.ddpg_replay_push(rec)
    host = dev.ddpg_replay_get()
    n, pushed = dev.ddpg_replay_size()
    assert pushed == 4 * N and n == min(size, pushed)
    host["pushed"] = pushed
    return host


OUTPUTS = ("critic_loss", "actor_loss", "grad_critic", "grad_actor", "index")


def device_update(dev, R, H, Hc, B, iterations, resample, draw_base, want=OUTPUTS):
    sizes = {"critic_loss": (iterations, torch.float32), "actor_loss": (iterations, torch.float32), "grad_critic": (n_critic(R, Hc), torch.float32),
             "grad_actor": (n_actor(R, H), torch.float32), "index": (B, torch.int32)}
    out = {k: torch.full((sizes[k][0],), 77, dtype=sizes[k][1], device="cuda") for k in want}
    torch.cuda.synchronize()
    dev.ddpg_update(B, iterations, resample, draw_base, out)
    dev.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_update_equal(dev, got, want_state, want, what):
    for k in got:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)
    st = dev.ddpg_state()
    assert st["t"] == want_state["t"], what
    for k in VECTORS:
        assert np.array_equal(bits(st[k]), bits(want_state[k])), (k,) + tuple(what)


UPDATE_SHAPES = [(5, 128, 128), (1, 1, 1), (62, 256, 256), (7, 9, 13), (6, 9, 131), (8, 131, 13), (5, 1, 256), (5, 256, 1)]


@pytest.mark.parametrize("shape", UPDATE_SHAPES)
def test_update_equals_host_entry(gpu, shape):
    """All four networks, all moments, both losses, both gradients and the slots: size in {1, 33, 1000} x B in {1, 32, 33, 250} with
    iterations, resample and tau rotating through the cases; then each output NULL in turn, a continuation across calls, and acting
    with the new parameters without any sync call.  The shapes with H != Hc are the first on the device in which okDdpgNetFloats,
    okLearnHiddenStride(H, Hc) and the strides rpa / rpc of the two gradient kernels are not the same for both networks:
      (7, 9, 13)    odd fans (identity staging) and widths that are no multiple of 8: a lane's last round of hidden units is partial
      (6, 9, 131)   R = 2 mod 4 with odd H: the actor's first layer (54 floats) ends inside a 16-byte load of okActorStage with a
                    shift of 9; the critic's (8 x 131) ends on one; H < Hc
      (8, 131, 13)  R = 0 mod 4: the actor's first layer ends on a load, the critic's (10 x 13 = 130 floats) inside one with a
                    shift of 13; H > Hc
      (5, 1, 256), (5, 256, 1)   the widest ratio either way: the staged region and the hidden rows are sized by the other network"""
    R, H, Hc = shape
    N = 257
    rng = np.random.default_rng(sum(shape) + 3)
    case = 0
    for size in (1, 33, 1000):
        for B in (1, 32, 33, 250):
            iterations, resample, tau = (1, 3)[case % 2], case % 2 == 1, (0.005, 1.0, 0.0, 0.005)[case % 4]
            case += 1
            cfg = dict(CFG, tau=tau, sample_seed=R, noise=(5.0, 0.5))
            if B == 1:  # (a new ring per size)
                if case > 1:
                    dev.close()
                dev, _, _ = make_env(gpu, N, R, H, Hc, env_seed=R + H + size, **cfg)
                ring = ring_on_device(dev, N, R, size)
            else:
                dev.ddpg_create(H, Hc, **cfg)  # (the ring stays; parameters, moments and t are forgotten)
            scale = 0.3 if R < 62 else 0.05
            actor, critic = (rng.standard_normal(n_actor(R, H)) * scale).astype(f32), (rng.standard_normal(n_critic(R, Hc)) * scale).astype(f32)
            dev.ddpg_set_params(actor, critic)
            st = {"actor": actor, "critic": critic, "actor_target": actor, "critic_target": critic, "t": 0}
            for net in ("actor", "critic"):
                st[net + "_m"], st[net + "_v"] = np.zeros_like(st[net]), np.zeros_like(st[net])
            got = device_update(dev, R, H, Hc, B, iterations, resample, 5)
            config = gpu.capi.ddpg_config(H, Hc, **cfg)
            want_state, want = gpu.ddpg_update_host(config, R, st, ring, B, iterations, resample, 5)
            assert_update_equal(dev, got, want_state, want, (shape, size, B, iterations, resample, tau))
    # (the ring of 1000 and the last case's configuration from here on)
    st = dev.ddpg_state()
    for skip in OUTPUTS + (None,):
        names = tuple(k for k in OUTPUTS if k != skip)
        got = device_update(dev, R, H, Hc, 33, 2, True, 9, names)
        st, want = gpu.ddpg_update_host(config, R, st, ring, 33, 2, True, 9)
        assert_update_equal(dev, got, st, want, (shape, "without", skip))
    dev.ddpg_update(33, 2, True, 11, None)  # a NULL output struct
    st, _ = gpu.ddpg_update_host(config, R, st, ring, 33, 2, True, 11)
    assert_update_equal(dev, {}, st, {}, (shape, "no outputs"))
    # acting with the new parameters, no call in between
    rec = record_tensors(N, R)
    dist, crashed, count = dev.get(gpu.capi.F_DIST), dev.get(gpu.capi.F_CRASHED), dev.step_count
    dev.ddpg_act(rec)
    dev.sync()
    want = gpu.ddpg_act_host(config, st["actor"], dist, crashed, count)
    assert np.array_equal(bits(rec["action"].cpu().numpy()), bits(want["action"]))
    dev.close()


def test_an_empty_ring_leaves_the_online_parameters_alone(gpu):
    R, H, Hc = 5, 128, 128
    dev, actor, critic = make_env(gpu, 8, R, H, Hc, env_seed=2)
    dev.ddpg_replay_create(64)
    got = device_update(dev, R, H, Hc, 33, 3, False, 0)
    st = dev.ddpg_state()
    assert st["t"] == 3 and np.array_equal(bits(st["actor"]), bits(actor)) and np.array_equal(bits(st["critic"]), bits(critic))
    assert not any(st[k].any() for k in ("actor_m", "actor_v", "critic_m", "critic_v")) and not any(got[k].any() for k in OUTPUTS)
    dev.close()


# ---- the torch layer -----------------------------------------------------------------------------------------------------------------

def make_venv(gpu, N, auto_reset, seed=5, **cfg):
    from openkitchen_amd.torch_env import VectorEnvironment
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=FAN, auto_reset=auto_reset, seed=seed)
    torch.manual_seed(3)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 2)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(7, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    venv.enable_ddpg(actor, critic, **dict(dict(noise=(20.0, 2.0)), **cfg))
    return venv, actor, critic


def test_graph_of_act_step_push_equals_the_eager_loop(gpu):
    """ddpg_act + step + ddpg_replay_push captured once and replayed 64 times: the eager loop's ring (it wraps), counter and state."""
    N, replays = 300, 64
    results = []
    for use_graph in (False, True):
        venv, _, _ = make_venv(gpu, N, auto_reset=True)
        venv.enable_ddpg_replay(5000)
        rec = record_tensors(N, 5)

        def body():
            venv.ddpg_act(rec)
            venv.step()
            venv.ddpg_replay_push(rec)

        graph = venv.capture(body, warmup=0) if use_graph else None
        for _ in range(replays):
            graph.replay() if use_graph else body()
        torch.cuda.synchronize()
        results.append((venv.env.ddpg_replay_get(), venv.env.ddpg_replay_size(), {n: t.cpu().numpy() for n, t in venv._state_tensors().items()}))
        venv.close()
    (e_ring, e_size, e_state), (g_ring, g_size, g_state) = results
    assert e_size == g_size and e_size[0] == 5000 and 5000 < e_size[1] <= N * replays
    for k in RING_FIELDS:
        assert np.array_equal(bits(e_ring[k]), bits(g_ring[k])), k
    for k in e_state:
        assert np.array_equal(e_state[k], g_state[k]), k


def test_collect_episode_ddpg_and_ddpg_update(gpu):
    """Two episodes of 64 agents, eager and in chunks of 32: the same ring; the first episode's ring equals a per-step replay through
    the host entries; rollout.ddpg_update behind them equals okenv_ddpg_update_host chained the same way; pull_ddpg hands the modules
    those parameters; re-creating the ring drops the captured chunk."""
    from openkitchen_amd.rollout import collect_episode_ddpg, ddpg_update
    N, capacity = 64, 4096
    rings = {}
    for chunk in (0, 32):
        venv, actor, critic = make_venv(gpu, N, auto_reset=False, seed=8, sample_seed=21)
        venv.enable_ddpg_replay(capacity)
        st0 = venv.env.ddpg_state()
        first = collect_episode_ddpg(venv, max_steps=320, check_every=32, graph_chunk=chunk)
        ring1 = venv.env.ddpg_replay_get()
        ring1["pushed"] = venv.env.ddpg_replay_size()[1]
        second = collect_episode_ddpg(venv, max_steps=320, check_every=32, graph_chunk=chunk)
        ring2 = venv.env.ddpg_replay_get()
        ring2["pushed"] = venv.env.ddpg_replay_size()[1]
        rings[chunk] = (first["steps"], ring1, second["steps"], ring2)
        assert ring2["pushed"] > ring1["pushed"] > 0
        if chunk == 0:  # the per-step replay of the first episode through the host entries, on a fresh environment
            twin, _, _ = make_venv(gpu, N, auto_reset=False, seed=8)
            twin.reset()
            host = gpu.ddpg_ring(capacity, 5)
            config = gpu.capi.ddpg_config(128, 128, **dict(CFG, noise=(20.0, 2.0), seed=8))
            for _ in range(first["steps"]):
                dist, crashed, count = twin.distances.cpu().numpy(), twin.crashed.cpu().numpy().astype(np.uint8), twin.env.step_count
                act = gpu.ddpg_act_host(config, st0["actor"], dist, crashed, count)
                twin.env.set(gpu.capi.F_THROTTLE, act["throttle"])
                twin.env.set(gpu.capi.F_STEER, act["steer"])
                twin.step()
                torch.cuda.synchronize()
                gpu.ddpg_replay_push_host(host, act["state"], act["action"], act["alive"], twin.distances.cpu().numpy(), twin.crashed.cpu().numpy())
            twin.close()
            assert host["pushed"] == ring1["pushed"]
            for k in RING_FIELDS:
                assert np.array_equal(bits(host[k]), bits(ring1[k])), k
        else:
            losses = [ddpg_update(venv, batch=100, iterations=3), ddpg_update(venv, batch=100, iterations=2, resample=False)]
            venv.pull_ddpg()
            torch.cuda.synchronize()
            config = gpu.capi.ddpg_config(128, 128, **dict(CFG, noise=(20.0, 2.0), seed=8, sample_seed=21))
            st, out_a = gpu.ddpg_update_host(config, 5, st0, ring2, 100, 3, True, 0)
            st, out_b = gpu.ddpg_update_host(config, 5, st, ring2, 100, 2, False, 3)
            for got, want in zip(losses, (out_a, out_b)):
                assert np.array_equal(bits(got[0].cpu().numpy()), bits(want["critic_loss"])) and np.array_equal(bits(got[1].cpu().numpy()), bits(want["actor_loss"]))
            dst = venv.env.ddpg_state()
            assert dst["t"] == 5
            for k in VECTORS:
                assert np.array_equal(bits(dst[k]), bits(st[k])), k
            for module, k in ((actor, "actor"), (critic, "critic")):
                assert np.array_equal(bits(torch.cat([p.detach().reshape(-1) for p in module.parameters()]).cpu().numpy()), bits(st[k])), k
            assert venv._ddpg_graphs
            venv.enable_ddpg_replay(512, push_all=True)  # the captured chunk carries the old ring: dropped
            assert not venv._ddpg_graphs and venv.env.ddpg_replay_size() == (0, 0)
            third = collect_episode_ddpg(venv, max_steps=64, check_every=32, graph_chunk=chunk)
            assert third["steps"] == 64 and venv.env.ddpg_replay_size() == (512, 64 * N)
        venv.close()
    assert rings[0][0] == rings[32][0] and rings[0][2] == rings[32][2]
    for which in (1, 3):
        assert rings[0][which]["pushed"] == rings[32][which]["pushed"]
        for k in RING_FIELDS:
            assert np.array_equal(bits(rings[0][which][k]), bits(rings[32][which][k])), (which, k)


# ---- isolation and validation --------------------------------------------------------------------------------------------------------

def test_a_shared_network_actor_on_the_same_handle_is_left_alone(gpu):
    """A section 14 actor, its learner and its Deep-Q ring beside a DDPG object: after DDPG's act, pushes and an update the actor's
    parameters, moments and ring hold the same bytes, and DDPG's own objects are untouched by the actor's calls."""
    N, R = 65, 5
    dev, _, _ = make_env(gpu, N, R, 16, 16, env_seed=6, noise=(10.0, 1.0))
    table = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(5))
    rng = np.random.default_rng(6)
    policy = (rng.standard_normal(L_.n_params(R, 16, 5)) * 0.3).astype(f32)
    dev.actor_create(16, table, 0, "eps_greedy", 0.5, seed=6, agent_base=0)
    dev.actor_set_params(policy, None)
    dev.learner_create(lr=1e-4)
    dev.replay_create(300)
    arec = {"state": torch.zeros((N, R), device="cuda"), "action": torch.zeros(N, dtype=torch.int64, device="cuda"),
            "alive": torch.zeros(N, dtype=torch.uint8, device="cuda")}
    for _ in range(3):
        dev.actor_act(arec)
        dev.step(1)
        dev.replay_push(arec)
    dev.dqn_update(33, 2)
    dev.sync()
    before = (dev.actor_get_params()[0], dev.learner_state(), dev.replay_get(), dev.replay_size())
    dev.ddpg_replay_create(200)
    rec = record_tensors(N, R)
    for _ in range(3):
        dev.ddpg_act(rec)
        dev.step(1)
        dev.ddpg_replay_push(rec)
    dev.ddpg_update(33, 2, True, 0)
    dev.sync()
    after = (dev.actor_get_params()[0], dev.learner_state(), dev.replay_get(), dev.replay_size())
    assert np.array_equal(bits(before[0]), bits(after[0])) and before[3] == after[3] and before[1]["t"] == after[1]["t"] == 2
    for k in ("policy_m", "policy_v"):
        assert np.array_equal(bits(before[1][k]), bits(after[1][k])), k
    for k in RING_FIELDS:
        assert np.array_equal(bits(before[2][k]), bits(after[2][k])), k
    mine = (dev.ddpg_state(), dev.ddpg_replay_get(), dev.ddpg_replay_size())
    dev.actor_act(arec)
    dev.step(1)
    dev.replay_push(arec)
    dev.dqn_update(33, 1)
    dev.sync()
    again = (dev.ddpg_state(), dev.ddpg_replay_get(), dev.ddpg_replay_size())
    assert mine[2] == again[2] and mine[0]["t"] == again[0]["t"] == 2
    for k in VECTORS:
        assert np.array_equal(bits(mine[0][k]), bits(again[0][k])), k
    for k in RING_FIELDS:
        assert np.array_equal(bits(mine[1][k]), bits(again[1][k])), k
    dev.close()


def test_validation_on_a_handle(gpu):
    L = gpu.capi.load()
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=FAN)
    h = dev._h
    rec = record_tensors(8, 5)
    full = gpu.capi.fill_pointers(gpu.capi.OkenvDdpgRecord(), rec, "record")
    err = lambda: L.okenv_last_error(h).decode()
    assert L.okenv_ddpg_act(h, None) == -5 and "okenv_ddpg_create" in err()
    assert L.okenv_ddpg_update(h, 4, 1, 0, 0, None) == -5 and L.okenv_ddpg_set_params(h, None, None) == -5
    assert L.okenv_ddpg_replay_push(h, C.byref(full), None) == -5 and "okenv_ddpg_replay_create" in err()
    assert L.okenv_ddpg_create(h, None) == -1
    for bad in (dict(gamma=1.5), dict(gamma=float("nan")), dict(tau=-0.1), dict(tau=float("nan")), dict(noise=(-1.0, 0.0)), dict(lr_actor=0.0), dict(eps=0.0)):
        assert L.okenv_ddpg_create(h, C.byref(gpu.capi.ddpg_config(16, 16, **bad))) == -1, bad
    assert L.okenv_ddpg_create(h, C.byref(gpu.capi.ddpg_config(0, 16))) == -1 and L.okenv_ddpg_create(h, C.byref(gpu.capi.ddpg_config(16, 257))) == -1 and "width" in err()
    assert dev.ddpg_create(16, 16) == (n_actor(5, 16), n_critic(5, 16))
    assert L.okenv_ddpg_act(h, None) == -5 and "okenv_ddpg_set_params" in err()  # acting before the parameters
    dev.ddpg_set_params(np.zeros(n_actor(5, 16), f32), None)
    assert L.okenv_ddpg_act(h, None) == 0
    assert L.okenv_ddpg_update(h, 4, 1, 0, 0, None) == -5 and "both networks" in err()  # an update before the critic's parameters
    dev.ddpg_set_params(None, np.zeros(n_critic(5, 16), f32))
    assert L.okenv_ddpg_update(h, 4, 1, 0, 0, None) == -5 and "okenv_ddpg_replay_create" in err()  # and before the ring
    assert L.okenv_ddpg_replay_create(h, 0, 0) == -1 and L.okenv_ddpg_replay_create(h, 16, 2) == -1 and "unknown flags" in err()
    assert L.okenv_ddpg_replay_create(h, 16, 0) == 0
    assert L.okenv_ddpg_replay_push(h, None, None) == -1
    for missing in ("state", "action", "alive"):
        part = gpu.capi.fill_pointers(gpu.capi.OkenvDdpgRecord(), {k: v for k, v in rec.items() if k != missing}, "record")
        assert L.okenv_ddpg_replay_push(h, C.byref(part), None) == -1 and missing in err(), missing
    assert L.okenv_ddpg_update(h, 0, 1, 0, 0, None) == -1 and L.okenv_ddpg_update(h, 4, 0, 0, 0, None) == -1 and "at least 1" in err()
    assert L.okenv_ddpg_update(h, 4, 1, 0, 0, None) == 0
    ms = (C.c_double * 4)()
    assert L.okenv_debug_ddpg_timing(h, C.cast(ms, C.c_void_p)) == -5  # it ran untimed
    dev.set_timing(True)
    dev.ddpg_update(33, 2)
    t = dev.ddpg_timing()
    assert set(t) == set(gpu.capi.DDPG_KERNELS) and all(v > 0 for v in t.values())
    dev.set_timing(False)
    dev.close()
    # more than 62 rays
    wide = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=gpu.default_ray_fan(63))
    assert L.okenv_ddpg_create(wide._h, C.byref(gpu.capi.ddpg_config(16, 16))) == -1 and "62 rays" in L.okenv_last_error(wide._h).decode()
    assert L.okenv_ddpg_replay_create(wide._h, 16, 0) == -1
    wide.close()


@pytest.mark.parametrize("path", ["--device-update", "--torch-update"])
def test_ddpg_racer_example_runs(gpu, path):
    """Three episodes at 64 agents: finite losses, the parameters move and the targets differ from the online networks (the example
    asserts the last two itself).  Whether it learns is not asserted."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ddpg_racer.py"), "--agents", "64", "--episodes", "3", "--max-steps", "192",
                          "--iterations", "10", "--capacity", "20000", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-2000:]
    lines = [ln for ln in text.splitlines() if ln.startswith("episode")]
    assert len(lines) == 3
    stored = [int(ln.split("stored")[1].split()[0]) for ln in lines]
    assert 0 < stored[0] < stored[1] < stored[2]
    assert "largest parameter movement" in text
