"""REINFORCE on the device (okenv_actor_set_dropout, okenv_reinforce_update; openkitchen_amd/csrc/ok_actor.h, ok_reinforce.h): the
dropout instantiation of the act kernel and the update's kernels bit-equal to the host entries that share their rule; NULL outputs;
continuation; acting with the new parameters; end to end behind collect_episode_device and prepare_batch, eager and as a replayed
graph; the refusals while dropout is on; the example."""
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
HP = dict(lr=0.01, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8)
SHAPES = [(1, 1, 2), (5, 128, 3), (6, 9, 4), (5, 33, 3), (64, 256, 8)]
TABLE8 = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(8))
PPO_FAN = np.array([-70, -30, 0, 30, 70], dtype=f32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def fan_of(gpu, R):
    return gpu.default_ray_fan(R) if R > 1 else np.zeros(1, dtype=f32)


def record_tensors(N, R):
    rec = {"state": torch.full((N, R), -7.0, device="cuda"), "action": torch.full((N,), -7, dtype=torch.int64, device="cuda"),
           "prob": torch.full((N,), -7.0, device="cuda"), "value": torch.full((N,), -7.0, device="cuda"),
           "alive": torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    return rec


# ---- acting ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 257, 4096])
@pytest.mark.parametrize("shape", SHAPES)
def test_act_device_equals_host(gpu, shape, N):
    """p in {0, 0.6}, crashed agents, agent_base != 0, a value network on every other case, each record pointer NULL in turn; with
    p = 0 the bits of a handle that never heard of dropout."""
    R, H, A = shape
    Hv = 16 if (H + N) % 2 else 0
    rng = np.random.default_rng(N + 3 * H)
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan_of(gpu, R))
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(3)
    crashed = dev.get(gpu.capi.F_CRASHED)
    crashed[rng.random(N) < 0.2] = 1
    dev.set(gpu.capi.F_CRASHED, crashed)
    dist = dev.get(gpu.capi.F_DIST)
    count, base = dev.step_count, 3_000_000_000
    policy = (rng.standard_normal(L_.n_params(R, H, A)) * 0.7).astype(f32)
    value = (rng.standard_normal(L_.n_params(R, Hv, 1)) * 0.5).astype(f32) if Hv else None
    ap = gpu.capi.actor_params(H, TABLE8[:A], Hv, "sample", 0.0, 13, base)
    dev.actor_create(H, TABLE8[:A], Hv, "sample", 0.0, seed=13, agent_base=base)
    dev.actor_set_params(policy, value)
    never = record_tensors(N, R)
    dev.actor_act(never)  # a handle that never called okenv_actor_set_dropout
    dev.sync()
    for p in (0.6, 0.0):
        dev.actor_set_dropout(p, 99)
        want = gpu.actor_act_dropout_host(ap, p, 99, policy, value, dist, crashed=crashed, draw_index=count)
        for skip in (None,) + tuple(never):
            rec = record_tensors(N, R)
            dev.actor_act({k: (None if k == skip else v) for k, v in rec.items()})
            dev.sync()
            assert same(dev.get(gpu.capi.F_THROTTLE), want["throttle"]) and same(dev.get(gpu.capi.F_STEER), want["steer"]), (p, skip)
            for k in rec:
                if k == skip or (k == "value" and Hv == 0):
                    assert (rec[k].cpu().numpy() == (9 if k == "alive" else -7)).all(), (p, skip, k)
                else:
                    assert same(rec[k].cpu().numpy(), want[k]), (p, skip, k)
                    if p == 0.0:
                        assert same(rec[k].cpu().numpy(), never[k].cpu().numpy()), (skip, k)
        if p > 0 and H >= 9 and N > 1:
            assert not same(want["prob"], never["prob"].cpu().numpy())  # the mask does something
    dev.close()


# ---- the update --------------------------------------------------------------------------------------------------------------------

def fresh_state(rng, shape, scale=0.4):
    R, H, A = shape
    st = {"policy": (rng.standard_normal(L_.n_params(R, H, A)) * scale).astype(f32), "t": 0}
    st["policy_m"], st["policy_v"] = np.zeros_like(st["policy"]), np.zeros_like(st["policy"])
    return st


def random_batch(rng, shape, M, N):
    R, H, A = shape
    T = (M + N - 1) // N + 2
    return {"state": rng.random((M, R)).astype(f32), "action": rng.integers(0, A, M).astype(np.int64), "ret": rng.standard_normal(M).astype(f32),
            "index": np.sort(rng.choice(T * N, M, replace=False)).astype(np.int32)}


def handle_for(gpu, shape, st, base=0, n_agents=8):
    R, H, A = shape
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), n_agents, ray_angles_deg=fan_of(gpu, R))
    dev.actor_create(H, TABLE8[:A], 0, "sample", 0.0, 11, base)
    dev.actor_set_params(st["policy"], None)
    dev.learner_create(**HP)
    return dev


def on_device(dev, shape, batch, M, B, want=("loss", "grad_policy"), order=None, **cfg):
    R, H, A = shape
    steps = 1 if cfg.get("accumulate", True) else (M + B - 1) // B
    sizes = {"loss": steps, "grad_policy": L_.n_params(R, H, A)}
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    o = None if order is None else torch.from_numpy(order).cuda()
    out = {k: torch.full((sizes[k],), 77.0, device="cuda") for k in want}
    torch.cuda.synchronize()
    dev.reinforce_update(d, M, B, order=o, out=out, **cfg)
    dev.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def device_state(dev):
    st = dev.learner_state()
    return {"policy": dev.actor_get_params()[0], "policy_m": st["policy_m"], "policy_v": st["policy_v"], "t": st["t"]}


def assert_equal(got_out, got_state, want_out, want_state, what):
    for k in got_out:
        assert np.array_equal(bits(got_out[k]), bits(want_out[k])), (k,) + tuple(what)
    assert got_state["t"] == want_state["t"], what
    for k in ("policy", "policy_m", "policy_v"):
        assert np.array_equal(bits(got_state[k]), bits(want_state[k])), (k,) + tuple(what)


def run_case(gpu, dev, rng, shape, M, B, accumulate, reduce, p, N=7, base=0, permuted=False, want=("loss", "grad_policy"), st=None, batch=None):
    st = fresh_state(rng, shape) if st is None else st
    batch = random_batch(rng, shape, M, N) if batch is None else batch
    order = rng.permutation(M).astype(np.int32) if permuted else None
    dev.actor_set_params(st["policy"], None)
    dev.learner_reset()
    dev.actor_set_dropout(p, 21)
    cfg = dict(accumulate=accumulate, reduce=reduce, num_agents=N, draw_first=4_294_967_290)
    got = on_device(dev, shape, batch, M, B, want=want, order=order, **cfg)
    want_state, want_out = gpu.reinforce_update_host(gpu.capi.learner_params(**HP), shape, st, batch, B, p=p, dropout_seed=21, agent_base=base, order=order, **cfg)
    assert_equal(got, device_state(dev), want_out, want_state, (shape, M, B, accumulate, reduce, p, permuted))
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_update_device_equals_host(gpu, shape):
    """M in {1, 33, 1000} x B in {1, 32, 33, 1000} x accumulate x reduce x p in {0, 0.6} on one handle per shape (the moments are reset
    between the cases): a chunk edge, a partial last chunk, a partial last slice, a padded tree, the accumulator over up to a
    thousand slices."""
    rng = np.random.default_rng(sum(shape) + 2)
    base = 1000
    dev = handle_for(gpu, shape, fresh_state(rng, shape), base=base)
    i = 0
    for M in (1, 33, 1000):
        for B in (1, 32, 33, 1000):
            for accumulate in (True, False):
                for reduce in ("sum", "mean"):
                    for p in (0.0, 0.6):
                        run_case(gpu, dev, rng, shape, M, B, accumulate, reduce, p, base=base, permuted=i % 3 == 0)
                        i += 1
    dev.close()


def test_update_geometry_513_chunks_and_four_slices(gpu):
    rng = np.random.default_rng(40)
    shape = (1, 1, 2)
    dev = handle_for(gpu, shape, fresh_state(rng, shape))
    run_case(gpu, dev, rng, shape, 16416, 16416, True, "sum", 0.6)  # 513 chunks in one slice, above the 130 the column sum has run at
    run_case(gpu, dev, rng, shape, 16416, 16416, False, "mean", 0.0)
    dev.close()
    shape = (5, 33, 3)
    dev = handle_for(gpu, shape, fresh_state(rng, shape))
    for accumulate in (True, False):  # M = 3 B + 1: four slices, the last of one sample
        run_case(gpu, dev, rng, shape, 3 * 50 + 1, 50, accumulate, "sum", 0.6, permuted=True)
    dev.close()


def test_null_outputs_continuation_and_acting_with_the_new_parameters(gpu):
    rng = np.random.default_rng(41)
    shape = R, H, A = (5, 128, 3)
    N, base = 8, 70
    st = fresh_state(rng, shape)
    batch = random_batch(rng, shape, 300, N)
    dev = handle_for(gpu, shape, st, base=base, n_agents=N)
    for want in (("loss",), ("grad_policy",), ()):
        run_case(gpu, dev, rng, shape, 300, 128, True, "sum", 0.6, N=N, base=base, want=want, st=st, batch=batch)
    dev.actor_set_params(st["policy"], None)
    dev.learner_reset()
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    torch.cuda.synchronize()
    cfg = dict(accumulate=False, reduce="mean", num_agents=N, draw_first=6)
    dev.reinforce_update(d, 300, 128, **cfg)  # no output struct at all
    host = dict(p=0.6, dropout_seed=21, agent_base=base, **cfg)
    lp = gpu.capi.learner_params(**HP)
    one, _ = gpu.reinforce_update_host(lp, shape, st, batch, 128, **host)
    assert_equal({}, device_state(dev), {}, one, ("no outputs",))
    # a second call continues t, m and v
    got = on_device(dev, shape, batch, 300, 128, **cfg)
    two, want = gpu.reinforce_update_host(lp, shape, one, batch, 128, **host)
    assert two["t"] == 6
    assert_equal(got, device_state(dev), want, two, ("continuation",))
    # acting with the new parameters, no sync_actor: the dropout instantiation reads what the update wrote
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(2)
    rec = record_tensors(N, R)
    dist, draw = dev.get(gpu.capi.F_DIST), dev.step_count
    dev.actor_act(rec)
    dev.sync()
    ap = gpu.capi.actor_params(H, TABLE8[:A], 0, "sample", 0.0, 11, base)
    acted = gpu.actor_act_dropout_host(ap, 0.6, 21, two["policy"], None, dist, draw_index=draw)
    assert same(rec["action"].cpu().numpy(), acted["action"]) and same(rec["prob"].cpu().numpy(), acted["prob"])
    assert not np.array_equal(bits(two["policy"]), bits(st["policy"]))
    # timing
    E = gpu.capi.OkenvError
    with pytest.raises(E):
        dev.reinforce_timing()  # the latest call ran untimed
    dev.set_timing(True)
    dev.reinforce_update(d, 300, 128, **cfg)
    times = dev.reinforce_timing()
    assert set(times) == set(gpu.capi.REINFORCE_KERNELS) and all(v > 0.0 for v in times.values())
    dev.close()


def test_refusals_while_dropout_is_on(gpu):
    E = gpu.capi.OkenvError
    rng = np.random.default_rng(42)
    shape = (5, 8, 3)
    st = fresh_state(rng, shape)
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=PPO_FAN)

    def code(fn, *a, **kw):
        with pytest.raises(E) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(dev.actor_set_dropout, 0.5) == -5  # no actor
    assert gpu.capi.load().okenv_actor_set_dropout(None, 0.5, 0) == -1
    dev.actor_create(8, TABLE8[:3], 0, "sample", 0.0, 1, 0)
    for bad in (-0.1, 1.0, float("nan")):
        assert code(dev.actor_set_dropout, bad) == -1, bad
    dev.actor_set_params(st["policy"], None)
    b = random_batch(rng, shape, 10, 4)
    batch = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    ppo = {"state": batch["state"], "action": batch["action"], "ret": batch["ret"], "adv": batch["ret"], "prob": torch.full((10,), 0.3, device="cuda")}
    torch.cuda.synchronize()
    assert code(dev.reinforce_update, batch, 10, 4, num_agents=4) == -5  # no learner
    dev.learner_create(**HP)
    dev.replay_create(64)
    dev.dqn_params()
    dev.actor_set_dropout(0.6, 3)
    assert code(dev.ppo_update, ppo, 10, 4) == -5 and code(dev.dqn_update, 4, 1) == -5
    no_index = {k: v for k, v in batch.items() if k != "index"}
    assert code(dev.reinforce_update, no_index, 10, 4, num_agents=4) == -1 and code(dev.reinforce_update, batch, 10, 4, num_agents=0) == -1
    assert code(dev.reinforce_update, batch, 0, 4, num_agents=4) == -1 and code(dev.reinforce_update, batch, 10, 0, num_agents=4) == -1
    assert code(dev.reinforce_update, batch, 10, 4, reduce=2, num_agents=4) == -1
    for drop in ("state", "action", "ret"):
        assert code(dev.reinforce_update, {k: v for k, v in batch.items() if k != drop}, 10, 4, num_agents=4) == -1, drop
    dev.reinforce_update(batch, 10, 4, num_agents=4)
    dev.actor_set_dropout(0.0)
    dev.ppo_update(ppo, 10, 4)  # works again
    dev.reinforce_update(no_index, 10, 4)  # and the index may be NULL
    dev.dqn_update(4, 1)  # (an empty ring: zeros everywhere, but not refused)
    dev.sync()
    dev.actor_set_dropout(0.6, 3)
    dev.actor_create(8, TABLE8[:3], 0, "sample", 0.0, 1, 0)  # a new actor switches it off again
    dev.actor_set_params(st["policy"], None)
    dev.learner_create(**HP)
    dev.ppo_update(ppo, 10, 4)
    dev.sync()
    dev.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def reinforce_network(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy().astype(f32)


def make_venv(net, N=64, seed=3):
    from openkitchen_amd.torch_env import VectorEnvironment
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=PPO_FAN, auto_reset=False, seed=seed, reward="step")
    venv.enable_actor(net)
    venv.enable_learner(**HP)
    venv.set_actor_dropout(0.6)
    return venv


def test_end_to_end_eager_chunked_and_replayed(gpu):
    """64 agents on Silverstone, dropout 0.6: collect_episode_device -> prepare_batch -> reinforce_update.  The eager episode's rows
    equal okenv_actor_act_dropout_host on the distances read before every act, and the update equals okenv_batch_prepare_host ->
    okenv_reinforce_update_host on the record; an episode collected as replays of a captured chunk of 32 iterations, and the first
    64 rows of one collected as 64 replays of a single captured actor_act + step, carry the same bits (fresh masks on every replay);
    set_actor_dropout drops the captured chunks."""
    from openkitchen_amd.rollout import collect_episode_device, prepare_batch, reinforce_update

    N, steps = 64, 256
    net = reinforce_network(4)
    policy = flat(net)
    runs = {}
    for name, chunk, limit in (("eager", 0, steps), ("chunked", 32, steps), ("single", 1, 64)):
        venv = make_venv(net, N)
        seen = []
        if chunk == 0:  # read what every act is about to see
            act = venv.actor_act

            def spy(record=None, venv=venv, act=act, seen=seen):
                venv.env.sync()
                seen.append((venv.env.distances(), venv.env.get(gpu.capi.F_CRASHED), venv.env.step_count))
                act(record)

            venv.actor_act = spy
        ep = collect_episode_device(venv, max_steps=limit, graph_chunk=chunk)
        if chunk == 0:
            del venv.actor_act
        else:
            assert venv._actor_graphs
        first, recorded = venv._episode_draw_first[1], venv._episode_probs[1].cpu().numpy()
        batch = prepare_batch(venv, ep, gamma=0.99, normalize="returns")
        assert batch["draw_first"] == first
        if chunk == 0:  # a batch that is not this episode's carries no draw index, and the update refuses it
            stale = prepare_batch(venv, dict(ep, log_probs=ep["log_probs"].clone()), gamma=0.99, normalize="returns")
            assert "draw_first" not in stale
            with pytest.raises(AssertionError):
                reinforce_update(venv, stale, slice=4096)
        out = reinforce_update(venv, batch, slice=4096, grads=True)
        venv.env.sync()
        runs[name] = (ep, batch, {k: v.cpu().numpy() for k, v in out.items()}, device_state(venv.env), seen, first, recorded)
        if chunk:
            venv.set_actor_dropout(0.6)
            assert venv._actor_graphs == {}
        venv.close()
    ep, batch, out, state, seen, first, recorded = runs["eager"]
    T = ep["states"].shape[0]
    assert T > 50 and len(seen) >= T and first == seen[0][2]
    ap = gpu.capi.actor_params(128, ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0)), 0, "sample", 0.0, 3, 0)
    for t in range(T):
        dist, crashed, draw = seen[t]
        assert draw == first + t
        host = gpu.actor_act_dropout_host(ap, 0.6, 3, policy, None, dist, crashed=crashed, draw_index=draw)
        assert same(ep["states"][t].cpu().numpy(), host["state"]) and same(ep["actions"][t].cpu().numpy(), host["action"]), t
        assert same(ep["alive"][t].cpu().numpy().astype(np.uint8), host["alive"]), t
        assert same(recorded[t], host["prob"]), t
    for name in ("chunked", "single"):
        other = runs[name][0]
        rows = other["states"].shape[0]
        assert rows == (T if name == "chunked" else min(T, 64))
        for k in ("states", "actions", "log_probs", "rewards", "alive"):
            assert same(other[k].cpu().numpy(), ep[k][:rows].cpu().numpy()), (name, k)
    assert runs["chunked"][5] == first
    for k in out:
        assert same(runs["chunked"][2][k], out[k]), k
    assert_equal({}, runs["chunked"][3], {}, state, ("chunked",))
    # the host chain on the record
    M = batch["count"]
    rec = {"reward": ep["rewards"].cpu().numpy(), "alive": ep["alive"].cpu().numpy().astype(np.uint8), "state": ep["states"].cpu().numpy(),
           "action": ep["actions"].cpu().numpy()}
    hb = gpu.batch_prepare_host(**rec, gamma=0.99, normalize=1)
    assert hb["M"] == M and same(hb["index"], batch["index"].cpu().numpy())
    st = {"policy": policy, "policy_m": np.zeros_like(policy), "policy_v": np.zeros_like(policy), "t": 0}
    want_state, want = gpu.reinforce_update_host(gpu.capi.learner_params(**HP), (5, 128, 3), st, {"state": hb["state"], "action": hb["action"], "ret": hb["ret"],
                                                 "index": hb["index"]}, 4096, p=0.6, dropout_seed=3, agent_base=0, num_agents=N, draw_first=first)
    assert_equal(out, state, want, want_state, ("end to end",))
    # the recomputed probabilities were the recorded ones: the loss is the sum of -log(recorded) * G in the rule's order
    assert np.isfinite(out["loss"]).all() and out["grad_policy"].any()


def test_example_runs_on_both_paths(gpu):
    for extra in (["--device-update"], []):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "reinforce_racer.py"), "--agents", "64", "--episodes", "2", "--max-steps", "200"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [line for line in r.stdout.splitlines() if line.startswith("episode")]
        assert len(lines) == 2 and all("loss" in line for line in lines), r.stdout
        assert "parameters finite True" in r.stdout, r.stdout
