"""PPO's update on the device (okenv_ppo_update, openkitchen_amd/csrc/ok_learn.h): bit-equal to the host entry that shares its rule
for parameters, moments, losses, clip counts and gradients; NULL outputs; continuation across calls; acting with the new parameters
without sync_actor; end to end behind collect_episode_device and prepare_batch; pull_actor; validation on a handle; the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _learn_numpy as L_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HP = dict(lr=3e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8)
# (6, 9, 4, 13): R = 2 mod 4 with odd widths, so the first layer of both networks (54 / 78 floats) ends inside a 16-byte load of
# okActorStage while everything behind it is shifted (by 9 / 13 floats).  (8, 131, 3, 9): R = 0 mod 4, both first layers end on a
# load with a non-zero shift, H > Hv, and the value network is staged into a place sized by the policy's.
SHAPES = [(5, 128, 3, 128), (1, 1, 2, 1), (7, 9, 4, 16), (64, 256, 8, 256), (6, 9, 4, 13), (8, 131, 3, 9)]
TABLE8 = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(8))
OUTS = ("actor_loss", "critic_loss", "clipped", "grad_policy", "grad_value")


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def fresh_state(rng, shape, scale=0.3):
    R, H, A, Hv = shape
    st = {"policy": (rng.standard_normal(L_.n_params(R, H, A)) * scale).astype(f32), "t": 0}
    st["policy_m"], st["policy_v"] = np.zeros_like(st["policy"]), np.zeros_like(st["policy"])
    if Hv:
        st["value"] = (rng.standard_normal(L_.n_params(R, Hv, 1)) * scale).astype(f32)
        st["value_m"], st["value_v"] = np.zeros_like(st["value"]), np.zeros_like(st["value"])
    return st


def random_batch(rng, shape, M, with_adv=False):
    R, H, A, Hv = shape
    b = {"state": rng.random((M, R)).astype(f32), "action": rng.integers(0, A, M).astype(np.int64),
         "prob": (0.05 + 0.9 * rng.random(M)).astype(f32), "ret": rng.standard_normal(M).astype(f32)}
    if with_adv:
        b["adv"] = rng.standard_normal(M).astype(f32)
    return b


def handle_for(gpu, shape, st, n_agents=8):
    R, H, A, Hv = shape
    fan = np.linspace(-80.0, 80.0, R).astype(f32) if R > 1 else np.zeros(1, f32)
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), n_agents, ray_angles_deg=fan)
    dev.actor_create(H, TABLE8[:A], Hv, "sample", 0.0, 11, 0)
    dev.actor_set_params(st["policy"], st.get("value"))
    dev.learner_create(**HP)
    return dev


def on_device(dev, batch, M, B, epochs, order, shape, want=OUTS):
    """okenv_ppo_update on device copies; returns the outputs as numpy arrays.  Outputs that are not asked for are passed as NULL."""
    R, H, A, Hv = shape
    n = epochs * ((M + B - 1) // B)
    sizes = {"actor_loss": (n, torch.float32), "critic_loss": (n, torch.float32), "clipped": (n, torch.int32),
             "grad_policy": (L_.n_params(R, H, A), torch.float32), "grad_value": (L_.n_params(R, Hv, 1), torch.float32)}
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    o = None if order is None else torch.from_numpy(order).cuda()
    out = {k: torch.full((sizes[k][0],), 77, dtype=sizes[k][1], device="cuda") for k in want if sizes[k][0] > 0}
    torch.cuda.synchronize()
    dev.ppo_update(d, M, B, epochs, o, out)
    dev.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def device_state(dev):
    policy, value = dev.actor_get_params()
    st = dev.learner_state()
    st["policy"] = policy
    if value is not None:
        st["value"] = value
    return st


def assert_state_equal(got, want, what):
    assert got["t"] == want["t"], what
    for k, v in want.items():
        if k != "t":
            assert np.array_equal(bits(got[k]), bits(v)), (k,) + tuple(what)


def assert_outputs_equal(got, want, what):
    for k in got:
        if k == "clipped":
            assert np.array_equal(got[k], want[k]), (k,) + tuple(what)
        else:
            assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)


@pytest.mark.parametrize("shape", SHAPES)
def test_device_equals_host(gpu, shape):
    """M in {1, 33, 1000} x B in {1, 32, 100, 4096} x order NULL / permuted: a chunk edge, a partial last chunk, a partial last
    minibatch and a padded tree (B = 100: four chunks of which the last holds four positions; M = 1000 in one minibatch: 32 chunks of
    which the last holds eight).  One handle per shape; the moments are reset between the cases."""
    rng = np.random.default_rng(sum(shape) + 1)
    lp = gpu.capi.learner_params(**HP)
    st0 = fresh_state(rng, shape)
    dev = handle_for(gpu, shape, st0)
    for M in (1, 33, 1000):
        for B in (1, 32, 100, 4096):
            for permuted in (False, True):
                M_run = M
                batch = random_batch(rng, shape, M_run, with_adv=(M + B) % 2 == 1)
                order = rng.permutation(M_run).astype(np.int32)[None, :] if permuted else None
                st = fresh_state(rng, shape)
                dev.actor_set_params(st["policy"], st.get("value"))
                dev.learner_reset()
                got = on_device(dev, batch, M_run, B, 1, order, shape)
                want_state, want = gpu.ppo_update_host(lp, shape, st, batch, B, 1, order)
                what = (shape, M, B, permuted)
                assert_outputs_equal(got, want, what)
                assert_state_equal(device_state(dev), want_state, what)
    dev.close()


def test_each_output_null_in_turn_and_epochs(gpu):
    shape = (5, 128, 3, 128)
    rng = np.random.default_rng(12)
    lp = gpu.capi.learner_params(**HP)
    st = fresh_state(rng, shape)
    batch = random_batch(rng, shape, 333)
    order = np.stack([rng.permutation(333) for _ in range(3)]).astype(np.int32)
    want_state, want = gpu.ppo_update_host(lp, shape, st, batch, 100, 3, order)
    dev = handle_for(gpu, shape, st)
    for skip in OUTS + (None,):
        dev.actor_set_params(st["policy"], st["value"])
        dev.learner_reset()
        got = on_device(dev, batch, 333, 100, 3, order, shape, want=tuple(k for k in OUTS if k != skip))
        assert skip not in got
        assert_outputs_equal(got, want, (skip,))
        assert_state_equal(device_state(dev), want_state, (skip,))
    dev.actor_set_params(st["policy"], st["value"])
    dev.learner_reset()
    torch.cuda.synchronize()
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    dev.ppo_update(d, 333, 100, 3, torch.from_numpy(order).cuda(), None)  # no output struct at all
    assert_state_equal(device_state(dev), want_state, ("none",))
    dev.close()


def test_second_call_continues(gpu):
    shape = (7, 9, 4, 16)
    rng = np.random.default_rng(13)
    lp = gpu.capi.learner_params(**HP)
    st = fresh_state(rng, shape)
    batch = random_batch(rng, shape, 200)
    dev = handle_for(gpu, shape, st)
    on_device(dev, batch, 200, 64, 2, None, shape)
    got = on_device(dev, batch, 200, 64, 1, None, shape)
    whole_state, whole = gpu.ppo_update_host(lp, shape, st, batch, 64, 3, None)
    assert device_state(dev)["t"] == 12
    assert_state_equal(device_state(dev), whole_state, ("continuation",))
    assert np.array_equal(bits(got["actor_loss"]), bits(whole["actor_loss"][8:]))
    # okenv_actor_set_params leaves the moments alone; okenv_learner_reset zeroes them
    dev.actor_set_params(st["policy"], st["value"])
    assert np.array_equal(bits(dev.learner_state()["policy_m"]), bits(whole_state["policy_m"]))
    dev.learner_reset()
    s = dev.learner_state()
    assert s["t"] == 0 and not s["policy_m"].any() and not s["value_v"].any()
    dev.close()


PPO_FAN = np.array([-70, -30, 0, 30, 70], dtype=f32)


def make_venv(N, seed=5):
    from openkitchen_amd.torch_env import VectorEnvironment
    return VectorEnvironment("Silverstone", N, ray_angles_deg=PPO_FAN, auto_reset=False, seed=seed, reward="step")


def ppo_networks(seed=0):
    torch.manual_seed(seed)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    return actor, critic


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy().astype(f32)


def test_end_to_end_acting_and_pull(gpu):
    """collect_episode_device -> prepare_batch -> ppo_update on 64 agents against the host entries chained the same way; then
    actor_act without sync_actor equals okenv_actor_act_host with the parameters okenv_actor_get_params returns; pull_actor brings
    exactly those into the modules."""
    from openkitchen_amd.rollout import collect_episode_device, ppo_update, prepare_batch

    N = 64
    venv = make_venv(N, seed=3)
    actor, critic = ppo_networks(2)
    venv.enable_actor(actor, critic)
    venv.enable_learner(**HP)
    st = {"policy": flat(actor), "value": flat(critic), "t": 0}
    for k in ("policy", "value"):
        st[k + "_m"], st[k + "_v"] = np.zeros_like(st[k]), np.zeros_like(st[k])
    ep = collect_episode_device(venv, max_steps=400)
    batch = prepare_batch(venv, ep, gamma=0.99, normalize="returns")
    M = batch["count"]
    assert M > 200 and "probs" in batch
    torch.manual_seed(7)
    out = ppo_update(venv, batch, epochs=2, minibatch=256, shuffle=True, grads=True)
    order = venv._update_inputs[1].cpu().numpy()
    # the host chain: okenv_batch_prepare_host on the record (the recorded probabilities as the per-sample field), okenv_ppo_update_host
    rec = {"reward": ep["rewards"].cpu().numpy(), "alive": ep["alive"].cpu().numpy().astype(np.uint8), "state": ep["states"].cpu().numpy(),
           "action": ep["actions"].cpu().numpy(), "prob": venv._episode_probs[1].cpu().numpy()}
    hb = gpu.batch_prepare_host(**rec, gamma=0.99, normalize=1)
    assert hb["M"] == M
    want_state, want = gpu.ppo_update_host(gpu.capi.learner_params(**HP), (5, 128, 3, 128), st,
                                           {"state": hb["state"], "action": hb["action"], "prob": hb["prob"], "ret": hb["ret"]}, 256, 2, order)
    assert_outputs_equal({k: v.cpu().numpy() for k, v in out.items()}, want, ("end to end",))
    assert_state_equal(device_state(venv.env), want_state, ("end to end",))
    assert int(out["clipped"][0]) == 0  # first minibatch: the ratio is exactly 1
    # acting with the new parameters, no sync_actor
    policy, value = venv.env.actor_get_params()
    rec_dev = {"action": torch.empty(N, dtype=torch.int64, device="cuda"), "prob": torch.empty(N, device="cuda"), "value": torch.empty(N, device="cuda")}
    dist = venv.env.distances()
    draw = venv.env.step_count
    venv.actor_act(rec_dev)
    venv.env.sync()
    host = gpu.actor_act_host(venv.env.actor_params, policy, value, dist, draw_index=draw)
    assert np.array_equal(rec_dev["action"].cpu().numpy(), host["action"])
    assert np.array_equal(bits(rec_dev["prob"].cpu().numpy()), bits(host["prob"])) and np.array_equal(bits(rec_dev["value"].cpu().numpy()), bits(host["value"]))
    assert not np.array_equal(bits(policy), bits(st["policy"]))
    # pull_actor
    venv.pull_actor()
    assert np.array_equal(bits(flat(actor)), bits(policy)) and np.array_equal(bits(flat(critic)), bits(value))
    venv.sync_actor()  # and back again: a round trip changes nothing
    p2, v2 = venv.env.actor_get_params()
    assert np.array_equal(bits(p2), bits(policy)) and np.array_equal(bits(v2), bits(value))
    venv.close()


def test_validation_on_a_handle(gpu):
    E = gpu.capi.OkenvError
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=PPO_FAN)
    shape = (5, 8, 3, 4)
    rng = np.random.default_rng(2)
    st = fresh_state(rng, shape)
    batch = {k: torch.from_numpy(v).cuda() for k, v in random_batch(rng, shape, 10).items()}
    torch.cuda.synchronize()

    def code(fn, *a, **kw):
        with pytest.raises(E) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(dev.learner_create) == -5            # no actor
    assert code(dev.actor_get_params) == -5
    dev.actor_create(8, TABLE8[:3], 4, "sample", 0.0, 1, 0)
    assert code(dev.learner_create) == -5            # no parameters
    assert code(dev.ppo_update, batch, 10, 4) == -5  # no learner
    assert code(dev.learner_reset) == -5 and code(dev.update_timing) == -5 and code(dev.learner_state) == -5
    dev.actor_set_params(st["policy"], st["value"])
    for bad in (dict(lr=0.0), dict(lr=float("nan")), dict(clip=-0.1), dict(clip=1.0), dict(beta1=1.0), dict(beta2=-0.5), dict(eps=0.0)):
        assert code(dev.learner_create, **dict(HP, **bad)) == -1, bad
    dev.learner_create(**HP)
    for drop in ("state", "action", "prob", "ret"):
        assert code(dev.ppo_update, {k: v for k, v in batch.items() if k != drop}, 10, 4) == -1, drop
    assert code(dev.ppo_update, batch, 0, 4) == -1 and code(dev.ppo_update, batch, 10, 0) == -1 and code(dev.ppo_update, batch, 10, 4, 0) == -1
    dev.ppo_update(batch, 10, 4)
    assert code(dev.update_timing) == -5             # that call ran untimed
    dev.set_timing(True)
    dev.ppo_update(batch, 10, 4, 2)
    times = dev.update_timing()
    assert set(times) == set(gpu.capi.UPDATE_KERNELS) and all(v > 0.0 for v in times.values())
    dev.set_timing(False)
    assert dev.learner_state()["t"] == 9
    # without a critic the advantage must be given
    dev.actor_create(8, TABLE8[:3], 0, "sample", 0.0, 1, 0)
    assert code(dev.ppo_update, batch, 10, 4) == -5  # a new actor: its learner is gone
    dev.actor_set_params(st["policy"], None)
    dev.learner_create(**HP)
    assert code(dev.ppo_update, batch, 10, 4) == -1
    dev.ppo_update(dict(batch, adv=batch["ret"]), 10, 4)
    dev.sync()
    dev.close()


def test_example_runs_with_the_device_update(gpu):
    """Two short episodes at a small population: it finishes, every parameter is finite, and every parameter that had a gradient
    (a non-zero second moment) has changed.  The others belong to hidden units that no recorded state activates (about a seventh
    of the units of torch's default initialisation on inputs in [0, 1]); they keep their weights under any optimiser."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_racer.py"), "--device-actor", "--device-batch", "--device-update",
                        "--agents", "256", "--episodes", "2", "--max-steps", "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [line for line in r.stdout.splitlines() if line.startswith("episode")]
    assert len(lines) == 2 and all("update" in line for line in lines), r.stdout
    m = re.search(r"device update: parameters finite True, changed (\d+) of the (\d+) that had a gradient \((\d+) parameters, (\d+) optimiser steps\)", r.stdout)
    assert m, r.stdout
    changed, stepped, total, steps = (int(v) for v in m.groups())
    assert total == 1155 + 897 and steps >= 10
    assert changed == stepped and stepped > 0, r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_racer.py"), "--device-update", "--episodes", "1"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "requires --device-actor --device-batch" in r.stderr
