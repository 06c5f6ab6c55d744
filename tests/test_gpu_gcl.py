"""Guided cost learning on the device (okenv_gcl_*; openkitchen_amd/csrc/ok_gcl.h): the act kernel, the cost forward and the three
updates' kernels bit-equal to the host entries that share their rule, at the edges of their launch geometry; NULL outputs; continuation
across calls; a captured act + step graph with the draw-offset word; the whole pipeline behind collect_episode_gcl, gcl_cost_update,
gcl_rewards, prepare_gcl_batch and gcl_policy_update, eager and as replayed graph chunks, against the host entries; coexistence with a
Gaussian actor and a section 14 actor on one handle; the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HP = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
CLIP = 0.2
SHAPES = [(7, 64, 64), (1, 1, 1), (6, 9, 13), (5, 33, 31), (62, 64, 64)]
REC = ("state", "eps", "pre", "squashed", "action", "logp", "alive")
NETS = ("policy", "value", "cost")


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def fan_of(gpu, R):
    return gpu.default_ray_fan(R) if R > 1 else np.zeros(1, dtype=f32)


def fresh(gpu, rng, which, shape, scale=0.3, log_std=(0.0, -0.5)):
    par = (rng.standard_normal(gpu.capi.gcl_num_params(which, *shape)) * scale).astype(f32)
    if which == "policy":
        par[:2] = log_std
    return {"params": par, "m": np.zeros_like(par), "v": np.zeros_like(par), "t": 0}


def record_tensors(N, R):
    rec = {k: torch.full((N, 2), -7.0, device="cuda") for k in ("eps", "pre", "squashed", "action")}
    rec.update(state=torch.full((N, R), -7.0, device="cuda"), logp=torch.full((N,), -7.0, device="cuda"),
               alive=torch.full((N,), 9, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return rec


def rel_xy(gpu, dev):
    return np.stack([dev.get(gpu.capi.F_REL_X), dev.get(gpu.capi.F_REL_Y)], axis=-1).reshape(dev.N, dev.R, 2)


def handle_for(gpu, shape, states, n_agents=8, seed=11):
    R, H1, H2 = shape
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), n_agents, ray_angles_deg=fan_of(gpu, R))
    sizes = dev.gcl_create(hidden1=H1, hidden2=H2, cost_hidden1=H1, cost_hidden2=H2, seed=seed)
    assert sizes == {k: gpu.capi.gcl_num_params(k, *shape) for k in NETS}
    load(dev, states)
    return dev


def load(dev, states):
    """Parameters in, moments zeroed, step counts 0."""
    for k in NETS:
        dev.gcl_set_params(k, states[k]["params"])
    dev.gcl_learner_create(clip=CLIP, cost_lr=HP["lr"], **HP)


def assert_state(got, want, what):
    assert got["t"] == want["t"], what
    for k in ("params", "m", "v"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)


# ---- acting ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 257, 1025])
@pytest.mark.parametrize("shape", SHAPES)
def test_act_device_equals_host(gpu, shape, N):
    """N = 1 is one lane group, 257 a second workgroup with one agent, 1025 a partly filled last workgroup; crashed agents,
    agent_base != 0, each record pointer NULL in turn with its buffer's sentinel untouched, greedy, and two calls without a sync."""
    R, H1, H2 = shape
    rng = np.random.default_rng(N + 3 * H1)
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan_of(gpu, R))
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(3)
    crashed = dev.get(gpu.capi.F_CRASHED)
    crashed[rng.random(N) < 0.2] = 1
    dev.set(gpu.capi.F_CRASHED, crashed)
    rel = rel_xy(gpu, dev)
    count, base = dev.step_count, 3_000_000_000
    st = fresh(gpu, rng, "policy", shape, log_std=(0.0, 1.0) if N == 257 else (-3.0, 0.0))
    scale, bias = (50.0, 10.0), (50.0, 0.0)
    dev.gcl_create(hidden1=H1, hidden2=H2, cost_hidden1=1, cost_hidden2=1, scale=scale, bias=bias, seed=13, agent_base=base)
    dev.gcl_set_params("policy", st["params"])
    for greedy in (False, True):
        dev.gcl_set_greedy(greedy)
        want = gpu.gcl_act_host(gpu.capi.gcl_config(H1, H2, 1, 1, scale, bias, greedy, 13, base), st["params"], rel, crashed, count)
        for skip in (None,) + REC:
            rec = record_tensors(N, R)
            dev.gcl_act({k: (None if k == skip else v) for k, v in rec.items()})
            if skip is None:  # a second call without a sync in between: the same record
                dev.gcl_act(rec)
            dev.sync()
            assert same(dev.get(gpu.capi.F_THROTTLE), want["throttle"]) and same(dev.get(gpu.capi.F_STEER), want["steer"]), (greedy, skip)
            for k in rec:
                got = rec[k].cpu().numpy()
                if k == skip or (k == "eps" and greedy):
                    assert (got == (9 if k == "alive" else -7)).all(), (greedy, skip, k)
                else:
                    assert same(got, want[k]), (greedy, skip, k)
    dev.gcl_act(None)  # no record at all
    dev.sync()
    assert same(dev.get(gpu.capi.F_THROTTLE), want["throttle"])
    dev.close()


# ---- the cost network ----------------------------------------------------------------------------------------------------------------

def cost_case(gpu, dev, rng, shape, states, E, Mp, Me, want=("loss", "grad"), reload=True):
    R = shape[0]
    if reload:
        load(dev, states)
    st = states["cost"] if reload else dict(dev.gcl_state("cost"))
    bank = {"state": rng.random((E, R)).astype(f32), "action": (rng.random((E, 2)) * 2 - 1).astype(f32)}
    batch = {"state": rng.random((Mp, R)).astype(f32), "squashed": (rng.random((Mp, 2)) * 2 - 1).astype(f32)}
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    dev.gcl_set_expert(torch.from_numpy(bank["state"]).cuda(), torch.from_numpy(bank["action"]).cuda())
    sizes = {"loss": 1, "grad": st["params"].size}
    out = {k: torch.full((sizes[k],), 77.0, device="cuda") for k in want}
    logits = torch.full((Mp,), 77.0, device="cuda")
    torch.cuda.synchronize()
    dev.gcl_cost(d["state"], d["squashed"], logits)
    dev.gcl_cost_update(d, Mp, Me, out=out)
    dev.sync()
    what = (shape, E, Mp, Me)
    assert same(logits.cpu().numpy(), gpu.gcl_cost_host(st["params"], shape, batch["state"], batch["squashed"])), what
    new, host = gpu.gcl_cost_update_host(gpu.capi.learner_params(clip=0.0, **HP), 11, shape, st, bank, batch, Me)
    for k in want:
        assert np.array_equal(bits(out[k].cpu().numpy()), bits(host[k])), (k,) + what
    assert_state(dev.gcl_state("cost"), new, what)


@pytest.mark.parametrize("shape", SHAPES)
def test_cost_forward_and_update_device_equal_host(gpu, shape):
    """Mp and Me in {1, 33, 1000} crossed (Mp != Me in six of the nine), banks of 1, 33 and 5000 rows; chunk counts 1, 2, 3, 17 and 129
    in either set; NULL outputs; three updates in a row without reloading (the update number moves the expert draws)."""
    rng = np.random.default_rng(sum(shape) + 5)
    states = {k: fresh(gpu, rng, k, shape) for k in NETS}
    dev = handle_for(gpu, shape, states)
    for i, (Mp, Me) in enumerate((a, b) for a in (1, 33, 1000) for b in (1, 33, 1000)):
        cost_case(gpu, dev, rng, shape, states, (1, 33, 5000)[i % 3], Mp, Me)
    for i, chunks in enumerate((1, 2, 3, 17, 129)):
        M = 32 * chunks - (5 if chunks > 1 else 0)
        cost_case(gpu, dev, rng, shape, states, 700, M if i % 2 else 40, 40 if i % 2 else M)
    for want in (("loss",), ("grad",), ()):
        cost_case(gpu, dev, rng, shape, states, 50, 70, 45, want=want)
    load(dev, states)
    for _ in range(3):
        cost_case(gpu, dev, rng, shape, states, 90, 64, 65, reload=False)
    assert dev.gcl_state("cost")["t"] == 3
    dev.close()


# ---- the policy / value update -----------------------------------------------------------------------------------------------------

OUT = ("policy_loss", "value_loss", "clipped", "grad_policy", "grad_value", "adv")


def policy_case(gpu, dev, rng, shape, states, M, B, accumulate, reduce, permuted=False, want=OUT, reload=True, batch=None):
    R = shape[0]
    if reload:
        load(dev, states)
    pol, val = (states["policy"], states["value"]) if reload else (dict(dev.gcl_state("policy")), dict(dev.gcl_state("value")))
    if batch is None:
        batch = {"state": rng.random((M, R)).astype(f32), "pre": (rng.standard_normal((M, 2)) * 0.7).astype(f32), "ret": rng.standard_normal(M).astype(f32)}
        # logp_old near the logp of (state, pre) under the policy, so that ratios fall below, inside and above the range
        import _gcl_numpy as N_
        batch["logp"] = (N_.logp_of(pol["params"], shape, batch["state"], batch["pre"]) + rng.standard_normal(M) * 0.3).astype(f32)
    order = rng.permutation(M).astype(np.int32) if permuted else None
    steps = 1 if accumulate else (M + B - 1) // B
    sizes = {"policy_loss": steps, "value_loss": steps, "clipped": steps, "grad_policy": pol["params"].size, "grad_value": val["params"].size, "adv": M}
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    o = None if order is None else torch.from_numpy(order).cuda()
    out = {k: (torch.full((sizes[k],), 77, dtype=torch.int32, device="cuda") if k == "clipped" else torch.full((sizes[k],), 77.0, device="cuda")) for k in want}
    torch.cuda.synchronize()
    dev.gcl_policy_update(d, M, B, accumulate=accumulate, reduce=reduce, order=o, out=out)
    dev.sync()
    newp, newv, host = gpu.gcl_policy_update_host(gpu.capi.learner_params(clip=CLIP, **HP), shape, pol, val, batch, B, accumulate, reduce, order)
    what = (shape, M, B, accumulate, reduce, permuted)
    for k in want:
        got = out[k].cpu().numpy()
        assert (np.array_equal(got, host[k]) if k == "clipped" else np.array_equal(bits(got), bits(host[k]))), (k,) + what
    assert_state(dev.gcl_state("policy"), newp, what)
    assert_state(dev.gcl_state("value"), newv, what)
    return host


@pytest.mark.parametrize("shape", SHAPES)
def test_policy_update_device_equals_host(gpu, shape):
    """M in {1, 33, 1000} x B in {1, 32, 33, 1000} x accumulate x reduce on one handle per shape, an order on every third case: a chunk
    edge, a partial last chunk, a partial last slice, a padded tree, the accumulator over up to a thousand slices, the advantages'
    tree over 1, 2 and 32 chunks, every edge of the register tiles of the weight matrices."""
    rng = np.random.default_rng(sum(shape) + 2)
    states = {k: fresh(gpu, rng, k, shape) for k in NETS}
    dev = handle_for(gpu, shape, states)
    i = clipped = 0
    for M in (1, 33, 1000):
        for B in (1, 32, 33, 1000):
            for accumulate in (True, False):
                for reduce in ("sum", "mean"):
                    clipped += int(policy_case(gpu, dev, rng, shape, states, M, B, accumulate, reduce, permuted=i % 3 == 0)["clipped"].sum())
                    i += 1
    assert clipped > 0
    dev.close()


def test_policy_chunk_counts_four_slices_null_outputs_and_continuation(gpu):
    rng = np.random.default_rng(40)
    shape = (6, 9, 13)
    states = {k: fresh(gpu, rng, k, shape) for k in NETS}
    dev = handle_for(gpu, shape, states)
    for i, chunks in enumerate((1, 2, 3, 17, 129)):
        M = 32 * chunks - (5 if chunks > 1 else 0)
        policy_case(gpu, dev, rng, shape, states, M, M, i % 2 == 0, "sum" if i % 2 else "mean")
    for accumulate in (True, False):  # M = 3 B + 1: four slices, the last of one sample
        policy_case(gpu, dev, rng, shape, states, 3 * 50 + 1, 50, accumulate, "mean", permuted=True)
    for want in (("policy_loss",), ("clipped",), ("adv", "grad_value"), ()):
        policy_case(gpu, dev, rng, shape, states, 300, 128, True, "mean", want=want)
    # continuation: calls that start from the state the call before left on the device
    load(dev, states)
    for k in range(3):
        policy_case(gpu, dev, rng, shape, states, 100 + k, 64, k == 1, "mean", reload=False)
    assert dev.gcl_state("policy")["t"] == dev.gcl_state("value")["t"] == 2 + 1 + 2
    # the next act uses the stepped parameters
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(2)
    rec = record_tensors(dev.N, shape[0])
    dev.gcl_act(rec)
    dev.sync()
    want = gpu.gcl_act_host(gpu.capi.gcl_config(shape[1], shape[2], shape[1], shape[2], seed=11), dev.gcl_state("policy")["params"], rel_xy(gpu, dev),
                            dev.get(gpu.capi.F_CRASHED), dev.step_count)
    for k in REC:
        assert same(rec[k].cpu().numpy(), want[k]), k
    dev.close()


def test_recorded_on_the_device_the_ratio_is_one(gpu):
    """Records of okenv_gcl_act fed back to okenv_gcl_policy_update before any step: nothing is clipped, and the loss is the one the host
    entry gives for ratios of exactly 1."""
    rng = np.random.default_rng(43)
    shape = (7, 64, 64)
    N, T = 200, 6
    states = {k: fresh(gpu, rng, k, shape, scale=0.15) for k in NETS}
    dev = handle_for(gpu, shape, states, n_agents=N)
    dev.reset_random(None, 1, 5, 0, 0)
    recs = []
    for _ in range(T):
        dev.step(1)
        rec = record_tensors(N, 7)
        dev.gcl_act(rec)
        recs.append(rec)
    dev.sync()
    batch = {k: torch.cat([r[k] for r in recs]).cpu().numpy() for k in ("state", "pre", "logp")}
    batch["ret"] = rng.standard_normal(N * T).astype(f32)
    host = policy_case(gpu, dev, rng, shape, states, N * T, 4096, True, "mean", batch=batch)
    assert host["clipped"][0] == 0
    import _gcl_numpy as N_
    want = N_.policy_update(states["policy"], states["value"], shape, batch, 4096, clip=CLIP, **HP)[2]
    assert (want["r"] == 1).all() and np.array_equal(bits(want["policy_loss"]), bits(host["policy_loss"]))
    dev.close()


# ---- coexistence -------------------------------------------------------------------------------------------------------------------

def test_coexistence_with_a_gaussian_actor_and_a_section_14_actor(gpu):
    rng = np.random.default_rng(50)
    R, N = 5, 40
    shape = (R, 33, 31)
    states = {k: fresh(gpu, rng, k, shape) for k in NETS}
    dev = handle_for(gpu, shape, states, n_agents=N, seed=3)
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(2)
    table = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0))
    n_pol, _ = dev.actor_create(16, table, 0, "sample", 0.0, seed=1)
    dev.actor_set_params((rng.standard_normal(n_pol) * 0.5).astype(f32), None)
    dev.learner_create(lr=0.01)
    gpar = (rng.standard_normal(dev.gauss_create(16, 16, seed=2)) * 0.3).astype(f32)
    dev.gauss_set_params(gpar)
    dev.gauss_learner_create(**HP)

    def others():
        g = dev.gauss_state()
        return [dev.actor_get_params()[0]] + [dev.learner_state()[k] for k in ("policy_m", "policy_v")] + [g[k] for k in ("params", "m", "v")]

    def ours():
        return [dev.gcl_state(k)[v] for k in NETS for v in ("params", "m", "v")]

    before = [a.copy() for a in others()]
    M = 100
    batch = {"state": rng.random((M, R)).astype(f32), "pre": (rng.standard_normal((M, 2)) * 0.7).astype(f32), "logp": (-2.5 - rng.random(M)).astype(f32),
             "ret": rng.standard_normal(M).astype(f32)}
    d = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    sq = torch.tanh(d["pre"])
    dev.gcl_act(record_tensors(N, R))
    dev.gcl_set_expert(d["state"][:30].contiguous(), sq[:30].contiguous())
    dev.gcl_cost_update({"state": d["state"], "squashed": sq}, M, 64)
    dev.gcl_policy_update(d, M, 64)
    dev.sync()
    for a, b in zip(before, others()):
        assert same(a, b)
    mine = [a.copy() for a in ours()]
    assert dev.gcl_state("policy")["t"] == 1 and dev.gcl_state("cost")["t"] == 1 and not same(mine[0], states["policy"]["params"])
    # the reverse: their act and updates leave the GCL object alone
    arec = {"state": torch.zeros((N, R), device="cuda"), "action": torch.zeros(N, dtype=torch.int64, device="cuda"), "prob": torch.zeros(N, device="cuda"),
            "alive": torch.zeros(N, dtype=torch.uint8, device="cuda")}
    dev.actor_act(arec)
    dev.reinforce_update({"state": d["state"], "action": torch.from_numpy(rng.integers(0, 3, M).astype(np.int64)).cuda(), "ret": d["ret"]}, M, 64)
    dev.gauss_act(None)
    dev.gauss_update({"state": d["state"], "eps": d["pre"], "ret": d["ret"]}, M, 64)
    dev.sync()
    for a, b in zip(mine, ours()):
        assert same(a, b)
    assert not same(before[0], dev.actor_get_params()[0]) and not same(before[3], dev.gauss_state()["params"])  # (their updates did run)
    dev.close()


# ---- through torch_env and rollout -----------------------------------------------------------------------------------------------------

FAN7 = np.linspace(-90, 90, 7).astype(f32)


def modules(R=7, H=64):
    class Net(torch.nn.Module):  # built like RLRacers/GuidedCostLearning/Networks.hpp
        def __init__(self, n_in, out, log_std):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = torch.nn.Linear(n_in, H), torch.nn.Linear(H, H), torch.nn.Linear(H, out)
            if log_std:
                self.log_std = torch.nn.Parameter(torch.zeros(2))

    torch.manual_seed(3)
    policy, value, cost = Net(R, 2, True).cuda(), Net(R, 1, False).cuda(), Net(R + 2, 1, False).cuda()
    cost.fc3.weight.data.mul_(0.1)
    cost.fc3.bias.data.mul_(0.0)
    return policy, value, cost


def flat_of(module):
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()]).cpu().numpy()


def make_venv(gpu, N, auto_reset, track="Silverstone", seed=7):
    from openkitchen_amd.torch_env import VectorEnvironment
    venv = VectorEnvironment(gpu.track_path(track), N, num_rays=7, ray_angles_deg=FAN7, auto_reset=auto_reset, randomize_lane=True, randomize_heading=True,
                             seed=seed, agent_base=100)
    nets = modules()
    venv.enable_gcl(*nets)
    return venv, nets


def test_graph_of_act_and_step_with_the_draw_offset_word(gpu):
    """gcl_act + step captured once and replayed 64 times, the draw index carried by the caller-owned offset word: every replay's
    record equals the host entry's at that draw index on the hits the replay saw."""
    N, replays = 300, 64
    venv, (policy, _, _) = make_venv(gpu, N, False)
    venv.reset()
    rec = record_tensors(N, 7)
    rel_before = torch.empty((2, N, 7), device="cuda")
    offset = torch.zeros(1, dtype=torch.int32, device="cuda")

    def body():
        rel_before[0].copy_(venv.rel_x)
        rel_before[1].copy_(venv.rel_y)
        venv.gcl_act(rec)
        venv.step()
        offset.add_(1)

    offset.add_(0)
    rel_before[0].copy_(venv.rel_x)
    base = venv.env.step_count
    venv.env.gcl_set_draw_offset(offset)
    graph = venv.capture(body, warmup=0)
    offset.zero_()
    cfg = gpu.capi.gcl_config(64, 64, 64, 64, seed=7, agent_base=100)
    par = flat_of(policy)
    assert [n for n, _ in policy.named_parameters()][0] == "log_std"
    for k in range(replays):
        crashed = venv.crashed.cpu().numpy().copy()
        graph.replay()
        torch.cuda.synchronize()
        rel = rel_before.cpu().numpy()
        want = gpu.gcl_act_host(cfg, par, np.stack([rel[0], rel[1]], axis=-1), crashed, base + k)
        for name in REC:
            assert same(rec[name].cpu().numpy(), want[name]), (k, name)
    assert int(offset.item()) == replays
    venv.env.gcl_set_draw_offset(None)
    venv.close()


def test_whole_pipeline_eager_equals_chunked_equals_the_host_entries(gpu):
    """64 agents on Silverstone, two episodes of collect_demonstrations -> set_gcl_expert -> collect_episode_gcl -> gcl_cost_update ->
    collect_episode_gcl -> gcl_rewards -> prepare_gcl_batch -> gcl_policy_update: eager == graph_chunk = 8 == the host entries fed the
    same records; the bank's rows equal the device actor's state formula bit for bit."""
    import _gcl_numpy as N_
    from openkitchen_amd.demonstrations import collect_demonstrations
    from openkitchen_amd.rollout import collect_episode_gcl, gcl_cost_update, gcl_policy_update, gcl_rewards, prepare_gcl_batch
    N, T, shape = 64, 24, (7, 64, 64)
    lp = gpu.capi.learner_params(lr=0.01, clip=CLIP)
    runs = {}
    for chunk in (0, 8):
        venv, nets = make_venv(gpu, N, True)
        venv.enable_gcl_learner(lr=0.01, clip=CLIP, cost_lr=0.01)
        venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=10.0)
        demos = collect_demonstrations(venv, 16, seed=1)
        E = venv.set_gcl_expert(demos)
        bank = {"state": venv._gcl_bank[0].cpu().numpy(), "action": venv._gcl_bank[1].cpu().numpy()}
        keep = demos["alive"].cpu().numpy().reshape(-1) != 0
        acts = demos["actions"].cpu().numpy().reshape(-1, 2)[keep]
        assert E == int(keep.sum()) > 0
        assert same(bank["state"], N_.state_of(demos["rel_xy"].cpu().numpy().reshape(-1, 7, 2)[keep]))
        assert same(bank["action"], np.stack([((acts[:, 0] / f32(100.0)) - f32(0.5)) * f32(2.0), acts[:, 1] / f32(10.0)], axis=1))
        states = {k: dict(venv.env.gcl_state(k)) for k in NETS}
        log = []
        for episode in range(2):
            ep1 = collect_episode_gcl(venv, T, graph_chunk=chunk)
            c_out = gcl_cost_update(venv, ep1, grads=True)
            ep2 = collect_episode_gcl(venv, T, graph_chunk=chunk)
            rewards = gcl_rewards(venv, ep2)
            batch = prepare_gcl_batch(venv, ep2, rewards)
            p_out = gcl_policy_update(venv, batch, slice=1024, grads=True)
            venv.synchronize()
            h = lambda d: {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
            log.append((h(ep1), h(c_out), h(ep2), rewards.cpu().numpy(), h(batch), h(p_out), {k: dict(venv.env.gcl_state(k)) for k in NETS}))
        before = flat_of(nets[0])
        venv.pull_gcl()
        assert same(flat_of(nets[0]), log[-1][6]["policy"]["params"]) and not same(before, flat_of(nets[0]))
        assert same(flat_of(nets[2]), log[-1][6]["cost"]["params"])
        runs[chunk] = (states, log)
        venv.close()
    (st, eager), (_, chunked) = runs[0], runs[8]
    for a, b in zip(eager, chunked):
        for x, y in zip(a, b):
            if isinstance(x, dict):
                for k in x:
                    if isinstance(x[k], dict):
                        assert all(same(x[k][v], y[k][v]) for v in ("params", "m", "v")), k
                    elif k not in ("stats", "count"):
                        assert same(x[k], y[k]), k
            else:
                assert same(x, y)
    # the host entries fed the same records
    for ep1, c_out, ep2, rewards, batch, p_out, after in eager:
        assert ep1["alive"].any() and ep1["states"].shape == (T, N, 7)
        keep = ep1["alive"].reshape(-1)
        cb = {"state": ep1["states"].reshape(-1, 7)[keep], "squashed": ep1["squashed"].reshape(-1, 2)[keep]}
        st["cost"], host = gpu.gcl_cost_update_host(lp, 7, shape, st["cost"], bank, cb, int(keep.sum()))
        assert same(c_out["loss"], host["loss"]) and same(c_out["grad"], host["grad"])
        assert_state(after["cost"], st["cost"], ("cost",))
        assert same(rewards.reshape(-1), -gpu.gcl_cost_host(st["cost"]["params"], shape, ep2["states"].reshape(-1, 7), ep2["squashed"].reshape(-1, 2)))
        flat = batch["index"].astype(np.int64)
        assert same(batch["pre"], ep2["pre"].reshape(-1, 2)[flat]) and same(batch["log_probs"], ep2["log_probs"].reshape(-1)[flat])
        assert same(batch["states"], ep2["states"].reshape(-1, 7)[flat]) and batch["count"] == int(ep2["alive"].sum())
        hb = {"state": batch["states"], "pre": batch["pre"], "logp": batch["log_probs"], "ret": batch["returns"]}
        st["policy"], st["value"], host = gpu.gcl_policy_update_host(lp, shape, st["policy"], st["value"], hb, 1024, True, "mean")
        for k in p_out:
            assert same(p_out[k], host[k]), k
        assert p_out["clipped"][0] == 0  # recorded with the parameters the update starts from: every ratio is exactly 1
        assert_state(after["policy"], st["policy"], ("policy",))
        assert_state(after["value"], st["value"], ("value",))


@pytest.mark.parametrize("extra", [(), ("--device-update",)])
def test_example_runs(extra):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "gcl_racer.py"), "--episodes", "2", "--agents", "64", "--steps", "16", "--expert-steps", "8"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "episode   1:" in r.stdout and "expert bank:" in r.stdout and "parameters finite True" in r.stdout
