"""The image drivers at the populations where their launch geometry changes (tests/_population_cases.py; DESIGN.md sections 27, 28 and
29): okenv_world_act, okenv_memory_act, the frame ring's push and batch, and once each okenv_cnn_act, okenv_bev_encode and okenv_qcnn_act,
against their host entries bit for bit.  The shapes are the cheapest the mirrors have; what varies is the number of agents and which
of them are crashed or alive, set directly with dev.set(F_CRASHED) on frames of random bytes, so every case is asserted whatever a
driven population would have done.

The list of okWorldListKernel is not read back: the handle has no entry that returns the work space's list, and none was added.  The
record pins it instead: controllers, headings, hidden states and frames differ from agent to agent, so under first_only_alive,
last_only_alive and alternate a slot that held another agent, or a count off by one, changes a record row or leaves a sentinel."""
import numpy as np
import pytest
import torch

import _bev_encoder_numpy as bev_mirror
import _cnn_numpy as cnn_mirror
import _memory_numpy as mmirror
import _population_cases as P
import _qcnn_numpy as qmirror
import _world_numpy as wmirror
from test_gpu_bev_encoder import RAYS, fan, same
from test_gpu_memory import act_both, assert_equal, attach, configs, drawn
from test_gpu_qcnn import config, record
from test_gpu_world import RECORD, host_act, record_tensors

pytestmark = pytest.mark.gpu

f32 = np.float32
RING_FIELDS = ("state", "next_state", "action", "reward", "done")


def population(gpu, N):
    """N agents placed on Austin, one step taken so that every field holds a value; nothing is driven."""
    from openkitchen_amd.torch_env import VectorEnvironment
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=False, seed=3)
    venv.env.reset_random(None, 1, 5, 0, 0)
    venv.env.step(1)
    return venv


def set_state(capi, dev, crashed, seed):
    """The crashed flags as given; headings and stored actions drawn, every agent its own."""
    N = crashed.size
    rng = np.random.default_rng(8000 + seed)
    dev.set(capi.F_CRASHED, crashed)
    dev.set(capi.F_ROT, rng.uniform(-180.0, 180.0, N).astype(f32))
    dev.set(capi.F_THROTTLE, rng.uniform(20.0, 100.0, N).astype(f32))
    dev.set(capi.F_STEER, rng.uniform(-5.0, 5.0, N).astype(f32))


def random_frames(N, S, seed):
    frames = torch.from_numpy(np.random.default_rng(7000 + seed).integers(0, 256, (N, S, S, 4), dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return frames


# ---- a. the world act --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, N, skip, pattern", P.WORLD_CASES)
def test_world_act_device_equals_host(gpu, name, N, skip, pattern):
    capi = gpu.capi
    shape = wmirror.SHAPES[name]
    S, Z = shape["image_size"], shape["latent"]
    cfg = capi.world_config(**dict(shape, skip_crashed=skip))
    assert capi.world_plan(cfg) == wmirror.PATHS[name]
    enc, ctrl = wmirror.draw_params(shape, N, N)
    venv = population(gpu, N)
    dev = venv.env
    crashed = P.crashed(pattern, N)
    set_state(capi, dev, crashed, N)
    gone = (crashed != 0) if skip else np.zeros(N, bool)
    alive = ~gone
    assert int(alive.sum()) == (N - int(crashed.sum()) if skip else N)
    frames = random_frames(N, S, N)
    sentinels = dict(mu=-7.0, state=-7.0, out=-7.0, throttle=-3.0, steer=-3.0, alive=9)
    into = dict(mu=np.full((N, Z), -7.0, f32), state=np.full((N, Z + 2), -7.0, f32), out=np.full(N, -7.0, f32), throttle=np.full(N, -3.0, f32),
                steer=np.full(N, -3.0, f32), alive=np.full(N, 9, np.uint8))
    want = host_act(capi, cfg, enc, ctrl, frames, dev, into=into)
    if alive.any():  # a wrong slot would show: every alive agent has a latent and an output of its own
        assert np.isfinite(want["mu"][alive]).all() and (np.abs(want["out"][alive]) < 1).all()
        assert len(set(want["out"][alive].tolist())) == int(alive.sum()) and len({r.tobytes() for r in want["mu"][alive]}) == int(alive.sum())
    assert dev.world_create(cfg) == (enc.size, ctrl.shape[1])
    dev.world_set_params("encoder", enc)
    dev.world_set_params("controllers", ctrl)
    rec = record_tensors(N, Z)
    dev.set(capi.F_THROTTLE, np.full(N, -3.0, f32))
    dev.set(capi.F_STEER, np.full(N, -3.0, f32))
    torch.cuda.synchronize()
    dev.world_act(frames, rec)  # (an empty list too: the call returns OK, capi.check raises otherwise)
    torch.cuda.synchronize()
    got = {k: rec[k].cpu().numpy() for k in RECORD}
    got.update(throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER))
    for k, v in got.items():
        w = np.stack([want["throttle"], want["steer"]], axis=1) if k == "action" else want[k]
        assert same(v[alive], w[alive]), "%s: %d of %d alive agents differ, the first at agent %d" % (
            k, int((v[alive] != w[alive]).reshape(int(alive.sum()), -1).any(1).sum()), int(alive.sum()),
            int(np.flatnonzero((v != w).reshape(N, -1).any(1) & alive)[0]))
        # under skip_crashed a crashed agent keeps its sentinels in the record and in the action fields
        assert (v[gone] == (-7.0 if k == "action" else sentinels[k])).all(), "%s: written for a crashed agent" % k
    assert np.array_equal(got["alive"][alive], (crashed[alive] == 0).astype(np.uint8))
    venv.close()


# ---- b. the memory act -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, N, carry, skip, pattern", P.MEMORY_CASES)
def test_memory_act_device_equals_host(gpu, name, N, carry, skip, pattern):
    """Two acts in a row with a step between them: the second reads, through the list, the hidden state the first wrote."""
    capi = gpu.capi
    w, mem, Z, H, L, h = mmirror.shape_of(name)
    wc, mc = configs(capi, name, carry, skip)
    assert capi.memory_plan(wc, mc) == mmirror.PATHS[name][:6] + (carry, L)
    enc, net, ctrl, hidden = drawn(name, N + carry, N)
    venv = population(gpu, N)
    dev = venv.env
    attach(dev, wc, mc, enc, net, ctrl)
    first = P.crashed(pattern, N) != 0
    set_state(capi, dev, first.astype(np.uint8), N)
    dev.memory_set_hidden(hidden)
    seen = []
    for t in range(2):
        crashed = dev.get(capi.F_CRASHED) != 0
        assert (crashed[first]).all()  # (without auto-reset a crashed agent stays crashed; a step may add some)
        got, want = act_both(capi, dev, wc, mc, enc, net, ctrl, random_frames(N, w["image_size"], 2 * N + t))
        assert_equal(got, want, "act %d" % t)
        alive = ~crashed if skip else np.ones(N, bool)
        if alive.any():
            assert np.isfinite(got["hidden_state"]).all() and np.abs(got["hidden_state"][alive]).max() < 1 and (np.abs(got["out"][alive]) < 1).all()
            assert np.array_equal(got["alive"][alive], (~crashed[alive]).astype(np.uint8))
            assert len(set(got["out"][alive].tolist())) == int(alive.sum())  # every agent its own: a wrong slot would show
        if skip:  # a crashed agent's hidden state is what memory_set_hidden put there, its record entries the sentinels
            assert same(got["hidden_state"][first], hidden[first])
            assert (got["mu"][crashed] == -7.0).all() and (got["hidden"][crashed] == -7.0).all() and (got["alive"][crashed] == 9).all()
        seen.append((got, alive))
        dev.step(1)
    both = seen[0][1] & seen[1][1]
    if both.any():
        assert not same(seen[0][0]["hidden_state"][both], seen[1][0]["hidden_state"][both])
    venv.close()


# ---- c. the frame ring ---------------------------------------------------------------------------------------------------------------------

def batch_tensors(B, S):
    f = dict(dtype=torch.float32, device="cuda")
    return dict(state=torch.empty((B, S, S), **f), next_state=torch.empty((B, S, S), **f), action=torch.empty(B, dtype=torch.int64, device="cuda"),
                reward=torch.empty(B, **f), done=torch.empty(B, **f), index=torch.empty(B, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("case", range(len(P.RING_CASES)), ids=["%s-%d-%s-%d" % c for c in P.RING_CASES])
def test_ring_push_and_batch_device_equal_host(gpu, case):
    """Three pushes; after each one every ring field, `pushed` and `size`, a SEQUENTIAL batch of size + 3 (it wraps) and a UNIFORM batch
    of 50 against the host entries.  The handle has no entry that sets the ring's fields, so both rings start from zeros.  Every
    second case hands a reward array over, the others take the clearance rule from F_DIST."""
    capi = gpu.capi
    name, N, selection, capacity = P.RING_CASES[case]
    with_reward = case % 2 == 1
    shape = qmirror.SHAPES[name]
    S, A = shape["image_size"], shape["num_actions"]
    push_all = selection == "push_all"
    cfg = config(capi, name, "eps_greedy", 0.5)
    assert capi.qcnn_plan(cfg)[2] == (1 if name == "tiny" else 0)  # planes as 16-byte vectors, or float by float
    venv = population(gpu, N)
    dev = venv.env
    dev.qcnn_create(cfg)
    dev.qcnn_ring_create(capacity, push_all)
    host_ring = capi.qcnn_ring(capacity, S)
    dist = dev.get(capi.F_DIST).reshape(N, RAYS)
    assert np.isfinite(dist).all() and 0.0 < dist.min() < 200.0 and len(set(dist.min(1).tolist())) > 1
    pushes = [P.ring_inputs(S, A, N, selection, push, RAYS) for push in range(P.RING_PUSHES)]
    if selection == "nobody":  # ... and then a ring that holds something: everybody, then nobody again
        pushes += [dict(P.ring_inputs(S, A, N, "all", 3, RAYS)), P.ring_inputs(S, A, N, selection, 4, RAYS)]
    expected = 0
    for t, x in enumerate(pushes):
        n = N if x["alive"] is None else int(x["alive"].sum())
        before = {k: host_ring[k].copy() for k in RING_FIELDS}
        dev.set(capi.F_CRASHED, x["crashed"])
        alive = x["alive"] if x["alive"] is not None else (np.arange(N) % 3 == 0).astype(np.uint8)  # PUSH_ALL does not read it
        rec = {"action": torch.from_numpy(x["action"]).cuda(), "alive": torch.from_numpy(alive).cuda()}
        cur, nxt, reward = torch.from_numpy(x["frames"]).cuda(), torch.from_numpy(x["next_frames"]).cuda(), torch.from_numpy(x["reward"]).cuda()
        torch.cuda.synchronize()
        dev.qcnn_push(rec, cur, nxt, reward if with_reward else None)
        torch.cuda.synchronize()
        capi.qcnn_push_host(host_ring, x["action"], x["alive"], x["frames"], x["next_frames"], x["crashed"], x["reward"] if with_reward else None, dist, push_all)
        expected += n
        assert host_ring["pushed"] == expected
        size = min(expected, capacity)
        assert dev.qcnn_ring_size() == (size, expected), "push %d" % t
        got = dev.qcnn_ring_get()
        for k in RING_FIELDS:
            assert same(got[k], host_ring[k]), "push %d, %s: %d slots differ" % (t, k, int((got[k] != host_ring[k]).reshape(capacity, -1).any(1).sum()))
        if n == 0:
            assert all(same(host_ring[k], before[k]) for k in RING_FIELDS)  # the empty selection leaves the ring as it was
        elif x["alive"] is not None and n > capacity:  # where the survivors lie
            unit = P.REPLAY_THREADS if N > P.REPLAY_THREADS else P.WAVE
            assert len(set((np.flatnonzero(x["alive"])[-capacity:] // unit).tolist())) > 1, "the survivors must be spread over workgroups (waves, in one)"
        for B, mode, start in ((size + 3, "sequential", 5 + t), (50, "uniform", t)):
            out = batch_tensors(B, S)
            dev.qcnn_batch(B, out, mode, start)
            torch.cuda.synchronize()
            want = capi.qcnn_batch_host(host_ring, B, mode, start, seed=cfg.seed)
            for k, v in want.items():
                assert same(out[k].cpu().numpy(), v), (t, B, mode, k)
            assert size == 0 or 0 <= int(out["index"].min()) <= int(out["index"].max()) < size
    if selection == "nobody":
        assert expected == N
    elif selection == "four_corners":
        assert expected == 4 * P.RING_PUSHES
    elif selection == "group1_gone":
        assert expected == (N - P.REPLAY_THREADS) * P.RING_PUSHES < capacity
    venv.close()


# ---- d. the per-frame kernels once at a population beyond one workgroup of 256 ----------------------------------------------------------------

PER_FRAME_N = P.LIST_THREADS + 1


def test_cnn_act_device_equals_host_at_257_agents(gpu):
    capi = gpu.capi
    N, shape = PER_FRAME_N, cnn_mirror.SHAPES["tiny"]
    cfg, params = capi.cnn_config(throttle=80.0, steer_scale=7.0, **shape), cnn_mirror.draw_params(shape, 5)
    venv = population(gpu, N)
    dev = venv.env
    crashed = P.crashed("random30", N)
    set_state(capi, dev, crashed, N)
    frames = random_frames(N, shape["image_size"], 31)
    want = capi.cnn_act_host(cfg, params, frames.cpu().numpy(), crashed)
    dev.cnn_create(cfg)
    dev.cnn_set_params(params)
    rec = {"out": torch.full((N,), -7.0, device="cuda"), "action": torch.full((N, 2), -7.0, device="cuda"), "alive": torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    dev.cnn_act(frames, rec)
    torch.cuda.synchronize()
    assert same(rec["out"].cpu().numpy(), want["out"]) and same(rec["alive"].cpu().numpy(), want["alive"])
    assert same(rec["action"].cpu().numpy(), np.stack([want["throttle"], want["steer"]], axis=1))
    assert same(dev.get(capi.F_THROTTLE), want["throttle"]) and same(dev.get(capi.F_STEER), want["steer"])
    assert np.array_equal(want["alive"], (crashed == 0).astype(np.uint8)) and len(set(want["out"].tolist())) > N // 2
    venv.close()


def test_bev_encode_device_equals_host_at_257_agents(gpu):
    capi = gpu.capi
    N, shape = PER_FRAME_N, bev_mirror.SHAPES["tiny"]
    cfg, params = capi.bev_config(**shape), bev_mirror.draw_params(shape, 5)
    venv = population(gpu, N)
    dev = venv.env
    frames = random_frames(N, shape["image_size"], 32)
    want = capi.bev_encode_host(cfg, params, frames.cpu().numpy())
    dev.bev_create(cfg)
    dev.bev_set_params(params)
    out = torch.full((N, shape["embed_dim"]), -7.0, device="cuda")
    torch.cuda.synchronize()
    dev.bev_encode(frames, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert same(got, want), "%d of %d rows differ" % (int((got != want).any(1).sum()), N)
    assert np.isfinite(want).all() and len({r.tobytes() for r in want}) == N
    venv.close()


def test_qcnn_act_device_equals_host_at_257_agents(gpu):
    capi = gpu.capi
    N, shape = PER_FRAME_N, qmirror.SHAPES["tiny"]
    A = shape["num_actions"]
    cfg, params = config(capi, "tiny", "eps_greedy", 0.5), qmirror.draw_params(shape, 5)
    venv = population(gpu, N)
    dev = venv.env
    crashed = P.crashed("random30", N)
    set_state(capi, dev, crashed, N)
    frames = random_frames(N, shape["image_size"], 33)
    want = capi.qcnn_act_host(cfg, params, frames.cpu().numpy(), crashed, dev.step_count)
    dev.qcnn_create(cfg)
    dev.qcnn_set_params(params)
    rec = record(N, A)
    torch.cuda.synchronize()
    dev.qcnn_act(frames, rec)
    torch.cuda.synchronize()
    for k in ("q", "action", "value", "alive"):
        assert same(rec[k].cpu().numpy(), want[k]), k
    assert same(dev.get(capi.F_THROTTLE), want["throttle"]) and same(dev.get(capi.F_STEER), want["steer"])
    assert np.array_equal(want["alive"], (crashed == 0).astype(np.uint8)) and len(set(want["action"].tolist())) == A
    venv.close()
