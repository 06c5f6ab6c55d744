"""The flow-matching driver on the device (okenv_flow_*; openkitchen_amd/csrc/ok_flow.h): the act kernel bit-equal to the host entry
that shares its rule, at the edges of its launch geometry; with and without the noise; a draw-offset word; NULL record slots;
parameters from host and device pointers; the order of calls; the draw index; act + step captured in a graph."""
import ctypes as C

import numpy as np
import pytest
import torch

import _flow_numpy as mirror

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, STATE = -1, -5
RAYS = 7
REC = {"x0": lambda N: torch.full((N, 2), -7.0, device="cuda"), "x": lambda N: torch.full((N, 2), -7.0, device="cuda"),
       "action": lambda N: torch.full((N, 2), -7.0, device="cuda"), "alive": lambda N: torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
# Random-action steps on Austin after which the population holds crashed and alive agents alike, for 15 .. 33 agents (tests/test_gpu_lidar.py's
# recipe: 8 calls of rollout_random(25, seed 11) behind reset_random(seed 5) leave 1 .. 3 agents crashed)
RANDOM_CHUNKS, RANDOM_CHUNK_STEPS = 8, 25
OFFSET = 5  # the draw-offset word of the runs with noise


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def fan(R):
    return np.linspace(-90.0, 90.0, R).astype(f32)


def driven_population(gpu, N, R):
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan(R))
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    for i in range(RANDOM_CHUNKS):
        dev.rollout_random(RANDOM_CHUNK_STEPS, 11, 0, RANDOM_CHUNK_STEPS * i)
    return dev


# the widest shape of the rule: the activations leave no room in the LDS for a block of W2, and layer 2 reads it from global memory
WIDE = dict(cond_dim=512, hidden=512, steps=2)


def act_case(gpu, name, N):
    shape = WIDE if name == "wide" else mirror.SHAPES[name]
    capi = gpu.capi
    # the staging of W2 the shape was chosen for is the one its plan selects (tests/_flow_numpy.py)
    plan = mirror.plan(shape)
    assert plan["bytes"] == capi.flow_lds_bytes(capi.flow_config(**shape)) <= capi.FLOW_LDS_BUDGET
    assert (name in mirror.PATHS) == (name in mirror.NEW_SHAPES) and (name not in mirror.PATHS or mirror.PATHS[name](shape, plan)), plan
    rng = np.random.default_rng(7 * N + shape["hidden"])
    base = 2 ** 32 - 10  # the global ids wrap past 2^32 inside the larger populations
    cfgs = {noise: capi.flow_config(noise=noise, seed=13, agent_base=base, **shape) for noise in (0, 1)}
    params = mirror.random_params(capi, cfgs[1], rng)
    cond_host = rng.uniform(-1.0, 1.0, (N, shape["cond_dim"])).astype(f32)
    cond = torch.from_numpy(cond_host).cuda()
    dev = driven_population(gpu, N, RAYS)
    L, h = dev._L, dev._h
    assert L.okenv_flow_act(h, capi.ptr(cond), None) == STATE  # before create
    n = C.c_int32()
    assert L.okenv_flow_num_params(h, C.byref(n)) == STATE and L.okenv_flow_set_params(h, capi.ptr(params)) == STATE
    assert L.okenv_flow_set_draw_offset(h, None) == STATE
    # what a live handle refuses
    for bad in (dict(cond_dim=8), dict(cond_dim=24), dict(cond_dim=528), dict(hidden=8), dict(hidden=24), dict(hidden=528), dict(steps=0), dict(steps=257),
                dict(noise=2), dict(action_lo=(float("nan"), 0.0)), dict(action_hi=(1.0, float("inf")))):
        assert L.okenv_flow_create(h, C.byref(capi.flow_config(**dict(shape, **bad)))) == INVALID, bad
    assert L.okenv_flow_create(h, None) == INVALID and L.okenv_flow_act(h, capi.ptr(cond), None) == STATE
    assert dev.flow_create(cfgs[1]) == params.size
    assert L.okenv_flow_act(h, capi.ptr(cond), None) == STATE  # before set_params
    assert L.okenv_flow_get_params(h, capi.ptr(np.empty_like(params))) == STATE
    crashed = dev.get(capi.F_CRASHED)
    if N >= 15:
        assert 0 < int((crashed != 0).sum()) < N, "the population must hold crashed and alive agents"
    count = dev.step_count
    word = torch.full((1,), OFFSET, dtype=torch.int32, device="cuda")
    want = {}
    for noise, cfg in cfgs.items():
        want[noise] = capi.flow_act_host(cfg, params, cond_host, crashed, draw_index=count + (OFFSET if noise else 0))
        want[noise]["action"] = np.stack([want[noise]["throttle"], want[noise]["steer"]], axis=1)
    assert not same(want[0]["x"], want[1]["x"]) and np.abs(want[1]["x0"]).max() > 0
    assert same(want[1]["x0"], mirror.noise(13, (base + np.arange(N)) % 2 ** 32, count + OFFSET))

    def check(rec, noise, label):
        dev.sync()
        assert same(dev.get(capi.F_THROTTLE), want[noise]["throttle"]), label + ": throttle"
        assert same(dev.get(capi.F_STEER), want[noise]["steer"]), label + ": steer"
        for slot, t in rec.items():
            assert same(t.cpu().numpy(), want[noise][slot]), label + ": " + slot

    def fresh_rec():
        rec = {k: make(N) for k, make in REC.items()}
        torch.cuda.synchronize()  # the handle has a stream of its own
        return rec

    dev.flow_set_params(params)  # from a host pointer
    assert L.okenv_flow_act(h, None, None) == INVALID  # a NULL cond
    assert same(dev.flow_get_params(), params)
    for noise in (1, 0):
        dev.flow_create(cfgs[noise])  # (replaces the attachment: the parameters are forgotten)
        assert L.okenv_flow_act(h, capi.ptr(cond), None) == STATE
        dev.flow_set_params(params)
        dev.flow_set_draw_offset(word if noise else None)
        rec = fresh_rec()
        dev.flow_act(cond, rec)
        check(rec, noise, "noise %d" % noise)
        # every slot NULL in turn: the others are written, its buffer keeps the sentinel; no record at all
        for skip in REC:
            dev.set_actions(np.zeros(N, dtype=f32), np.zeros(N, dtype=f32))
            rec = fresh_rec()
            kept = rec[skip].clone()
            torch.cuda.synchronize()
            dev.flow_act(cond, dict(rec, **{skip: None}))
            check({k: v for k, v in rec.items() if k != skip}, noise, "noise %d without %s" % (noise, skip))
            assert torch.equal(rec[skip], kept)
        dev.set_actions(np.zeros(N, dtype=f32), np.zeros(N, dtype=f32))
        dev.flow_act(cond)
        check({}, noise, "noise %d, no record" % noise)
    # from a device pointer, other values first so that the hand-over shows (noise 0 is attached, no offset word)
    zeros, on_device = np.zeros_like(params), torch.from_numpy(params).cuda()  # (alive until the copies have run)
    dev.flow_set_params(zeros)
    dev.flow_set_params(on_device)
    rec = fresh_rec()
    dev.flow_act(cond, rec)
    check(rec, 0, "device pointer")
    got = torch.empty(params.size, device="cuda")
    dev.flow_get_params(got)
    assert same(got.cpu().numpy(), params)
    for noise in (0, 1):
        assert not np.isnan(want[noise]["action"]).any()
        assert np.all(want[noise]["action"] >= np.array(list(cfgs[noise].action_lo))) and np.all(want[noise]["action"] <= np.array(list(cfgs[noise].action_hi)))
    # (the comparison is one of bits, and x0 and the action fields are compared too; still, x must not be the clamp's constant throughout)
    assert float((np.abs(want[1]["x"]) == 1.0).mean()) < 0.75 or N < 15
    dev.close()


T = 16  # the kernel's agents per workgroup; asserted against the binding's constant below


@pytest.mark.parametrize("N", [1, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_act_device_equals_host(gpu, name, N):
    """Item 6: one agent, a tile short of one row, a full tile, a second workgroup with one agent, a third."""
    assert gpu.capi.FLOW_AGENTS == T
    act_case(gpu, name, N)


def test_act_device_equals_host_reference_shape(gpu):
    act_case(gpu, "reference", 2 * T + 1)


def test_act_device_equals_host_widest_shape(gpu):
    cfg = gpu.capi.flow_config(**WIDE)
    assert gpu.capi.flow_lds_bytes(cfg) <= gpu.capi.FLOW_LDS_BUDGET < gpu.capi.flow_lds_bytes(cfg) + 16 * (WIDE["hidden"] + 4) * 4
    act_case(gpu, "wide", T + 1)


@pytest.mark.parametrize("name", mirror.NEW_SHAPES)
def test_act_device_equals_host_room_limited_staging(gpu, name):
    """The widths at which the LDS's room decides the staged block of W2 (mirror.PATHS names it, act_case asserts it first): 48
    columns (three column tiles for four waves), 32 and 16 with many blocks an Euler step, a short last block behind them, the
    plans that end next to the budget.  A full workgroup plus one agent."""
    act_case(gpu, name, T + 1)


def test_act_device_equals_host_three_column_tiles_one_agent(gpu):
    act_case(gpu, "stage48", 1)


def test_draw_index(gpu):
    """Item 7: a step between two acts changes x0, none leaves it, the offset word changes it."""
    N = 2 * T + 1
    shape = mirror.SHAPES["tiny"]
    cfg = gpu.capi.flow_config(seed=3, **shape)
    rng = np.random.default_rng(1)
    params = mirror.random_params(gpu.capi, cfg, rng)
    cond = torch.from_numpy(rng.uniform(-1.0, 1.0, (N, shape["cond_dim"])).astype(f32)).cuda()
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan(RAYS))
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    dev.flow_create(cfg)
    dev.flow_set_params(params)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def x0_now():
        rec = {"x0": torch.empty((N, 2), device="cuda")}
        torch.cuda.synchronize()
        dev.flow_act(cond, rec)
        dev.sync()
        return rec["x0"].cpu().numpy()

    count = dev.step_count
    first, again = x0_now(), x0_now()
    assert same(first, again) and same(first, mirror.noise(3, np.arange(N), count))
    dev.step(1)
    stepped = x0_now()
    assert not same(first, stepped) and same(stepped, mirror.noise(3, np.arange(N), count + 1))
    dev.flow_set_draw_offset(word)
    assert same(x0_now(), stepped)
    word.fill_(9)
    torch.cuda.synchronize()
    moved = x0_now()
    assert not same(moved, stepped) and same(moved, mirror.noise(3, np.arange(N), count + 10))
    dev.flow_set_draw_offset(None)
    assert same(x0_now(), stepped)
    dev.close()


def test_graph_of_act_and_step_equals_eager(gpu):
    """Item 8: flow_act + step captured once (a linear graph) and replayed 8 times, against the same 8 iterations launched one by one on
    a second environment; the noise moves on from replay to replay."""
    from openkitchen_amd.torch_env import VectorEnvironment
    N = 2 * T + 1
    shape = mirror.SHAPES["small"]
    rng = np.random.default_rng(4)
    params = mirror.random_params(gpu.capi, gpu.capi.flow_config(**shape), rng)
    cond = torch.from_numpy(rng.uniform(-1.0, 1.0, (N, shape["cond_dim"])).astype(f32)).cuda()
    venvs = []
    for _ in range(2):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=True, seed=3, agent_base=50)
        venv.enable_flow_policy(dict(shape), params)
        assert (venv.flow_config.seed, venv.flow_config.agent_base) == (3, 50)
        venv.reset()
        venvs.append(venv)
    eager, graphed = venvs
    rec = {"x0": torch.zeros((N, 2), device="cuda")}
    torch.cuda.synchronize()

    def body():
        graphed.flow_act(cond, rec)
        graphed.step()

    graph = graphed.capture(body, warmup=0)
    seen = []
    for _ in range(8):
        eager.flow_act(cond)
        eager.step()
        graph.replay()
        seen.append(rec["x0"].clone())
    torch.cuda.synchronize()
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    assert float(eager.throttle.abs().max()) > 0
    for a, b in zip(seen, seen[1:]):
        assert not torch.equal(a, b)
    with pytest.raises(ValueError):
        eager.flow_act(cond[:, :-1])
    for venv in venvs:
        venv.close()
