"""The lidar transformer driver on the device (okenv_lidar_*; openkitchen_amd/csrc/ok_lidar.h): the matrix-core linear piece and the
act kernel bit-equal to the host entries that share their rule, at the edges of their launch geometry; NULL record slots; parameters
from host and device pointers; the order of calls; act + step captured in a graph."""
import ctypes as C

import numpy as np
import pytest
import torch

import _lidar_numpy as mirror

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, STATE = -1, -5
REC = {"action": lambda N, R: torch.full((N, 2), -7.0, device="cuda"), "input": lambda N, R: torch.full((N, R, 2), -7.0, device="cuda"),
       "alive": lambda N, R: torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
# Random-action steps on Austin after which the population holds crashed and alive agents alike, for 15 .. 33 agents and both ray fans
# (found with the CPU oracle: 8 calls of rollout_random(25, seed 11) behind reset_random(seed 5) leave 1 .. 3 agents crashed)
RANDOM_CHUNKS, RANDOM_CHUNK_STEPS = 8, 25
# ... and so they do at 17 agents with fans of 2, 5, 6 and 16 rays (1 or 2 crashed; a crash depends on the fan).  A single ray leaves
# nobody crashed behind the 8th call and one agent behind the 7th (the driver re-places crashed agents, so the count does not grow)
CHUNKS_BY_RAYS = {1: 7}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the linear piece -----------------------------------------------------------------------------------------------------------------

def linear_data(kind, M, K, N, rng):
    if kind == "uniform":
        x, w, b = (rng.uniform(-1.0, 1.0, s) for s in ((M, K), (N, K), (N,)))
    elif kind == "cancellation":  # magnitudes 2^-40 .. 2^40, mixed signs: the chain's order decides every bit
        x, w, b = (np.ldexp(rng.uniform(1.0, 2.0, s), rng.integers(-20, 21, s)) * rng.choice([-1.0, 1.0], s) for s in ((M, K), (N, K), (N,)))
    else:  # f32 subnormals among the inputs, the weights and the biases; products that land in the subnormal range
        x, w, b = (rng.uniform(-1.0, 1.0, s) for s in ((M, K), (N, K), (N,)))
        # every term of an even output lies far below 2^-126, so that up to 896 of them still sum to a subnormal; the odd outputs mix
        # such terms with ordinary ones
        x[:, ::3] *= 2.0 ** -140
        x[:, 2::3] *= 2.0 ** -70
        w[::2, 1::3] *= 2.0 ** -140
        w[::2, 2::3] *= 2.0 ** -72
        b[::2] *= 2.0 ** -137
    return x.astype(f32), w.astype(f32), b.astype(f32)


@pytest.mark.parametrize("kind", ["uniform", "cancellation", "subnormal"])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [16, 128, 896])
def test_linear_device_equals_host(gpu, kind, K, N):
    """Item 6: M = 1 .. 33 is one partly filled tile up to a third workgroup with one row."""
    for M in (1, 15, 16, 17, 33):
        rng = np.random.default_rng(1000 * K + 10 * N + M)
        x, w, b = linear_data(kind, M, K, N, rng)
        if kind == "subnormal":
            assert np.any((x != 0) & (np.abs(x) < 2.0 ** -126)) and np.any((w != 0) & (np.abs(w) < 2.0 ** -126))
        for relu in (False, True):
            host = gpu.capi.debug_lidar_linear(x, w, b, relu=relu)
            dev = gpu.capi.debug_lidar_linear(x, w, b, relu=relu, device=0)
            assert not np.isnan(host).any() and not np.isnan(dev).any()
            bad = int((host.view(np.uint32) != dev.view(np.uint32)).sum())
            assert bad == 0, "%s M %d K %d N %d relu %s: %d of %d outputs differ" % (kind, M, K, N, relu, bad, host.size)
        if kind == "subnormal":
            assert np.any((host != 0) & (np.abs(host) < 2.0 ** -126)), "no subnormal result: the case tests nothing"


# ---- acting ---------------------------------------------------------------------------------------------------------------------------

def fan(R):
    return np.linspace(-90.0, 90.0, R).astype(f32)


def driven_population(gpu, N, R):
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), N, ray_angles_deg=fan(R))
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    for i in range(CHUNKS_BY_RAYS.get(R, RANDOM_CHUNKS)):
        dev.rollout_random(RANDOM_CHUNK_STEPS, 11, 0, RANDOM_CHUNK_STEPS * i)
    return dev


def act_case(gpu, name, N):
    shape = mirror.SHAPES[name]
    R = shape["num_points"]
    cfg = gpu.capi.lidar_config(**shape)
    # the path of the kernel the shape was chosen for is the one its plan selects (tests/_lidar_numpy.py)
    plan = mirror.plan(shape)
    assert plan["bytes"] == gpu.capi.lidar_lds_bytes(cfg) <= gpu.capi.LIDAR_LDS_BUDGET
    assert (name in mirror.PATHS) == (name in mirror.NEW_SHAPES) and (name not in mirror.PATHS or mirror.PATHS[name](plan)), plan
    rng = np.random.default_rng(7 * N + R)
    params = mirror.random_params(gpu.capi, cfg, rng)
    dev = driven_population(gpu, N, R)
    L, h = dev._L, dev._h
    assert L.okenv_lidar_act(h, None) == STATE  # before create
    n = C.c_int32()
    assert L.okenv_lidar_num_params(h, C.byref(n)) == STATE and L.okenv_lidar_set_params(h, gpu.capi.ptr(params)) == STATE
    # what a live handle refuses: another point count than its rays, a shape outside the limits, one over the LDS budget
    for bad in (dict(num_points=R + 1), dict(d_model=24), dict(num_layers=9), dict(num_points=R, d_model=512, nhead=1, dim_feedforward=64)):
        assert L.okenv_lidar_create(h, C.byref(gpu.capi.lidar_config(**dict(shape, **bad)))) == INVALID, bad
    assert L.okenv_lidar_create(h, None) == INVALID and L.okenv_lidar_act(h, None) == STATE
    assert dev.lidar_create(cfg) == params.size
    assert L.okenv_lidar_act(h, None) == STATE  # before set_params
    assert L.okenv_lidar_get_params(h, gpu.capi.ptr(np.empty_like(params))) == STATE
    crashed = dev.get(gpu.capi.F_CRASHED)
    if N >= 15:
        assert 0 < int((crashed != 0).sum()) < N, "the population must hold crashed and alive agents"
    rel = np.stack([dev.get(gpu.capi.F_REL_X), dev.get(gpu.capi.F_REL_Y)], axis=2)
    want = gpu.capi.lidar_act_host(cfg, params, rel, crashed)
    want["action"] = np.stack([want["throttle"], want["steer"]], axis=1)
    if N >= 15:  # rays that all miss would feed every agent the same row, the ends of the range
        rows = want["input"].reshape(N, -1)
        assert len(np.unique(rows, axis=0)) > N // 2 and float((np.abs(rows) < 0.99).mean()) > 0.5

    def check(rec, label):
        dev.sync()
        assert same(dev.get(gpu.capi.F_THROTTLE), want["throttle"]), label + ": throttle"
        assert same(dev.get(gpu.capi.F_STEER), want["steer"]), label + ": steer"
        for slot, t in rec.items():
            assert same(t.cpu().numpy(), want[slot]), label + ": " + slot

    def fresh_rec():
        rec = {k: make(N, R) for k, make in REC.items()}
        torch.cuda.synchronize()  # the handle has a stream of its own
        return rec

    dev.lidar_set_params(params)  # from a host pointer
    rec = fresh_rec()
    dev.lidar_act(rec)
    check(rec, "host pointer")
    assert same(dev.lidar_get_params(), params)
    # every slot NULL in turn: the others are written, its buffer keeps the sentinel; no record at all
    for skip in REC:
        dev.set_actions(np.zeros(N, dtype=f32), np.zeros(N, dtype=f32))
        rec = fresh_rec()
        kept = rec[skip].clone()
        torch.cuda.synchronize()
        dev.lidar_act(dict(rec, **{skip: None}))
        check({k: v for k, v in rec.items() if k != skip}, "without " + skip)
        assert torch.equal(rec[skip], kept)
    dev.set_actions(np.zeros(N, dtype=f32), np.zeros(N, dtype=f32))
    dev.lidar_act()
    check({}, "no record")
    # from a device pointer, other values first so that the hand-over shows
    zeros, on_device = np.zeros_like(params), torch.from_numpy(params).cuda()  # (alive until the copies have run)
    dev.lidar_set_params(zeros)
    dev.lidar_set_params(on_device)
    rec = fresh_rec()
    dev.lidar_act(rec)
    check(rec, "device pointer")
    got = torch.empty(params.size, device="cuda")
    dev.lidar_get_params(got)
    assert same(got.cpu().numpy(), params)
    assert np.abs(want["action"]).max() < 1e3 and not np.isnan(want["action"]).any()
    dev.close()


@pytest.mark.parametrize("N", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_act_device_equals_host(gpu, name, N):
    """Item 7: one agent, a tile short of one row, a full tile, a second workgroup with one agent, a third."""
    act_case(gpu, name, N)


def test_act_device_equals_host_reference_shape(gpu):
    act_case(gpu, "reference", 33)


@pytest.mark.parametrize("N", [1, 17])
@pytest.mark.parametrize("name", mirror.NEW_SHAPES)
def test_act_device_equals_host_on_every_path(gpu, name, N):
    """The shapes that select what the three above never do (mirror.PATHS names it, act_case asserts it first): head groups of two
    and three column tiles, a head that starts inside a tile, heads of one column and seven attention tasks a thread, an even point
    count, one point and sixteen, every okLidarUnit<1 .. 4> as the tail of a row block, a short column block behind full ones in
    out_proj and in the feed-forward, LDS regions sized by the head.  One agent, and a full workgroup plus one."""
    act_case(gpu, name, N)


def test_graph_of_act_and_step_equals_eager(gpu):
    """Item 8: lidar_act + step captured once (a linear graph) and replayed 8 times, against the same 8 iterations launched one by
    one on a second environment."""
    from openkitchen_amd.torch_env import VectorEnvironment
    shape = mirror.SHAPES["small"]
    cfg = gpu.capi.lidar_config(**shape)
    params = mirror.random_params(gpu.capi, cfg, np.random.default_rng(4))
    venvs = []
    for _ in range(2):
        venv = VectorEnvironment(gpu.track_path("Austin"), 33, num_rays=7, ray_angles_deg=fan(7), auto_reset=True, seed=3, agent_base=50)
        venv.enable_lidar_policy(cfg, params)
        venv.reset()
        venvs.append(venv)
    eager, graphed = venvs

    def body():
        graphed.lidar_act()
        graphed.step()

    graph = graphed.capture(body, warmup=0)
    for _ in range(8):
        eager.lidar_act()
        eager.step()
        graph.replay()
    torch.cuda.synchronize()
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    assert float(eager.throttle.abs().max()) > 0
    for venv in venvs:
        venv.close()
