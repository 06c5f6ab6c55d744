"""The memory's training on the device: okenv_memory_update and okenv_memory_eval against the host entries bit
for bit at every shape and geometry (every output and the state), with no agent field and no hidden state moved; the act after an
update against the host act with the updated vector; the order of calls and the drops; one captured update replayed."""
import functools

import numpy as np
import pytest
import torch

import _memtrain_numpy as N_
from test_gpu_bev_encoder import driven_population, last_error, same
from test_gpu_memory import FIELDS, act_both, assert_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, STATE = -1, -5
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, clip_grad=1.0)
AGENTS, SIDE = 3, 16
CASES = [(s, g) for s in N_.MIRRORED for g in N_.GEOMETRIES] + [(N_.WIDE, N_.WIDE_GEOMETRY)]


@pytest.fixture(scope="module")
def venv(gpu):
    return driven_population(gpu, AGENTS, SIDE)


def configs(capi, shape):
    Z, H, L = N_.SHAPES[shape]
    return capi.world_config(**N_.world_members(Z)), capi.memory_config(hidden=H, layers=L, ctrl_hidden=2)


def fresh_state(shape, seed=0):
    Z, H, L = N_.SHAPES[shape]
    T = N_.trainable(Z, H, L)
    return dict(params=N_.draw_network(Z, H, L, seed), m=np.zeros(T, f32), v=np.zeros(T, f32), t=0)


def attach(capi, dev, shape, geometry, net, **over):
    """The racers, a memory of the shape with the network set, and the learner for the geometry's windows."""
    M, B, S, epochs, stride = N_.GEOMETRIES[geometry]
    wc, mc = configs(capi, shape)
    dev.world_create(wc)
    dev.memory_create(mc)
    dev.memory_set_params("network", net)
    dev.memory_learner_create(seq_len=S, max_batch=min(B, M), **dict(HP, **over))
    return wc, mc


@functools.lru_cache(maxsize=None)
def host_case(shape, geometry):
    """The host entry's update and the eval behind it, computed once: (data, new state, outputs, eval losses)."""
    import openkitchen_amd as ok
    capi = ok.capi
    M, B, S, epochs, stride = N_.GEOMETRIES[geometry]
    data = N_.draw_data(N_.SHAPES[shape][0], geometry, 0)
    wc, mc = configs(capi, shape)
    learner = capi.memory_learner_config(seq_len=S, max_batch=min(B, M), **HP)
    new, out = capi.memory_update_host(wc, mc, learner, fresh_state(shape), data[0], data[1], data[2], B, stride, epochs, data[3])
    return data, new, out, capi.memory_eval_host(wc, mc, learner, new["params"], data[0], data[1], data[2], B, stride)


def device_data(data):
    latent, action, start, order = data
    return (torch.from_numpy(latent).cuda(), torch.from_numpy(action).cuda(), torch.from_numpy(start).cuda(),
            None if order is None else torch.from_numpy(order).cuda())


def device_update(dev, shape, geometry, data, epochs=None, order="given"):
    M, B, S, eg, stride = N_.GEOMETRIES[geometry]
    epochs = eg if epochs is None else epochs
    latent, action, start, drawn = data
    steps = epochs * -(-M // B)
    out = dict(loss=torch.full((steps,), -7.0, device="cuda"), norm=torch.full((steps,), -7.0, device="cuda"),
               grad=torch.full((N_.trainable(*N_.SHAPES[shape]),), -7.0, device="cuda"))
    dev.memory_update(latent, action, latent.shape[0], start, M, B, stride, epochs, drawn if isinstance(order, str) else order, None, out)
    return out


def snapshot(venv):
    torch.cuda.synchronize()
    return dict({k: getattr(venv, k).cpu().numpy().copy() for k in FIELDS}, hidden=venv.env.memory_get_hidden())


@pytest.mark.parametrize("shape,geometry", CASES, ids=["%s-%s" % c for c in CASES])
def test_update_and_eval_equal_the_host_entries(gpu, venv, shape, geometry):
    capi, dev = gpu.capi, venv.env
    Z, H, L = N_.SHAPES[shape]
    M, B, S, epochs, stride = N_.GEOMETRIES[geometry]
    data, want, wout, weval = host_case(shape, geometry)
    st = fresh_state(shape)
    wc, mc = attach(capi, dev, shape, geometry, st["params"])
    assert capi.memory_learner_workspace_bytes(wc, mc, dev.memory_learner_config) == 4 * N_.workspace_words(Z, H, L, S, min(B, M))
    dev.memory_set_hidden(np.random.default_rng(1).uniform(-0.5, 0.5, (AGENTS, L, H)).astype(f32))
    before = snapshot(venv)
    on_device = device_data(data)
    out = device_update(dev, shape, geometry, on_device)
    loss = torch.full((-(-M // B),), -7.0, device="cuda")
    dev.memory_eval(on_device[0], on_device[1], on_device[0].shape[0], on_device[2], M, B, loss, stride)
    got = dev.memory_learner_state()
    for k in ("loss", "norm", "grad"):
        assert same(out[k].cpu().numpy(), wout[k]), "%s: by up to %.3g" % (k, float(np.abs(out[k].cpu().numpy() - wout[k]).max()))
    assert got["t"] == want["t"] == epochs * -(-M // B)
    for k in ("params", "m", "v"):
        assert same(got[k], want[k]), "%s: %d of %d differ" % (k, int((got[k] != want[k]).sum()), got[k].size)
    assert same(loss.cpu().numpy(), weval), "eval"
    T = N_.trainable(Z, H, L)
    vector = dev.memory_get_params("network")
    assert same(vector, want["params"]) and same(vector[T:], st["params"][T:]), "okenv_memory_get_params: the updated vector, the statistics untouched"
    after = snapshot(venv)
    for k, v in before.items():
        assert same(after[k], v), "%s moved during the update" % k


def test_the_act_after_an_update_acts_with_the_new_network(gpu, venv):
    """okenv_memory_act's record equals okenv_memory_act_host with the updated vector: the act's packed matrices follow the step."""
    import _world_numpy as wmirror
    capi, dev = gpu.capi, venv.env
    shape, geometry = "48-48-2", "short_last_minibatch"
    Z, H, L = N_.SHAPES[shape]
    data, want, _, _ = host_case(shape, geometry)
    wc, mc = attach(capi, dev, shape, geometry, fresh_state(shape)["params"])
    enc = wmirror.draw_params(N_.world_members(Z), 5, 1)[0]
    ctrl = np.random.default_rng(6).uniform(-0.2, 0.2, (AGENTS, dev.memory_num_params()[1])).astype(f32)
    dev.world_set_params("encoder", enc)
    dev.memory_set_params("controllers", ctrl)
    device_update(dev, shape, geometry, device_data(data))
    torch.manual_seed(2)
    frames = torch.randint(0, 256, (AGENTS, SIDE, SIDE, 4), dtype=torch.uint8, device="cuda")
    for t in range(2):
        got, host = act_both(capi, dev, wc, mc, enc, want["params"], ctrl, frames)
        assert_equal(got, host, "act %d after the update" % t)


def test_order_of_calls_and_drops(gpu, venv):
    capi, dev = gpu.capi, venv.env
    shape, geometry = "16-16-1", "two_steps"
    wc, mc = configs(capi, shape)
    learner = capi.memory_learner_config(seq_len=2, max_batch=3, **HP)
    data = device_data(N_.draw_data(16, geometry, 0))
    net = fresh_state(shape)["params"]
    L_ = dev._L

    def create():
        return L_.okenv_memory_learner_create(dev._h, learner)

    def update():
        return L_.okenv_memory_update(dev._h, capi.ptr(data[0]), capi.ptr(data[1]), data[0].shape[0], capi.ptr(data[2]), 3, 1, 3, 1, None, None, None)

    dev.world_create(wc)
    assert create() == STATE and b"okenv_memory_create" in last_error(dev), "learner before memory"
    dev.memory_create(mc)
    assert create() == STATE, "learner before the network's parameters"
    assert update() == STATE
    dev.memory_set_params("network", net)
    assert create() == 0 and update() == 0
    assert L_.okenv_memory_learner_create(dev._h, capi.memory_learner_config(seq_len=17, max_batch=3, **HP)) == INVALID
    assert update() == 0, "a refused create leaves the learner as it was"
    assert L_.okenv_memory_update(dev._h, capi.ptr(data[0]), capi.ptr(data[1]), data[0].shape[0], capi.ptr(data[2]), 3, 1, 0, 1, None, None, None) == INVALID
    assert L_.okenv_memory_update(dev._h, None, capi.ptr(data[1]), data[0].shape[0], capi.ptr(data[2]), 3, 1, 3, 1, None, None, None) == INVALID
    dev.memory_learner_reset()
    assert dev.memory_learner_state()["t"] == 0 and not dev.memory_learner_state()["m"].any()
    dev.memory_create(mc)  # a second memory drops the learner
    dev.memory_set_params("network", net)
    assert update() == STATE and L_.okenv_memory_learner_reset(dev._h) == STATE
    assert create() == 0 and update() == 0
    dev.world_create(wc)  # ... and so do new racers
    assert update() == STATE and create() == STATE
    torch.cuda.synchronize()


def test_a_captured_update_replayed_twice_equals_three_eager_calls(gpu, venv):
    """The step number lives on the device: a replay takes the steps that follow the capture's."""
    capi, dev = gpu.capi, venv.env
    shape, geometry = "48-48-2", "short_last_minibatch"
    data = device_data(N_.draw_data(48, geometry, 0))
    net = fresh_state(shape)["params"]
    attach(capi, dev, shape, geometry, net)
    eager = [device_update(dev, shape, geometry, data) for _ in range(3)]
    torch.cuda.synchronize()
    want = dev.memory_learner_state()
    assert want["t"] == 9
    dev.memory_set_params("network", net)
    dev.memory_learner_reset()
    side = torch.cuda.Stream(device=venv.device)
    side.wait_stream(torch.cuda.current_stream(venv.device))
    try:
        with torch.cuda.stream(side):
            venv.use_stream(side)
            first = device_update(dev, shape, geometry, data)
        side.synchronize()
        first = {k: v.clone() for k, v in first.items()}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = device_update(dev, shape, geometry, data)
        outs = [first]
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            outs.append({k: v.clone() for k, v in out.items()})
    finally:
        venv.use_stream(torch.cuda.current_stream(venv.device))
    got = dev.memory_learner_state()
    assert got["t"] == 9
    for k in ("params", "m", "v"):
        assert same(got[k], want[k]), k
    for call in range(3):
        for k in ("loss", "norm", "grad"):
            assert same(outs[call][k].cpu().numpy(), eager[call][k].cpu().numpy()), (call, k)
