"""The Deep-Q image racers on the device (okenv_qcnn_*; openkitchen_amd/csrc/ok_qcnn.h): the act's two kernels bit-equal to the host
entry that shares their rule, on every path the plan has (okenv_qcnn_plan), with frames of random bytes and frames the camera rendered,
crashed agents among them, greedy and epsilon-greedy; parameters from host and device pointers; the order of calls; the frame ring's
push and batch bit-equal to their host entries; step + camera + act + push captured in a graph; the Q-values against PyTorch."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _qcnn_numpy as mirror
from test_gpu_bev_encoder import INVALID, RAYS, STATE, driven_population, fan, last_error, same

pytestmark = pytest.mark.gpu
f32 = np.float32
# |device Q-values - fp32 PyTorch on the GPU| with the same weights (mirror.draw_params, seed 3) and frames (the camera's and random bytes
# alternating), 33 agents: torch sums its convolutions and its linear layers in its library's order.  The largest differences measured
# on the MI355X on the first run were 1.937e-7 at the reference shape (dqn_cnn.QCNN itself; |q| up to 0.160) and 7.823e-8 at tiny (|q|
# up to 0.098); the bound is 4 x that.  (examples/dqn_cnn_racer.py's first step at 48 x 48 frames, torch's default init, is held to the
# reference shape's bound in tests/test_gpu_dqn_cnn_example.py: 4.47e-8 was measured there, with and without graph chunks.)
TORCH_MEASURED = {"reference": 1.937e-7, "tiny": 7.823e-8}
TORCH_TOL = {k: 4 * v for k, v in TORCH_MEASURED.items()}
SENTINEL = -7.0
MODES = (("greedy", 0.0), ("eps_greedy", 0.5), ("eps_greedy", 1.0))
MEMBERS = ("q", "action", "value", "alive")


def config(capi, name, mode="greedy", epsilon=0.0, **more):
    return capi.qcnn_config(mode=mode, epsilon=epsilon, seed=77, agent_base=1000, **dict(mirror.SHAPES[name], **more))


def record(N, A):
    return {"q": torch.empty((N, A), device="cuda"), "action": torch.empty(N, dtype=torch.int64, device="cuda"),
            "value": torch.empty(N, device="cuda"), "alive": torch.empty(N, dtype=torch.uint8, device="cuda")}


def act_case(gpu, name, N, refusals=True):
    capi = gpu.capi
    shape = mirror.SHAPES[name]
    S, A = shape["image_size"], shape["num_actions"]
    cfg = config(capi, name)
    # the path the shape was chosen for is the one its plan selects
    assert capi.qcnn_plan(cfg) == mirror.PATHS[name] and capi.qcnn_lds_bytes(cfg) == mirror.lds_bytes(shape) <= capi.QCNN_LDS_BUDGET
    params = mirror.draw_params(shape, N)
    venv = driven_population(gpu, N, S)
    dev, L, h = venv.env, venv.env._L, venv.env._h
    crashed = dev.get(capi.F_CRASHED)
    if N >= 15:
        assert 0 < int((crashed != 0).sum()) < N, "the population must hold crashed and alive agents"
    rendered = venv.camera()
    torch.manual_seed(N)
    frames = {"camera": rendered, "random": torch.randint(0, 256, (N, S, S, 4), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    assert int(rendered[..., :3].max()) > int(rendered[..., :3].min()), "the camera drew nothing"
    draw = dev.step_count
    assert draw > 0
    host = {k: t.cpu().numpy() for k, t in frames.items()}
    with ThreadPoolExecutor(6) as pool:  # (the host entry is one scalar chain per output: the six runs side by side)
        jobs = {(kind, mode): pool.submit(capi.qcnn_act_host, config(capi, name, *mode), params, host[kind], crashed, draw) for kind in frames for mode in MODES}
        want = {k: j.result() for k, j in jobs.items()}
    greedy = want["camera", MODES[0]]
    assert not same(greedy["q"], want["random", MODES[0]]["q"])
    assert all(np.isfinite(w["q"]).all() and np.abs(w["q"]).max() > 0 and np.array_equal(w["alive"], crashed == 0) for w in want.values())
    if N >= 15:
        half, full = want["camera", MODES[1]], want["camera", MODES[2]]
        assert 0 < int((half["action"] != greedy["action"]).sum()) and int((half["action"] != full["action"]).sum()) > 0
    rec = record(N, A)
    nbytes = N * S * S * 4

    def fill():
        rec["q"].fill_(SENTINEL), rec["value"].fill_(SENTINEL), rec["action"].fill_(-7), rec["alive"].fill_(9)
        venv.throttle.fill_(SENTINEL), venv.steering.fill_(SENTINEL)

    def untouched():
        torch.cuda.synchronize()
        return (all(float(t.min()) == float(t.max()) == SENTINEL for t in (rec["q"], rec["value"], venv.throttle, venv.steering))
                and int(rec["alive"].min()) == int(rec["alive"].max()) == 9 and int(rec["action"].min()) == int(rec["action"].max()) == -7)

    struct = capi.fill_pointers(capi.OkenvQcnnRecord(), rec, "record")
    fill()
    if refusals:  # the order of calls
        assert L.okenv_qcnn_act(h, capi.ptr(rendered), nbytes, C.byref(struct)) == STATE and b"okenv_qcnn_act: call okenv_qcnn_create first" in last_error(dev)
        assert L.okenv_qcnn_act(None, capi.ptr(rendered), nbytes, C.byref(struct)) == INVALID
        n = C.c_int32()
        assert L.okenv_qcnn_num_params(h, C.byref(n)) == STATE and L.okenv_qcnn_set_params(h, capi.ptr(params)) == STATE
        assert L.okenv_qcnn_num_params(h, None) == INVALID and L.okenv_qcnn_set_params(h, None) == INVALID
        assert L.okenv_qcnn_num_params(None, C.byref(n)) == INVALID and L.okenv_qcnn_get_params(None, capi.ptr(params)) == INVALID
        assert L.okenv_qcnn_set_epsilon(h, 0.5) == STATE and L.okenv_qcnn_set_draw_offset(h, None) == STATE
        assert L.okenv_qcnn_ring_create(h, 8, 0) == STATE and b"okenv_qcnn_ring_create: call okenv_qcnn_create first" in last_error(dev)
        for entry in (L.okenv_qcnn_ring_reset(h), L.okenv_qcnn_ring_size(h, None, None), L.okenv_qcnn_push(h, C.byref(struct), capi.ptr(rendered), capi.ptr(rendered), nbytes, None),
                      L.okenv_qcnn_batch(h, 4, 0, 0, C.byref(capi.OkenvQcnnBatchOut())), L.okenv_qcnn_ring_get(h, C.byref(capi.OkenvQcnnRing()))):
            assert entry == STATE and b"call okenv_qcnn_ring_create first" in last_error(dev)
        for bad in (dict(image_size=12), dict(image_size=136), dict(kernel=(9, 3, 2)), dict(stride=(5, 1, 1)), dict(padding=(4, 1, 1)),
                    dict(channels=(16, 8, 16)), dict(hidden=520), dict(num_actions=9)):
            assert L.okenv_qcnn_create(h, C.byref(config(capi, name, **bad))) == INVALID, bad
            assert b"okenv_qcnn_create: shape outside the limits" in last_error(dev)
        assert L.okenv_qcnn_create(h, C.byref(config(capi, name, "eps_greedy", 1.5))) == INVALID and b"okenv_qcnn_create: epsilon outside [0, 1]" in last_error(dev)
        assert L.okenv_qcnn_create(h, C.byref(config(capi, name, "sample"))) == INVALID and b"unknown mode" in last_error(dev)
        assert L.okenv_qcnn_create(h, C.byref(config(capi, name, action_table=((float("nan"), 0.0),)))) == INVALID and b"action table" in last_error(dev)
        assert L.okenv_qcnn_create(h, None) == INVALID and L.okenv_qcnn_create(None, C.byref(cfg)) == INVALID
        assert L.okenv_qcnn_act(h, capi.ptr(rendered), nbytes, C.byref(struct)) == STATE
    assert dev.qcnn_create(cfg) == params.size == mirror.num_params(shape)
    if refusals:
        assert L.okenv_qcnn_act(h, capi.ptr(rendered), nbytes, C.byref(struct)) == STATE
        assert b"okenv_qcnn_act: call okenv_qcnn_set_params first (the network needs its parameters)" in last_error(dev)
        assert L.okenv_qcnn_get_params(h, capi.ptr(np.empty_like(params))) == STATE
    dev.qcnn_set_params(params)  # from a host pointer
    assert same(dev.qcnn_get_params(), params)
    if refusals:
        for args in ((None, nbytes), (capi.ptr(rendered), nbytes - 4), (capi.ptr(rendered), nbytes + S * S * 4), (capi.ptr(rendered), 0),
                     (C.c_void_p(rendered.data_ptr() + 4), nbytes)):
            if args[0] is not None and args[0].value != rendered.data_ptr() and S * S % 4:
                continue  # (a 4-byte aligned pointer is what such a shape takes)
            assert L.okenv_qcnn_act(h, *args, C.byref(struct)) == INVALID, args
            assert b"okenv_qcnn_act: " in last_error(dev)
        assert L.okenv_qcnn_get_params(h, None) == INVALID and L.okenv_qcnn_set_epsilon(h, -0.5) == INVALID
        assert untouched()  # nothing was launched by a refused call

    def check(label, mode, members=MEMBERS):
        dev.qcnn_create(config(capi, name, *mode)) if label == "create" else dev.qcnn_set_epsilon(mode[1])
        if label == "create":
            dev.qcnn_set_params(params)
        for kind, t in frames.items():
            fill()
            dev.qcnn_act(t, {k: rec[k] for k in members} if members is not None else None)
            torch.cuda.synchronize()
            w = want[kind, mode]
            got = {k: rec[k].cpu().numpy() for k in MEMBERS}
            got.update(throttle=venv.throttle.cpu().numpy(), steer=venv.steering.cpu().numpy())
            for k in ("throttle", "steer"):
                assert same(got[k], w[k]), "%s %s, %s frames, %s: %d of %d differ" % (label, mode, kind, k, int((got[k] != w[k]).sum()), N)
            for k in MEMBERS:
                if k in (members or ()):
                    assert same(got[k], w[k]), "%s %s, %s frames, %s: %d of %d differ, by up to %.3g" % (
                        label, mode, kind, k, int((got[k] != w[k]).sum()), got[k].size, float(np.abs(got[k].astype(np.float64) - w[k]).max()))
                else:
                    assert float(got[k].min()) == float(got[k].max()) in (SENTINEL, 9.0), (label, kind, k)

    for mode in MODES:
        check("create", mode)
    check("set_epsilon", MODES[1])  # (the mode is still eps_greedy)
    check("no record", MODES[1], None)
    for member in MEMBERS:  # a record with single NULL members
        check("record without " + member, MODES[1], tuple(k for k in MEMBERS if k != member))
    # a second create, with another shape and back, forgets the parameters
    other = "tiny" if name != "tiny" else "nopad"
    dev.qcnn_create(config(capi, other))
    assert L.okenv_qcnn_act(h, capi.ptr(rendered), nbytes, None) == STATE  # (the state is looked at before the frames)
    dev.qcnn_create(config(capi, name, *MODES[1]))
    assert L.okenv_qcnn_act(h, capi.ptr(rendered), nbytes, None) == STATE
    # from a device pointer, other values first so that the hand-over shows
    zeros, on_device = np.zeros_like(params), torch.from_numpy(params).cuda()  # (alive until the copies have run)
    dev.qcnn_set_params(zeros)
    dev.qcnn_set_params(on_device)
    check("device pointer", MODES[1])
    got = torch.empty(params.size, device="cuda")
    dev.qcnn_get_params(got)
    assert same(got.cpu().numpy(), params)
    # the binding's hand-over and its own checks
    venv.enable_image_dqn(config(capi, name, *MODES[2]), params)
    with pytest.raises(ValueError):
        venv.image_dqn_act(rendered[:, :-1])
    with pytest.raises(ValueError):
        venv.image_dqn_act(rendered.to(torch.float32))
    fill()
    venv.image_dqn_act(frames["random"], {"action": rec["action"]})
    torch.cuda.synchronize()
    assert same(rec["action"].cpu().numpy(), want["random", MODES[2]]["action"]) and same(venv.steering.cpu().numpy(), want["random", MODES[2]]["steer"])
    venv.close()


@pytest.mark.parametrize("name", ["tiny", "nopad", "odd", "wide", "deep_pad", "two_tiles", "three_tiles"])
def test_act_device_equals_host(gpu, name):
    """33 agents: two full tiles of 16 agents and a partial one, crashed agents among them."""
    act_case(gpu, name, 33)


def test_act_device_equals_host_reference_shape(gpu):
    act_case(gpu, "reference", 33, refusals=False)


@pytest.mark.parametrize("N", [1, 16, 17])
def test_act_device_equals_host_small_populations(gpu, N):
    act_case(gpu, "tiny", N, refusals=False)


def ring_case(gpu, name, capacity, push_all, with_reward):
    """Pushes after real steps with the act's record, then batches in both modes: every ring field and every batch bit-equal to the
    host entries."""
    capi = gpu.capi
    shape = mirror.SHAPES[name]
    S, A, N = shape["image_size"], shape["num_actions"], 33
    venv = driven_population(gpu, N, S)
    dev, L, h = venv.env, venv.env._L, venv.env._h
    cfg = config(capi, name, "eps_greedy", 0.5)
    venv.enable_image_dqn(cfg, mirror.draw_params(shape, 2), capacity=capacity, push_all=push_all)
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    host_ring = capi.qcnn_ring(capacity, S)
    rec = record(N, A)
    bufs = [venv.camera(), torch.empty((N, S, S, 4), dtype=torch.uint8, device="cuda")]
    reward = torch.empty(N, device="cuda")
    out = venv.image_dqn_batch(5, "sequential", 3)
    torch.cuda.synchronize()
    assert dev.qcnn_ring_size() == (0, 0) and not any(bool(t.any()) for t in out.values())  # the empty ring: zeros, index 0
    nbytes = N * S * S * 4
    struct = capi.fill_pointers(capi.OkenvQcnnRecord(), rec, "record")
    for args in ((None, capi.ptr(bufs[0]), capi.ptr(bufs[1]), nbytes, None), (C.byref(capi.OkenvQcnnRecord()), capi.ptr(bufs[0]), capi.ptr(bufs[1]), nbytes, None),
                 (C.byref(struct), None, capi.ptr(bufs[1]), nbytes, None), (C.byref(struct), capi.ptr(bufs[0]), None, nbytes, None),
                 (C.byref(struct), capi.ptr(bufs[0]), capi.ptr(bufs[1]), nbytes - 4, None)):
        assert L.okenv_qcnn_push(h, *args) == INVALID and b"okenv_qcnn_push: " in last_error(dev)
    for args in ((0, 0, 0, C.byref(capi.OkenvQcnnBatchOut())), (4, 2, 0, C.byref(capi.OkenvQcnnBatchOut())), (4, 0, -1, C.byref(capi.OkenvQcnnBatchOut())), (4, 0, 0, None)):
        assert L.okenv_qcnn_batch(h, *args) == INVALID and b"okenv_qcnn_batch: " in last_error(dev)
    assert L.okenv_qcnn_ring_create(h, 0, 0) == INVALID and L.okenv_qcnn_ring_create(h, 8, 2) == INVALID
    assert dev.qcnn_ring_size() == (0, 0)
    for t in range(4):
        cur, nxt = bufs[t % 2], bufs[(t + 1) % 2]
        venv.image_dqn_act(cur, rec)
        dev.step(1 if t else 40)  # (some agents crash on the way)
        venv.camera(out=nxt)
        reward.copy_(torch.arange(N, device="cuda") * 0.5 - t)
        venv.image_dqn_push(rec, cur, nxt, reward if with_reward else None)
        torch.cuda.synchronize()
        crashed, alive = dev.get(capi.F_CRASHED), rec["alive"].cpu().numpy()
        capi.qcnn_push_host(host_ring, rec["action"].cpu().numpy(), None if push_all else alive, cur.cpu().numpy(), nxt.cpu().numpy(), crashed,
                            reward.cpu().numpy() if with_reward else None, dev.get(capi.F_DIST).reshape(N, RAYS), push_all)
        got = dev.qcnn_ring_get()
        assert dev.qcnn_ring_size() == (min(host_ring["pushed"], capacity), host_ring["pushed"])
        for k, v in got.items():
            assert same(v, host_ring[k]), "push %d, %s: %d slots differ" % (t, k, int((v != host_ring[k]).reshape(capacity, -1).any(1).sum()))
        size = min(host_ring["pushed"], capacity)
        for B, mode, start in ((1, "sequential", 0), (32, "sequential", 7), (50, "sequential", 123456), (50, "uniform", t), (1, "uniform", 9)):
            out = venv.image_dqn_batch(B, mode, start)
            torch.cuda.synchronize()
            want = capi.qcnn_batch_host(host_ring, B, mode, start, seed=cfg.seed)
            for k, v in want.items():
                assert same(out[k].cpu().numpy(), v), (t, B, mode, start, k)
            assert size == 0 or int(out["index"].max()) < size
    assert host_ring["pushed"] > capacity and (push_all or host_ring["pushed"] < 4 * N)  # it wrapped; crashed agents were left out
    on_device = {k: torch.empty_like(torch.from_numpy(v), device="cuda") for k, v in got.items()}
    dev.qcnn_ring_get(on_device)
    assert all(same(on_device[k].cpu().numpy(), host_ring[k]) for k in got)
    dev.qcnn_ring_reset()
    assert dev.qcnn_ring_size() == (0, 0)
    # a network of another image_size drops the ring
    dev.qcnn_create(config(capi, "odd" if S != 37 else "tiny"))
    assert L.okenv_qcnn_ring_reset(h) == STATE
    venv.close()


@pytest.mark.parametrize("name, capacity, push_all, with_reward", [("tiny", 40, False, False), ("tiny", 8, False, True), ("odd", 40, True, False),
                                                                    ("odd", 8, False, False)])
def test_push_and_batch_device_equal_host(gpu, name, capacity, push_all, with_reward):
    """C = 40 (wraps on the second push) and C = 8 < n (only the last 8 of a push survive); tiny moves its planes as 16-byte vectors,
    odd (37 x 37) float by float."""
    ring_case(gpu, name, capacity, push_all, with_reward)


def test_graph_of_step_camera_act_push_equals_eager(gpu):
    """step + camera + act + push captured once (a linear graph on the handle's stream) on the tiny shape at 64 agents with auto-reset
    on and replayed 3 times, against the same iterations launched one by one on a second environment: the ring, the record, the
    frames and every field, bit for bit; the draws move on from replay to replay."""
    from openkitchen_amd.torch_env import VectorEnvironment
    N, shape = 64, mirror.SHAPES["tiny"]
    S, A = shape["image_size"], shape["num_actions"]
    cfg, params = config(gpu.capi, "tiny", "eps_greedy", 0.5), mirror.draw_params(shape, 9)
    venvs, recs, bufs = [], [], []
    for _ in range(2):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=True, seed=3, agent_base=50,
                                 randomize_lane=True, randomize_heading=True)
        venv.enable_camera(width=S, height=S, fmt="rgba")
        venv.enable_image_dqn(cfg, params, capacity=150)
        venv.reset()
        venvs.append(venv)
        recs.append(record(N, A))
        bufs.append([venv.camera(), torch.zeros((N, S, S, 4), dtype=torch.uint8, device="cuda")])
    eager, graphed = venvs
    torch.cuda.synchronize()

    def iteration(i):
        cur, nxt = bufs[i]
        venvs[i].image_dqn_act(cur, recs[i])
        venvs[i].step()
        venvs[i].camera(out=nxt)
        venvs[i].image_dqn_push(recs[i], cur, nxt)
        venvs[i].image_dqn_act(nxt, recs[i])  # (the next step's act, on the frame the push has just stored)
        venvs[i].step()
        venvs[i].camera(out=cur)
        venvs[i].image_dqn_push(recs[i], nxt, cur)

    graph = graphed.capture(lambda: iteration(1), warmup=0)
    seen = []
    for _ in range(3):
        iteration(0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(bufs[0], bufs[1])) and all(torch.equal(recs[0][k], recs[1][k]) for k in recs[0])
        assert torch.equal(eager.throttle, graphed.throttle) and torch.equal(eager.steering, graphed.steering)
        seen.append(recs[1]["action"].clone())
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    rings = [v.env.qcnn_ring_get() for v in venvs]
    assert eager.env.qcnn_ring_size() == graphed.env.qcnn_ring_size() and eager.env.qcnn_ring_size()[1] > 150
    assert all(same(rings[0][k], rings[1][k]) for k in rings[0]) and float(np.abs(rings[0]["state"]).max()) > 0
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])  # other draws, other frames
    for venv in venvs:
        venv.close()


def torch_q(shape, params, planes):
    """The network in fp32 PyTorch on the GPU: planes [N, S, S] -> q [N, A]."""
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mirror.split(shape, params).items()}
    x = planes[:, None]
    for l in range(3):
        x = torch.relu(torch.nn.functional.conv2d(x, p["conv%d.weight" % (l + 1)], p["conv%d.bias" % (l + 1)], stride=shape["stride"][l], padding=shape["padding"][l]))
    x = torch.relu(torch.nn.functional.linear(x.flatten(1), p["fc1.weight"], p["fc1.bias"]))
    return torch.nn.functional.linear(x, p["fc2.weight"], p["fc2.bias"])


@pytest.mark.parametrize("name", ["reference", "tiny"])
def test_q_values_against_pytorch(gpu, name):
    """33 agents: fp32 PyTorch on the GPU with the same weights and frames -- the reference shape through dqn_cnn.QCNN itself.  See
    TORCH_MEASURED."""
    from openkitchen_amd import dqn_cnn
    shape = mirror.SHAPES[name]
    N, S, A = 33, shape["image_size"], shape["num_actions"]
    params = mirror.draw_params(shape, 3)
    venv = driven_population(gpu, N, S)
    venv.enable_image_dqn(config(gpu.capi, name), params)
    frames = venv.camera()
    torch.manual_seed(2)
    frames[1::2] = torch.randint(0, 256, (N // 2, S, S, 4), dtype=torch.uint8, device="cuda")
    got = torch.empty((N, A), device="cuda")
    venv.image_dqn_act(frames, {"q": got})
    with torch.no_grad():
        if name == "reference":
            model = dqn_cnn.QCNN(S).cuda()
            model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in mirror.split(shape, params).items()})
            assert torch.equal(dqn_cnn.qcnn_params_from_state_dict(model.state_dict(), image_size=S).cpu(), torch.from_numpy(params))
            want = model(dqn_cnn.gray(frames))
        else:
            want = torch_q(shape, params, dqn_cnn.gray(frames))
    torch.cuda.synchronize()
    diff = float((got - want).abs().max())
    print("device vs fp32 PyTorch Q-values, %s: %.3e (largest |q| %.3f)" % (name, diff, float(want.abs().max())))
    assert float(want.abs().max()) > 0.01
    assert diff <= TORCH_TOL[name]
    venv.close()


@pytest.mark.parametrize("policy, chunk", [("torch", 0), ("device", 0), ("device", 2)])
def test_run_episode_fills_the_ring_with_either_policy(gpu, policy, chunk):
    """dqn_cnn.run_episode at 16 agents, 48 x 48 frames, 4 steps, without auto-reset (a graph chunk then advances the draw-offset word):
    every agent is alive on the first step, so the ring holds between 16 and 64 transitions whose actions are valid indices and whose
    next_state is the following transition's state for an agent that lived on; eager and chunked device episodes fill the same ring."""
    from openkitchen_amd import dqn_cnn
    from openkitchen_amd.torch_env import VectorEnvironment
    N, S = 16, 48
    torch.manual_seed(5)
    model = dqn_cnn.QCNN(S).cuda().eval()
    rings = []
    for K in sorted({0, chunk}):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=False, seed=3, randomize_lane=True)
        venv.enable_camera(width=S, height=S, fmt="rgba")
        cfg = dqn_cnn.qcnn_config_from_state_dict(model.state_dict(), image_size=S, mode="eps_greedy", epsilon=0.5, seed=9)
        venv.enable_image_dqn(cfg, dqn_cnn.qcnn_params_from_state_dict(model.state_dict(), image_size=S), capacity=128)
        assert dqn_cnn.run_episode(venv, model, max_steps=4, graph_chunk=K, policy=policy)["steps"] == 4
        size, pushed = venv.env.qcnn_ring_size()
        assert N <= size == pushed <= 4 * N
        ring = venv.env.qcnn_ring_get()
        assert 0 <= int(ring["action"][:size].min()) and int(ring["action"][:size].max()) < 5 and float(ring["state"][:size].max()) > 0
        assert same(ring["next_state"][0], ring["state"][N]) or ring["done"][0] == 1.0  # agent 0's second transition follows its first
        rings.append((size, ring))
        with pytest.raises(ValueError, match="needs the camera at the network's size"):
            venv.enable_camera(width=S + 8, height=S + 8, fmt="rgba")
            dqn_cnn.run_episode(venv, model, max_steps=2, policy=policy)
        venv.close()
    if len(rings) == 2:
        assert rings[0][0] == rings[1][0] and all(same(rings[0][1][k], rings[1][1][k]) for k in rings[0][1])


@pytest.mark.parametrize("name, N", [("wide", 33), ("tiny", 17)])
def test_head_with_32_agents_equals_host(gpu, name, N):
    """OKENV_QCNN_STAGE_HEAD_32, the head's tiling that was measured and not chosen (two row tiles a workgroup: one full workgroup and a
    partial one at 33 agents, one partial at 17), behind the conv stage: the record and the action fields bit-equal to the host entry."""
    capi = gpu.capi
    shape = mirror.SHAPES[name]
    S, A = shape["image_size"], shape["num_actions"]
    cfg, params = config(capi, name, "eps_greedy", 0.5), mirror.draw_params(shape, 4)
    venv = driven_population(gpu, N, S)
    venv.enable_image_dqn(cfg, params)
    frames, rec = venv.camera(), record(N, A)
    torch.cuda.synchronize()
    want = capi.qcnn_act_host(cfg, params, frames.cpu().numpy(), venv.env.get(capi.F_CRASHED), venv.env.step_count)
    for t in rec.values():
        t.fill_(7)
    venv.env.qcnn_act(frames, None, stages=capi.QCNN_STAGE_CONV)
    venv.env.qcnn_act(frames, rec, stages=capi.QCNN_STAGE_HEAD_32)
    torch.cuda.synchronize()
    for k in MEMBERS:
        assert same(rec[k].cpu().numpy(), want[k]), k
    assert same(venv.throttle.cpu().numpy(), want["throttle"]) and same(venv.steering.cpu().numpy(), want["steer"])
    venv.close()
