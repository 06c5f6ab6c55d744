"""The world-model racers' memory on the device: okenv_memory_act against the host entry bit for bit on every
path its plan names, over consecutive acts, with carry and skip_crashed; the record's members one by one; reset and the hidden state's
round trips; the order of calls and every refusal; the closed loop eagerly and as a replayed graph; okenv_world_act untouched; and the
reference shape against the float64 PyTorch modules."""
import ctypes as C

import numpy as np
import pytest
import torch

import _memory_numpy as mirror
import _world_numpy as wmirror
from test_gpu_bev_encoder import driven_population, fan, last_error, same

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, STATE = -1, -5
FIELDS = ("pos_x", "pos_y", "rot", "speed", "acceleration", "throttle", "steering", "crashed", "timed_out")

# test_reference_shape_against_the_float64_modules: S = 128, Z = 32, H = 512, L = 3, 17 agents, one act from a drawn hidden state:
# the largest deviation from the float64 PyTorch modules (Encoder, GRUDynamics) of the device and of the fp32 modules on the CPU.
# The test requires device <= 4 x fp32 modules for each quantity.  Measured on the MI355X on the first run:
#   mu          device 2.82e-07, fp32 modules 1.92e-07 (up to 0.146)
#   hidden      device 5.98e-08, fp32 modules 1.00e-07 (up to 0.474)
#   prediction  device 7.86e-09, fp32 modules 1.17e-08 (up to 0.073)
#   out         device 1.13e-08, fp32 modules 6.66e-09 (up to 0.075)
# (With every sum as one fused chain from the bias, before the rule's chains were blocked: hidden 2.22e-07, prediction 2.53e-08.)


def configs(capi, name, carry=1, skip_crashed=0, **more):
    wname, mem = mirror.SHAPES[name]
    return capi.world_config(**dict(mirror.WORLDS[wname], skip_crashed=skip_crashed)), capi.memory_config(**dict(mem, carry=carry, **more))


def drawn(name, seed, N):
    w, mem, Z, H, L, h = mirror.shape_of(name)
    enc = wmirror.draw_params(w, seed, 1)[0]
    net, ctrl = mirror.draw_params(name, seed, N)
    hidden = np.random.default_rng(300 + seed).uniform(-0.9, 0.9, (N, L, H)).astype(f32)
    return enc, net, ctrl, hidden


def record_tensors(N, Z, H, fill=-7.0):
    sizes = {"mu": (N, Z), "hidden": (N, H), "prediction": (N, Z), "state": (N, Z + H), "out": (N,), "action": (N, 2)}
    rec = {k: torch.full(s, fill, device="cuda") for k, s in sizes.items()}
    rec["alive"] = torch.full((N,), 9, dtype=torch.uint8, device="cuda")
    return rec


def host_record(N, Z, H, fill=-7.0):
    sizes = {"mu": (N, Z), "hidden": (N, H), "prediction": (N, Z), "state": (N, Z + H), "out": (N,), "action": (N, 2)}
    rec = {k: np.full(s, fill, f32) for k, s in sizes.items()}
    rec["alive"] = np.full(N, 9, np.uint8)
    return rec


def attach(dev, wc, mc, enc, net, ctrl):
    dev.world_create(wc)
    dev.world_set_params("encoder", enc)
    counts = dev.memory_create(mc)
    dev.memory_set_params("network", net)
    dev.memory_set_params("controllers", ctrl)
    return counts


def act_both(capi, dev, wc, mc, enc, net, ctrl, frames, members=None):
    """One okenv_memory_act on `frames` and the host entry on the same frames and the device's state before it.  Returns
    (device record, fields and hidden state; the host's): dicts of numpy arrays under the same keys."""
    N, Z, H = dev.N, wc.latent, mc.hidden
    members = capi.MEMORY_RECORD if members is None else members
    before = dict(hidden_state=dev.memory_get_hidden(), throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER))
    want = dict(host_record(N, Z, H), **before)
    capi.memory_act_host(wc, mc, enc, net, ctrl, frames.cpu().numpy(), None, None, None, dev.get(capi.F_CRASHED), into=want)
    rec = record_tensors(N, Z, H)
    dev.memory_act(frames, {k: rec[k] for k in members} if members else None)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    got.update(hidden_state=dev.memory_get_hidden(), throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER))
    return got, want


def assert_equal(got, want, label, members=None):
    for k, w in want.items():
        g = got[k]
        if members is not None and k in ("mu", "hidden", "prediction", "state", "out", "action", "alive") and k not in members:
            assert (g == (9 if k == "alive" else -7.0)).all(), (label, k, "written though NULL")
            continue
        assert same(g, w), "%s, %s: %d of %d differ, by up to %.3g" % (label, k, int((g != w).sum()), g.size, float(np.abs(g.astype(f32) - w.astype(f32)).max()))


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("carry", [0, 1])
@pytest.mark.parametrize("N", mirror.COUNTS)
@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_act_device_equals_host(gpu, name, N, carry, skip):
    capi = gpu.capi
    w, mem, Z, H, L, h = mirror.shape_of(name)
    wc, mc = configs(capi, name, carry, skip)
    # the path the shape was chosen for is the one its plan selects
    assert capi.memory_plan(wc, mc) == mirror.PATHS[name][:6] + (carry, L) and capi.memory_lds_bytes(wc, mc) == mirror.lds_bytes()
    enc, net, ctrl, hidden = drawn(name, N + carry, N)
    S = w["image_size"]
    venv = driven_population(gpu, N, S)
    dev = venv.env
    assert attach(dev, wc, mc, enc, net, ctrl) == mirror.num_params(Z, H, L, h)
    torch.manual_seed(N)
    for kind in ("camera", "random"):
        dev.memory_set_hidden(hidden)
        dev.set(capi.F_THROTTLE, np.full(N, 100.0, f32))
        dev.set(capi.F_STEER, np.linspace(-4.0, 4.0, N, dtype=f32))
        firsts = []
        for t in range(3):
            crashed = dev.get(capi.F_CRASHED) != 0
            if N >= 15 and t == 0:
                assert 0 < int(crashed.sum()) < N, "the population must hold crashed and alive agents"
            frames = venv.camera() if kind == "camera" else torch.randint(0, 256, (N, S, S, 4), dtype=torch.uint8, device="cuda")
            got, want = act_both(capi, dev, wc, mc, enc, net, ctrl, frames)
            assert_equal(got, want, "%s act %d" % (kind, t))
            alive = ~crashed if skip else np.ones(N, bool)
            assert (np.abs(got["hidden_state"][alive]).max() < 1) and np.isfinite(got["hidden_state"]).all() and (np.abs(got["out"][alive]) < 1).all()
            assert np.array_equal(got["alive"][alive], (~crashed[alive]).astype(np.uint8))
            if skip and crashed.any():  # a crashed agent's hidden state, action fields and record entries are as they were
                assert same(got["hidden_state"][crashed], hidden[crashed] if t == 0 else firsts[-1]["hidden_state"][crashed])
                assert (got["mu"][crashed] == -7.0).all() and (got["alive"][crashed] == 9).all()
            firsts.append(got)
            dev.step(1)
        if alive.any():
            assert not same(firsts[0]["hidden_state"][alive], firsts[1]["hidden_state"][alive])
    venv.close()


def test_each_record_member_null_in_turn(gpu):
    capi = gpu.capi
    name, N = "h48", 17
    w, mem, Z, H, L, h = mirror.shape_of(name)
    wc, mc = configs(capi, name)
    enc, net, ctrl, hidden = drawn(name, 2, N)
    venv = driven_population(gpu, N, w["image_size"])
    dev = venv.env
    attach(dev, wc, mc, enc, net, ctrl)
    frames = venv.camera()
    for members in [tuple(m for m in capi.MEMORY_RECORD if m != k) for k in capi.MEMORY_RECORD] + [()]:
        dev.memory_set_hidden(hidden)
        got, want = act_both(capi, dev, wc, mc, enc, net, ctrl, frames, members)
        assert_equal(got, want, "without %s" % (set(capi.MEMORY_RECORD) - set(members)), members)
    venv.close()


def test_reset_and_hidden_round_trips(gpu):
    capi = gpu.capi
    name, N = "h48", 17
    w, mem, Z, H, L, h = mirror.shape_of(name)
    wc, mc = configs(capi, name)
    enc, net, ctrl, hidden = drawn(name, 3, N)
    venv = driven_population(gpu, N, w["image_size"])
    dev = venv.env
    attach(dev, wc, mc, enc, net, ctrl)
    assert (dev.memory_get_hidden() == 0).all()  # create zeroes the state
    dev.memory_set_hidden(hidden)  # from a host pointer
    assert same(dev.memory_get_hidden(), hidden)
    on_device = torch.from_numpy(hidden * f32(0.5)).cuda()
    dev.memory_set_hidden(on_device)  # from a device pointer
    back = torch.empty_like(on_device)
    dev.memory_get_hidden(back)
    assert torch.equal(back, on_device) and same(dev.memory_get_hidden(), hidden * f32(0.5))
    dev.memory_reset()
    assert (dev.memory_get_hidden() == 0).all()
    # an act from the reset state is the host's act from zeros; a second create zeroes the state again and forgets the parameters
    frames = venv.camera()
    got, want = act_both(capi, dev, wc, mc, enc, net, ctrl, frames)
    assert_equal(got, want, "from reset")
    assert np.abs(got["hidden_state"]).max() > 0.01
    assert same(dev.memory_get_params("network"), net) and same(dev.memory_get_params("controllers").reshape(ctrl.shape), ctrl)
    dev.memory_create(mc)
    assert (dev.memory_get_hidden() == 0).all()
    assert dev._L.okenv_memory_act(dev._h, capi.ptr(frames), frames.numel(), None) == STATE
    venv.close()


def test_order_of_calls_and_every_refusal(gpu):
    capi = gpu.capi
    name, N = "h16", 17
    w, mem, Z, H, L, h = mirror.shape_of(name)
    wc, mc = configs(capi, name)
    enc, net, ctrl, hidden = drawn(name, 4, N)
    S = w["image_size"]
    venv = driven_population(gpu, N, S)
    dev, L_, hd = venv.env, venv.env._L, venv.env._h
    frames = venv.camera()
    nbytes = N * S * S * 4
    rec = record_tensors(N, Z, H)
    struct = capi.fill_pointers(capi.OkenvMemoryRecord(), rec, "record")
    thr0, steer0 = dev.get(capi.F_THROTTLE), dev.get(capi.F_STEER)
    a, b = C.c_int32(), C.c_int32()
    # before okenv_world_create
    assert L_.okenv_memory_create(hd, C.byref(mc)) == STATE and b"okenv_memory_create: call okenv_world_create first" in last_error(dev)
    assert L_.okenv_memory_act(hd, capi.ptr(frames), nbytes, C.byref(struct)) == STATE and b"okenv_memory_act: call okenv_memory_create first" in last_error(dev)
    dev.world_create(wc)
    # before okenv_memory_create
    assert L_.okenv_memory_act(hd, capi.ptr(frames), nbytes, C.byref(struct)) == STATE and b"okenv_memory_act: call okenv_memory_create first" in last_error(dev)
    assert L_.okenv_memory_num_params(hd, C.byref(a), C.byref(b)) == STATE and L_.okenv_memory_set_params(hd, 0, capi.ptr(net)) == STATE
    assert L_.okenv_memory_reset(hd) == STATE and L_.okenv_memory_set_hidden(hd, capi.ptr(hidden)) == STATE
    assert L_.okenv_memory_get_hidden(hd, capi.ptr(hidden.copy())) == STATE and L_.okenv_memory_get_params(hd, 0, capi.ptr(net.copy())) == STATE
    assert L_.okenv_memory_num_params(hd, None, C.byref(b)) == INVALID and L_.okenv_memory_set_params(hd, 0, None) == INVALID
    assert L_.okenv_memory_set_hidden(hd, None) == INVALID and L_.okenv_memory_get_hidden(hd, None) == INVALID
    for bad in (dict(hidden=24), dict(hidden=528), dict(layers=0), dict(layers=5), dict(ctrl_hidden=3), dict(ctrl_hidden=66)):
        assert L_.okenv_memory_create(hd, C.byref(configs(capi, name, **bad)[1])) == INVALID, bad
        assert b"okenv_memory_create: shape outside the limits" in last_error(dev)
    assert L_.okenv_memory_create(hd, C.byref(configs(capi, name, carry=2)[1])) == INVALID and b"carry must be 0 or 1" in last_error(dev)
    assert L_.okenv_memory_create(hd, None) == INVALID and L_.okenv_memory_create(None, C.byref(mc)) == INVALID
    assert dev.memory_create(mc) == mirror.num_params(Z, H, L, h)
    # before the parameters
    assert L_.okenv_memory_act(hd, capi.ptr(frames), nbytes, None) == STATE
    assert b"okenv_memory_act: call okenv_world_set_params first (the encoder needs its parameters)" in last_error(dev)
    dev.world_set_params("encoder", enc)
    assert L_.okenv_memory_act(hd, capi.ptr(frames), nbytes, None) == STATE
    assert b"okenv_memory_act: call okenv_memory_set_params first (the network and the controllers need their parameters)" in last_error(dev)
    assert L_.okenv_memory_get_params(hd, 0, capi.ptr(net.copy())) == STATE
    dev.memory_set_params("network", net)
    assert L_.okenv_memory_act(hd, capi.ptr(frames), nbytes, None) == STATE  # the controllers are still missing
    assert L_.okenv_memory_get_params(hd, 1, capi.ptr(ctrl.copy())) == STATE and L_.okenv_memory_set_params(hd, 2, capi.ptr(net)) == INVALID
    dev.memory_set_params("controllers", ctrl)
    for args in ((None, nbytes), (capi.ptr(frames), nbytes - 4), (capi.ptr(frames), nbytes + S * S * 4), (capi.ptr(frames), 0)):
        assert L_.okenv_memory_act(hd, *args, C.byref(struct)) == INVALID, args
        assert b"okenv_memory_act: " in last_error(dev)
    assert L_.okenv_memory_act(None, capi.ptr(frames), nbytes, None) == INVALID
    torch.cuda.synchronize()
    # nothing was launched by a refused call
    assert all(float(t.float().min()) == float(t.float().max()) for t in rec.values())
    assert same(dev.get(capi.F_THROTTLE), thr0) and same(dev.get(capi.F_STEER), steer0) and (dev.memory_get_hidden() == 0).all()
    # the racers' own controllers are not needed; and the act works
    got, want = act_both(capi, dev, wc, mc, enc, net, ctrl, frames)
    assert_equal(got, want, "first act")
    # a later okenv_world_create detaches the memory
    dev.world_create(wc)
    assert L_.okenv_memory_act(hd, capi.ptr(frames), nbytes, None) == STATE and b"okenv_memory_act: call okenv_memory_create first" in last_error(dev)
    assert L_.okenv_memory_reset(hd) == STATE
    venv.close()


def closed_loop(gpu, mode, carry, iterations=8, N=16):
    """camera -> act -> step -> score, `iterations` times, on h16 with skip_crashed; mode "device" (eager), "graph" (one captured
    iteration replayed) or "host" (every act replaced by the host entry).  Returns the state fields and the hidden state after every
    iteration, and the fitness."""
    from openkitchen_amd.torch_env import VectorEnvironment
    capi = gpu.capi
    name = "h16"
    w, mem, Z, H, L, h = mirror.shape_of(name)
    wc, mc = configs(capi, name, carry, 1)
    enc, net, ctrl, hidden = drawn(name, 40, N)
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=7, ray_angles_deg=fan(7), auto_reset=False, seed=3)
    venv.enable_camera(width=w["image_size"], height=w["image_size"], fmt="rgba")
    dev = venv.env
    attach(dev, wc, mc, enc, net, ctrl)
    dev.world_set_lane_widths(venv.track.wl, venv.track.wr)
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    dev.world_score_begin()
    dev.memory_set_hidden(hidden)
    dev.memory_reset()
    frame = torch.zeros(venv.camera_shape, dtype=torch.uint8, device="cuda")

    def iteration():
        venv.camera(out=frame)
        if mode == "host":
            torch.cuda.synchronize()
            state = dict(hidden_state=dev.memory_get_hidden(), throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER))
            got = capi.memory_act_host(wc, mc, enc, net, ctrl, frame.cpu().numpy(), None, None, None, dev.get(capi.F_CRASHED),
                                       into=dict(host_record(N, Z, H), **state))
            dev.memory_set_hidden(got["hidden_state"])
            dev.set(capi.F_THROTTLE, got["throttle"])
            dev.set(capi.F_STEER, got["steer"])
        else:
            dev.memory_act(frame)
        venv.step()
        dev.world_score()

    graph = venv.capture(iteration, warmup=0) if mode == "graph" else None
    history = []
    for _ in range(iterations):
        if graph is not None:
            graph.replay()
        else:
            iteration()
        torch.cuda.synchronize()
        history.append(dict({k: getattr(venv, k).cpu().numpy().copy() for k in FIELDS}, hidden=dev.memory_get_hidden()))
    fitness = dev.world_fitness()
    venv.close()
    return history, fitness


@pytest.mark.parametrize("carry", [1, 0])
def test_closed_loop_device_equals_host_and_graph(gpu, carry):
    """The test that catches a double buffer kept on the host: a replayed graph must advance the hidden state exactly as eager calls."""
    runs = {mode: closed_loop(gpu, mode, carry) for mode in ("host", "device", "graph")}
    want, want_fitness = runs["host"]
    for mode in ("device", "graph"):
        history, fitness = runs[mode]
        for it, (a, b) in enumerate(zip(history, want)):
            for k in FIELDS + ("hidden",):
                assert same(a[k], b[k]), (mode, it, k)
        assert same(fitness, want_fitness), mode
    # the loop did something: the agents steered, moved and scored, the state moved every iteration, and the candidates differ
    assert len(set(want[0]["steering"].tolist())) > 8 and not same(want[0]["pos_x"], want[-1]["pos_x"])
    assert all(not same(want[i]["hidden"], want[i + 1]["hidden"]) for i in range(len(want) - 1))
    assert (want_fitness > 0).any() and len(set(want_fitness.tolist())) > 4


def test_world_act_is_unchanged_beside_a_memory(gpu):
    """After okenv_memory_create, and after memory acts, okenv_world_act still equals its own host entry bit for bit."""
    capi = gpu.capi
    name, N = "h48", 17
    w, mem, Z, H, L, h = mirror.shape_of(name)
    wc, mc = configs(capi, name)
    enc, net, ctrl, hidden = drawn(name, 6, N)
    wctrl = wmirror.draw_params(w, 6, N)[1]
    venv = driven_population(gpu, N, w["image_size"])
    dev = venv.env
    attach(dev, wc, mc, enc, net, ctrl)
    dev.world_set_params("controllers", wctrl)
    frames = venv.camera()
    dev.memory_act(frames)
    rec = {"mu": torch.zeros(N, Z, device="cuda"), "state": torch.zeros(N, Z + 2, device="cuda"), "out": torch.zeros(N, device="cuda")}
    rot = dev.get(capi.F_ROT)
    dev.world_act(frames, rec)
    torch.cuda.synchronize()
    want = capi.world_act_host(wc, enc, wctrl, frames.cpu().numpy(), rot, dev.get(capi.F_CRASHED))
    for k in rec:
        assert same(rec[k].cpu().numpy(), want[k]), k
    assert same(dev.get(capi.F_STEER), want["steer"]) and same(dev.get(capi.F_THROTTLE), want["throttle"])
    # ... and the memory's state was not touched by it
    before = dev.memory_get_hidden()
    dev.world_act(frames)
    assert same(dev.memory_get_hidden(), before) and np.abs(before).max() > 0.01
    venv.close()


def test_reference_shape_against_the_float64_modules(gpu):
    """Reference shape (S = 128, Z = 32, H = 512, L = 3, h = 16), 17 agents, one act with carry from a drawn hidden state, against the
    float64 PyTorch modules with the same weights, under the rule of tests/test_world_rule.py: the device's largest deviation is at
    most 4 x that of the fp32 modules on the CPU, for mu, the top hidden state, the prediction and the controller's output.
    The figures of the first run on the MI355X are in this file's header."""
    import copy
    from openkitchen_amd import worldmodel as wm
    from openkitchen_amd.cmaes import BatchedController
    from openkitchen_amd.torch_env import VectorEnvironment
    from test_world_rule import randomised_encoder
    capi = gpu.capi
    shape = wmirror.SHAPES["reference"]
    N, S, Z, H, L, h = 17, 128, 32, 512, 3, 16
    torch.manual_seed(5)
    encoder = randomised_encoder(shape, 11)
    memory = wm.GRUDynamics(Z, H, L).eval()
    rng = np.random.default_rng(12)
    stats = {"z_mean": rng.uniform(-0.05, 0.05, Z), "z_std": rng.uniform(0.05, 0.15, Z), "a_mean": np.array([90.0, 0.25]), "a_std": np.array([20.0, 2.5])}
    frames = wmirror.draw_frames(S, 21, N)
    hidden = rng.uniform(-0.5, 0.5, (N, L, H)).astype(f32)
    ctrl = (rng.uniform(-1, 1, (N, capi.memory_num_params(capi.world_config(), capi.memory_config())[1])) * 2 / np.sqrt(Z + H)).astype(f32)
    action = np.stack([np.full(N, 100.0), np.linspace(-4, 4, N)], axis=1).astype(f32)
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=7, ray_angles_deg=fan(7), auto_reset=False, seed=3)
    dev = venv.env
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    wc = wm.world_config_from_state_dict(encoder.state_dict(), image_size=S)
    mc = wm.memory_config_from_state_dict(memory.state_dict(), ctrl_hidden=h)
    attach(dev, wc, mc, wm.world_params_from_state_dict(encoder.state_dict(), image_size=S).numpy(),
           wm.memory_params_from_state_dict(memory.state_dict(), stats).numpy(), ctrl)
    dev.memory_set_hidden(hidden)
    dev.set(capi.F_THROTTLE, action[:, 0].copy())
    dev.set(capi.F_STEER, action[:, 1].copy())
    rec = record_tensors(N, Z, H)
    dev.memory_act(torch.from_numpy(frames).cuda(), rec)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    x = wm.frames_to_input(torch.from_numpy(frames))
    out = {}
    for dtype in (torch.float64, torch.float32):
        st = {k: torch.as_tensor(v).to(dtype) for k, v in stats.items()}
        with torch.no_grad():
            mu = copy.deepcopy(encoder).to(dtype)(x.to(dtype))[0]
            xin = torch.cat([(mu - st["z_mean"]) / st["z_std"], (torch.from_numpy(action).to(dtype) - st["a_mean"]) / st["a_std"]], dim=1)
            m = copy.deepcopy(memory).to(dtype)
            y, hn = m.gru(xin[:, None], torch.from_numpy(hidden).to(dtype).transpose(0, 1).contiguous())
            pred = m.head(y[:, 0]) * st["z_std"] + st["z_mean"]
            state = torch.cat([mu, hn[-1]], dim=1)
            if dtype == torch.float64:
                v, at = state.numpy(), 0
                for n_in, n_out in ((Z + H, h), (h, h // 2), (h // 2, 1)):
                    wgt = ctrl[:, at:at + n_out * n_in].reshape(N, n_out, n_in).astype(np.float64)
                    at += n_out * n_in
                    v = np.tanh(np.einsum("noi,ni->no", wgt, v) + ctrl[:, at:at + n_out])
                    at += n_out
                o = v[:, 0]
            else:
                controller = BatchedController(Z + H, h, 1, "cpu", N)
                controller.set_params(ctrl)
                o = controller.forward(state)[:, 0].numpy()
        out[dtype] = dict(mu=mu.double().numpy(), hidden=hn[-1].double().numpy(), prediction=pred.double().numpy(), out=np.asarray(o, np.float64))
    exact, single = out[torch.float64], out[torch.float32]
    failures = []
    for k in ("mu", "hidden", "prediction", "out"):
        device_dev, single_dev = float(np.abs(got[k] - exact[k]).max()), float(np.abs(single[k] - exact[k]).max())
        print("reference %s: device %.3e, fp32 modules on the CPU %.3e from the float64 modules; up to %.3f in size" % (k, device_dev, single_dev, float(np.abs(exact[k]).max())))
        assert np.abs(exact[k]).max() > 0.02 and single_dev > 0
        if not device_dev <= 4 * single_dev:
            failures.append((k, device_dev, single_dev))
    assert not failures, failures
    venv.close()
