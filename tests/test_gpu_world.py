"""The world-model racers on the device: okenv_world_act against the host entry bit for bit on every path its
plan names, skip_crashed, the order of calls and every refusal, the score against the mirror, the closed loop eagerly and as a
replayed graph, and the reference shape against the float64 PyTorch module."""
import ctypes as C

import numpy as np
import pytest
import torch

import _oracle as O
import _world_numpy as mirror
from test_gpu_bev_encoder import driven_population, fan, last_error, same
from test_world_rule import fold_deviations

pytestmark = pytest.mark.gpu

f32 = np.float32
INVALID, STATE = -1, -5
RECORD = ("mu", "state", "out", "action", "alive")
FIELDS = ("pos_x", "pos_y", "rot", "speed", "acceleration", "throttle", "steering", "crashed", "timed_out")


def record_tensors(N, Z, fill=-7.0):
    return {"mu": torch.full((N, Z), fill, device="cuda"), "state": torch.full((N, Z + 2), fill, device="cuda"),
            "out": torch.full((N,), fill, device="cuda"), "action": torch.full((N, 2), fill, device="cuda"),
            "alive": torch.full((N,), 9, dtype=torch.uint8, device="cuda")}


def host_act(capi, cfg, enc, ctrl, frames, dev, into=None):
    """The host entry on the device's frames, headings and crashed flags, in the record's form."""
    got = capi.world_act_host(cfg, enc, ctrl, frames.cpu().numpy(), dev.get(capi.F_ROT), dev.get(capi.F_CRASHED), into=into)
    return dict(got, action=np.stack([got["throttle"], got["steer"]], axis=1))


def act_case(gpu, name, N):
    capi = gpu.capi
    shape = mirror.SHAPES[name]
    cfg = capi.world_config(**shape)
    S, Z = shape["image_size"], shape["latent"]
    # the path the shape was chosen for is the one its plan selects
    assert capi.world_plan(cfg) == mirror.PATHS[name] and capi.world_lds_bytes(cfg) == mirror.lds_bytes(shape) <= capi.WORLD_LDS_BUDGET
    enc, ctrl = mirror.draw_params(shape, N, N)
    venv = driven_population(gpu, N, S)
    dev, L, h = venv.env, venv.env._L, venv.env._h
    crashed = dev.get(capi.F_CRASHED) != 0
    if N >= 15:
        assert 0 < int(crashed.sum()) < N, "the population must hold crashed and alive agents"
    rendered = venv.camera()
    torch.manual_seed(N)
    frames = {"camera": rendered, "random": torch.randint(0, 256, (N, S, S, 4), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    assert int(rendered[..., :3].max()) > int(rendered[..., :3].min()), "the camera drew nothing"
    want = {kind: host_act(capi, cfg, enc, ctrl, t, dev) for kind, t in frames.items()}
    assert not same(want["camera"]["mu"], want["random"]["mu"])
    assert all(np.abs(w["mu"]).max() > 0.01 and np.isfinite(w["mu"]).all() and (np.abs(w["out"]) < 1).all() for w in want.values())
    assert np.array_equal(want["camera"]["alive"], (~crashed).astype(np.uint8))
    nbytes = N * S * S * 4
    rec = record_tensors(N, Z)
    struct = capi.fill_pointers(capi.OkenvWorldRecord(), rec, "record")
    thr0, steer0 = dev.get(capi.F_THROTTLE), dev.get(capi.F_STEER)

    # the order of calls
    assert L.okenv_world_act(h, capi.ptr(rendered), nbytes, C.byref(struct)) == STATE and b"okenv_world_act: call okenv_world_create first" in last_error(dev)
    a, b = C.c_int32(), C.c_int32()
    assert L.okenv_world_num_params(h, C.byref(a), C.byref(b)) == STATE and L.okenv_world_set_params(h, 0, capi.ptr(enc)) == STATE
    assert L.okenv_world_num_params(h, None, C.byref(b)) == INVALID and L.okenv_world_set_params(h, 0, None) == INVALID
    assert L.okenv_world_score(h) == STATE and L.okenv_world_score_begin(h) == STATE and L.okenv_world_fitness(h, capi.ptr(thr0.copy())) == STATE
    assert L.okenv_world_set_lane_widths(h, capi.ptr(venv.track.wl), capi.ptr(venv.track.wr), venv.track.P) == STATE
    for bad in (dict(image_size=24), dict(image_size=144), dict(channels=(16, 8, 16, 16)), dict(channels=(16, 16, 16, 528)), dict(latent=24),
                dict(latent=144), dict(hidden=3), dict(hidden=66)):
        assert L.okenv_world_create(h, C.byref(capi.world_config(**dict(shape, **bad)))) == INVALID, bad
        assert b"okenv_world_create: shape outside the limits" in last_error(dev)
    assert L.okenv_world_create(h, C.byref(capi.world_config(**dict(shape, skip_crashed=2)))) == INVALID
    assert L.okenv_world_create(h, None) == INVALID and L.okenv_world_create(None, C.byref(cfg)) == INVALID
    assert dev.world_create(cfg) == (enc.size, ctrl.shape[1]) == mirror.num_params(shape)
    assert L.okenv_world_act(h, capi.ptr(rendered), nbytes, None) == STATE
    assert b"okenv_world_act: call okenv_world_set_params first (the encoder and the controllers need their parameters)" in last_error(dev)
    assert L.okenv_world_get_params(h, 0, capi.ptr(np.empty_like(enc))) == STATE
    dev.world_set_params("encoder", enc)  # from a host pointer
    assert L.okenv_world_act(h, capi.ptr(rendered), nbytes, None) == STATE  # the controllers are still missing
    assert L.okenv_world_get_params(h, 1, capi.ptr(np.empty_like(ctrl))) == STATE
    assert L.okenv_world_set_params(h, 2, capi.ptr(enc)) == INVALID
    dev.world_set_params("controllers", ctrl)
    assert same(dev.world_get_params("encoder"), enc) and same(dev.world_get_params("controllers").reshape(ctrl.shape), ctrl)
    for args in ((None, nbytes), (capi.ptr(rendered), nbytes - 4), (capi.ptr(rendered), nbytes + S * S * 4), (capi.ptr(rendered), 0)):
        assert L.okenv_world_act(h, *args, C.byref(struct)) == INVALID, args
        assert b"okenv_world_act: " in last_error(dev)
    assert L.okenv_world_score(h) == STATE and b"okenv_world_set_lane_widths first" in last_error(dev)
    assert L.okenv_world_set_lane_widths(h, capi.ptr(venv.track.wl), capi.ptr(venv.track.wr), venv.track.P - 1) == INVALID
    assert L.okenv_world_set_lane_widths(h, None, capi.ptr(venv.track.wr), venv.track.P) == INVALID
    torch.cuda.synchronize()
    # nothing was launched by a refused call
    assert all(float(t.float().min()) == float(t.float().max()) for t in rec.values())
    assert same(dev.get(capi.F_THROTTLE), thr0) and same(dev.get(capi.F_STEER), steer0)

    def check(label, members=RECORD):
        for kind, t in frames.items():
            rec = record_tensors(N, Z)
            dev.set(capi.F_THROTTLE, np.full(N, -3.0, f32))
            dev.set(capi.F_STEER, np.full(N, -3.0, f32))
            dev.world_act(t, {k: rec[k] for k in members} if members else None)
            torch.cuda.synchronize()
            w = want[kind]
            for k in RECORD:
                got = rec[k].cpu().numpy()
                if k in members:
                    assert same(got, w[k]), "%s, %s frames, %s: %d of %d differ, by up to %.3g" % (
                        label, kind, k, int((got != w[k]).sum()), got.size, float(np.abs(got.astype(f32) - w[k]).max()))
                else:
                    assert (got == (9 if k == "alive" else -7.0)).all(), (label, kind, k)
            assert same(dev.get(capi.F_THROTTLE), w["throttle"]) and same(dev.get(capi.F_STEER), w["steer"]), (label, kind)

    check("host pointer")
    for k in RECORD:  # each single member NULL
        check("without " + k, tuple(m for m in RECORD if m != k))
    check("no record", ())
    # a second create, with another shape and back, forgets both vectors
    other = "tiny" if name != "tiny" else "odd"
    dev.world_create(capi.world_config(**mirror.SHAPES[other]))
    assert L.okenv_world_act(h, capi.ptr(rendered), nbytes, None) == STATE
    dev.world_create(cfg)
    assert L.okenv_world_act(h, capi.ptr(rendered), nbytes, None) == STATE
    # from device pointers, other values first so that the hand-over shows
    on_device = torch.from_numpy(enc).cuda(), torch.from_numpy(ctrl).cuda()  # (alive until the copies have run)
    dev.world_set_params("encoder", np.zeros_like(enc))
    dev.world_set_params("controllers", np.zeros_like(ctrl))
    dev.world_set_params("encoder", on_device[0])
    dev.world_set_params("controllers", on_device[1])
    check("device pointer")
    got = torch.empty(ctrl.shape, device="cuda")
    dev.world_get_params("controllers", got)
    assert same(got.cpu().numpy(), ctrl)

    # skip_crashed: sentinels survive in the fields and the record of crashed agents, the alive ones are the rule's
    dev.world_create(capi.world_config(**dict(shape, skip_crashed=1)))
    dev.world_set_params("encoder", enc)
    dev.world_set_params("controllers", ctrl)
    for kind, t in frames.items():
        rec = record_tensors(N, Z)
        dev.set(capi.F_THROTTLE, np.full(N, -3.0, f32))
        dev.set(capi.F_STEER, np.full(N, -3.0, f32))
        dev.world_act(t, rec)
        torch.cuda.synchronize()
        got = {k: rec[k].cpu().numpy() for k in RECORD}
        got.update(throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER))
        for k, v in got.items():
            sentinel = 9 if k == "alive" else (-3.0 if k in ("throttle", "steer") else -7.0)
            assert same(v[~crashed], want[kind][k][~crashed]), (kind, k)
            assert (v[crashed] == sentinel).all(), (kind, k)
        assert (got["alive"][~crashed] == 1).all()

    # the binding's hand-over and its own checks
    venv.enable_world_racers(cfg, enc, ctrl)
    with pytest.raises(ValueError):
        venv.world_act(rendered[:, :-1])
    venv.world_act(frames["random"])
    assert same(venv.steering.cpu().numpy(), want["random"]["steer"])
    venv.close()


@pytest.mark.parametrize("N", [1, 17, 33])
@pytest.mark.parametrize("name", ["tiny", "odd", "wide", "ragged"])
def test_act_device_equals_host(gpu, name, N):
    act_case(gpu, name, N)


def test_act_device_equals_host_reference_shape(gpu):
    act_case(gpu, "reference", 3)


def test_score_equals_the_mirror(gpu):
    """Four agents held at zero throttle until the standstill logic fires, four steered hard into a wall, eight re-placed behind
    that; then random-rollout chunks: the fitness after every chunk against 1 - oracle_lane_center_distance accumulated by the mirror."""
    from openkitchen_amd.torch_env import VectorEnvironment
    capi = gpu.capi
    N = 24
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=7, ray_angles_deg=fan(7), auto_reset=False, seed=3)
    dev, t = venv.env, venv.track
    dev.world_create(capi.world_config(**mirror.SHAPES["tiny"]))
    dev.world_set_lane_widths(t.wl, t.wr)
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    dev.world_score_begin()
    want = np.zeros(N, f32)

    def score_and_compare(label):
        nonlocal want
        dev.world_score()
        x, y = dev.get(capi.F_POS_X), dev.get(capi.F_POS_Y)
        crashed, timed_out = dev.get(capi.F_CRASHED), dev.get(capi.F_TIMED_OUT)
        d = np.zeros(N, f32)
        O.lib().oracle_lane_center_distance(t.x, t.y, t.wl, t.wr, t.P, x, y, N, d)
        want = mirror.score(want, d, crashed, timed_out)
        got = dev.world_fitness()
        assert same(got, want), (label, got, want)
        on_device = torch.empty(N, device="cuda")
        dev.world_fitness(on_device)
        assert same(on_device.cpu().numpy(), want) and same(venv.world_fitness().cpu().numpy(), want)
        return crashed != 0, timed_out != 0

    thr, steer = np.full(N, 40.0, f32), np.zeros(N, f32)
    thr[:4] = 0.0
    thr[4:8], steer[4:8] = 100.0, 5.0
    for chunk in range(7):  # 210 steps: the standstill timeout fires at the 201st
        dev.set(capi.F_THROTTLE, thr)
        dev.set(capi.F_STEER, steer)
        dev.step(30)
        crashed, timed_out = score_and_compare("held %d" % chunk)
    assert timed_out[:4].all() and crashed[:4].all(), "the held agents must have timed out"
    assert (crashed[4:8] & ~timed_out[4:8]).any(), "an agent must have crashed without timing out"
    assert (want[:4] == 0).all()  # fitness = 0 for a candidate that timed out
    before = want.copy()
    dev.reset_random(np.arange(8, 16, dtype=np.int32), 1, 9, 2, 0)
    dev.step(1)
    crashed, timed_out = score_and_compare("all three kinds")
    assert timed_out.any() and (crashed & ~timed_out).any() and (~crashed).any(), "the population must hold all three kinds"
    assert (want[~crashed] > before[~crashed]).all() and same(want[crashed & ~timed_out], before[crashed & ~timed_out]) and (want[timed_out] == 0).all()
    # okenv_rollout_random re-places crashed agents at the start of every step, so a chunk leaves alive agents and fresh crashes
    for chunk in range(3):
        dev.rollout_random(25, 11, 0, 25 * chunk)
        crashed, timed_out = score_and_compare("random %d" % chunk)
    assert (~crashed).any() and (want > 0).any()
    dev.world_score_begin()
    assert (dev.world_fitness() == 0).all()
    venv.close()


def closed_loop(gpu, mode, iterations=40, N=16):
    """camera -> act -> step -> score, `iterations` times, on `tiny`; mode "device" (eager), "graph" (one captured iteration replayed) or
    "host" (every act replaced by the host entry on the downloaded frames).  Returns the state fields after every iteration and the
    fitness."""
    from openkitchen_amd.torch_env import VectorEnvironment
    capi = gpu.capi
    shape = mirror.SHAPES["tiny"]
    cfg = capi.world_config(**dict(shape, skip_crashed=1))
    enc, ctrl = mirror.draw_params(shape, 40, N)
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=7, ray_angles_deg=fan(7), auto_reset=False, seed=3)
    venv.enable_camera(width=shape["image_size"], height=shape["image_size"], fmt="rgba")
    venv.enable_world_racers(cfg, enc, ctrl)
    dev = venv.env
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    dev.world_score_begin()
    frame = torch.zeros(venv.camera_shape, dtype=torch.uint8, device="cuda")

    def iteration():
        venv.camera(out=frame)
        if mode == "host":
            torch.cuda.synchronize()
            into = dict(mu=np.zeros((N, shape["latent"]), f32), state=np.zeros((N, shape["latent"] + 2), f32), out=np.zeros(N, f32),
                        throttle=dev.get(capi.F_THROTTLE), steer=dev.get(capi.F_STEER), alive=np.zeros(N, np.uint8))
            got = host_act(capi, cfg, enc, ctrl, frame, dev, into=into)
            dev.set(capi.F_THROTTLE, got["throttle"])
            dev.set(capi.F_STEER, got["steer"])
        else:
            venv.world_act(frame)
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
        history.append({k: getattr(venv, k).cpu().numpy().copy() for k in FIELDS})
    fitness = dev.world_fitness()
    venv.close()
    return history, fitness


def test_closed_loop_device_equals_host_and_graph(gpu):
    runs = {mode: closed_loop(gpu, mode) for mode in ("host", "device", "graph")}
    want, want_fitness = runs["host"]
    for mode in ("device", "graph"):
        history, fitness = runs[mode]
        for it, (a, b) in enumerate(zip(history, want)):
            for k in FIELDS:
                assert same(a[k], b[k]), (mode, it, k)
        assert same(fitness, want_fitness), mode
    # the loop did something: the agents steered, moved and scored, and the candidates differ
    assert len(set(want[0]["steering"].tolist())) > 8 and not same(want[0]["pos_x"], want[-1]["pos_x"])
    assert (want_fitness > 0).any() and len(set(want_fitness.tolist())) > 4


def test_reference_shape_against_the_float64_module(gpu):
    """Reference shape, three frames: mu and the controller's output against the float64 PyTorch module with randomised running
    statistics and affine terms, under the rule of tests/test_world_rule.py: the device's largest deviation is at most 4 x that of
    the fp32 module on the CPU (both are fp32 sums of the same terms in different orders).  Measured on the MI355X on the first run
    (docs/HISTORY.md section 39): mu, up to 0.146 in size: device 2.19e-07, fp32 module 1.67e-07; the controller's output, up to 0.396:
    device 6.06e-07, fp32 PyTorch (the module's mu into cmaes.BatchedController) 5.13e-07."""
    from openkitchen_amd.torch_env import VectorEnvironment
    capi = gpu.capi
    shape = mirror.SHAPES["reference"]
    N, S, Z = 3, shape["image_size"], shape["latent"]
    frames = mirror.draw_frames(S, 21, N)
    ctrl = mirror.draw_params(shape, 3, N)[1]
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=7, ray_angles_deg=fan(7), auto_reset=False, seed=3)
    dev = venv.env
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    rot = dev.get(capi.F_ROT)
    seen = {}

    def device_mu(cfg, enc):
        venv.enable_world_racers(cfg, enc, ctrl)
        rec = record_tensors(N, Z)
        venv.world_act(torch.from_numpy(frames).cuda(), rec)
        torch.cuda.synchronize()
        seen.update({k: v.cpu().numpy() for k, v in rec.items()})
        return seen["mu"]

    device, single, scale, exact_mu, single_mu = fold_deviations(capi, "reference", frames, device_mu)
    print("reference mu: device %.3e, fp32 module on the CPU %.3e from the float64 module; mu up to %.3f" % (device, single, scale))
    assert scale > 0.05 and single > 0
    assert device <= 4 * single, (device, single)
    # the controller's output: from the float64 module's mu in float64, and from the fp32 module's mu in fp32 PyTorch
    # (cmaes.BatchedController, the torch path of worldmodel.WorldModelRacers), the degrees taken as stored
    from openkitchen_amd.cmaes import BatchedController
    x = np.concatenate([exact_mu, np.sin(rot.astype(np.float64))[:, None], np.cos(rot.astype(np.float64))[:, None]], axis=1)
    i, h, at = Z + 2, shape["hidden"], 0
    for n_in, n_out in ((i, h), (h, h // 2), (h // 2, 1)):
        w = ctrl[:, at:at + n_out * n_in].reshape(N, n_out, n_in).astype(np.float64)
        at += n_out * n_in
        x = np.tanh(np.einsum("noi,ni->no", w, x) + ctrl[:, at:at + n_out])
        at += n_out
    exact_out = x[:, 0]
    controller = BatchedController(i, h, 1, "cpu", N)
    controller.set_params(ctrl)
    r = torch.from_numpy(rot)
    single_out = controller.forward(torch.cat([torch.from_numpy(single_mu), torch.sin(r)[:, None], torch.cos(r)[:, None]], dim=1))[:, 0].numpy()
    device_dev, single_dev = float(np.abs(seen["out"] - exact_out).max()), float(np.abs(single_out - exact_out).max())
    print("reference out: device %.3e, fp32 PyTorch %.3e from float64; |out| up to %.3f" % (device_dev, single_dev, float(np.abs(exact_out).max())))
    assert device_dev <= 4 * single_dev, (device_dev, single_dev)
    venv.close()
