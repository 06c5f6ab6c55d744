"""The expert drivers on the device (okenv_expert_create / okenv_expert_act, openkitchen_amd/csrc/ok_expert.h): bit-equal to the
host entry that shares their rule, in closed loops against the oracle's Environment::step, the record slots, HIP-graph capture,
collect_demonstrations and the argument validation."""
import numpy as np
import pytest
import torch

from test_expert_rule import COLLECTOR, FANS, bits, cpu_loop

pytestmark = pytest.mark.gpu
f32 = np.float32
STATE = ["pos_x", "pos_y", "rot", "speed", "acc", "thr", "steer", "mode", "crashed", "timed_out", "disp_ctr", "disp_x", "disp_y", "disp_to",
         "hit_x", "hit_y", "rel_x", "rel_y", "dist"]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def fan_of(gpu, R):
    return FANS[R] if R in FANS else gpu.default_ray_fan(R)


def make_env(gpu, track, N, fan, seed):
    t = gpu.Track(track)
    dev = gpu.BatchedEnvironment.from_track(t, N, ray_angles_deg=fan)
    dev.set_lane_bounds(t.li, t.ri)
    dev.reset_random(None, 1 | 2 | 4, seed, 0, 0)
    dev.step(1)
    return t, dev


def record_tensors(N, R):
    rec = {"action": torch.full((N, 2), -7.0, device="cuda"), "dist": torch.full((N, R), -7.0, device="cuda"),
           "rel_xy": torch.full((N, R, 2), -7.0, device="cuda"), "alive": torch.full((N,), 9, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("track,kind,R,N", [
    ("Austin", "potfield", 5, 1), ("Silverstone", "potfield", 7, 257), ("Monza", "potfield", 64, 4096), ("Austin", "potfield", 19, 4096),
    ("Silverstone", "potfield", 7, 4096), ("Austin", "vfh", 19, 4096), ("Silverstone", "vfh", 64, 257), ("Monza", "vfh", 5, 1),
    ("Monza", "vfh", 7, 4096), ("Silverstone", "vfh", 19, 257)])
def test_device_equals_host(gpu, track, kind, R, N):
    """Same state, same bits: agents on the track, crashed ones, agents far off the grid, |rot| up to 7200 degrees; both goal
    modes, clamp on and off, VFH thresholds 0 and 1."""
    fan = fan_of(gpu, R)
    t, dev = make_env(gpu, track, N, fan, seed=R + N)
    rng = np.random.default_rng(N * 131 + R)
    dev.step(3)
    px, py, rot, crashed = dev.get(gpu.capi.F_POS_X), dev.get(gpu.capi.F_POS_Y), dev.get(gpu.capi.F_ROT), dev.get(gpu.capi.F_CRASHED)
    far = rng.random(N) < 0.1
    px[far] += rng.uniform(-5000, 5000, int(far.sum())).astype(f32)
    py[far] += rng.uniform(-5000, 5000, int(far.sum())).astype(f32)
    wild = rng.random(N) < 0.4
    rot[wild] = rng.uniform(-7200, 7200, int(wild.sum())).astype(f32)
    crashed[rng.random(N) < 0.2] = 1
    # agents near the end of the centre line: the two goal modes differ there
    k = min(N, 8)
    px[:k], py[:k] = t.x[t.P - 1 - np.arange(k) % 3], t.y[t.P - 1 - np.arange(k) % 3]
    for f, v in ((gpu.capi.F_POS_X, px), (gpu.capi.F_POS_Y, py), (gpu.capi.F_ROT, rot), (gpu.capi.F_CRASHED, crashed)):
        dev.set(f, v)
    dist = dev.get(gpu.capi.F_DIST)
    for wrap in (False, True):
        for variant in (0, 1):
            params = dict(lookahead=2, goal_wrap=wrap, clamp_deg=10.0 * variant) if kind == "potfield" else \
                dict(lookahead=2 + variant, goal_wrap=wrap, vfh_threshold=variant)
            ep = dev.expert_create(kind, **params)
            dev.expert_act()
            thr, steer = dev.get(gpu.capi.F_THROTTLE), dev.get(gpu.capi.F_STEER)
            want_thr, want_steer = gpu.expert_act_host(ep, fan, px, py, rot, dist, centerline=(t.x, t.y))
            assert np.array_equal(bits(thr), bits(want_thr)), (wrap, variant)
            assert np.array_equal(bits(steer), bits(want_steer)), (wrap, variant)
    dev.close()


@pytest.mark.parametrize("track,kind,auto_reset", [("Silverstone", "potfield", False), ("Monza", "potfield", True), ("Austin", "vfh", True),
                                                   ("Silverstone", "vfh", False)])
def test_closed_loop_against_the_cpu_loop(gpu, oracle, track, kind, auto_reset):
    """600 steps of `expert_act; step` against the oracle's step + the host expert: every state field and every recorded slot."""
    N, steps, seed = 96, 600, 21
    fan = FANS[7] if kind == "potfield" else FANS[19]
    params = COLLECTOR if kind == "potfield" else dict(lookahead=2, goal_wrap=True, vfh_threshold=0)
    orc, _, want = cpu_loop(gpu, oracle, track, N, steps, seed, kind=kind, fan=fan, auto_reset=auto_reset, params=params, record=True)
    t = gpu.Track(track)
    dev = gpu.BatchedEnvironment.from_track(t, N, ray_angles_deg=fan)
    dev.set_lane_bounds(t.li, t.ri)
    dev.set_auto_reset(auto_reset, 1 | 2 | 4, seed, 0)
    dev.reset_random(None, 1 | 2 | 4, seed, 0, 0)
    dev.step(1)
    dev.expert_create(kind, **params)
    R = fan.size
    rec = {"action": torch.zeros((steps, N, 2), device="cuda"), "dist": torch.zeros((steps, N, R), device="cuda"),
           "rel_xy": torch.zeros((steps, N, R, 2), device="cuda"), "alive": torch.zeros((steps, N), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    for s in range(steps):
        dev.expert_act({k: v[s] for k, v in rec.items()})
        dev.step(1)
    dev.sync()
    d, o = dev.snapshot(), orc.snapshot()
    for k in STATE:
        assert same(d[k], o[k]), k
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    for s in range(steps):
        assert same(got["action"][s], want[s]["action"]), s
        assert same(got["dist"][s], want[s]["dist"]), s
        assert same(got["rel_xy"][s][..., 0], want[s]["rel_x"]) and same(got["rel_xy"][s][..., 1], want[s]["rel_y"]), s
        assert same(got["alive"][s], want[s]["alive"]), s
    print("%s %s auto_reset=%d: %d of %d alive after %d steps" % (track, kind, auto_reset, int((d["crashed"] == 0).sum()), N, steps))
    dev.close()


def test_record_slots_and_untouched_fields(gpu):
    N, R = 300, 15
    fan = FANS[15]
    t, dev = make_env(gpu, "Silverstone", N, fan, seed=5)
    dev.step(40)
    crashed = dev.get(gpu.capi.F_CRASHED)
    crashed[::7] = 1
    dev.set(gpu.capi.F_CRASHED, crashed)
    dev.expert_create("potfield", clamp_deg=10.0)
    before = dev.snapshot()
    rec = record_tensors(N, R)
    dev.expert_act(rec)
    dev.sync()
    after = dev.snapshot()
    for k in STATE:
        if k not in ("thr", "steer"):
            assert same(before[k], after[k]), k
    assert not same(before["steer"], after["steer"])
    assert same(rec["action"].cpu().numpy()[:, 0], after["thr"]) and same(rec["action"].cpu().numpy()[:, 1], after["steer"])
    assert same(rec["dist"].cpu().numpy(), before["dist"])
    assert same(rec["rel_xy"].cpu().numpy()[..., 0], before["rel_x"]) and same(rec["rel_xy"].cpu().numpy()[..., 1], before["rel_y"])
    assert np.array_equal(rec["alive"].cpu().numpy(), (before["crashed"] == 0).astype(np.uint8))
    # NULL members are skipped
    for keep in ("action", "dist", "rel_xy", "alive"):
        rec2 = record_tensors(N, R)
        dev.expert_act({keep: rec2[keep]})
        dev.sync()
        for k in rec2:
            if k == keep:
                assert torch.equal(rec2[k], rec[k]), k
            else:
                assert bool((rec2[k] == (9 if k == "alive" else -7.0)).all()), (keep, k)
    dev.close()


def venv_pair(gpu, N, fan, kind, camera, **params):
    from openkitchen_amd.torch_env import VectorEnvironment
    out = []
    for _ in range(2):
        v = VectorEnvironment(
            "Silverstone", N, ray_angles_deg=fan, auto_reset=True, pick_random_point=True, randomize_lane=True, randomize_heading=True, seed=9)
        v.env.set_lane_bounds(v.track.li, v.track.ri)
        v.enable_expert(kind, **params)
        if camera:
            v.enable_camera(32, 24)
        v.reset()
        out.append(v)
    return out


@pytest.mark.parametrize("kind,camera", [("potfield", False), ("vfh", False), ("potfield", True)])
def test_captured_graph_equals_eager(gpu, kind, camera):
    N = 512
    fan = FANS[7] if kind == "potfield" else FANS[19]
    params = COLLECTOR if kind == "potfield" else dict(vfh_threshold=0, goal_wrap=True)
    a, b = venv_pair(gpu, N, fan, kind, camera, **params)
    recs = []
    for v in (a, b):
        rec = {"action": torch.zeros((N, 2), device="cuda"), "dist": torch.zeros((N, fan.size), device="cuda"),
               "rel_xy": torch.zeros((N, fan.size, 2), device="cuda"), "alive": torch.zeros((N,), dtype=torch.uint8, device="cuda")}
        rec["frame"] = torch.zeros(v.camera_shape, dtype=torch.uint8, device="cuda") if camera else None
        recs.append(rec)

    def body_of(v, rec):
        def body():
            v.expert_act({k: rec[k] for k in ("action", "dist", "rel_xy", "alive")})
            if camera:
                v.camera(out=rec["frame"])
            v.step()
        return body

    graph = a.capture(body_of(a, recs[0]))
    eager = body_of(b, recs[1])
    for _ in range(256):
        graph.replay()
        eager()
    torch.cuda.synchronize()
    for name in a.FIELDS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for k in recs[0]:
        if recs[0][k] is not None:
            assert torch.equal(recs[0][k], recs[1][k]), k
    assert a.env.step_count == b.env.step_count
    a.close()
    b.close()


def test_collect_demonstrations_frames_are_the_camera_at_that_state(gpu):
    from openkitchen_amd.demonstrations import collect_demonstrations
    N, T = 128, 12
    a, b = venv_pair(gpu, N, FANS[7], "potfield", True, **COLLECTOR)
    out = collect_demonstrations(a, T, images=True, seed=77)
    torch.cuda.synchronize()
    assert out["frames"].shape == (T, N, 24, 32, 4) and out["actions"].shape == (T, N, 2) and out["dist"].shape == (T, N, 7)
    assert out["rel_xy"].shape == (T, N, 7, 2) and out["alive"].shape == (T, N)
    b.env.reset_random(None, 1 | 2 | 4, 77, 0, b.agent_base)
    # the same sequence by hand
    b.env.step(1)
    for t in range(T):
        b.expert_act()
        frame = b.camera()
        torch.cuda.synchronize()
        assert torch.equal(out["frames"][t], frame), t
        assert torch.equal(out["actions"][t, :, 0], b.throttle) and torch.equal(out["actions"][t, :, 1], b.steering), t
        assert torch.equal(out["dist"][t], b.distances) and torch.equal(out["alive"][t], (b.crashed == 0).to(torch.uint8)), t
        b.env.step(1)
    assert len(torch.unique(out["frames"])) > 2
    a.close()
    b.close()


def test_argument_validation(gpu):
    capi = gpu.capi
    t = gpu.Track("Austin")
    L = capi.load()
    # no centre line
    bare = gpu.BatchedEnvironment(t.segments, 16, FANS[7])
    with pytest.raises(capi.OkenvError) as e:
        bare.expert_create("potfield")
    assert e.value.code == -5
    with pytest.raises(capi.OkenvError) as e:
        bare.expert_act()
    assert e.value.code == -5
    bare.close()
    dev = gpu.BatchedEnvironment.from_track(t, 16, ray_angles_deg=FANS[7])
    dev.step(1)
    dev.set_actions(np.full(16, 3.0, f32), np.full(16, -1.0, f32))
    with pytest.raises(capi.OkenvError) as e:
        dev.expert_act()  # before _create
    assert e.value.code == -5
    for bad in (dict(kind=2), dict(kind=-1), dict(kind="potfield", lookahead=-1), dict(kind="vfh", lookahead=-3)):
        with pytest.raises(capi.OkenvError) as e:
            dev.expert_create(**bad)
        assert e.value.code == -1, bad
    assert L.okenv_expert_create(dev._h, None) == -1
    with pytest.raises(capi.OkenvError) as e:
        dev.expert_act()  # still none attached
    assert e.value.code == -5
    one = gpu.BatchedEnvironment.from_track(t, 4, ray_angles_deg=np.zeros(1, f32))
    with pytest.raises(capi.OkenvError) as e:
        one.expert_create("vfh")
    assert e.value.code == -1
    one.expert_create("potfield")  # any fan for the potential field
    one.close()
    # nothing was launched: the actions are as set
    assert np.array_equal(dev.get(capi.F_THROTTLE), np.full(16, 3.0, f32)) and np.array_equal(dev.get(capi.F_STEER), np.full(16, -1.0, f32))
    # the host entry validates alike
    z = np.zeros(1, f32)
    assert L.okenv_expert_act_host(None, capi.ptr(FANS[7]), 7, capi.ptr(z), capi.ptr(z), 1, 1, capi.ptr(z), capi.ptr(z), capi.ptr(z),
                                   capi.ptr(np.zeros(7, f32)), None, None, capi.ptr(z.copy()), capi.ptr(z.copy())) == -1
    dev.close()
