"""The world-model racers' rule (include/okenv_world.h) without a GPU: the host entries okenv_world_act_host / okenv_world_score_host
against the numpy mirror bit for bit, the encoder vector's layout against the PyTorch module, the limits of the shape, the plan
functions, skip_crashed, the BatchNorm fold against the float64 module and the host forward under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _oracle as O
import _population_cases as P
import _world_numpy as mirror

f32 = np.float32
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_fold_and_host_entry_against_the_float64_module: the largest |mu - float64 module's mu| over two frames of random bytes, randomised running
# statistics and affine terms, measured on the CPU: the host entry (BatchNorm folded in float64, rounded once) and the fp32 PyTorch
# module, both fp32 sums of the same terms in different orders.  The test requires host <= 4 x torch, whatever the two are.
#   odd       host 5.15e-08, torch fp32 1.91e-08 (mu up to 0.199)
#   reference host 2.02e-07, torch fp32 1.28e-07 (mu up to 0.146)
FOLD_SHAPES = ("odd", "reference")


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def config(capi, name_or_members, **more):
    members = mirror.SHAPES[name_or_members] if isinstance(name_or_members, str) else name_or_members
    return capi.world_config(**dict(members, **more))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_host_entry_equals_the_mirror_bit_for_bit(capi, name):
    cfg = mirror.SHAPES[name]
    n = 1 if name == "reference" else 2
    enc, ctrl = mirror.draw_params(cfg, len(name), n)
    frames = mirror.draw_frames(cfg["image_size"], len(name), n)
    rot = np.array([-123.5, 47.25], f32)[:n]
    want = mirror.act(cfg, enc, ctrl, frames, rot)
    got = capi.world_act_host(config(capi, name), enc, ctrl, frames, rot)
    for k in ("mu", "state", "out", "throttle", "steer"):
        assert same(got[k], want[k]), "%s %s: differ by up to %.3g" % (name, k, float(np.abs(got[k] - want[k]).max()))
    assert np.array_equal(got["alive"], np.ones(n, np.uint8))
    # a wrong term would show: the latents are of size, the controllers do not saturate and every agent has an action of its own
    assert 0.05 < np.abs(got["mu"]).max() < 50 and np.isfinite(got["mu"]).all() and (np.abs(got["out"]) < 1).all()
    assert same(got["state"][:, :cfg["latent"]], got["mu"]) and len(set(got["out"].tolist())) == n
    # the state's last two entries are the sine and cosine of the degrees taken as they are stored
    assert np.allclose(got["state"][:, -2], np.sin(rot.astype(np.float64)), atol=1e-6)
    assert np.allclose(got["state"][:, -1], np.cos(rot.astype(np.float64)), atol=1e-6)


@pytest.mark.parametrize("name", ["reference", "odd"])
def test_layout_equals_the_pytorch_module(capi, name):
    from openkitchen_amd import worldmodel as wm
    shape = mirror.SHAPES[name]
    model = wm.Encoder(shape["image_size"], shape["latent"], shape["channels"])
    sd = model.state_dict()
    cfg = wm.world_config_from_state_dict(sd, image_size=shape["image_size"], hidden=shape["hidden"])
    assert (cfg.image_size, tuple(cfg.channels), cfg.latent, cfg.hidden) == (shape["image_size"], shape["channels"], shape["latent"], shape["hidden"])
    assert (cfg.throttle, cfg.steer_scale, cfg.skip_crashed) == (100.0, 5.0, 0)
    # torch's parameters() order with the BatchNorm layers (folded) and fc_logvar (not read) taken out
    want = [(n, tuple(p.shape)) for n, p in model.named_parameters() if not n.startswith("fc_logvar") and n.split(".")[1] not in ("3", "6", "9")]
    assert [(n, tuple(s)) for n, a, s in capi.world_layout(cfg)] == want == [(n, tuple(s)) for n, a, s in mirror.layout(shape)]
    assert [a for n, a, s in capi.world_layout(cfg)] == [a for n, a, s in mirror.layout(shape)]
    assert capi.world_num_params(cfg) == mirror.num_params(shape)
    assert capi.world_num_params(cfg)[1] == sum(p.numel() for p in _controller(shape))
    # without running statistics to fold (a fresh module: mean 0, variance 1, affine 1 and 0) only 1 / sqrt(1 + eps) is folded in
    flat = wm.world_params_from_state_dict(sd, image_size=shape["image_size"])
    assert flat.dtype == torch.float32 and flat.numel() == capi.world_num_params(cfg)[0]
    first = capi.world_layout(cfg)[0]
    assert torch.equal(flat[:int(np.prod(first[2]))], sd["net.0.weight"].reshape(-1))


def _controller(shape):
    i, h = shape["latent"] + 2, shape["hidden"]
    return list(torch.nn.Sequential(torch.nn.Linear(i, h), torch.nn.Linear(h, h // 2), torch.nn.Linear(h // 2, 1)).parameters())


BAD_SHAPES = [dict(image_size=0), dict(image_size=8), dict(image_size=24), dict(image_size=144), dict(channels=(8, 128, 256, 512)),
              dict(channels=(64, 128, 256, 528)), dict(channels=(64, 72, 256, 512)), dict(channels=(64, 128, 0, 512)), dict(latent=0),
              dict(latent=8), dict(latent=40), dict(latent=144), dict(hidden=0), dict(hidden=3), dict(hidden=66), dict(hidden=-2)]


def test_shape_limits(capi):
    L = capi.load()
    ref = mirror.SHAPES["tiny"]
    enc, ctrl = mirror.draw_params(ref, 0, 1)
    frames, rot, out = np.zeros((1, 16, 16, 4), np.uint8), np.zeros(1, f32), np.empty(1, f32)
    plan = (C.c_int32 * 12)()

    def act_host(cfg):
        return L.okenv_world_act_host(C.byref(cfg), capi.ptr(enc), capi.ptr(ctrl), 1, capi.ptr(frames), capi.ptr(rot), None, None, None,
                                      capi.ptr(out), None, None, None)

    for bad in BAD_SHAPES:
        cfg = config(capi, "reference", **bad)
        assert capi.world_lds_bytes(cfg) == 0 and capi.world_workspace_bytes(cfg, 4) == 0, bad
        assert L.okenv_world_plan(C.byref(cfg), plan) == INVALID, bad
        assert b"okenv_world_plan: shape outside the limits" in L.okenv_last_error(None)
        assert act_host(cfg) == INVALID and b"okenv_world_act_host: shape outside the limits" in L.okenv_last_error(None), bad
    # F = 512 x 8 x 8 = 32768 is the limit itself; the same frame with 528 channels is refused above by the channel limit, and there is
    # no shape inside the other limits with more features
    assert capi.world_lds_bytes(config(capi, "reference")) > 0
    for bad in (dict(throttle=float("nan")), dict(throttle=float("inf")), dict(steer_scale=float("-inf")), dict(steer_scale=float("nan"))):
        assert act_host(config(capi, "tiny", **bad)) == INVALID and b"throttle / steer_scale must be finite" in L.okenv_last_error(None), bad
    for bad in (2, -1):
        assert act_host(config(capi, "tiny", skip_crashed=bad)) == INVALID and b"skip_crashed must be 0 or 1" in L.okenv_last_error(None)
    assert act_host(config(capi, "tiny")) == 0
    # the corners of the limits are inside
    for good in (dict(image_size=16, channels=(16, 16, 16, 16), latent=16, hidden=2),
                 dict(image_size=128, channels=(512, 512, 512, 512), latent=128, hidden=64)):
        assert capi.world_lds_bytes(config(capi, good)) > 0, good


def test_plan_functions_equal_the_mirror(capi):
    L = capi.load()
    for name, cfg in mirror.SHAPES.items():
        assert capi.world_lds_bytes(config(capi, name)) == mirror.lds_bytes(cfg) <= capi.WORLD_LDS_BUDGET, name
        assert capi.world_plan(config(capi, name)) == mirror.plan(cfg) == mirror.PATHS[name], name
        for n in (1, 33):
            assert capi.world_workspace_bytes(config(capi, name), n) == 4 * mirror.workspace_words(cfg, n), (name, n)
    layers = [p for paths in mirror.PATHS.values() for p in paths[1:]]
    # every path of the conv kernel is among the shapes: one and several workgroups of columns, one and several K blocks per tap, a
    # last block as long as the others and a shorter one, blocks of 16, 32, 48 and 64 channels
    assert {p[0] for p in layers} >= {1, 2, 4} and {p[1] for p in layers} >= {1, 2, 3, 8} and {p[2] for p in layers} == {16, 32, 48, 64}
    assert any(p[1] > 1 and p[2] < 64 for p in layers)
    assert (mirror.COLS, mirror.CHUNK) == (capi.WORLD_COLS, capi.WORLD_CHUNK)
    plan = (C.c_int32 * 12)()
    assert L.okenv_world_plan(None, plan) == INVALID and L.okenv_world_plan(C.byref(config(capi, "tiny")), None) == INVALID
    assert L.okenv_world_lds_bytes(None) == 0 and L.okenv_world_workspace_bytes(None, 4) == 0
    assert capi.world_workspace_bytes(config(capi, "tiny"), 0) == 0


def test_skip_crashed_leaves_crashed_agents_alone(capi):
    cfg = mirror.SHAPES["tiny"]
    enc, ctrl = mirror.draw_params(cfg, 5, 4)
    frames, rot = mirror.draw_frames(16, 5, n=4), np.array([0.0, 90.0, -45.0, 300.0], f32)
    crashed = np.array([0, 1, 0, 7], np.uint8)
    plain = capi.world_act_host(config(capi, "tiny"), enc, ctrl, frames, rot)
    every = capi.world_act_host(config(capi, "tiny"), enc, ctrl, frames, rot, crashed)
    assert np.array_equal(every["alive"], [1, 0, 1, 0]) and np.array_equal(plain["alive"], [1, 1, 1, 1])
    for k in ("mu", "state", "out", "throttle", "steer"):
        assert same(every[k], plain[k])
    into = {k: np.full_like(v, 77) for k, v in plain.items()}
    got = capi.world_act_host(config(capi, "tiny", skip_crashed=1), enc, ctrl, frames, rot, crashed, into=into)
    for k, v in plain.items():
        assert same(got[k][[0, 2]], v[[0, 2]]) and (got[k][[1, 3]] == 77).all(), k
    L = capi.load()
    c = config(capi, "tiny")
    args = [capi.ptr(enc), capi.ptr(ctrl), 4, capi.ptr(frames), capi.ptr(rot)] + [None] * 7
    assert L.okenv_world_act_host(C.byref(c), *args) == 0  # every output may be NULL
    for at in (0, 1, 3, 4):
        bad = list(args)
        bad[at] = None
        assert L.okenv_world_act_host(C.byref(c), *bad) == INVALID, at
    assert L.okenv_world_act_host(C.byref(c), *(args[:2] + [-1] + args[3:])) == INVALID
    assert L.okenv_world_act_host(None, *args) == INVALID


@pytest.mark.parametrize("pattern", P.HOST_PATTERNS)
def test_skip_crashed_host_entry_at_a_population_pattern(capi, pattern):
    """The host entry with skip_crashed at 129 agents under a crashed pattern of tests/_population_cases.py, which
    tests/test_gpu_image_populations.py takes as the truth for the device: against the mirror, bit for bit as everywhere in this file,
    at the agents on both sides of every wave's edge (the mirror is slow); for every other agent what needs no mirror."""
    cfg = mirror.SHAPES["tiny"]
    N, Z = P.HOST_N, cfg["latent"]
    enc, ctrl = mirror.draw_params(cfg, 6, N)
    frames = mirror.draw_frames(16, 6, n=N)
    rot = np.random.default_rng(6).uniform(-180.0, 180.0, N).astype(f32)
    crashed = P.crashed(pattern, N)
    into = dict(mu=np.full((N, Z), 77, f32), state=np.full((N, Z + 2), 77, f32), out=np.full(N, 77, f32), throttle=np.full(N, 77, f32),
                steer=np.full(N, 77, f32), alive=np.full(N, 77, np.uint8))
    got = capi.world_act_host(config(capi, "tiny", skip_crashed=1), enc, ctrl, frames, rot, crashed, into=into)
    at = [a for a in P.HOST_MIRRORED if not crashed[a]]
    assert len(at) >= 3 and any(crashed[a] for a in P.HOST_MIRRORED)
    want = mirror.act(cfg, enc, ctrl[at], frames[at], rot[at])
    for k in ("mu", "state", "out", "throttle", "steer"):
        assert same(got[k][at], want[k]), "%s %s: differ by up to %.3g" % (pattern, k, float(np.abs(got[k][at] - want[k]).max()))
    gone = crashed != 0
    for k, v in got.items():
        assert (v[gone] == 77).all(), k  # crashed agents untouched
        assert np.isfinite(v[~gone]).all() and (v[~gone].reshape(int((~gone).sum()), -1) != 77).all(), k
    assert (got["alive"][~gone] == 1).all() and len(set(got["out"][~gone].tolist())) == int((~gone).sum())


@pytest.mark.parametrize("track", ["Austin", "Silverstone"])
def test_score_host_equals_the_oracle(ok, capi, track):
    """1 - oracle_lane_center_distance accumulated over probe points along and beside the track, with crashed and timed-out entries."""
    t = ok.Track(track)
    rng = np.random.default_rng(len(track))
    n, steps = 64, 5
    fitness, want = np.zeros(n, f32), np.zeros(n, f32)
    saw = set()
    for step in range(steps):
        at = rng.integers(0, t.P, n)
        x = (t.x[at] + rng.uniform(-30, 30, n)).astype(f32)
        y = (t.y[at] + rng.uniform(-30, 30, n)).astype(f32)
        crashed = (rng.uniform(size=n) < 0.3).astype(np.uint8)
        timed_out = ((rng.uniform(size=n) < 0.5) & (crashed != 0)).astype(np.uint8)
        d = np.zeros(n, f32)
        O.lib().oracle_lane_center_distance(t.x, t.y, t.wl, t.wr, t.P, x, y, n, d)
        want = mirror.score(want, d, crashed, timed_out)
        fitness = capi.world_score_host(t.x, t.y, t.wl, t.wr, x, y, crashed, timed_out, fitness)
        assert same(fitness, want), step
        saw |= set(zip(crashed.tolist(), timed_out.tolist()))
    assert saw == {(0, 0), (1, 0), (1, 1)} and (fitness == 0).any() and (fitness > 1).any()
    L = capi.load()
    z, b = np.zeros(1, f32), np.zeros(1, np.uint8)
    assert L.okenv_world_score_host(capi.ptr(t.x), capi.ptr(t.y), capi.ptr(t.wl), capi.ptr(t.wr), 0, 1, capi.ptr(z), capi.ptr(z), capi.ptr(b),
                                    capi.ptr(b), capi.ptr(z)) == INVALID
    assert L.okenv_world_score_host(None, capi.ptr(t.y), capi.ptr(t.wl), capi.ptr(t.wr), t.P, 1, capi.ptr(z), capi.ptr(z), capi.ptr(b),
                                    capi.ptr(b), capi.ptr(z)) == INVALID


def randomised_encoder(shape, seed):
    """An Encoder in eval mode at torch's default init with randomised running statistics and affine terms."""
    from openkitchen_amd import worldmodel as wm
    torch.manual_seed(seed)
    model = wm.Encoder(shape["image_size"], shape["latent"], shape["channels"]).eval()
    with torch.no_grad():
        for m in model.net:
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 2.0)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return model


def fold_deviations(capi, name, frames, mu_of):
    """(|mu_of(...) - float64 module|, |fp32 module on the CPU - float64 module|, largest |mu|, the float64 module's mu, the fp32
    module's) for the shape's randomised encoder."""
    import copy
    from openkitchen_amd import worldmodel as wm
    shape = mirror.SHAPES[name]
    model = randomised_encoder(shape, 11)
    sd = model.state_dict()
    x = wm.frames_to_input(torch.from_numpy(frames))
    with torch.no_grad():
        exact = copy.deepcopy(model).double()(x.double())[0].numpy()
        single = model(x)[0].numpy()
    cfg = wm.world_config_from_state_dict(sd, image_size=shape["image_size"], hidden=shape["hidden"])
    got = mu_of(cfg, wm.world_params_from_state_dict(sd, image_size=shape["image_size"]).numpy())
    return float(np.abs(got.astype(np.float64) - exact).max()), float(np.abs(single.astype(np.float64) - exact).max()), float(np.abs(exact).max()), exact, single


@pytest.mark.parametrize("name", FOLD_SHAPES)
def test_fold_and_host_entry_against_the_float64_module(capi, name):
    shape = mirror.SHAPES[name]
    n = 2
    frames = mirror.draw_frames(shape["image_size"], 21, n)
    ctrl = np.zeros((n, mirror.num_params(shape)[1]), f32)
    host, single, scale, _, _ = fold_deviations(capi, name, frames, lambda cfg, enc: capi.world_act_host(cfg, enc, ctrl, frames, np.zeros(n, f32))["mu"])
    print("%s: host entry %.3e, fp32 module %.3e from the float64 module; mu up to %.3f" % (name, host, single, scale))
    assert scale > 0.05 and single > 0
    assert host <= 4 * single, (host, single)


def test_host_forward_stays_inside_its_work_space(tmp_path):
    """The host forward and score as a stand-alone program under AddressSanitizer and UBSan (tests/cpp/world_host_check.cpp), on frames,
    parameter vectors and work spaces of exactly their sizes."""
    exe = str(tmp_path / "world_host_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "world_host_check.cpp")], check=True)
    shapes = [(s["image_size"],) + tuple(s["channels"]) + (s["latent"], s["hidden"]) for n, s in mirror.SHAPES.items() if n in ("tiny", "odd", "ragged")]
    shapes += [(128, 16, 16, 16, 16, 128, 64),  # the largest frame, latent and controller on the narrowest layers
               (24, 16, 16, 16, 16, 16, 2)]     # a frame that is no multiple of 16
    args = [str(v) for shape in shapes[:-1] for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(shapes) - 1)], r.stdout[-1000:] + r.stderr[-4000:]
    r = subprocess.run([exe] + [str(v) for v in shapes[-1]], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2  # the program refuses a shape outside the limits
