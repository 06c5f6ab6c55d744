"""The image transformer driver on the device (okenv_vit_*; openkitchen_amd/csrc/ok_vit.h): the attention kernel alone and the whole
act bit-equal to the host entries that share their rule, at every shape of tests/_vit_numpy.py, on frames the camera rendered and on
random bytes, with crashed agents among them; populations that fill less than a row tile, share a tile between agents and take several
passes; the paths a shape and a pass select in the launch geometry (mirror.PATHS, mirror.geometry); parameters from host and device
pointers; the order of calls and the refusals; step + camera + act captured in a graph; the output against the PyTorch module."""
import ctypes as C

import numpy as np
import pytest
import torch

import _vit_numpy as mirror
from test_gpu_bev_encoder import INVALID, RAYS, STATE, driven_population, fan, last_error, same

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = -7.0
# |device output - fp32 dino.ViT on the GPU| of the head's output, the same weights (torch's default init, TORCH_SEED) and frames (the
# camera's and random bytes alternating), 4 agents: torch sums its products and its softmax in its library's order and evaluates GELU
# and LayerNorm its own way.  Measured on the MI355X on the first run: see TORCH_MEASURED; the bound is 4 x that.
TORCH_SEED = 0
TORCH_MEASURED = {"tiny": 1.490e-08, "reference_depth": 8.754e-08}  # (the embeddings: 5.07e-7 and 4.11e-6)
SHAPE_LIMITS = ("shape outside the limits (patch 4, 8 or 16; image_size a multiple of patch with at most 1024 tokens; dim a multiple of 16 up to 768; "
                "dim / heads a multiple of 16 up to 64; depth 1 .. 12; dim_feedforward a multiple of 16 up to 4 dim; head_hidden1/2 multiples of 16 up "
                "to 2048)")


def attend_case(gpu, T, dh, heads, seqs):
    """Uniform data and scores spread over 2^+-20, where most of a softmax row underflows: the device against the host entry bit for
    bit, the host entry against the float64 mirror."""
    capi = gpu.capi
    rng = np.random.default_rng(1000 * T + dh)
    uniform = rng.uniform(-1.0, 1.0, (seqs, T, 3 * heads * dh)).astype(f32)
    spread = uniform.copy()
    spread[..., :2 * heads * dh] *= np.exp2(rng.uniform(-20.0, 20.0, (seqs, T, 1))).astype(f32)  # q and k rows scaled, v as it was
    for label, qkv in (("uniform", uniform), ("spread", spread)):
        want = capi.debug_vit_attend(qkv, heads)
        got = capi.debug_vit_attend(qkv, heads, device=0)
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert same(got, want), "%s: %d of %d differ, by up to %.3g" % (label, int((got != want).sum()), want.size, float(np.abs(got - want).max()))
        assert np.abs(want - mirror.attend(qkv, heads)).max() <= 1e-4 * max(1.0, float(np.abs(want).max()))
    if T >= 15:  # the spread case does underflow: in a quarter of its softmax rows most weights are below fp32's smallest subnormal
        q, k = spread.astype(np.float64).reshape(seqs, T, 3, heads, dh).transpose(2, 0, 3, 1, 4)[:2]
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(float(dh))
        under = (s - s.max(axis=-1, keepdims=True) < -104.0).mean(axis=-1)
        assert float((under > 0.5).mean()) > 0.25


@pytest.mark.parametrize("dh", [16, 64])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 785])
def test_attend_device_equals_host(gpu, T, dh):
    """One key; one short of a tile; a tile; one key and one query past it; the reference's row of 49 key tiles and one key.  Two heads
    and two sequences."""
    attend_case(gpu, T, dh, 2, 2)


@pytest.mark.parametrize("T,dh,heads,seqs", [(17, 32, 3, 3), (40, 48, 3, 3), (1024, 64, 1, 1), (1009, 48, 1, 1)])
def test_attend_device_equals_host_other_heads(gpu, T, dh, heads, seqs):
    """The context phase on two and on three waves, heads that start at multiples of 32 and of 48, score chains of two and three
    groups, the unit decode with three heads and three sequences of two and three query tiles; the largest plan (64 key tiles, no dead
    key, 16 x (68 + 1028) x 4 = 70 144 B of LDS); 1009 keys at dh 48: 15 dead keys in the last tile."""
    dead = -(-T // 16) * 16 - T
    assert (dh // 16, dead) == {17: (2, 15), 40: (3, 8), 1024: (4, 0), 1009: (3, 15)}[T]
    assert 4 * mirror.QUERIES * (dh + T + dead + 2 * mirror.PAD) <= mirror.LDS_BUDGET
    attend_case(gpu, T, dh, heads, seqs)


def act_case(gpu, name, N, agents_per_pass=0, lifecycle=False):
    capi = gpu.capi
    shape = mirror.SHAPES[name]
    cfg = capi.vit_config(throttle=80.0, steer_scale=7.0, agents_per_pass=agents_per_pass, **shape)
    S, D = shape["image_size"], shape["dim"]
    assert capi.vit_tokens(cfg) == mirror.TOKENS[name] and capi.vit_lds_bytes(cfg) == mirror.lds_bytes(shape) <= capi.VIT_LDS_BUDGET
    assert (name in mirror.PATHS) == (name in mirror.NEW_SHAPES) and (name not in mirror.PATHS or (mirror.PATHS[name][0] == N and mirror.reaches(name))), name
    params = mirror.random_params(capi, cfg, np.random.default_rng(N), scale=2.0)
    venv = driven_population(gpu, N, S)
    dev, L, h = venv.env, venv.env._L, venv.env._h
    rendered = venv.camera()
    crashed = (np.arange(N) % 3 == 1).astype(np.uint8)
    dev.set(capi.F_CRASHED, crashed)
    crashed = dev.get(capi.F_CRASHED)
    if N >= 2:
        assert 0 < int((crashed != 0).sum()) < N, "the population must hold crashed and alive agents"
    torch.manual_seed(N)
    frames = {"camera": rendered, "random": torch.randint(0, 256, (N, S, S, 4), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    assert int(rendered[..., :3].max()) > int(rendered[..., :3].min()), "the camera drew nothing"
    want = {kind: capi.vit_act_host(cfg, params, t.cpu().numpy(), crashed) for kind, t in frames.items()}
    assert not same(want["camera"]["output"], want["random"]["output"])
    assert all(np.abs(w["output"]).max() > 0 and np.isfinite(w["embedding"]).all() and np.array_equal(w["alive"], crashed == 0) for w in want.values())
    rec = {"action": torch.empty((N, 2), device="cuda"), "output": torch.empty(N, device="cuda"), "embedding": torch.empty((N, D), device="cuda"),
           "alive": torch.empty(N, dtype=torch.uint8, device="cuda")}
    members = tuple(rec)
    nbytes = N * S * S * 4

    def fill():
        for k in ("action", "output", "embedding"):
            rec[k].fill_(SENTINEL)
        rec["alive"].fill_(9)
        venv.throttle.fill_(SENTINEL), venv.steering.fill_(SENTINEL)

    def untouched():
        torch.cuda.synchronize()
        return (all(float(t.min()) == float(t.max()) == SENTINEL for t in (rec["action"], rec["output"], rec["embedding"], venv.throttle, venv.steering))
                and int(rec["alive"].min()) == int(rec["alive"].max()) == 9)

    record = capi.fill_pointers(capi.OkenvVitRecord(), rec, "record")
    fill()
    if lifecycle:
        # the order of calls
        assert L.okenv_vit_act(h, capi.ptr(rendered), nbytes, C.byref(record)) == STATE and b"okenv_vit_act: call okenv_vit_create first" in last_error(dev)
        assert L.okenv_vit_act(None, capi.ptr(rendered), nbytes, C.byref(record)) == INVALID
        n = C.c_int32()
        assert L.okenv_vit_num_params(h, C.byref(n)) == STATE and L.okenv_vit_set_params(h, capi.ptr(params)) == STATE
        assert L.okenv_vit_num_params(h, None) == INVALID and L.okenv_vit_set_params(h, None) == INVALID
        assert L.okenv_vit_num_params(None, C.byref(n)) == INVALID and L.okenv_vit_get_params(None, capi.ptr(params)) == INVALID
        for bad in (dict(patch=2), dict(image_size=20), dict(image_size=256, patch=8), dict(dim=24), dict(dim=784), dict(dim=32, heads=4), dict(dim=128, heads=1),
                    dict(depth=0), dict(depth=13), dict(dim_feedforward=72), dict(dim_feedforward=4 * D + 16), dict(head_hidden1=8), dict(head_hidden2=2064)):
            assert L.okenv_vit_create(h, C.byref(capi.vit_config(**dict(shape, **bad)))) == INVALID, bad
            assert last_error(dev) == ("okenv_vit_create: " + SHAPE_LIMITS).encode(), bad
        for bad, text in ((dict(head_hidden1=2048, head_hidden2=2048), "the kernels' LDS (okenv_vit_lds_bytes) does not fit 160 KB"),
                          (dict(std=(0.2, 0.0, 0.2)), "mean must be finite, std finite and > 0"), (dict(mean=(float("nan"), 0.0, 0.0)), "mean must be finite, std finite and > 0"),
                          (dict(ln_eps=0.0), "ln_eps must be finite and > 0"), (dict(steer_scale=float("inf")), "throttle must be finite, steer_scale finite and >= 0"),
                          (dict(agents_per_pass=-1), "agents_per_pass and workspace_bytes must not be negative")):
            assert L.okenv_vit_create(h, C.byref(capi.vit_config(**dict(shape, **bad)))) == INVALID, bad
            assert last_error(dev) == ("okenv_vit_create: " + text).encode(), bad
        assert L.okenv_vit_create(h, None) == INVALID and L.okenv_vit_create(None, C.byref(cfg)) == INVALID
        assert L.okenv_vit_act(h, capi.ptr(rendered), nbytes, C.byref(record)) == STATE
    assert dev.vit_create(cfg) == params.size == capi.vit_num_params(cfg)
    if lifecycle:
        assert L.okenv_vit_act(h, capi.ptr(rendered), nbytes, C.byref(record)) == STATE
        assert b"okenv_vit_act: call okenv_vit_set_params first (the policy needs its parameters)" in last_error(dev)
        assert L.okenv_vit_get_params(h, capi.ptr(np.empty_like(params))) == STATE
    dev.vit_set_params(params)  # from a host pointer
    if lifecycle:
        assert same(dev.vit_get_params(), params)
        for args, text in (((None, nbytes), b"NULL argument"), ((capi.ptr(rendered), nbytes - 4), b"frame_bytes is not num_agents x image_size x image_size x 4"),
                           ((capi.ptr(rendered), nbytes + S * S * 4), b"frame_bytes is not"), ((capi.ptr(rendered), 0), b"frame_bytes is not"),
                           ((capi.ptr(rendered.data_ptr() + 1), nbytes), b"frames must be 4-byte aligned")):
            assert L.okenv_vit_act(h, *args, C.byref(record)) == INVALID, args
            assert b"okenv_vit_act: " + text in last_error(dev)
        assert L.okenv_vit_get_params(h, None) == INVALID
        assert untouched()  # nothing was launched by a refused call

    def check(label, members=members):
        for kind, t in frames.items():
            fill()
            dev.vit_act(t, {k: rec[k] for k in members} if members is not None else None)
            torch.cuda.synchronize()
            w = want[kind]
            got = {k: rec[k].cpu().numpy() for k in rec}
            got.update(throttle=venv.throttle.cpu().numpy(), steer=venv.steering.cpu().numpy())
            for k in ("throttle", "steer"):
                assert same(got[k], w[k]), "%s, %s frames, %s: %d of %d differ, by up to %.3g" % (
                    label, kind, k, int((got[k] != w[k]).sum()), N, float(np.abs(got[k] - w[k]).max()))
            assert np.array_equal(w["throttle"], np.full(N, 80.0, f32)) and np.array_equal(w["steer"], np.clip(w["output"] * f32(7.0), -7.0, 7.0))
            for k in ("output", "embedding", "alive"):
                if k in (members or ()):
                    assert same(got[k], w[k]), "%s, %s frames, %s: %d of %d differ, by up to %.3g" % (
                        label, kind, k, int((got[k] != w[k]).sum()), w[k].size, float(np.abs(got[k].astype(f32) - w[k].astype(f32)).max()))
                else:
                    assert float(got[k].min()) == float(got[k].max()) in (SENTINEL, 9.0), (label, kind, k)
            if "action" in (members or ()):
                assert same(got["action"][:, 0], w["throttle"]) and same(got["action"][:, 1], w["steer"]), (label, kind)
            else:
                assert float(got["action"].min()) == float(got["action"].max()) == SENTINEL

    check("host pointer")
    if lifecycle:
        check("no record", None)
        for member in members:  # a record with single NULL members
            check("record without " + member, tuple(k for k in members if k != member))
        # a second create, with another shape and back, forgets the parameters
        dev.vit_create(capi.vit_config(**mirror.SHAPES["ten_tokens"]))
        assert L.okenv_vit_act(h, capi.ptr(rendered), nbytes, None) == STATE
        dev.vit_create(cfg)
        assert L.okenv_vit_act(h, capi.ptr(rendered), nbytes, None) == STATE
        # from a device pointer, other values first so that the hand-over shows
        zeros, on_device = np.zeros_like(params), torch.from_numpy(params).cuda()  # (alive until the copies have run)
        dev.vit_set_params(zeros)
        dev.vit_set_params(on_device)
        check("device pointer")
        got = torch.empty(params.size, device="cuda")
        dev.vit_get_params(got)
        assert same(got.cpu().numpy(), params)
        # the binding's hand-over and its own checks
        venv.enable_vit_policy(cfg, params)
        with pytest.raises(ValueError):
            venv.vit_act(frames=rendered[:, :-1])
        with pytest.raises(ValueError):
            venv.vit_act(frames=rendered.to(torch.float32))
        fill()
        venv.vit_act({"output": rec["output"]}, frames=frames["random"])
        torch.cuda.synchronize()
        assert same(rec["output"].cpu().numpy(), want["random"]["output"]) and same(venv.steering.cpu().numpy(), want["random"]["steer"])
    venv.close()


@pytest.mark.parametrize("N", [1, 3, 4, 33])
def test_act_device_equals_host_tiny(gpu, N):
    """T 5.  5 rows: less than a row tile; 15 rows: three agents in one partial tile; 20 rows: a full tile that ends inside the fourth
    agent and a partial one; 165 rows: three workgroups of the linear kernel, three of the final kernel."""
    act_case(gpu, "tiny", N, lifecycle=N == 3)


def test_act_device_equals_host_in_three_passes(gpu):
    """agents_per_pass 2 with 5 agents: two full passes and one of a single agent."""
    assert mirror.agents_per_pass(mirror.SHAPES["tiny"], 5, 2) == 2
    act_case(gpu, "tiny", 5, agents_per_pass=2)


@pytest.mark.parametrize("N,per_pass", [(40, 24), (41, 20)])
def test_act_device_equals_host_in_later_passes(gpu, N, per_pass):
    """40 agents in passes of 24: the first pass has a full and a half workgroup of the final kernel, the second starts at a0 = 24 with
    one full workgroup.  41 in passes of 20: the second pass starts at a0 = 20 and has a second workgroup itself, which reads the
    pass's rows from b0 = 16 on and stores at a0 + b0; the third is a single agent at a0 = 40."""
    shape = mirror.SHAPES["tiny"]
    assert mirror.agents_per_pass(shape, N, per_pass) == per_pass
    blocks = [mirror.geometry(shape, min(per_pass, N - a0))["final_blocks"] for a0 in range(0, N, per_pass)]
    assert blocks == {(40, 24): [2, 1], (41, 20): [2, 2, 1]}[N, per_pass]
    act_case(gpu, "tiny", N, agents_per_pass=per_pass)


@pytest.mark.parametrize("name", [n for n in mirror.SHAPES if n != "tiny" and n not in mirror.NEW_SHAPES])
def test_act_device_equals_host_other_shapes(gpu, name):
    act_case(gpu, name, 2)


@pytest.mark.parametrize("name", mirror.NEW_SHAPES)
def test_act_device_equals_host_paths(gpu, name):
    """The shapes that select what the seven above never do (mirror.PATHS names it and the population it needs, act_case asserts it
    first): the context phase on two and three waves; patch 16; every linear launch with several workgroups in x and y, short last
    column workgroups and dead upper waves; the head 2048 wide at 17 agents; a second hidden layer wider than the first; the attention
    kernel launched from the act above 64 KB of dynamic LDS."""
    if name == "most_tokens":
        assert mirror.geometry(mirror.SHAPES[name], 1)["attend_lds"] > 65536
    act_case(gpu, name, mirror.PATHS[name][0])


def test_workspace_bytes_sets_the_pass(gpu):
    """workspace_bytes for one agent and a half: passes of one agent; the result is the single pass's."""
    capi = gpu.capi
    shape = mirror.SHAPES["ten_tokens"]
    per_agent = 4 * mirror.agent_floats(shape)
    assert mirror.agents_per_pass(shape, 3, 0, per_agent * 3 // 2) == 1 and mirror.agents_per_pass(shape, 3, 0, 1) == 1 and mirror.agents_per_pass(shape, 3) == 3
    S = shape["image_size"]
    outs = []
    venv = driven_population(gpu, 3, S)
    frames = venv.camera()
    for room in (0, per_agent * 3 // 2):
        cfg = capi.vit_config(workspace_bytes=room, **shape)
        params = mirror.random_params(capi, cfg, np.random.default_rng(5), scale=2.0)
        venv.enable_vit_policy(cfg, params)
        out = torch.empty(3, device="cuda")
        venv.vit_act({"output": out}, frames=frames)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert same(outs[0], outs[1]) and same(outs[0], capi.vit_act_host(cfg, params, frames.cpu().numpy())["output"])
    venv.close()


def vit_policy(seed, name):
    """dino.ViT at torch's default init, and what the device takes from it."""
    from openkitchen_amd import dino
    shape = mirror.SHAPES[name]
    torch.manual_seed(seed)
    model = dino.ViT(**shape).cuda().eval()
    sd = model.state_dict()
    return model, dino.vit_config_from_state_dict(sd, heads=shape["heads"]), dino.vit_params_from_state_dict(sd, heads=shape["heads"])


def test_graph_of_step_camera_act_equals_eager(gpu):
    """step + camera + vit_act captured once (a linear graph) on the tiny shape at 64 agents with auto_reset and replayed 4 times,
    against the same 4 iterations launched one by one on a second environment: the record, the frames and every field, bit for bit."""
    from openkitchen_amd.torch_env import VectorEnvironment
    N, shape = 64, mirror.SHAPES["tiny"]
    S, D = shape["image_size"], shape["dim"]
    cfg = gpu.capi.vit_config(agents_per_pass=48, **shape)  # (two passes inside the capture)
    params = mirror.random_params(gpu.capi, cfg, np.random.default_rng(9), scale=2.0)
    venvs, recs, frames = [], [], []
    for _ in range(2):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=True, seed=3, agent_base=50,
                                 randomize_lane=True, randomize_heading=True)
        venv.enable_camera(width=S, height=S, fmt="rgba")
        venv.enable_vit_policy(cfg, params)
        venv.reset()
        venvs.append(venv)
        recs.append({"action": torch.zeros((N, 2), device="cuda"), "output": torch.zeros(N, device="cuda"), "embedding": torch.zeros((N, D), device="cuda"),
                     "alive": torch.zeros(N, dtype=torch.uint8, device="cuda")})
        frames.append(torch.zeros((N, S, S, 4), dtype=torch.uint8, device="cuda"))
    eager, graphed = venvs
    torch.cuda.synchronize()

    def iteration(i):
        venvs[i].step()
        venvs[i].camera(out=frames[i])
        venvs[i].vit_act(recs[i], frames=frames[i])

    graph = graphed.capture(lambda: iteration(1), warmup=0)
    seen = []
    for _ in range(4):
        iteration(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(frames[0], frames[1]) and all(torch.equal(recs[0][k], recs[1][k]) for k in recs[0])
        assert torch.equal(eager.throttle, graphed.throttle) and torch.equal(eager.steering, graphed.steering)
        assert torch.equal(recs[1]["action"][:, 1], graphed.steering)
        seen.append(recs[1]["output"].clone())
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    assert float(eager.throttle.min()) == float(eager.throttle.max()) == 100.0 and float(eager.steering.abs().max()) > 0
    for a, b in zip(seen, seen[1:]):
        assert not torch.equal(a, b)  # the agents moved: another frame, another output
    for venv in venvs:
        venv.close()


def test_drive_with_the_device_policy(gpu):
    """dino.drive(policy="device") eagerly and in graph chunks reaches the same state; a camera of another size is refused in words."""
    from openkitchen_amd import dino
    from openkitchen_amd.torch_env import VectorEnvironment
    N, S = 32, 16
    model, cfg, params = vit_policy(1, "tiny")
    ends = []
    for chunk in (0, 4):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=True, seed=5, randomize_lane=True)
        venv.enable_camera(width=S, height=S, fmt="rgba")
        venv.enable_vit_policy(cfg, params)
        assert dino.drive(venv, None, 8, graph_chunk=chunk, policy="device") == 8
        torch.cuda.synchronize()
        ends.append({name: getattr(venv, name).clone() for name in VectorEnvironment.FIELDS})
        if chunk:
            assert list(venv._vit_graphs) == [(4, "device")]
            assert dino.drive(venv, model, 4, graph_chunk=4) == 4  # the PyTorch forward's chunk is kept apart
            assert len(venv._dino_graphs) == 1
        else:
            venv.enable_camera(width=S + 8, height=S + 8, fmt="rgba")
            with pytest.raises(ValueError, match="needs the camera at the policy's size"):
                dino.drive(venv, None, 1, policy="device")
        venv.close()
    assert float(ends[0]["throttle"].max()) == 100.0 and float(ends[0]["steering"].abs().max()) > 0
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(ends[0][name], ends[1][name]), name


@pytest.mark.parametrize("name", ["tiny", "reference_depth"])
def test_device_output_against_the_pytorch_module(gpu, name):
    """4 agents: the fp32 module on the GPU with the same weights and frames.  See TORCH_MEASURED."""
    from openkitchen_amd import dino
    N, S = 4, mirror.SHAPES[name]["image_size"]
    model, cfg, params = vit_policy(TORCH_SEED, name)
    venv = driven_population(gpu, N, S)
    venv.enable_vit_policy(cfg, params)
    frames = venv.camera()
    torch.manual_seed(2)
    frames[1::2] = torch.randint(0, 256, (N // 2, S, S, 4), dtype=torch.uint8, device="cuda")
    got, emb = torch.empty(N, device="cuda"), torch.empty((N, cfg.dim), device="cuda")
    venv.vit_act({"output": got, "embedding": emb}, frames=frames)
    allow_tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        with torch.no_grad():
            x = dino.frames_to_input(frames)
            want, want_emb = model(x)[:, 0], model.embed(x)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = allow_tf32
    torch.cuda.synchronize()
    diff, diff_emb = float((got - want).abs().max()), float((emb - want_emb).abs().max())
    print("%s: device vs fp32 dino.ViT: output %.3e (largest |o| %.3f), embedding %.3e" % (name, diff, float(want.abs().max()), diff_emb))
    assert float(want.abs().max()) > 0.01
    assert diff <= 4 * TORCH_MEASURED[name]
    venv.close()
