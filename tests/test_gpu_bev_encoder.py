"""The flow driver's image encoder on the device (okenv_bev_*; openkitchen_amd/csrc/ok_bev.h): the three kernels bit-equal to the host
entry that shares their rule, on every path the two conv kernels have (the side of their output tile, okenv_bev_tiles), with frames of
random bytes and frames the camera rendered, crashed agents among them; parameters from host and device pointers; the order of calls;
step + camera + encode + act captured in a graph; the embedding against the PyTorch module."""
import ctypes as C

import numpy as np
import pytest
import torch

import _bev_encoder_numpy as mirror

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, STATE = -1, -5
RAYS = 7
# Random-action steps on Austin after which the population holds crashed and alive agents alike (tests/test_gpu_flow.py's recipe)
RANDOM_CHUNKS, RANDOM_CHUNK_STEPS = 8, 25
# |device embedding - fp32 PyTorch module on the GPU|, reference shape, 33 agents, the same weights (torch's default init, seed 0) and
# frames (the camera's and random bytes alternating): torch sums its convolutions in its library's order and divides the pool its own
# way.  The largest difference measured on the MI355X on the first run was 9.69e-8, with embeddings up to 0.111 in size; the bound is
# 4 x that.  (examples/flow_racer.py's trained encoder at 32 x 32 frames, conditions up to 0.34 in size, is held to the same bound in
# tests/test_gpu_bev_encoder_example.py: 2.09e-7 and 1.79e-7 were measured there.)
TORCH_MEASURED = 9.69e-8
TORCH_TOL = 4 * TORCH_MEASURED


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def fan(R):
    return np.linspace(-90.0, 90.0, R).astype(f32)


def driven_population(gpu, N, S):
    """N agents on Austin after random driving, the camera at S x S."""
    from openkitchen_amd.torch_env import VectorEnvironment
    venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=False, seed=3)
    venv.enable_camera(width=S, height=S, fmt="rgba")
    dev = venv.env
    dev.reset_random(None, 1, 5, 0, 0)
    dev.step(1)
    for i in range(RANDOM_CHUNKS):
        dev.rollout_random(RANDOM_CHUNK_STEPS, 11, 0, RANDOM_CHUNK_STEPS * i)
    return venv


def last_error(dev):
    return dev._L.okenv_last_error(dev._h)


def encode_case(gpu, name, N):
    capi = gpu.capi
    shape = mirror.SHAPES[name]
    cfg = capi.bev_config(**shape)
    S, E = shape["image_size"], shape["embed_dim"]
    # the path the shape was chosen for is the one its plan selects
    assert capi.bev_tiles(cfg) == mirror.PATHS[name] and capi.bev_lds_bytes(cfg) == mirror.lds_bytes(shape) <= capi.BEV_LDS_BUDGET
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
    want = {kind: capi.bev_encode_host(cfg, params, t.cpu().numpy()) for kind, t in frames.items()}
    assert not same(want["camera"], want["random"]) and all(np.abs(w).max() > 0 and np.isfinite(w).all() for w in want.values())
    out = torch.full((N, E), -7.0, device="cuda")
    nbytes = N * S * S * 4

    # the order of calls
    assert L.okenv_bev_encode(h, capi.ptr(rendered), nbytes, capi.ptr(out)) == STATE and b"okenv_bev_encode: call okenv_bev_create first" in last_error(dev)
    n = C.c_int32()
    assert L.okenv_bev_num_params(h, C.byref(n)) == STATE and L.okenv_bev_set_params(h, capi.ptr(params)) == STATE
    assert L.okenv_bev_num_params(h, None) == INVALID and L.okenv_bev_set_params(h, None) == INVALID
    for bad in (dict(image_size=12), dict(image_size=136), dict(kernel=(5, 4, 3)), dict(channels=(32, 8, 16)), dict(channels=(16, 16, 144)), dict(embed_dim=520)):
        assert L.okenv_bev_create(h, C.byref(capi.bev_config(**dict(shape, **bad)))) == INVALID, bad
        assert b"okenv_bev_create: shape outside the limits" in last_error(dev)
    assert L.okenv_bev_create(h, None) == INVALID and L.okenv_bev_create(None, C.byref(cfg)) == INVALID
    assert L.okenv_bev_encode(h, capi.ptr(rendered), nbytes, capi.ptr(out)) == STATE
    assert dev.bev_create(cfg) == params.size == mirror.num_params(shape)
    assert L.okenv_bev_encode(h, capi.ptr(rendered), nbytes, capi.ptr(out)) == STATE
    assert b"okenv_bev_encode: call okenv_bev_set_params first (the encoder needs its parameters)" in last_error(dev)
    assert L.okenv_bev_get_params(h, capi.ptr(np.empty_like(params))) == STATE
    dev.bev_set_params(params)  # from a host pointer
    assert same(dev.bev_get_params(), params)
    for args in ((None, nbytes, capi.ptr(out)), (capi.ptr(rendered), nbytes, None), (capi.ptr(rendered), nbytes - 4, capi.ptr(out)),
                 (capi.ptr(rendered), nbytes + S * S * 4, capi.ptr(out)), (capi.ptr(rendered), 0, capi.ptr(out))):
        assert L.okenv_bev_encode(h, *args) == INVALID, args
        assert b"okenv_bev_encode: " in last_error(dev)
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == -7.0  # nothing was launched by a refused call

    def check(label):
        for kind, t in frames.items():
            out.fill_(-7.0)
            dev.bev_encode(t, out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert same(got, want[kind]), "%s, %s frames: %d of %d differ, by up to %.3g" % (
                label, kind, int((got != want[kind]).sum()), got.size, float(np.abs(got - want[kind]).max()))

    check("host pointer")
    # a second create, with another shape and back, forgets the parameters
    other = "tiny" if name != "tiny" else "odd"
    dev.bev_create(capi.bev_config(**mirror.SHAPES[other]))
    assert L.okenv_bev_encode(h, capi.ptr(rendered), nbytes, capi.ptr(out)) == STATE
    dev.bev_create(cfg)
    assert L.okenv_bev_encode(h, capi.ptr(rendered), nbytes, capi.ptr(out)) == STATE
    # from a device pointer, other values first so that the hand-over shows
    zeros, on_device = np.zeros_like(params), torch.from_numpy(params).cuda()  # (alive until the copies have run)
    dev.bev_set_params(zeros)
    dev.bev_set_params(on_device)
    check("device pointer")
    got = torch.empty(params.size, device="cuda")
    dev.bev_get_params(got)
    assert same(got.cpu().numpy(), params)
    # the binding's hand-over and its own checks
    venv.enable_bev_encoder(cfg, params)
    with pytest.raises(ValueError):
        venv.bev_encode(rendered[:, :-1])
    with pytest.raises(ValueError):
        venv.bev_encode(rendered, out=out[:, :-1])
    assert same(venv.bev_encode(frames["random"]).cpu().numpy(), want["random"])
    venv.close()


@pytest.mark.parametrize("N", [1, 2, 17])
@pytest.mark.parametrize("name", ["tiny", "odd"])
def test_encode_device_equals_host(gpu, name, N):
    """Layer sides below a tile (8 / 4 / 2: tiles of 4) and not a multiple of one (20 / 10 / 5: tiles of 8, partial at every edge), one
    16-column tile, k = 5 on every layer; one frame, two, and seventeen with crashed agents among them."""
    assert mirror.reaches(name, N)
    encode_case(gpu, name, N)


def test_encode_device_equals_host_reference_shape(gpu):
    assert mirror.reaches("reference")
    encode_case(gpu, "reference", 3)


def test_encode_device_equals_host_mixed_shape(gpu):
    """Mixed kernels, the widest channel count against the narrowest, the widest projection, sides 12 / 6 / 3: tiles of 8, then of 4."""
    assert mirror.reaches("mixed")
    encode_case(gpu, "mixed", 5)


def test_encode_device_equals_host_front_tile_limited_by_the_lds(gpu):
    """The one path the four shapes above do not reach: the front kernel on tiles of 4 because 128 channels with k1 = 5 leave no room for
    a tile of 8, the back kernel on tiles of 8."""
    assert mirror.reaches("front4_back8")
    encode_case(gpu, "front4_back8", 2)


def path_case(gpu, name):
    """A shape that exists for one path of the two conv kernels, at the frames its predicate names: the predicate first (mirror.REACHES,
    restated from the kernels' prose and held to the source in tests/test_bev_encoder_rule.py), so that an edit to the shape cannot
    leave the path unnoticed."""
    N = mirror.REACHES[name][0]
    assert name in mirror.NEW_SHAPES and mirror.reaches(name, N), (name, mirror.geometry(mirror.SHAPES[name], N))
    encode_case(gpu, name, N)


def test_encode_device_equals_host_front_tiles_of_4_with_a_partial_one(gpu):
    """The front kernel at T = 4 (one row tile a unit of layer 1) with a partial last tile: layer 1 is 10 wide, three tiles a side of
    4, 4 and 2, the last one's stores guarded at the right and bottom edge; tile (1, 1) reads no padding.  The back kernel on one
    tile of 8 of which 5 x 5 are stored."""
    path_case(gpu, "front4_ragged")


def test_encode_device_equals_host_back_tiles_of_4_several_a_frame(gpu):
    """The back kernel at T = 4 -- okConv<OkConvWalk, 1, 4, true>, one row tile a unit -- with several tiles a frame: 128 channels
    under k2 = 5 leave no room for a tile of 8 (186 656 B), layer 2 is 5 wide, so two tiles a side of 4 and 1: origins other than
    (0, 0), a patch that starts inside the image (at row 6 of layer 1's 10), the guarded store at the right and bottom edge.  Three
    frames: twelve workgroups, the frame of one its index over four."""
    path_case(gpu, "back4_tiles")


def test_encode_device_equals_host_tiles_of_8_with_a_partial_last(gpu):
    """Both kernels at T = 8 with a partial tile behind full ones: the front 3 x 3 tiles of 8, 8 and 4, of which tile (1, 1) reads no
    padding in its patch of layer 0's output or of the frame; the back 2 x 2 tiles of 8 and 2."""
    path_case(gpu, "back8_ragged")


def test_encode_device_equals_host_tiles_of_4_in_both_kernels(gpu):
    """Both kernels at T = 4 with several tiles: 128 channels under k = 5 in front of layer 1 and of layer 2; 3 x 3 tiles in front (4,
    4, 2), 2 x 2 behind (4, 1); k0 = 5, seven groups of layer 0 with three filler taps; 32 channels pooled, 48 projected."""
    path_case(gpu, "both4_tiles")


def flow_policy(seed, frame_size):
    """The reference's policy at torch's default init, and what the device takes from it."""
    from openkitchen_amd import flow
    torch.manual_seed(seed)
    model = flow.ConditionalFlowMatchingPolicy().cuda().eval()
    sd = model.state_dict()
    return model, (flow.flow_config_from_state_dict(sd, steps=4), flow.flow_params_from_state_dict(sd)), (
        flow.bev_config_from_state_dict(sd, image_size=frame_size), flow.bev_params_from_state_dict(sd))


def test_graph_of_step_camera_encode_act_equals_eager(gpu):
    """step + camera + bev_encode + flow_act captured once (a linear graph) and replayed 4 times, against the same 4 iterations launched
    one by one on a second environment: the actions, the state and cond, bit for bit."""
    from openkitchen_amd.torch_env import VectorEnvironment
    N, S = 64, 32
    _, (flow_cfg, flow_params), (bev_cfg, bev_params) = flow_policy(0, S)
    venvs, conds, frames = [], [], []
    for _ in range(2):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=True, seed=3, agent_base=50,
                                 randomize_lane=True, randomize_heading=True)
        venv.enable_camera(width=S, height=S, fmt="rgba")
        venv.enable_flow_policy(flow_cfg, flow_params)
        venv.enable_bev_encoder(bev_cfg, bev_params)
        venv.reset()
        venvs.append(venv)
        conds.append(torch.zeros((N, bev_cfg.embed_dim), device="cuda"))
        frames.append(torch.zeros((N, S, S, 4), dtype=torch.uint8, device="cuda"))
    eager, graphed = venvs
    torch.cuda.synchronize()

    def iteration(i):
        venvs[i].step()
        venvs[i].camera(out=frames[i])
        venvs[i].bev_encode(frames[i], out=conds[i])
        venvs[i].flow_act(conds[i])

    graph = graphed.capture(lambda: iteration(1), warmup=0)
    seen = []
    for _ in range(4):
        iteration(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(conds[0], conds[1]) and torch.equal(frames[0], frames[1])
        assert torch.equal(eager.throttle, graphed.throttle) and torch.equal(eager.steering, graphed.steering)
        seen.append(conds[1].clone())
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    assert float(eager.throttle.abs().max()) > 0 and float(conds[0].abs().max()) > 0
    for a, b in zip(seen, seen[1:]):
        assert not torch.equal(a, b)  # the agents moved: another frame, another condition
    for venv in venvs:
        venv.close()


def test_drive_with_the_device_encoder(gpu):
    """flow.drive(encoder="device") eagerly and in graph chunks reaches the same state; a camera of another size is refused in words."""
    from openkitchen_amd import flow
    from openkitchen_amd.torch_env import VectorEnvironment
    N, S = 64, 32
    model, (flow_cfg, flow_params), (bev_cfg, bev_params) = flow_policy(1, S)
    ends = []
    for chunk in (0, 4):
        venv = VectorEnvironment(gpu.track_path("Austin"), N, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=True, seed=5, randomize_lane=True)
        venv.enable_camera(width=S, height=S, fmt="rgba")
        venv.enable_flow_policy(flow_cfg, flow_params)
        venv.enable_bev_encoder(bev_cfg, bev_params)
        assert flow.drive(venv, None, 8, graph_chunk=chunk, encoder="device") == 8
        torch.cuda.synchronize()
        ends.append({name: getattr(venv, name).clone() for name in VectorEnvironment.FIELDS})
        if chunk:
            assert list(venv._flow_graphs) == [(4, "device")]
            assert flow.drive(venv, model, 4, graph_chunk=4) == 4  # the torch encoder's chunk is keyed apart
            assert len(venv._flow_graphs) == 2
        else:
            venv.enable_camera(width=S + 8, height=S + 8, fmt="rgba")
            with pytest.raises(ValueError, match="needs the camera at the encoder's size"):
                flow.drive(venv, None, 1, encoder="device")
        venv.close()
    assert float(ends[0]["throttle"].abs().max()) > 0
    for name in VectorEnvironment.FIELDS:
        assert torch.equal(ends[0][name], ends[1][name]), name


def test_device_embedding_against_the_pytorch_module(gpu):
    """Reference shape, 33 agents: the fp32 module on the GPU with the same weights and frames.  See TORCH_MEASURED."""
    from openkitchen_amd import flow
    N, S = 33, 128
    model, _, (bev_cfg, bev_params) = flow_policy(0, S)
    venv = driven_population(gpu, N, S)
    venv.enable_bev_encoder(bev_cfg, bev_params)
    frames = venv.camera()
    torch.manual_seed(2)
    frames[1::2] = torch.randint(0, 256, (N // 2, S, S, 4), dtype=torch.uint8, device="cuda")
    got = venv.bev_encode(frames)
    with torch.no_grad():
        want = model.bev_encoder(flow.frames_to_input(frames))
    torch.cuda.synchronize()
    diff = float((got - want).abs().max())
    print("device vs fp32 PyTorch encoder: %.3e (largest |embedding| %.3f)" % (diff, float(want.abs().max())))
    assert float(want.abs().max()) > 0.01
    assert diff <= TORCH_TOL
    venv.close()
