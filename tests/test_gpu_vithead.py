"""The image transformer driver's training on the device (okenv_vit_embed, okenv_vit_head_*; openkitchen_amd/csrc/ok_vithead.h): the
head's update and eval bit-equal to the host entries that share their rule at every head shape and launch geometry of
tests/_vithead_numpy.py, the embed against the host act's embedding over several passes and a partial one and in passes of a whole
population (one, two and three workgroups of its last kernel), the act after an update, the order of calls, and a second
okenv_vit_create dropping the learner."""
import ctypes as C

import numpy as np
import pytest
import torch

import _vit_numpy as V_
import _vithead_numpy as N_
from test_gpu_bev_encoder import INVALID, RAYS, STATE, driven_population, fan, last_error, same

pytestmark = pytest.mark.gpu
f32 = np.float32
_ENVS = {}


def head_env(gpu, shape):
    """A population of two with a backbone as small as the head's width allows (two tokens, one block), one per head shape."""
    if shape not in _ENVS:
        from openkitchen_amd.torch_env import VectorEnvironment
        D, H1, H2 = shape
        cfg = gpu.capi.vit_config(image_size=8, patch=8, dim=D, heads=D // 64 if D % 64 == 0 else D // 16, depth=1, dim_feedforward=16,
                                  head_hidden1=H1, head_hidden2=H2, steer_scale=N_.STEER_SCALE)
        venv = VectorEnvironment(gpu.track_path("Austin"), 2, num_rays=RAYS, ray_angles_deg=fan(RAYS), auto_reset=False, seed=3)
        _ENVS[shape] = (venv, cfg, V_.random_params(gpu.capi, cfg, np.random.default_rng(shape[0])))
    return _ENVS[shape]


def on_device(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@pytest.mark.parametrize("geometry", N_.GEOMETRIES, ids=[g[0] for g in N_.GEOMETRIES])
@pytest.mark.parametrize("shape", N_.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_update_and_eval_equal_the_host_entries(gpu, shape, geometry):
    capi = gpu.capi
    venv, cfg, backbone = head_env(gpu, shape)
    st, emb, steer, B, epochs, order = N_.case(shape, geometry)
    st = N_.fresh_state(st["params"])  # (the device's moments start from zero; every geometry but one takes several steps)
    at = capi.vit_head_offset(cfg)
    full = backbone.copy()
    full[at:] = st["params"]
    hp = capi.vit_head_params(**N_.HP)
    want, out = capi.vit_head_update_host(hp, shape, cfg.steer_scale, st, emb, steer, B, epochs, order)
    want_eval = capi.vit_head_eval_host(hp, shape, cfg.steer_scale, want["params"], emb, steer, B)
    venv.enable_vit_policy(cfg, full)
    venv.enable_vit_head_learner(**N_.HP)
    d_emb, d_steer, d_order = on_device(emb), on_device(steer), on_device(order, torch.int32)
    grad = torch.full((st["params"].size,), -7.0, device="cuda")
    before = venv.vit_head_eval(d_emb, d_steer, B)
    loss = venv.vit_head_update(d_emb, d_steer, B, epochs, d_order, grad=grad)
    after = venv.vit_head_eval(d_emb, d_steer, B)
    got = venv.env.vit_head_state()
    params = venv.env.vit_get_params()
    assert got["t"] == want["t"] == epochs * -(-emb.shape[0] // B)
    for k, a, b in (("loss", loss.cpu().numpy(), out["loss"]), ("grad", grad.cpu().numpy(), out["grad"]), ("head", got["params"], want["params"]),
                    ("m", got["m"], want["m"]), ("v", got["v"], want["v"]), ("eval after", after.cpu().numpy(), want_eval)):
        assert same(a, b), "%s: %d of %d differ, by up to %.3g" % (k, int((a != b).sum()), b.size, float(np.abs(a - b).max()))
    assert same(params[:at], backbone[:at]) and same(params[at:], want["params"])
    # the eval before the update: the first minibatch's loss of a sequential first epoch is update's own
    want_before = capi.vit_head_eval_host(hp, shape, cfg.steer_scale, st["params"], emb, steer, B)
    assert same(before.cpu().numpy(), want_before)
    if order is None:
        assert same(before.cpu().numpy()[:1], out["loss"][:1])


def embed_case(gpu, N=3, agents_per_pass=2, name="tiny"):
    capi = gpu.capi
    shape = V_.SHAPES[name]
    cfg = capi.vit_config(agents_per_pass=agents_per_pass, **shape)
    venv = driven_population(gpu, N, shape["image_size"])
    params = V_.random_params(capi, cfg, np.random.default_rng(N), scale=2.0)
    return venv, cfg, params


def test_embed_equals_the_host_over_several_passes(gpu):
    """Three agents and two per pass: m = 1 is one partial pass, 7 three passes and a partial one, 33 sixteen and one; m = N equals the
    act's record; no agent field moves."""
    capi = gpu.capi
    venv, cfg, params = embed_case(gpu)
    dev, S, D, N = venv.env, cfg.image_size, cfg.dim, 3
    venv.enable_vit_policy(cfg, params)
    venv.throttle.fill_(-7.0), venv.steering.fill_(-7.0)
    torch.cuda.synchronize()
    snap = dev.snapshot()
    torch.manual_seed(5)
    for m in (1, 7, 33):
        frames = torch.randint(0, 256, (m, S, S, 4), dtype=torch.uint8, device="cuda")
        out = torch.full((m + 1, D), -7.0, device="cuda")
        got = venv.vit_embed(frames, out=out[:m])
        torch.cuda.synchronize()
        want = capi.vit_act_host(cfg, params, frames.cpu().numpy())["embedding"]
        assert got.data_ptr() == out.data_ptr() and same(got.cpu().numpy(), want), m
        assert float(out[m].min()) == float(out[m].max()) == -7.0 and np.isfinite(want).all() and np.abs(want).max() > 0
    after = dev.snapshot()
    assert set(after) == set(snap) and all(same(after[k], snap[k]) for k in snap), "the embed moved an agent field"
    frames = venv.camera()
    rec = {"embedding": torch.empty((N, D), device="cuda")}
    venv.vit_act(rec, frames=frames)
    assert same(venv.vit_embed(frames).cpu().numpy(), rec["embedding"].cpu().numpy())
    assert float(venv.throttle.min()) == cfg.throttle  # (the act did write them)


@pytest.mark.parametrize("name,N,ms", [("tiny", 40, (1, 31, 32, 33, 40, 41, 100)), ("ten_tokens", 35, (71,)), ("tiny", 70, (65, 70))],
                         ids=["tiny-40", "ten_tokens-35", "tiny-70"])
def test_embed_equals_the_host_in_passes_of_the_population(gpu, name, N, ms):
    """The default pass holds the whole population.  tiny at 40 agents: m = 1 and 31 fill part of okVitEmbedKernel's first workgroup,
    32 all of it, 33 and 40 a second one (one row; a wave of eight), 41 is a pass of 40 and one of 1, 100 two of 40 and one of 20.
    ten_tokens at 35 agents, two blocks: m = 71 is passes of 35, 35 and 1.  tiny at 70 agents: m = 65 and 70 reach a third workgroup,
    the first whose rows no other workgroup's stride could cover (one row; six)."""
    capi = gpu.capi
    venv, cfg, params = embed_case(gpu, N, 0, name)
    S, D = cfg.image_size, cfg.dim
    shape = V_.SHAPES[name]
    assert V_.agents_per_pass(shape, N) == N
    counts = {m: [min(N, m - a0) for a0 in range(0, m, N)] for m in ms}
    blocks = {m: [V_.geometry(shape, c)["embed_blocks"] for c in counts[m]] for m in ms}
    if N == 40:
        assert [counts[m] for m in ms] == [[1], [31], [32], [33], [40], [40, 1], [40, 40, 20]]
        assert [blocks[m] for m in ms] == [[1], [1], [1], [2], [2], [2, 1], [2, 2, 1]]
    elif N == 70:
        assert [counts[m] for m in ms] == [[65], [70]] and [blocks[m] for m in ms] == [[3], [3]]
    else:
        assert counts[71] == [35, 35, 1] and blocks[71] == [2, 2, 1] and cfg.depth == 2
    venv.enable_vit_policy(cfg, params)
    torch.manual_seed(N)
    for m in ms:
        frames = torch.randint(0, 256, (m, S, S, 4), dtype=torch.uint8, device="cuda")
        out = torch.full((m + 1, D), -7.0, device="cuda")
        got = venv.vit_embed(frames, out=out[:m])
        torch.cuda.synchronize()
        want = capi.vit_act_host(cfg, params, frames.cpu().numpy())["embedding"]
        got = got.cpu().numpy()
        assert same(got, want), "m %d: %d of %d rows differ, the first %d" % (m, int((got != want).any(axis=1).sum()), m, int((got != want).any(axis=1).argmax()))
        assert float(out[m].min()) == float(out[m].max()) == -7.0 and np.isfinite(want).all() and np.abs(want).max() > 0
        assert len({row.tobytes() for row in want}) == m  # (every frame has an embedding of its own: a row taken from another frame shows)
    venv.close()


def test_act_after_update_acts_with_the_new_head(gpu):
    capi = gpu.capi
    venv, cfg, params = embed_case(gpu)
    dev, S, D, N = venv.env, cfg.image_size, cfg.dim, 3
    shape = (cfg.dim, cfg.head_hidden1, cfg.head_hidden2)
    venv.enable_vit_policy(cfg, params)
    venv.enable_vit_head_learner(**N_.HP)
    torch.manual_seed(6)
    frames = torch.randint(0, 256, (9, S, S, 4), dtype=torch.uint8, device="cuda")
    steer = torch.linspace(-12.0, 12.0, 9, device="cuda")
    emb = venv.vit_embed(frames)
    rec = {"output": torch.empty(N, device="cuda")}
    venv.vit_act(rec, frames=frames[:N])
    old = rec["output"].cpu().numpy()
    venv.vit_head_update(emb, steer, 4, 3)
    venv.vit_act(rec, frames=frames[:N])  # the next act on the stream
    at = capi.vit_head_offset(cfg)
    host_emb = capi.vit_act_host(cfg, params, frames.cpu().numpy())["embedding"]
    new, _ = capi.vit_head_update_host(capi.vit_head_params(**N_.HP), shape, cfg.steer_scale, N_.fresh_state(params[at:]), host_emb, steer.cpu().numpy(), 4, 3)
    updated = params.copy()
    updated[at:] = new["params"]
    want = capi.vit_act_host(cfg, updated, frames[:N].cpu().numpy())
    got = rec["output"].cpu().numpy()
    assert same(got, want["output"]) and not same(got, old) and same(venv.steering.cpu().numpy(), want["steer"])
    assert same(dev.vit_get_params(), updated) and new["t"] == 9


def test_order_of_calls_and_a_second_create(gpu):
    capi = gpu.capi
    venv, cfg, params = embed_case(gpu)
    dev, L, h = venv.env, venv.env._L, venv.env._h
    S, D = cfg.image_size, cfg.dim
    frames = torch.zeros((4, S, S, 4), dtype=torch.uint8, device="cuda")
    emb, steer, loss = torch.zeros((4, D), device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda")
    hp = capi.vit_head_params(**N_.HP)
    st = capi.OkenvVitHeadState()
    embed = lambda m=4, nbytes=4 * S * S * 4, f=frames, e=emb: L.okenv_vit_embed(h, capi.ptr(f), m, nbytes, capi.ptr(e))  # noqa: E731
    update = lambda: L.okenv_vit_head_update(h, capi.ptr(emb), capi.ptr(steer), 4, 2, 1, None, None)  # noqa: E731
    # before okenv_vit_create
    assert embed() == STATE and b"okenv_vit_embed: call okenv_vit_create first" in last_error(dev)
    assert L.okenv_vit_head_learner_create(h, C.byref(hp)) == STATE and b"okenv_vit_create, okenv_vit_set_params" in last_error(dev)
    assert update() == STATE and b"okenv_vit_head_update: call okenv_vit_head_learner_create first" in last_error(dev)
    dev.vit_create(cfg)
    assert embed() == STATE and b"okenv_vit_embed: call okenv_vit_set_params first" in last_error(dev)
    assert L.okenv_vit_head_learner_create(h, C.byref(hp)) == STATE
    dev.vit_set_params(params)
    # before the learner's create
    assert update() == STATE
    assert L.okenv_vit_head_eval(h, capi.ptr(emb), capi.ptr(steer), 4, 2, capi.ptr(loss)) == STATE and b"okenv_vit_head_eval: call okenv_vit_head_learner_create first" in last_error(dev)
    assert L.okenv_vit_head_learner_get_state(h, C.byref(st)) == STATE and L.okenv_vit_head_learner_reset(h) == STATE
    # the embed's own refusals
    for call, text in ((lambda: embed(m=0, nbytes=0), b"m must be at least 1"), (lambda: embed(nbytes=4 * S * S * 4 - 4), b"frame_bytes"),
                       (lambda: embed(f=None), b"NULL argument"), (lambda: embed(e=None), b"NULL argument"),
                       (lambda: embed(f=frames.data_ptr() + 1), b"4-byte aligned")):
        assert call() == INVALID and b"okenv_vit_embed: " in last_error(dev) and text in last_error(dev)
    assert embed() == 0
    assert L.okenv_vit_head_learner_create(h, C.byref(capi.vit_head_params(lr=0.0))) == INVALID and b"lr must be positive" in last_error(dev)
    assert L.okenv_vit_head_learner_create(h, None) == INVALID
    assert update() == STATE  # (a refused create attaches nothing)
    dev.vit_head_learner_create(hp)
    assert L.okenv_vit_head_update(h, capi.ptr(emb), None, 4, 2, 1, None, None) == INVALID and b"NULL argument" in last_error(dev)
    assert L.okenv_vit_head_update(h, capi.ptr(emb), capi.ptr(steer), 4, 0, 1, None, None) == INVALID and b"at least 1" in last_error(dev)
    assert L.okenv_vit_head_eval(h, capi.ptr(emb), capi.ptr(steer), 4, 2, None) == INVALID
    assert update() == 0 and dev.vit_head_state()["t"] == 2
    dev.vit_head_learner_reset()
    state = dev.vit_head_state()
    assert state["t"] == 0 and not state["m"].any() and not state["v"].any()
    # a second okenv_vit_create drops the learner
    assert update() == 0
    dev.vit_create(cfg)
    dev.vit_set_params(params)
    assert update() == STATE and b"okenv_vit_head_learner_create first" in last_error(dev)
    dev.vit_head_learner_create(hp)
    assert update() == 0 and dev.vit_head_state()["t"] == 2
    # a steer_scale of 0 cannot be trained against
    dev.vit_create(capi.vit_config(**dict(V_.SHAPES["tiny"], steer_scale=0.0)))
    dev.vit_set_params(params)
    assert L.okenv_vit_head_learner_create(h, C.byref(hp)) == INVALID and b"steer_scale" in last_error(dev)
