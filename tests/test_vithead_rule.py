"""The rule of the image transformer driver's head update (include/okenv_vithead.h) without a GPU: the host entries against the numpy
restatement bit for bit at every head shape and launch geometry, the persistence of Adam's state, constructed cases of the label, the
weight and ReLU's derivative, the first step against autograd in float64, the forward against the act's, the refusals and the LDS plan."""
import ctypes as C

import numpy as np
import pytest

import _vithead_numpy as N_

f32 = np.float32
U = N_.U
INVALID, STATE = -1, -5
bits = N_.bits


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def hp_struct(capi, **over):
    return capi.vit_head_params(**dict(N_.HP, **over))


def host_update(capi, shape, st, emb, steer, B, epochs=1, order=None, **over):
    return capi.vit_head_update_host(hp_struct(capi, **over), shape, N_.STEER_SCALE, st, emb, steer, B, epochs, order)


def same_state(a, b):
    return a["t"] == b["t"] and all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("params", "m", "v"))


# ---- the host entry equals the numpy restatement bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("geometry", N_.GEOMETRIES, ids=[g[0] for g in N_.GEOMETRIES])
@pytest.mark.parametrize("shape", N_.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_entry_equals_numpy(capi, shape, geometry):
    st, emb, steer, B, epochs, order = N_.case(shape, geometry)
    new, out = host_update(capi, shape, st, emb, steer, B, epochs, order)
    want, losses, grad = N_.update(N_.HP, shape, N_.STEER_SCALE, st, emb, steer, B, epochs, order)
    assert new["t"] == want["t"] == st["t"] + epochs * -(-emb.shape[0] // B)
    assert np.array_equal(bits(out["loss"]), bits(losses)), "losses"
    assert np.array_equal(bits(out["grad"]), bits(grad)), "last gradient"
    assert same_state(new, want)
    assert np.abs(grad).max() > 1e-4 and not np.array_equal(bits(new["params"]), bits(st["params"]))


@pytest.mark.parametrize("shape", N_.SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_of_one_epoch_equal_one_call_of_two(capi, shape):
    """t, m and v persist across calls."""
    st, emb, steer, B, epochs, order = N_.case(shape, N_.GEOMETRIES[4])
    assert epochs == 2
    both, out = host_update(capi, shape, st, emb, steer, B, 2, order)
    first, out1 = host_update(capi, shape, st, emb, steer, B, 1, order[:1])
    second, out2 = host_update(capi, shape, first, emb, steer, B, 1, order[1:])
    assert same_state(both, second) and both["t"] == st["t"] + 6
    assert np.array_equal(bits(out["loss"]), bits(np.concatenate([out1["loss"], out2["loss"]])))
    assert np.array_equal(bits(out["grad"]), bits(out2["grad"]))


# ---- constructed cases -----------------------------------------------------------------------------------------------------------------

SMALL = (16, 16, 16)


def one_sample(capi, head, emb, steer, **over):
    """One minibatch of one sample from a fresh state: (new state, loss, grad)."""
    new, out = host_update(capi, SMALL, N_.fresh_state(head), np.asarray(emb, f32)[None, :], np.asarray([steer], f32), 1, **over)
    return new, float(out["loss"][0]), out["grad"]


def test_label_exactly_at_the_threshold_takes_weight_one(capi):
    """threshold 0.25 and steer 2.5 = 0.25 x 10: |y| > threshold is false, so the weight is 1; the next float32 up takes 5."""
    rng = np.random.default_rng(5)
    head, emb = N_.random_head(SMALL, rng), rng.standard_normal(16).astype(f32)
    o = float(N_.positions(head, SMALL, emb[None, :], np.zeros(1, f32), N_.STEER_SCALE, 5.0, 0.25)["o"][0])
    for steer, weight in ((2.5, 1.0), (-2.5, 1.0), (float(np.nextafter(f32(2.5), f32(3))), 5.0)):
        _, loss, _ = one_sample(capi, head, emb, steer, threshold=0.25)
        y = f32(f32(steer) / f32(10))
        assert loss == float(f32(weight) * f32(f32(f32(o) - y) * f32(f32(o) - y))), (steer, weight)


def test_steering_beyond_the_scale_is_clamped(capi):
    rng = np.random.default_rng(6)
    head, emb = N_.random_head(SMALL, rng), rng.standard_normal(16).astype(f32)
    for beyond, edge in ((37.0, 10.0), (-1e6, -10.0)):
        a, b = one_sample(capi, head, emb, beyond), one_sample(capi, head, emb, edge)
        assert a[1] == b[1] and np.array_equal(bits(a[2]), bits(b[2])) and same_state(a[0], b[0])
    y, _ = N_.label_weight(np.array([37.0, -1e6, 3.0], f32), 10.0, 5.0, 0.1)
    assert list(y) == [1.0, -1.0, f32(3.0) / f32(10.0)]


def test_zero_pre_activation_passes_no_gradient(capi):
    """Unit 0 of hidden layer 1 has s1 = 0 exactly (a zero row and a zero bias) and a weight into layer 2; unit 1 has s1 > 0.  ReLU's
    derivative at 0 is 0: row 0 of W1 and b1[0] get no gradient, and no step."""
    D, H1, H2 = SMALL
    rng = np.random.default_rng(7)
    head = N_.random_head(SMALL, rng)
    W1, b1, W2, b2, W3, b3 = N_.split(head, *SMALL)  # views
    W1[0], b1[0] = 0.0, 0.0
    W1[1], b1[1] = 0.0, 0.5
    W2[:, 0], W2[:, 1] = 1.0, 1.0
    b2[:], W3[0, :] = 0.25, 0.5
    emb = rng.standard_normal(D).astype(f32)
    new, loss, grad = one_sample(capi, head, emb, 4.0)
    gW1, gb1 = N_.split(grad, *SMALL)[:2]
    assert loss > 0 and (gW1[0] == 0).all() and gb1[0] == 0 and gb1[1] != 0
    assert np.array_equal(bits(N_.split(new["params"], *SMALL)[0][0]), bits(W1[0])) and N_.split(new["params"], *SMALL)[1][1] != b1[1]


def test_dead_unit_keeps_the_adam_state_of_a_zero_gradient(capi):
    """Unit 3 of hidden layer 1 is dead for every sample of the minibatch (bias -100): its row's gradient is +0.0f, and m, v and the
    parameters of the row move exactly as ok_learn_adam moves them for g = 0 from the moments they had."""
    D, H1, H2 = SMALL
    st, emb, steer, B, _, _ = N_.case(SMALL, N_.GEOMETRIES[0])
    W1, b1 = N_.split(st["params"], *SMALL)[:2]
    b1[3] = -100.0
    new, out = host_update(capi, SMALL, st, emb[:5], steer[:5], 5)
    row = slice(3 * D, 4 * D)
    assert (bits(out["grad"][row]) == 0).all() and bits(out["grad"][H1 * D + 3: H1 * D + 4])[0] == 0
    p, m, v = N_.adam(st["params"][row], st["m"][row], st["v"][row], np.zeros(D, f32), st["t"] + 1, **{k: N_.HP[k] for k in ("lr", "beta1", "beta2", "eps")})
    assert np.array_equal(bits(new["params"][row]), bits(p)) and np.array_equal(bits(new["m"][row]), bits(m)) and np.array_equal(bits(new["v"][row]), bits(v))
    assert np.abs(out["grad"]).max() > 0


@pytest.mark.parametrize("shape", N_.SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_eval_changes_nothing_and_equals_the_loss_before_the_step(capi, shape):
    st, emb, steer, B, _, _ = N_.case(shape, N_.GEOMETRIES[2])
    head = st["params"].copy()
    loss = capi.vit_head_eval_host(hp_struct(capi), shape, N_.STEER_SCALE, head, emb, steer, B)
    assert np.array_equal(bits(head), bits(st["params"])) and loss.shape == (2,)
    assert np.array_equal(bits(loss), bits(N_.evaluate(N_.HP, shape, N_.STEER_SCALE, head, emb, steer, B)))
    # the first minibatch's loss is what update reports before its step; so is the second's, evaluated on its own with the same parameters
    _, out = host_update(capi, shape, st, emb[:B], steer[:B], B)
    assert bits(out["loss"])[0] == bits(loss)[0]
    _, out = host_update(capi, shape, st, emb[B:], steer[B:], B)
    assert bits(out["loss"])[0] == bits(loss)[1]


# ---- against autograd in float64 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", N_.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_step_against_torch_float64(capi, shape):
    """dino.weighted_mse of dino.PolicyHead against steering / steer_scale, autograd in float64; torch's own float32 run must meet the
    same bound.  The bound: mlp_bounds / grad_bounds.  The label y = steer / steer_scale is one rounded division: e_y = u |y| (the clamp
    is exact), and no |y| lies within 1e-6 of the threshold (asserted), so both precisions weigh alike.  err = o - y: e_err = e_o + e_y +
    u |err|.  Seed 2 w err (the 2 and the w exact up to one rounding each product): E = 2 w e_err + 2 u |seed|.  Term w err^2:
    2 w |err| e_err + 2 u term.  The sums are divided by the count (one more u)."""
    import torch
    from openkitchen_amd import dino
    D, H1, H2 = shape
    M = 150
    rng = np.random.default_rng(D + H1)
    head = N_.random_head(shape, rng)
    emb, steer = N_.random_data(shape, M, rng)
    y32, w = N_.label_weight(steer, N_.STEER_SCALE, N_.HP["weight"], N_.HP["threshold"])
    assert (np.abs(np.abs(y32.astype(np.float64)) - N_.HP["threshold"]) > 1e-6).all() and (w == 5).any() and (w == 1).any()
    _, out = host_update(capi, shape, N_.fresh_state(head), emb, steer, M)
    pieces64 = [a.astype(np.float64) for a in N_.split(head, *shape)]
    results = {}
    for dtype in (torch.float64, torch.float32):
        model = dino.PolicyHead(D, H1, H2).to(dtype)
        with torch.no_grad():
            for p, a in zip(model.parameters(), pieces64):
                p.copy_(torch.tensor(a, dtype=dtype))
        label = (torch.tensor(steer).to(dtype)[:, None] / N_.STEER_SCALE).clamp(-1.0, 1.0)
        loss = dino.weighted_mse(model(torch.tensor(emb).to(dtype)), label, N_.HP["weight"], N_.HP["threshold"])
        loss.backward()
        results[dtype] = (torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().numpy(), float(loss.detach()))
    want, loss64 = results[torch.float64]
    x = emb.astype(np.float64)
    fwd, errs = N_.mlp_bounds(pieces64, x)
    y = np.clip(steer.astype(np.float64) / N_.STEER_SCALE, -1, 1)[:, None]
    w64 = w.astype(np.float64)[:, None]
    err = fwd[4] - y
    e_err = errs[2] + U * np.abs(y) + U * np.abs(err)
    dz = 2 * w64 * err
    E_dz = 2 * w64 * e_err + 2 * U * np.abs(dz)
    b, mag = N_.grad_bounds(pieces64, x, fwd, errs, dz, E_dz)
    bound = (b + U * mag) / M + 1e-300
    term = w64 * err * err
    lbound = ((2 * w64 * np.abs(err) * e_err + 2 * U * term).sum() + (M + 2) * U * term.sum()) / M
    e_ours, e_32 = np.abs(out["grad"].astype(np.float64) - want), np.abs(results[torch.float32][0] - want)
    print("head %s: max |g - g64| / bound = %.3g (torch fp32: %.3g), max |g| = %.3g; loss |ours - f64| / bound = %.3g (torch fp32: %.3g)" % (
        shape, (e_ours / bound).max(), (e_32 / bound).max(), np.abs(want).max(), abs(float(out["loss"][0]) - loss64) / lbound,
        abs(results[torch.float32][1] - loss64) / lbound))
    assert np.abs(want).max() > 1e-3
    assert (e_ours <= bound).all() and (e_32 <= bound).all()
    assert abs(float(out["loss"][0]) - loss64) <= lbound and abs(results[torch.float32][1] - loss64) <= lbound


# ---- the forward is the act's --------------------------------------------------------------------------------------------------------

def test_forward_equals_the_act_host(capi):
    """The loss of a one-sample minibatch with steer 0 is (1 x) o^2: eval_host's o is okenv_vit_act_host's output bit for bit, on the
    act's own embedding (weight 1: |0| is not beyond the threshold)."""
    import _vit_numpy as V_
    cfg = capi.vit_config(**V_.SHAPES["second_tile"])
    rng = np.random.default_rng(11)
    params = V_.random_params(capi, cfg, rng)
    frames = rng.integers(0, 256, (3, cfg.image_size, cfg.image_size, 4), dtype=np.uint8)
    act = capi.vit_act_host(cfg, params, frames)
    shape = (cfg.dim, cfg.head_hidden1, cfg.head_hidden2)
    head = params[capi.vit_head_offset(cfg):]
    assert head.size == capi.vit_head_num_params(*shape) == N_.num_params(*shape)
    loss = capi.vit_head_eval_host(hp_struct(capi), shape, cfg.steer_scale, head, act["embedding"], np.zeros(3, f32), 1)
    assert np.array_equal(bits(loss), bits(act["output"] * act["output"])) and (act["output"] != 0).all()
    assert np.array_equal(bits(N_.positions(head, shape, act["embedding"], np.zeros(3, f32), cfg.steer_scale, 5.0, 0.1)["o"]), bits(act["output"]))


# ---- refusals, in words ----------------------------------------------------------------------------------------------------------------

def refused(capi, words, call):
    with pytest.raises(capi.OkenvError) as e:
        call()
    assert e.value.code == INVALID and words in str(e.value), str(e.value)


@pytest.mark.parametrize("over,words", [(dict(lr=0.0), "lr must be positive"), (dict(lr=-1.0), "lr must be positive"), (dict(lr=float("nan")), "lr must be positive"),
                                        (dict(beta1=1.0), "beta outside [0, 1)"), (dict(beta2=-0.1), "beta outside [0, 1)"),
                                        (dict(beta1=float("nan")), "beta outside [0, 1)"), (dict(eps=0.0), "eps must be positive"),
                                        (dict(eps=float("nan")), "eps must be positive"), (dict(weight=float("nan")), "weight must be positive"),
                                        (dict(weight=0.0), "weight must be positive"), (dict(threshold=float("nan")), "threshold must be finite"),
                                        (dict(threshold=-0.5), "threshold must be finite")])
def test_parameters_are_validated(capi, over, words):
    st, emb, steer, B, _, _ = N_.case(SMALL, N_.GEOMETRIES[0])
    refused(capi, words, lambda: host_update(capi, SMALL, st, emb, steer, B, **over))
    refused(capi, words, lambda: capi.vit_head_eval_host(hp_struct(capi, **over), SMALL, N_.STEER_SCALE, st["params"], emb, steer, B))


def test_calls_are_validated(capi):
    st, emb, steer, B, _, _ = N_.case(SMALL, N_.GEOMETRIES[0])
    L, hp = capi.load(), hp_struct(capi)
    refused(capi, "at least 1", lambda: host_update(capi, SMALL, st, emb, steer, 0))
    refused(capi, "at least 1", lambda: host_update(capi, SMALL, st, emb, steer, B, epochs=0))
    refused(capi, "at least 1", lambda: host_update(capi, SMALL, st, emb[:0], steer[:0], B))
    refused(capi, "at least 1", lambda: capi.vit_head_eval_host(hp, SMALL, N_.STEER_SCALE, st["params"], emb, steer, 0))
    refused(capi, "params is NULL", lambda: capi.vit_head_update_host(None, SMALL, N_.STEER_SCALE, st, emb, steer, B))
    refused(capi, "NULL argument", lambda: capi.vit_head_update_host(hp, SMALL, N_.STEER_SCALE, st, None, steer, B))
    refused(capi, "NULL argument", lambda: capi.vit_head_update_host(hp, SMALL, N_.STEER_SCALE, dict(st, m=None), emb, steer, B))
    refused(capi, "steer_scale", lambda: capi.vit_head_update_host(hp, SMALL, 0.0, st, emb, steer, B))
    refused(capi, "shape outside the limits", lambda: capi.vit_head_update_host(hp, (16, 24, 16), N_.STEER_SCALE, st, emb, steer, B))
    out = capi.OkenvVitHeadOutput()
    args = (SMALL[0], SMALL[1], SMALL[2], C.c_float(10.0))
    state = capi.fill_pointers(capi.OkenvVitHeadState(), {k: st[k] for k in ("params", "m", "v")}, "state")
    assert L.okenv_vit_head_update_host(C.byref(hp), *args, None, capi.ptr(emb), capi.ptr(steer), 13, 5, 1, None, C.byref(out)) == INVALID
    assert b"NULL argument" in L.okenv_last_error(None)
    assert L.okenv_vit_head_eval_host(C.byref(hp), *args, capi.ptr(st["params"]), capi.ptr(emb), capi.ptr(steer), 13, 5, None) == INVALID
    assert b"NULL argument" in L.okenv_last_error(None)
    # the entries that take the handle refuse a NULL one in words, too
    for call, words in ((lambda: L.okenv_vit_embed(None, None, 1, 0, None), b"NULL handle"),
                        (lambda: L.okenv_vit_head_learner_create(None, C.byref(hp)), b"NULL handle"),
                        (lambda: L.okenv_vit_head_update(None, None, None, 1, 1, 1, None, None), b"NULL handle"),
                        (lambda: L.okenv_vit_head_eval(None, None, None, 1, 1, None), b"NULL handle"),
                        (lambda: L.okenv_vit_head_learner_get_state(None, C.byref(state)), b"NULL argument")):
        assert call() == INVALID and words in L.okenv_last_error(None)
    assert L.okenv_vit_head_learner_reset(None) == STATE and b"okenv_vit_head_learner_create first" in L.okenv_last_error(None)
    assert st["t"] == 3  # (nothing above stepped the caller's state)


# ---- the LDS plan ----------------------------------------------------------------------------------------------------------------------

def test_lds_plan_is_a_pure_host_function_and_bounds_the_shapes(capi):
    for shape in N_.SHAPES + [(768, 2048, 2048), (768, 512, 512), (16, 2048, 16)]:
        assert capi.vit_head_lds_bytes(*shape) == N_.lds_bytes(*shape) > 0, shape
    assert capi.vit_head_lds_bytes(*N_.SHAPES[2]) == 4 * (16 * (388 + 132 + 68 + 68) + 16) == 42048
    for bad in ((8, 16, 16), (16, 24, 16), (784, 16, 16), (16, 16, 4096)):
        assert capi.vit_head_lds_bytes(*bad) == 0, bad
    # inside the limits of the shape and beyond 160 KB: refused in words, by the host entries as by okenv_vit_head_learner_create
    big = (768, 2048, 2048)
    assert capi.vit_head_lds_bytes(*big) > N_.LDS_BUDGET
    n = N_.num_params(*big)
    st = dict(params=np.zeros(n, f32), m=np.zeros(n, f32), v=np.zeros(n, f32), t=0)
    refused(capi, "does not fit 160 KB", lambda: host_update(capi, big, st, np.zeros((1, 768), f32), np.zeros(1, f32), 1))
    fits = (768, 512, 512)
    assert 0 < capi.vit_head_lds_bytes(*fits) <= N_.LDS_BUDGET
