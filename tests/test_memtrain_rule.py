"""The rule of the memory's training (include/okenv_memtrain.h) without a GPU: the host entries against the numpy restatement bit for
bit at every shape and geometry, the persistence of Adam's state, the replay of a window through the act's step rule, plain Adam's
bits without decay and clipping, constructed clipping cases, the schedule, the statistics, the refusals and the plans, the first step
against autograd in float64, and a loss that falls."""
import numpy as np
import pytest

import _memory_numpy as mem
import _memtrain_numpy as N_

f32, f64 = np.float32, np.float64
INVALID, STATE = -1, -5
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, clip_grad=1.0)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def configs(capi, shape):
    Z, H, L = N_.SHAPES[shape]
    return capi.world_config(**N_.world_members(Z)), capi.memory_config(hidden=H, layers=L, ctrl_hidden=2)


def fresh_state(shape, seed=0):
    Z, H, L = N_.SHAPES[shape]
    T = N_.trainable(Z, H, L)
    return dict(params=N_.draw_network(Z, H, L, seed), m=np.zeros(T, f32), v=np.zeros(T, f32), t=0)


def host_update(capi, shape, geometry, st, data=None, epochs=None, order="drawn", lr_schedule=None, M=None, **over):
    Mg, B, S, eg, stride = N_.GEOMETRIES[geometry]
    latent, action, start, drawn = data if data is not None else N_.draw_data(N_.SHAPES[shape][0], geometry, 0)
    w, c = configs(capi, shape)
    learner = capi.memory_learner_config(seq_len=S, max_batch=min(B, Mg), **dict(HP, **over))
    return capi.memory_update_host(w, c, learner, st, latent, action, start if M is None else start[:M], B, stride, eg if epochs is None else epochs,
                                   drawn if isinstance(order, str) else order, lr_schedule)


def same_state(a, b):
    return a["t"] == b["t"] and all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("params", "m", "v"))


# ---- the host entries equal the numpy restatement bit for bit ---------------------------------------------------------------------------

@pytest.mark.parametrize("geometry", list(N_.GEOMETRIES))
@pytest.mark.parametrize("shape", N_.MIRRORED)
def test_host_entry_equals_numpy(capi, shape, geometry):
    Z, H, L = N_.SHAPES[shape]
    M, B, S, epochs, stride = N_.GEOMETRIES[geometry]
    st = fresh_state(shape)
    latent, action, start, order = N_.draw_data(Z, geometry, 0)
    new, out = host_update(capi, shape, geometry, st)
    want, wout = N_.update(Z, H, L, HP, st, latent, action, start, M, B, S, epochs, stride, order)
    assert new["t"] == want["t"] == epochs * -(-M // B)
    for k in ("loss", "norm", "grad"):
        assert np.array_equal(bits(out[k]), bits(wout[k])), k
    assert same_state(new, want)
    T = N_.trainable(Z, H, L)
    assert np.array_equal(bits(new["params"][T:]), bits(st["params"][T:])), "the statistics are never stepped"
    assert np.abs(out["grad"]).max() > 1e-5 and not np.array_equal(bits(new["params"][:T]), bits(st["params"][:T]))
    w, c = configs(capi, shape)
    learner = capi.memory_learner_config(seq_len=S, max_batch=min(B, M), **HP)
    got = capi.memory_eval_host(w, c, learner, new["params"], latent, action, start, B, stride)
    assert np.array_equal(bits(got), bits(N_.evaluate(Z, H, L, new["params"], latent, action, start, M, B, S, stride)))


def test_two_calls_of_one_epoch_equal_one_call_of_two(capi):
    """t, m and v persist across calls."""
    shape, geometry = "48-48-2", "two_epochs_strided"
    data = N_.draw_data(48, geometry, 0)
    st = fresh_state(shape)
    both, out = host_update(capi, shape, geometry, st, data)
    first, out1 = host_update(capi, shape, geometry, st, data, epochs=1, order=data[3][:1])
    second, out2 = host_update(capi, shape, geometry, first, data, epochs=1, order=data[3][1:])
    assert same_state(both, second) and both["t"] == 6
    for k in ("loss", "norm"):
        assert np.array_equal(bits(out[k]), bits(np.concatenate([out1[k], out2[k]])))
    assert np.array_equal(bits(out["grad"]), bits(out2["grad"]))


@pytest.mark.parametrize("shape", N_.MIRRORED)
def test_a_window_replayed_through_the_acts_step_rule(capi, shape):
    """From a zeroed state the act's rule with carry = 1 (the mirror's step) gives the update's hidden states bit for bit, and its
    prediction is the update's zn behind the act's denormalisation."""
    Z, H, L = N_.SHAPES[shape]
    S = 5
    net = N_.draw_network(Z, H, L, 3)
    latent, action, _, _ = N_.draw_data(Z, "second_block_of_one", 1)
    w, c = configs(capi, shape)
    hidden, zn = capi.memory_window_host(w, c, net, latent, action, 2, S)
    p = mem.split(Z, H, L, net)
    h = np.zeros((1, L, H), f32)
    for s in range(S):
        h, prediction = mem.step(Z, H, L, 1, net, latent[2 + s][None], action[2 + s][None], h)
        assert np.array_equal(bits(h[0]), bits(hidden[s])), "hidden state of step %d" % s
        assert np.array_equal(bits(prediction[0]), bits(zn[s] * p["z_std"] + p["z_mean"])), "prediction of step %d" % s
    assert np.abs(hidden[S - 1] - hidden[0]).max() > 1e-3


def test_without_decay_and_clipping_the_step_is_plain_adam(capi):
    shape, geometry = "48-48-2", "two_steps"
    Z, H, L = N_.SHAPES[shape]
    T = N_.trainable(Z, H, L)
    st = fresh_state(shape)
    st["m"] = np.random.default_rng(1).normal(0, 1e-3, T).astype(f32)
    st["v"] = np.random.default_rng(2).uniform(0, 1e-6, T).astype(f32)
    st["t"] = 4
    new, out = host_update(capi, shape, geometry, st, weight_decay=0.0, clip_grad=0.0)
    g, b1, b2, eps = out["grad"], f32(0.9), f32(0.999), f32(1e-8)
    m = b1 * st["m"] + f32(1.0 - f64(b1)) * g
    v = b2 * st["v"] + (f32(1.0 - f64(b2)) * g) * g
    step, bc2 = f32(f64(f32(1e-3)) / (1.0 - float(b1) ** 5)), f32(np.sqrt(1.0 - N_.powi(float(b2), 5)))
    assert step == f32(f64(f32(1e-3)) / (1.0 - N_.powi(float(b1), 5)))
    p = st["params"][:T] - step * (m / (np.sqrt(v.astype(f64)).astype(f32) / bc2 + eps))
    assert new["t"] == 5
    assert np.array_equal(bits(new["m"]), bits(m)) and np.array_equal(bits(new["v"]), bits(v)) and np.array_equal(bits(new["params"][:T]), bits(p))


def test_clipping_below_and_above_the_norm(capi):
    shape, geometry = "16-16-1", "two_steps"
    st = fresh_state(shape)
    _, off = host_update(capi, shape, geometry, st, clip_grad=0.0)
    norm = off["norm"][0]
    assert 1e-3 < norm < 1e3 and norm == N_.clip(N_.sumsq(off["grad"]), 0.0)[0]
    _, below = host_update(capi, shape, geometry, st, clip_grad=float(norm) * 4.0)
    assert np.array_equal(bits(below["grad"]), bits(off["grad"])), "a gradient below max_norm is multiplied by exactly 1.0f"
    assert below["norm"][0] == norm
    limit = f32(float(norm) / 8.0)
    _, above = host_update(capi, shape, geometry, st, clip_grad=float(limit))
    coef = limit / (norm + f32(1e-6))
    assert coef < 1 and np.array_equal(bits(above["grad"]), bits(off["grad"] * coef))
    assert above["norm"][0] == norm, "the reported norm is pre-clip"


def test_a_schedule_equals_single_calls_with_constant_rates(capi):
    shape, geometry = "16-16-1", "short_last_minibatch"
    M, B, S, epochs, stride = N_.GEOMETRIES[geometry]
    data = N_.draw_data(16, geometry, 0)
    rates = np.array([1e-3, 4e-4, 2.5e-5], f32)
    st = fresh_state(shape)
    whole, out = host_update(capi, shape, geometry, st, data, lr_schedule=rates)
    losses = []
    for k in range(3):
        part = (data[0], data[1], data[2][k * B:(k + 1) * B], None)
        st, o = host_update(capi, shape, geometry, st, part, order=None, lr=float(rates[k]))
        losses.append(o["loss"][0])
    assert same_state(whole, st) and np.array_equal(bits(out["loss"]), bits(np.array(losses, f32)))
    assert np.array_equal(bits(out["grad"]), bits(o["grad"]))


def test_the_wide_shape_on_the_host(capi):
    """The reference's width and depth at 39 positions: finite, and a step that moves every tensor of the vector."""
    Z, H, L = N_.SHAPES[N_.WIDE]
    st = fresh_state(N_.WIDE)
    new, out = host_update(capi, N_.WIDE, N_.WIDE_GEOMETRY, st)
    assert new["t"] == 3 and np.isfinite(out["loss"]).all() and np.isfinite(out["norm"]).all() and np.isfinite(new["params"]).all()
    for name, at, shp in mem.layout(Z, H, L)[:-4]:
        n = int(np.prod(shp))
        assert not np.array_equal(bits(new["params"][at:at + n]), bits(st["params"][at:at + n])), name


# ---- refusals and plans -----------------------------------------------------------------------------------------------------------------

def refused(capi, call, words):
    with pytest.raises(capi.OkenvError) as e:
        call()
    assert e.value.code == INVALID and words in str(e.value), str(e.value)


def test_refusals(capi):
    shape, geometry = "16-16-1", "two_steps"
    T = N_.trainable(*N_.SHAPES[shape])
    st = fresh_state(shape)
    for at, value, words in ((5, np.nan, "non-finite"), (T + 16 + 3, 0.0, "std"), (T + 2 * 16 + 2 + 1, -1.0, "std")):
        bad = dict(st, params=st["params"].copy())
        bad["params"][at] = value
        refused(capi, lambda: host_update(capi, shape, geometry, bad), words)
    w, c = configs(capi, shape)
    data = N_.draw_data(16, geometry, 0)
    for over, words in ((dict(seq_len=0), "seq_len"), (dict(seq_len=17), "seq_len"), (dict(max_batch=0), "max_batch"), (dict(lr=0.0), "lr"),
                        (dict(weight_decay=-1.0), "weight_decay"), (dict(clip_grad=float("nan")), "clip_grad"), (dict(beta1=1.0), "beta")):
        learner = capi.memory_learner_config(**dict(dict(HP, seq_len=2, max_batch=3), **over))
        refused(capi, lambda: capi.memory_update_host(w, c, learner, st, data[0], data[1], data[2], 3), words)
        assert capi.memory_learner_workspace_bytes(w, c, learner) == 0
    learner = capi.memory_learner_config(seq_len=2, max_batch=2, **HP)
    refused(capi, lambda: capi.memory_update_host(w, c, learner, st, data[0], data[1], data[2], 3), "max_batch")
    refused(capi, lambda: capi.memory_update_host(w, c, learner, st, data[0], data[1], data[2], 0), "at least 1")
    refused(capi, lambda: capi.memory_update_host(w, c, learner, st, None, data[1], data[2], 2), "NULL")
    refused(capi, lambda: capi.memory_update_host(w, c, learner, dict(st, m=None), data[0], data[1], data[2], 2), "state")


@pytest.mark.parametrize("shape", list(N_.SHAPES))
def test_workspace_and_lds_plans(capi, shape):
    Z, H, L = N_.SHAPES[shape]
    w, c = configs(capi, shape)
    for S, B in ((1, 1), (5, 256), (16, 7)):
        learner = capi.memory_learner_config(seq_len=S, max_batch=B, **HP)
        assert capi.memory_learner_workspace_bytes(w, c, learner) == 4 * N_.workspace_words(Z, H, L, S, B)
    assert capi.memory_learner_lds_bytes(w, c) == N_.lds_bytes() == 0
    assert capi.memory_trainable(w, c) == N_.trainable(Z, H, L)


# ---- the first step against float64 -----------------------------------------------------------------------------------------------------

def torch_first_step(Z, H, L, net, x, y, dtype):
    """The loss and the gradient (in the vector's order) of nn.GRU + nn.Linear + mse_loss on windows x [B][S][Z + 2], y [B][S][Z]."""
    import torch
    from torch import nn
    gru, head = nn.GRU(Z + 2, H, L, batch_first=True).to(dtype), nn.Linear(H, Z).to(dtype)
    p = mem.split(Z, H, L, net)
    with torch.no_grad():
        for l in range(L):
            for ours, theirs in (("gru.weight_ih_l%d", "weight_ih_l%d"), ("gru.weight_hh_l%d", "weight_hh_l%d"), ("gru.bias_ih_l%d", "bias_ih_l%d"),
                                 ("gru.bias_hh_l%d", "bias_hh_l%d")):
                getattr(gru, theirs % l).copy_(torch.from_numpy(p[ours % l]).to(dtype))
        head.weight.copy_(torch.from_numpy(p["head.weight"]).to(dtype))
        head.bias.copy_(torch.from_numpy(p["head.bias"]).to(dtype))
    loss = nn.functional.mse_loss(head(gru(torch.from_numpy(x).to(dtype))[0]), torch.from_numpy(y).to(dtype))
    loss.backward()
    grads = {}
    for l in range(L):
        for ours, theirs in (("gru.weight_ih_l%d", "weight_ih_l%d"), ("gru.weight_hh_l%d", "weight_hh_l%d"), ("gru.bias_ih_l%d", "bias_ih_l%d"),
                             ("gru.bias_hh_l%d", "bias_hh_l%d")):
            grads[ours % l] = getattr(gru, theirs % l).grad.double().numpy()
    grads["head.weight"], grads["head.bias"] = head.weight.grad.double().numpy(), head.bias.grad.double().numpy()
    return float(loss.detach().double()), grads


@pytest.mark.parametrize("shape", N_.MIRRORED)
def test_first_step_against_float64(capi, shape):
    """The first minibatch's loss and gradient (65 positions: 13 windows of 5 steps, clipping off) against autograd in float64 on the
    same normalised windows.  The bound is 4 x the deviation of torch's own float32 module from float64, per tensor, relative to the
    tensor's largest gradient entry (the loss: relative to the loss).  The margin: the blocked chains measured 1.1 .. 1.8 x torch's
    float32 deviation on the forward (okenv_memory.h, third departure), and the backward stacks L x S such stages.

    Measured (every figure is printed before the assertion), the deviation from float64 of the host entry / of torch's float32
    module, smallest .. largest over the tensors, and the range of their ratio:
        16-16-1    host 0.9e-07 .. 2.4e-07   torch 0.6e-07 .. 3.0e-07   ratio 0.39 .. 2.18   (loss 3.8e-08 / 3.5e-08: 1.11)
        48-48-2    host 1.0e-07 .. 3.1e-07   torch 0.9e-07 .. 3.3e-07   ratio 0.63 .. 3.16   (loss 8.3e-08 / 6.9e-08: 1.21)
        128-96-2   host 1.4e-07 .. 3.4e-07   torch 0.8e-07 .. 4.9e-07   ratio 0.44 .. 2.17   (loss 1.3e-07 / 5.4e-08: 2.43)
    The largest single ratio, 3.16, is gru.bias_hh_l1 at 48-48-2 (2.8e-07 against 8.8e-08)."""
    Z, H, L = N_.SHAPES[shape]
    geometry = "second_block_of_one"
    M, B, S, _, stride = N_.GEOMETRIES[geometry]
    st = fresh_state(shape)
    latent, action, start, _ = N_.draw_data(Z, geometry, 0)
    _, out = host_update(capi, shape, geometry, st, clip_grad=0.0, weight_decay=0.0)
    f = N_.forward(Z, H, L, st["params"], latent, action, list(start), S, stride)
    x = np.ascontiguousarray(f["x0"].reshape(S, M, Z + 2).transpose(1, 0, 2))
    y = np.ascontiguousarray(f["y"].reshape(S, M, Z).transpose(1, 0, 2))
    import torch
    loss64, g64 = torch_first_step(Z, H, L, st["params"], x, y, torch.float64)
    loss32, g32 = torch_first_step(Z, H, L, st["params"], x, y, torch.float32)
    rows = [("loss", abs(float(out["loss"][0]) - loss64) / loss64, abs(loss32 - loss64) / loss64)]
    for name, at, shp in mem.layout(Z, H, L)[:-4]:
        n = int(np.prod(shp))
        ours = out["grad"][at:at + n].reshape(shp).astype(f64)
        top = np.abs(g64[name]).max()
        rows.append((name, np.abs(ours - g64[name]).max() / top, np.abs(g32[name] - g64[name]).max() / top))
    for name, ours, torchs in rows:
        print("%s %-20s host %.3e  torch fp32 %.3e  ratio %.2f" % (shape, name, ours, torchs, ours / torchs if torchs > 0 else float("inf")))
    for name, ours, torchs in rows:
        assert ours <= 4.0 * torchs, (name, ours, torchs)


# ---- the loss falls ---------------------------------------------------------------------------------------------------------------------

def rotating_latents(T, N, Z, seed):
    """Each latent a fixed rotation of the one before (pairs of coordinates turned by fixed angles); constant actions with a little
    spread so that their std is not 0."""
    rng = np.random.default_rng(seed)
    z = np.zeros((T, N, Z), f64)
    z[0] = rng.normal(0, 1, (N, Z))
    angles = rng.uniform(0.2, 0.6, Z // 2)
    c, s = np.cos(angles), np.sin(angles)
    for t in range(1, T):
        a, b = z[t - 1, :, 0::2], z[t - 1, :, 1::2]
        z[t, :, 0::2], z[t, :, 1::2] = c * a - s * b, s * a + c * b
    action = np.stack([rng.normal(100.0, 1.0, (T, N)), rng.normal(0.0, 1.0, (T, N))], axis=2)
    return z.astype(f32), action.astype(f32)


def test_the_loss_falls(ok, capi):
    import torch
    from openkitchen_amd import worldmodel as wm
    shape, S, T_, N = "16-16-1", 5, 14, 8
    Z, H, L = N_.SHAPES[shape]
    z, a = rotating_latents(T_, N, Z, 7)
    alive = torch.ones(T_, N, dtype=torch.bool)
    # the data first: the PyTorch loop on the same windows ends below its start
    torch.manual_seed(0)
    model = wm.GRUDynamics(latent=Z, hidden=H, layers=L)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    losses, stats = wm.train_memory(model, torch.from_numpy(z), torch.from_numpy(a), alive, epochs=10, batch=18, seq_len=S)
    assert losses[-1] < losses[0], losses
    # the learner: the same initial weights and statistics, 40 steps at lr 1e-3
    net = wm.memory_params_from_state_dict(sd0, stats).numpy()
    start = wm.memory_window_starts(alive, S).numpy().astype(np.int32)
    M = start.size
    assert M == (T_ - S) * N
    w, c = configs(capi, shape)
    learner = capi.memory_learner_config(seq_len=S, max_batch=18, **HP)
    before = capi.memory_eval_host(w, c, learner, net, z, a, start, M if M <= 18 else 18, N)
    st = dict(params=net, m=np.zeros(N_.trainable(Z, H, L), f32), v=np.zeros(N_.trainable(Z, H, L), f32), t=0)
    new, out = capi.memory_update_host(w, c, learner, st, z, a, start, 18, N, 10)
    after = capi.memory_eval_host(w, c, learner, new["params"], z, a, start, 18, N)
    assert new["t"] == 40 and np.isfinite(out["loss"]).all()
    assert after.mean() < before.mean(), (before.mean(), after.mean())
