"""Deep-Q learning on the CPU (include/okenv_dqn.h; okenv_replay_push_host, okenv_dqn_update_host): the host
entries against an independent numpy restatement (tests/_dqn_numpy.py) bit for bit, the sampling's range, repetition and uniformity,
the continuation across calls, constructed ties and edges, the first iteration against torch autograd in float64 on the reference's
expressions with a derived bound, three iterations recorded, and validation."""
import ctypes as C

import numpy as np
import pytest

import _dqn_numpy as D_
import _learn_numpy as L_

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32
HP = dict(lr=1e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8)  # kLearningRate (DQAgent.hpp:34); clip is unread
SHAPES = [(5, 128, 5), (7, 9, 4), (64, 256, 8), (1, 1, 2), (6, 9, 4), (10, 13, 5)]
RING_FIELDS = ("state", "next_state", "action", "reward", "done")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


def same_ring(got, want, what):
    assert got["pushed"] == want["pushed"], what
    for k in RING_FIELDS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + tuple(what)


def step_data(rng, n, R, A, mask):
    """A record and the fields after a step for n agents: some crashed, some clearances beyond the sensor range."""
    state = rng.random((n, R)).astype(f32)
    action = rng.integers(0, A, n).astype(np.int64)
    dist = (rng.random((n, R)) * 150.0 + 0.5).astype(f32)
    dist[rng.random(n) < 0.2] = f32(200.0) + rng.random(R).astype(f32) * f32(50.0)  # nothing in range: the cap
    crashed = (rng.random(n) < 0.3).astype(np.uint8)
    alive = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
             "random": (rng.random(n) < 0.6).astype(np.uint8)}[mask]
    return state, action, alive, dist, crashed


def fresh_state(rng, shape, scale=0.3):
    R, H, A = shape
    st = {"policy": (rng.standard_normal(L_.n_params(R, H, A)) * scale).astype(f32), "t": 0}
    st["policy_m"], st["policy_v"] = np.zeros_like(st["policy"]), np.zeros_like(st["policy"])
    return st


def filled_ring(rng, R, A, capacity, size):
    rg = D_.ring(capacity, R)
    rg["state"][:] = rng.random((capacity, R)).astype(f32)
    rg["next_state"][:] = rng.random((capacity, R)).astype(f32)
    rg["action"][:] = rng.integers(0, A, capacity)
    rg["reward"][:] = np.where(rng.random(capacity) < 0.2, -200.0, rng.random(capacity) * 200.0).astype(f32)
    rg["done"][:] = (rg["reward"] == f32(-200.0)).astype(f32)
    rg["pushed"] = size
    return rg


def assert_same_update(got_state, got_out, want_state, want_out, what):
    assert got_state["t"] == want_state["t"], what
    for k in ("policy", "policy_m", "policy_v"):
        assert np.array_equal(bits(got_state[k]), bits(want_state[k])), (k,) + tuple(what)
    for k in ("loss", "grad_policy"):
        assert np.array_equal(bits(got_out[k]), bits(want_out[k])), (k,) + tuple(what)
    assert np.array_equal(got_out["index"], want_out["index"]), what


def cfg_of(ok, cfg):
    return ok.capi.dqn_config(cfg["gamma"], cfg["mask_done"], cfg["target_network"], cfg["seed"])


# ---- the push ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_push_host_equals_the_numpy_restatement(ok, n):
    """Every capacity (C = 1 and 7 are below what one call pushes), every mask, three calls in a row so the ring wraps across calls."""
    R, A = 5, 5
    for capacity in (1, 7, 64, 100, 1000):
        for mask in ("all", "none", "alternating", "random"):
            for push_all, own_reward in ((False, False), (True, False), (False, True)):
                rng = np.random.default_rng(n * 7919 + capacity)
                got, want = ok.replay_ring(capacity, R), D_.ring(capacity, R)
                for call in range(3):
                    state, action, alive, dist, crashed = step_data(rng, n, R, A, mask)
                    reward = rng.standard_normal(n).astype(f32) if own_reward else None
                    ok.replay_push_host(got, state, action, alive, dist, crashed, reward, push_all)
                    D_.push(want, state, action, alive, dist, crashed, reward, push_all)
                    same_ring(got, want, (n, capacity, mask, push_all, own_reward, call))
                if mask != "random":
                    per_call = n if (push_all or mask == "all") else (0 if mask == "none" else n // 2)
                    assert got["pushed"] == 3 * per_call


def test_push_rewards_and_next_state(ok):
    """Crashed agents: reward exactly -200 and done 1; the clearance is the smallest distance capped at 200; next_state is the IEEE
    division by 200."""
    R, n = 5, 6
    dist = np.array([[3, 9, 1.5, 8, 7], [250, 300, 201, 200.5, 999], [200, 200, 200, 200, 200], [10, 20, 30, 40, 50], [0.1, 0.2, 0.3, 0.05, 1],
                     [199.99, 250, 250, 250, 250]], dtype=f32)
    crashed = np.array([0, 0, 0, 1, 1, 0], np.uint8)
    rg = ok.replay_ring(8, R)
    ok.replay_push_host(rg, np.zeros((n, R), f32), np.arange(n), np.ones(n, np.uint8), dist, crashed)
    assert rg["pushed"] == n
    assert np.array_equal(rg["reward"][:n], np.array([1.5, 200.0, 200.0, -200.0, -200.0, 199.99], dtype=f32))
    assert np.array_equal(rg["done"][:n], crashed.astype(f32))
    assert np.array_equal(bits(rg["next_state"][:n]), bits(dist / f32(200.0)))
    assert np.array_equal(rg["action"][:n], np.arange(n))
    assert (rg["reward"][n:] == 0).all() and (rg["next_state"][n:] == 0).all()


# ---- sampling ------------------------------------------------------------------------------------------------------------------------

def drawn(ok, seed, draw, size, B):
    """The slots one iteration of the host entry samples (its `index` output), on the smallest network."""
    shape = (1, 1, 2)
    rng = np.random.default_rng(size)
    cfg = ok.capi.dqn_config(seed=seed)
    _, out = ok.dqn_update_host(ok.capi.learner_params(**HP), cfg, shape, fresh_state(rng, shape), filled_ring(rng, 1, 2, size, size), B, 1,
                                draw_base=draw, want=("index",))
    return out["index"]


def test_sampling_range_repetition_and_uniformity(ok):
    for size in (1, 2, 3, 1000):
        idx = drawn(ok, 11, 3, size, 4096)
        assert idx.min() >= 0 and idx.max() < size
        assert np.array_equal(idx, D_.sample(11, 3, size, 4096)), size
        assert size == 1000 or len(set(idx.tolist())) == size  # every slot of a small ring is reached
    # frequencies over 2^16 draws: each of 16 slots is binomial(n, 1/16); 5 sigma
    n, size = 1 << 16, 16
    counts = np.bincount(drawn(ok, 5, 0, size, n), minlength=size)
    sigma = np.sqrt(n * (1 / size) * (1 - 1 / size))
    assert np.abs(counts - n / size).max() <= 5 * sigma, counts
    # another draw number or seed gives other slots
    a, b, c = drawn(ok, 5, 0, 1000, 100), drawn(ok, 5, 1, 1000, 100), drawn(ok, 6, 0, 1000, 100)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_resample_off_repeats_the_batch_and_on_does_not(ok):
    shape = (5, 16, 5)
    rng = np.random.default_rng(3)
    rg = filled_ring(rng, 5, 5, 1000, 1000)
    st = fresh_state(rng, shape)
    lp, cfg = ok.capi.learner_params(**HP), ok.capi.dqn_config(seed=9)
    seen = {}
    for resample in (False, True):
        for iterations in (1, 2):
            _, out = ok.dqn_update_host(lp, cfg, shape, st, rg, 32, iterations, resample, draw_base=40)
            seen[resample, iterations] = out["index"]
    assert np.array_equal(seen[False, 1], seen[False, 2]) and np.array_equal(seen[False, 1], seen[True, 1])
    assert not np.array_equal(seen[True, 1], seen[True, 2])
    assert np.array_equal(seen[True, 2], D_.sample(9, 41, 1000, 32))
    assert np.array_equal(seen[False, 1], D_.sample(9, 40, 1000, 32))


# ---- the update against the numpy restatement -----------------------------------------------------------------------------------------

# (size, B, iterations, resample, mask_done, target_network): every value of every factor the issue lists, each shape runs all rows
CASES = [(1, 1, 1, False, False, False), (31, 32, 3, True, False, False), (33, 33, 1, False, True, False), (1000, 100, 3, False, False, True),
         (1000, 33, 1, True, True, True), (31, 100, 1, False, True, False)]


@pytest.mark.parametrize("shape", SHAPES)
def test_update_host_equals_the_numpy_restatement(ok, shape):
    R, H, A = shape
    rng = np.random.default_rng(sum(shape))
    lp = ok.capi.learner_params(**HP)
    for size, B, iterations, resample, mask_done, target_network in CASES:
        rg = filled_ring(rng, R, A, max(size, 40), size)
        st = fresh_state(rng, shape)
        st["t"] = 5  # a continued run: m and v are not zero either
        st["policy_m"] = (rng.standard_normal(st["policy"].size) * 1e-3).astype(f32)
        st["policy_v"] = (rng.random(st["policy"].size) * 1e-4).astype(f32)
        target = (st["policy"] + rng.standard_normal(st["policy"].size).astype(f32) * f32(0.05)) if target_network else None
        cfg = dict(gamma=0.99, mask_done=mask_done, target_network=target_network, seed=R)
        got = ok.dqn_update_host(lp, cfg_of(ok, cfg), shape, st, rg, B, iterations, resample, draw_base=7, target=target)
        want = D_.update(HP, cfg, shape, st, rg, B, iterations, resample, draw_base=7, target=target)
        assert_same_update(*got, *want, (shape, size, B, iterations, resample, mask_done, target_network))
        assert np.isfinite(got[1]["loss"]).all() and got[1]["loss"].size == iterations


@pytest.mark.parametrize("B", [513, 1500, 4096])
def test_update_host_equals_the_numpy_restatement_above_four_chunks(ok, B):
    """ok_learn_tree in the host entry at C = 17, 47 and 128 chunks (CASES stops at B = 100, four chunks): padded widths 32, 64 and
    128, the guard `i + h < n` false at the first level for C = 17 and 47 and never for 128.  These are the B of
    tests/test_gpu_update_geometry.py, whose device results are compared with this host entry."""
    shape = (7, 9, 4)
    R, H, A = shape
    rng = np.random.default_rng(B)
    lp = ok.capi.learner_params(**HP)
    for iterations, resample, mask_done, target_network in ((1, False, True, False), (3, True, False, True)):
        rg = filled_ring(rng, R, A, 1000, 1000)
        st = fresh_state(rng, shape)
        target = (st["policy"] + rng.standard_normal(st["policy"].size).astype(f32) * f32(0.05)) if target_network else None
        cfg = dict(gamma=0.99, mask_done=mask_done, target_network=target_network, seed=B)
        got = ok.dqn_update_host(lp, cfg_of(ok, cfg), shape, st, rg, B, iterations, resample, draw_base=7, target=target)
        want = D_.update(HP, cfg, shape, st, rg, B, iterations, resample, draw_base=7, target=target)
        assert_same_update(*got, *want, (shape, B, iterations, resample, mask_done, target_network))
        assert np.isfinite(got[1]["loss"]).all() and got[1]["loss"].size == iterations and got[1]["index"].size == B


def test_two_calls_continue_one_run(ok):
    shape = (5, 32, 5)
    rng = np.random.default_rng(21)
    rg = filled_ring(rng, 5, 5, 200, 200)
    st = fresh_state(rng, shape)
    lp, cfg = ok.capi.learner_params(**HP), ok.capi.dqn_config(seed=2)
    for resample in (False, True):
        whole, out = ok.dqn_update_host(lp, cfg, shape, st, rg, 33, 5, resample, draw_base=10)
        a, out_a = ok.dqn_update_host(lp, cfg, shape, st, rg, 33, 2, resample, draw_base=10)
        b, out_b = ok.dqn_update_host(lp, cfg, shape, a, rg, 33, 3, resample, draw_base=12 if resample else 10)
        assert b["t"] == whole["t"] == 5
        for k in ("policy", "policy_m", "policy_v"):
            assert np.array_equal(bits(b[k]), bits(whole[k])), (k, resample)
        assert np.array_equal(bits(np.concatenate([out_a["loss"], out_b["loss"]])), bits(out["loss"]))
        assert np.array_equal(bits(out_b["grad_policy"]), bits(out["grad_policy"])) and np.array_equal(out_b["index"], out["index"])


def test_an_empty_ring_leaves_fresh_parameters_alone(ok):
    for shape in SHAPES:
        rng = np.random.default_rng(shape[1])
        st = fresh_state(rng, shape)
        rg = ok.replay_ring(16, shape[0])
        rg["state"][:] = np.nan  # nothing may read the slots
        new, out = ok.dqn_update_host(ok.capi.learner_params(**HP), ok.capi.dqn_config(), shape, st, rg, 33, 3)
        assert new["t"] == 3 and np.array_equal(bits(new["policy"]), bits(st["policy"]))
        assert not new["policy_m"].any() and not new["policy_v"].any() and not out["loss"].any() and not out["grad_policy"].any()
        want = D_.update(HP, dict(gamma=0.99, mask_done=False, target_network=False, seed=0), shape, st, rg, 33, 3)
        assert_same_update(new, out, *want, shape)


def test_constructed_ties_zero_preactivations_done_and_zero_error(ok):
    """Rows 0 and 1 of the second layer are equal, so q'_0 == q'_1 is the maximum's tie wherever they lead; hidden unit 0 has weights and
    bias 0, so its pre-activation is exactly 0 and its derivative 0; done = 1 changes y only under the mask; with gamma = 0 and
    r = q_a the error is exactly 0: loss, gradient and Adam's step are 0."""
    shape = (5, 16, 5)
    R, H, A = shape
    rng = np.random.default_rng(8)
    st = fresh_state(rng, shape)
    w1, b1, w2, b2 = L_.split(st["policy"], R, H, A)
    w1[0], b1[0] = 0.0, 0.0
    w2[1], b2[1] = w2[0], b2[0] + f32(30.0)  # 0 and 1 lead
    b2[0] = b2[1]
    rg = filled_ring(rng, R, A, 64, 64)
    rg["done"][:] = 1.0
    lp = ok.capi.learner_params(**HP)
    zn, _, _ = L_.forward(st["policy"], R, H, A, rg["next_state"])
    assert (zn[:, 0] == zn[:, 1]).all() and (zn.argmax(axis=1) == 0).all()
    outs = {}
    for mask_done in (False, True):
        cfg = dict(gamma=0.99, mask_done=mask_done, target_network=False, seed=1)
        got = ok.dqn_update_host(lp, cfg_of(ok, cfg), shape, st, rg, 64, 1)
        assert_same_update(*got, *D_.update(HP, cfg, shape, st, rg, 64, 1), ("mask", mask_done))
        g = got[1]["grad_policy"]
        assert not g[:R].any() and g[H * R] == 0  # unit 0: ReLU'(0) = 0
        idx = got[1]["index"]
        z, _, _ = L_.forward(st["policy"], R, H, A, rg["state"][idx])
        y = rg["reward"][idx] if mask_done else rg["reward"][idx] + f32(0.99) * zn[idx, 0]
        e = z[np.arange(64), rg["action"][idx]] - y.astype(f32)
        assert got[1]["loss"][0] == L_.rule_sum((e * e)[:, None])[0] / f32(64 * A)
        outs[mask_done] = got[1]["loss"][0]
    assert outs[False] != outs[True]
    z, _, _ = L_.forward(st["policy"], R, H, A, rg["state"])
    rg["reward"][:] = z[np.arange(64), rg["action"]]
    new, out = ok.dqn_update_host(lp, ok.capi.dqn_config(gamma=0.0), shape, st, rg, 64, 2)
    assert not out["loss"].any() and not out["grad_policy"].any() and np.array_equal(bits(new["policy"]), bits(st["policy"]))


# ---- against the reference's expressions in torch float64 ----------------------------------------------------------------------------

def torch_net(shape, policy, dtype):
    import torch
    return [torch.tensor(np.array(a), dtype=dtype, requires_grad=True) for a in L_.split(policy, *shape)]


def torch_loss(net, x, xn, action, reward, done, gamma, mask_done):
    """updateDQN's expressions (DQAgent.hpp:129-145), restated: detached q', cloned target with y put at the action, mse over B * A."""
    import torch
    w1, b1, w2, b2 = net
    q = torch.relu(x @ w1.T + b1) @ w2.T + b2
    qn = (torch.relu(xn @ w1.T + b1) @ w2.T + b2).detach()
    best = torch.amax(qn, 1, True)
    y = reward + (1 - done) * gamma * best if mask_done else reward + gamma * best
    target = q.clone().detach()
    for b in range(target.shape[0]):
        target[b].index_put_((action[b],), y[b].squeeze())
    return torch.nn.functional.mse_loss(q, target)


@pytest.mark.parametrize("shape,scale,mask_done", [((5, 128, 5), 0.3, False), ((7, 9, 4), 0.5, True), ((64, 256, 8), 0.05, False)])
def test_first_iteration_against_torch_float64(ok, shape, scale, mask_done):
    """The first iteration's loss and gradient against autograd in float64 on the reference's expressions.

    The bound, per parameter, is derived as tests/test_learn_rule.py derives its own.  The gradient is (2 / (B A)) sum_b a_b c_b with a
    a seed (e on the chosen output, or the hidden seed w2[a][j] e where the unit is active) and c an input x_i or a hidden value h_j.
    With T = (2 / (B A)) sum_b |a_b| |c_b| in float64, the fp32 summation (a chunk of 32 in sequence, log2 of the chunk count in the
    tree, a multiplication per term, the doubling and the division) contributes (32 + log2 C + 3) u T; a hidden seed is one product
    and the remaining roundings of a term are covered by (R + A + 16) u T as they are there.  A hidden value h_j is a sum of R + 1
    terms that may cancel, so its error is NOT relative to h_j but to the float64 sum of absolute terms behind it,
    |h_j - h64_j| <= (R + 2) u (|b1_j| + |w1_j| |x|); for the second layer's weights that adds the absolute term
    E = (2 / (B A)) sum_b S_b (R + 2) u (|b1_j| + |w1_j| |x_b|) on the chosen output's row, with S as follows.
    The seed e = q_a(s) - (r + g max q'(s')) is a difference, so its error is taken relative to S = Z_a(s) + |r| + g max_k Z_k(s'), Z the float64 sum of absolute terms behind
    an output (|b2| + |w2| (|b1| + |w1| |x|)): an output is a sum of R + 1 and H / 8 + 4 terms, so it is within (R + H / 8 + 8) u Z of
    its float64 value, the maximum of outputs moves by no more than its largest member does, and (1 - done) g, g m, r + g m and the
    subtraction are four more roundings: |e - e64| <= k_e S with k_e = (R + H / 8 + 12) u, and S stands for |a_b| in T.  A hidden
    unit whose float64 pre-activation lies within its own rounding error (R + 2) u (|b1| + |w1| |x|) of 0 may be active on one side
    only; it counts as active in T, so the whole term is inside the bound.  Doubled for the second-order terms:
        |g - g64| <= 2 ((32 + log2 C + 3 + R + A + 16 + R + H / 8 + 12) u T + E).
    The loss is a mean of e^2 / A: |loss - loss64| <= 2 (32 + log2 C + 3 + 2 k_e / u + 2) u sum_b S_b^2 / (B A).
    torch's own float32 backward must meet the same bounds.

    Constructed, so that conventions are compared with autograd's: hidden unit 0 with weights and bias 0 (its pre-activation is
    exactly 0 on every side, its T is 0, so any derivative other than 0 breaks the bound), rows 0 and 1 of the second layer equal (ties
    in the maximum over q' on every side), a fifth of the transitions with done = 1."""
    import torch
    R, H, A = shape
    B, gamma = 200, 0.99
    rng = np.random.default_rng(R * H)
    st = fresh_state(rng, shape, scale)
    w1, b1, w2, b2 = L_.split(st["policy"], R, H, A)
    w1[0], b1[0] = 0.0, 0.0
    w2[1], b2[1] = w2[0], b2[0]
    rg = filled_ring(rng, R, A, 500, 500)
    cfg = ok.capi.dqn_config(gamma, mask_done, False, 4)
    _, out = ok.dqn_update_host(ok.capi.learner_params(**HP), cfg, shape, st, rg, B, 1)
    idx = out["index"]
    results = {}
    for dtype in (torch.float64, torch.float32):
        net = torch_net(shape, st["policy"], dtype)
        t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        loss = torch_loss(net, t(rg["state"][idx]), t(rg["next_state"][idx]), torch.tensor(rg["action"][idx]), t(rg["reward"][idx]).reshape(-1, 1),
                          t(rg["done"][idx]).reshape(-1, 1), float(f32(gamma)), mask_done)
        loss.backward()
        assert (net[0].grad[0] == 0).all() and net[1].grad[0] == 0  # autograd's ReLU'(0) is 0
        results[dtype] = (torch.cat([p.grad.reshape(-1) for p in net]).double().numpy(), float(loss.detach()))
    x, xn = rg["state"][idx].astype(np.float64), rg["next_state"][idx].astype(np.float64)
    W1, B1, W2, B2 = (a.astype(np.float64) for a in (w1, b1, w2, b2))

    def abs_sums(inp):
        hid = np.abs(B1) + np.abs(inp) @ np.abs(W1).T
        return hid, np.abs(B2) + hid @ np.abs(W2).T

    hid_abs, Z = abs_sums(x)
    _, Zn = abs_sums(xn)
    g = float(f32(gamma)) * ((1.0 - rg["done"][idx].astype(np.float64)) if mask_done else 1.0)
    rows, act = np.arange(B), rg["action"][idx]
    S = Z[rows, act] + np.abs(rg["reward"][idx].astype(np.float64)) + g * Zn.max(axis=1)
    pre = x @ W1.T + B1
    active = pre > -(R + 2) * U * hid_abs
    active[:, 0] = False  # exactly 0 on every side
    ds = S[:, None] * np.abs(W2)[act] * active
    seed = np.zeros((B, A))
    seed[rows, act] = S
    T = 2.0 / (B * A) * np.concatenate([(ds[:, :, None] * np.abs(x)[:, None, :]).reshape(B, -1).sum(0), ds.sum(0),
                                        (seed[:, :, None] * np.maximum(pre, 0.0)[:, None, :]).reshape(B, -1).sum(0), seed.sum(0)])
    E = np.zeros_like(T)
    E[H * R + H:H * R + H + A * H] = 2.0 / (B * A) * (seed[:, :, None] * ((R + 2) * U * hid_abs * active)[:, None, :]).reshape(B, -1).sum(0)
    assert (T[:R] == 0).all() and T[H * R] == 0
    sums = (32 + np.log2((B + 31) // 32) + 3) * U
    k_e = (R + H / 8.0 + 12.0) * U
    bound = 2.0 * ((sums + (R + A + 16) * U + k_e) * T + E) + 1e-300
    want, t32 = results[torch.float64][0], results[torch.float32][0]
    err, err32 = np.abs(out["grad_policy"].astype(np.float64) - want), np.abs(t32 - want)
    print("%s: max |g - g64| / bound = %.3g (torch fp32: %.3g), max |g| = %.3g, max bound = %.3g" % (
        shape, (err / bound).max(), (err32 / bound).max(), np.abs(want).max(), bound.max()))
    assert (err <= bound).all() and (err32 <= bound).all()
    lb = 2.0 * (sums + 2.0 * k_e + 2 * U) * (S ** 2).sum() / (B * A)
    e_l, e_l32 = abs(float(out["loss"][0]) - results[torch.float64][1]), abs(results[torch.float32][1] - results[torch.float64][1])
    print("    loss %.6g: |loss - f64| = %.3g (torch fp32: %.3g), bound %.3g" % (results[torch.float64][1], e_l, e_l32, lb))
    assert e_l <= lb and e_l32 <= lb


def test_three_iterations_against_torch_float64(ok):
    """Three iterations on one batch against the reference's loop in torch float64 with torch.optim.Adam: the parameters' largest
    deviation is printed as a fraction of steps * lr beside torch's own float32 loop and recorded in docs/HISTORY.md section 21, not
    asserted (Adam amplifies rounding where a gradient is near eps; the first iteration's bound above and section 16's Adam bound are
    the hard assertions)."""
    import torch
    shape = (5, 128, 5)
    R, H, A = shape
    B = 100
    rng = np.random.default_rng(77)
    st = fresh_state(rng, shape)
    rg = filled_ring(rng, R, A, 500, 500)
    got, out = ok.dqn_update_host(ok.capi.learner_params(**HP), ok.capi.dqn_config(seed=4), shape, st, rg, B, 3)
    idx = out["index"]
    lr, finals, losses = float(f32(HP["lr"])), {}, {}
    for dtype in (torch.float64, torch.float32):
        net = torch_net(shape, st["policy"], dtype)
        opt = torch.optim.Adam(net, lr=lr, betas=(float(f32(0.9)), float(f32(0.999))), eps=float(f32(1e-8)))
        t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        losses[dtype] = []
        for _ in range(3):
            loss = torch_loss(net, t(rg["state"][idx]), t(rg["next_state"][idx]), torch.tensor(rg["action"][idx]), t(rg["reward"][idx]).reshape(-1, 1),
                              t(rg["done"][idx]).reshape(-1, 1), float(f32(0.99)), False)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses[dtype].append(float(loss.detach()))
        finals[dtype] = torch.cat([p.detach().reshape(-1) for p in net]).double().numpy()
    dev = np.abs(got["policy"].astype(np.float64) - finals[torch.float64]).max() / (3 * lr)
    dev32 = np.abs(finals[torch.float32] - finals[torch.float64]).max() / (3 * lr)
    moved = np.abs(finals[torch.float64] - st["policy"].astype(np.float64)).max() / (3 * lr)
    print("largest parameter deviation from float64 = %.3g of steps * lr (torch fp32: %.3g); largest movement %.3g of steps * lr" % (dev, dev32, moved))
    print("losses: ours %s, float64 %s, torch fp32 %s" % (out["loss"].tolist(), losses[torch.float64], losses[torch.float32]))
    assert got["t"] == 3 and np.isfinite(got["policy"]).all() and np.isfinite(out["loss"]).all()


# ---- validation ----------------------------------------------------------------------------------------------------------------------

def test_validation(ok):
    L = ok.capi.load()
    shape = (5, 8, 5)
    rng = np.random.default_rng(1)
    st, rg = fresh_state(rng, shape), filled_ring(rng, 5, 5, 16, 16)
    lp = ok.capi.learner_params(**HP)

    def update(cfg=None, B=4, iterations=1, target=None, state=st, ring=rg, size=None, lp=lp, shape=shape):
        cfg = ok.capi.dqn_config() if cfg is None else cfg
        with pytest.raises(ok.capi.OkenvError) as e:
            ok.dqn_update_host(lp, cfg, shape, state, ring, B, iterations, target=target, size=size)
        assert e.value.code == -1, e.value
        return str(e.value)

    assert "B and iterations" in update(B=0) and "B and iterations" in update(iterations=0)
    assert "gamma" in update(ok.capi.dqn_config(gamma=1.5)) and "gamma" in update(ok.capi.dqn_config(gamma=float("nan")))
    assert "gamma" in update(ok.capi.dqn_config(gamma=-0.1))
    bad = ok.capi.dqn_config()
    bad.flags = 6
    assert "unknown flags" in update(bad)
    bad = ok.capi.dqn_config()
    bad.target_network = 2
    assert "target_network" in update(bad)
    assert "target is required" in update(ok.capi.dqn_config(target_network=True)) and "target is required" in update(target=st["policy"])
    assert "width" in update(shape=(5, 300, 5)) and "size" in update(size=-1)
    assert "lr" in update(lp=ok.capi.learner_params(lr=0.0))
    null_state = ok.capi.OkenvLearnerState()
    ring_s = ok.capi.fill_pointers(ok.capi.OkenvReplayRing(), {k: rg[k] for k in RING_FIELDS}, "ring")
    out = ok.capi.OkenvDqnOutput()
    cfg = ok.capi.dqn_config()
    assert L.okenv_dqn_update_host(C.byref(lp), C.byref(cfg), 5, 8, 5, C.byref(null_state), None, C.byref(ring_s), 16, 4, 1, 0, 0, C.byref(out)) == -1
    assert L.okenv_dqn_update_host(C.byref(lp), None, 5, 8, 5, C.byref(null_state), None, C.byref(ring_s), 16, 4, 1, 0, 0, C.byref(out)) == -1
    assert L.okenv_dqn_update_host(None, C.byref(cfg), 5, 8, 5, C.byref(null_state), None, C.byref(ring_s), 16, 4, 1, 0, 0, C.byref(out)) == -1
    no_reward = ok.capi.fill_pointers(ok.capi.OkenvReplayRing(), {k: rg[k] for k in RING_FIELDS if k != "reward"}, "ring")
    new = {k: st[k].copy() for k in ("policy", "policy_m", "policy_v")}
    full_state = ok.capi.fill_pointers(ok.capi.OkenvLearnerState(), new, "state")
    assert L.okenv_dqn_update_host(C.byref(lp), C.byref(cfg), 5, 8, 5, C.byref(full_state), None, C.byref(no_reward), 16, 4, 1, 0, 0, None) == -1
    assert L.okenv_dqn_update_host(C.byref(lp), C.byref(cfg), 5, 8, 5, C.byref(full_state), None, C.byref(ring_s), 16, 4, 1, 0, 0, None) == 0
    # the push
    n, R = 4, 5
    state, action, alive, dist, crashed = step_data(rng, n, R, 5, "all")
    pushed = C.c_uint64(0)
    p = ok.capi.ptr

    def push(ring=ring_s, capacity=16, rays=R, flags=0, n=n, state=state, action=action, alive=alive, dist=dist, crashed=crashed, counter=pushed):
        return L.okenv_replay_push_host(C.byref(ring) if ring is not None else None, capacity, rays, C.byref(counter) if counter is not None else None,
                                        flags, n, p(state), p(action), p(alive), p(dist), p(crashed), None)

    assert push() == 0 and pushed.value == 4
    assert push(capacity=0) == -1 and b"capacity" in L.okenv_last_error(None)
    assert push(flags=2) == -1 and b"unknown flags" in L.okenv_last_error(None)
    assert push(ring=None) == -1 and push(ring=no_reward) == -1 and push(counter=None) == -1
    assert push(state=None) == -1 and b"state and action" in L.okenv_last_error(None)
    assert push(action=None) == -1
    assert push(alive=None) == -1 and b"alive" in L.okenv_last_error(None)
    assert push(alive=None, flags=ok.capi.REPLAY_PUSH_ALL) == 0
    assert push(dist=None) == -1 and push(crashed=None) == -1 and push(rays=65) == -1 and push(n=-1) == -1
    assert pushed.value == 8
    # entries that take the handle refuse a NULL one
    assert L.okenv_replay_create(None, 8, 0) == -1 and L.okenv_replay_push(None, None, None) == -1 and L.okenv_dqn_update(None, 4, 1, 0, 0, None) == -1
    assert L.okenv_dqn_params(None, C.byref(cfg)) == -1 and L.okenv_dqn_sync_target(None) == -1
    assert L.okenv_replay_reset(None) == -5 and L.okenv_replay_size(None, None, None) == -5 and L.okenv_replay_get(None, None) == -1
