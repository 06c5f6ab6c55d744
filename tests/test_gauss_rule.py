"""The continuous REINFORCE learner's rule on the CPU (include/okenv_gauss.h; okenv_debug_normal, okenv_gauss_act_host,
okenv_gauss_update_host, okenv_gauss_lds_bytes): the normal draw, the parameter order, acting and the update against an independent
numpy restatement (tests/_gauss_numpy.py) bit for bit, constructed cases, a closed loop with the oracle's step, the first step against
autograd in float64 with a derived bound, and validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _gauss_numpy as G_

f32 = np.float32
U = 2.0 ** -24
HP = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
SHAPES = [(1, 1, 1), (5, 128, 128), (6, 9, 13), (5, 33, 31), (5, 8, 7), (64, 64, 64)]
MS = (1, 31, 32, 33, 1000)
BS = (1, 32, 33, 1000, 4096)
MODES = {"reference": 0, "score": 1}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def fresh_state(rng, shape, scale, log_std=(0.0, 0.0)):
    R, H1, H2 = shape[:3]
    A = shape[3] if len(shape) > 3 else 2
    par = (rng.standard_normal(G_.num_params(R, H1, H2, A)) * scale).astype(f32)
    par[:A] = np.resize(np.asarray(log_std, dtype=f32), A)
    return {"params": par, "m": np.zeros_like(par), "v": np.zeros_like(par), "t": 0}


def make_batch(rng, shape, M, log_std=(0.0, 0.0)):
    R = shape[0]
    A = shape[3] if len(shape) > 3 else 2
    eps = rng.standard_normal((M, A)).astype(f32)
    return {"state": rng.random((M, R)).astype(f32), "eps": eps, "pre": (rng.standard_normal((M, A)) * 0.7).astype(f32),
            "ret": rng.standard_normal(M).astype(f32)}


# ---- the draw ----------------------------------------------------------------------------------------------------------------------

def test_normal_host_entry_equals_the_restatement(ok):
    w0, w1 = G_.word_pairs()
    got0, got1 = ok.debug_normal(w0, w1, device=ok.capi.DEBUG_ON_HOST)
    want0, want1 = G_.normal_pair(w0, w1)
    assert np.array_equal(bits(got0), bits(want0)) and np.array_equal(bits(got1), bits(want1))
    zero = w0 < 256  # u1 = 1: r = 0
    assert zero.any() and (got0[zero] == 0).all() and (got1[zero] == 0).all()
    top = np.sqrt(48.0 * np.log(2.0))
    assert np.abs(got0).max() <= top and np.abs(got1).max() <= top
    assert max(np.abs(got0[w0 >= 0xFFFFFF00]).max(), np.abs(got1[w0 >= 0xFFFFFF00]).max()) > 5.7


def test_philox_restatement_matches_the_known_answer():
    assert tuple(int(v) for v in G_.philox4x32(0, 0, 0, 0, 0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)  # Random123's kat_vectors
    assert tuple(int(v) for v in G_.philox4x32(*(0xFFFFFFFF,) * 6)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)


def test_normal_moments_over_2_20_counters(ok):
    """2^20 consecutive counters on stream 10 (2^10 agents x 2^10 draws): mean, variance, skewness and excess kurtosis of each
    component within five standard errors of a normal's (sqrt(1/n), sqrt(2/n), sqrt(6/n), sqrt(24/n))."""
    agents, draws = np.meshgrid(np.arange(1024, dtype=np.uint64) + np.uint64(7), np.arange(1024, dtype=np.uint64))
    w = G_.philox4x32(agents.ravel(), draws.ravel(), G_.STREAM, 0, 11, G_.KEY1)
    e0, e1 = ok.debug_normal(w[0].astype(np.uint32), w[1].astype(np.uint32), device=ok.capi.DEBUG_ON_HOST)
    n = e0.size
    assert n == 1 << 20
    for name, e in (("eps_0", e0), ("eps_1", e1)):
        e = e.astype(np.float64)
        assert np.abs(e).max() <= np.sqrt(48.0 * np.log(2.0))
        mean, var = e.mean(), e.var()
        skew, kurt = ((e - mean) ** 3).mean() / var ** 1.5, ((e - mean) ** 4).mean() / var ** 2 - 3.0
        print("%s: mean %.5f var %.5f skew %.5f excess kurtosis %.5f" % (name, mean, var, skew, kurt))
        assert abs(mean) <= 5 * np.sqrt(1.0 / n) and abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)
        assert abs(skew) <= 5 * np.sqrt(6.0 / n) and abs(kurt) <= 5 * np.sqrt(24.0 / n)
    assert abs(np.corrcoef(e0, e1)[0, 1]) <= 5 * np.sqrt(1.0 / n)


# ---- the parameter order -----------------------------------------------------------------------------------------------------------

def test_parameter_order_is_torchs(ok):
    import torch

    class Policy(torch.nn.Module):  # built like RLRacers/ReinforceContinuous/Policy.hpp:17-30
        def __init__(self, R, H1, H2):
            super().__init__()
            self.log_std = torch.nn.Parameter(torch.full((2,), 2.5))
            self.fc1 = torch.nn.Linear(R, H1)
            self.fc2 = torch.nn.Linear(H1, H2)
            self.mean = torch.nn.Linear(H2, 2)

    R, H1, H2 = 6, 9, 13
    torch.manual_seed(0)
    mod = Policy(R, H1, H2)
    names = [n for n, _ in mod.named_parameters()]
    assert names == ["log_std", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "mean.weight", "mean.bias"]
    flat = torch.cat([p.detach().reshape(-1) for p in mod.parameters()]).numpy()
    assert flat.size == ok.capi.gauss_num_params(R, H1, H2) == G_.num_params(R, H1, H2)
    ls, W1, b1, W2, b2, W3, b3 = G_.split(flat, R, H1, H2)
    for ours, theirs in ((ls, mod.log_std), (W1, mod.fc1.weight), (b1, mod.fc1.bias), (W2, mod.fc2.weight), (b2, mod.fc2.bias), (W3, mod.mean.weight),
                         (b3, mod.mean.bias)):
        assert np.array_equal(ours, theirs.detach().numpy())
    # the host entry reads that layout: greedy acting at eps = 0 is tanh(mean(relu(fc2(relu(fc1(x)))))) * scale + bias to rounding
    dist = (np.random.default_rng(0).random((4, R)) * 200).astype(f32)
    out = ok.gauss_act_host(ok.capi.gauss_config(H1, H2, greedy=True), flat, dist)
    x = torch.tensor(dist / f32(200.0))
    mu = mod.mean(torch.relu(mod.fc2(torch.relu(mod.fc1(x))))).detach().numpy()
    assert np.allclose(out["pre"], mu, rtol=0, atol=1e-5)
    assert np.allclose(out["action"], np.tanh(mu) * np.array([50, 10]) + np.array([50, 0]), rtol=0, atol=1e-3)


# ---- acting --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_act_host_entry_equals_the_numpy_restatement(ok, shape):
    R, H1, H2 = shape
    rng = np.random.default_rng(R * 1000 + H1)
    saturated = unsaturated = 0
    for N, log_std, greedy in itertools.product((1, 63, 65), (-3.0, 0.0, 2.5), (False, True)):
        st = fresh_state(rng, shape, 0.3, (log_std, log_std))
        dist = (rng.random((N, R)) * 200).astype(f32)
        crashed = (rng.random(N) < 0.3).astype(np.uint8)
        seed, base, draw = int(rng.integers(1 << 32)), int(rng.integers(1 << 31)), int(rng.integers(1 << 32))
        scale, bias = (50.0, 10.0), (50.0, 0.0)
        cfg = ok.capi.gauss_config(H1, H2, scale, bias, greedy, seed, base)
        got = ok.gauss_act_host(cfg, st["params"], dist, crashed, draw)
        want = G_.act(st["params"], (R, H1, H2, 2), dist, seed, base, draw, greedy, scale, bias)
        for k in ("state", "pre", "action", "logp", "throttle", "steer"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (k, N, log_std, greedy)
        if greedy:
            assert np.isnan(got["eps"]).all()  # nothing drawn, nothing recorded
        else:
            assert np.array_equal(bits(got["eps"]), bits(want["eps"]))
            t = (got["action"] - np.array(bias, dtype=f32)) / np.array(scale, dtype=f32)
            saturated += int((np.abs(t) == 1).sum())
            unsaturated += int((np.abs(t) < 0.99).sum())
        assert np.array_equal(got["alive"], 1 - crashed)
        # a sharded population draws the unsharded streams
        if N == 65 and not greedy:
            lo = ok.gauss_act_host(ok.capi.gauss_config(H1, H2, scale, bias, greedy, seed, base + 40), st["params"], dist[40:], crashed[40:], draw)
            for k in ("eps", "pre", "action", "logp"):
                assert np.array_equal(bits(lo[k]), bits(got[k][40:]))
    assert saturated > 0 and unsaturated > 0  # t = +-1 exactly (c = 0) at log_std = 2.5, and samples well inside


# ---- the update ----------------------------------------------------------------------------------------------------------------------

def check_update(ok, shape, st, batch, B, accumulate, reduce, mode, order):
    lp = ok.capi.learner_params(clip=0.0, **HP)
    new, out = ok.gauss_update_host(lp, shape, st, batch, B, accumulate, reduce, mode, order)
    want_new, want = G_.update(st, tuple(shape[:3]) + (shape[3] if len(shape) > 3 else 2,), batch, B, accumulate, reduce, MODES[mode], order, **HP)
    tag = (shape, len(batch["ret"]), B, accumulate, reduce, mode, order is not None)
    assert new["t"] == want_new["t"], tag
    for k in ("params", "m", "v"):
        assert np.array_equal(bits(new[k]), bits(want_new[k])), (k,) + tag
    assert np.array_equal(bits(out["loss"]), bits(want["loss"])), tag
    assert np.array_equal(bits(out["grad"]), bits(want["grad"])), tag
    return new, out, want


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("shape", SHAPES)
def test_update_host_entry_equals_the_numpy_restatement(ok, shape, M):
    rng = np.random.default_rng(shape[0] * 7 + shape[1] + M)
    st = fresh_state(rng, shape, 0.3)
    st["t"] = 3
    st["m"] = (rng.standard_normal(st["params"].size) * 0.01).astype(f32)
    st["v"] = (rng.random(st["params"].size) * 0.01).astype(f32)
    batch = make_batch(rng, shape, M)
    perm = rng.permutation(M).astype(np.int32)
    perm[0] = -5 if M > 1 else 0  # an index outside 0 .. M-1 counts as the nearest valid one
    for B, accumulate, reduce, mode, order in itertools.product(BS, (True, False), ("sum", "mean"), MODES, (None, perm)):
        check_update(ok, shape, st, batch, B, accumulate, reduce, mode, order)


def test_every_batch_size_beyond_m_is_one_slice(ok):
    rng = np.random.default_rng(5)
    shape = (6, 9, 13)
    st, batch = fresh_state(rng, shape, 0.3), make_batch(rng, shape, 33)
    lp = ok.capi.learner_params(clip=0.0, **HP)
    ref = ok.gauss_update_host(lp, shape, st, batch, 33)
    for B in (1000, 4096):
        got = ok.gauss_update_host(lp, shape, st, batch, B)
        assert np.array_equal(bits(got[0]["params"]), bits(ref[0]["params"])) and np.array_equal(bits(got[1]["grad"]), bits(ref[1]["grad"]))


def test_output_size_one_and_value_shapes(ok):
    """The helpers take 1 <= A <= 8: a value-like network (A = 1) and A = 3 (the third component takes the second block's words)."""
    rng = np.random.default_rng(8)
    for A in (1, 3, 8):
        shape = (5, 9, 13, A)
        st, batch = fresh_state(rng, shape, 0.3), make_batch(rng, shape, 70)
        for mode in MODES:
            check_update(ok, shape, st, batch, 33, True, "sum", mode, None)


def test_two_calls_continue_one_run(ok):
    rng = np.random.default_rng(6)
    shape = (5, 33, 31)
    st, batch = fresh_state(rng, shape, 0.3), make_batch(rng, shape, 96)
    lp = ok.capi.learner_params(clip=0.0, **HP)
    for mode in MODES:
        one, _ = ok.gauss_update_host(lp, shape, st, batch, 32, False, "mean", mode)
        first = {k: v[:64] for k, v in batch.items()}
        second = {k: v[64:] for k, v in batch.items()}
        half, _ = ok.gauss_update_host(lp, shape, st, first, 32, False, "mean", mode)
        two, _ = ok.gauss_update_host(lp, shape, half, second, 32, False, "mean", mode)
        assert two["t"] == one["t"] == 3
        for k in ("params", "m", "v"):
            assert np.array_equal(bits(two[k]), bits(one[k]))


def test_constructed_cases(ok):
    rng = np.random.default_rng(9)
    shape = (5, 8, 7)
    R, H1, H2 = shape
    lp = ok.capi.learner_params(clip=0.0, **HP)
    # G = 0: zero loss and gradient (the seeds are -(0 * c)), the parameters do not move
    st, batch = fresh_state(rng, shape, 0.3), make_batch(rng, shape, 40)
    batch["ret"][:] = 0
    for mode in MODES:
        new, out, _ = check_update(ok, shape, st, batch, 4096, True, "sum", mode, None)
        assert (out["grad"] == 0).all() and out["loss"][0] == 0 and np.array_equal(bits(new["params"]), bits(st["params"]))
    # a pre-activation of exactly 0 in either hidden layer: ReLU's derivative there is 0
    st = fresh_state(rng, shape, 0.3)
    ls, W1, b1, W2, b2, W3, b3 = G_.split(st["params"], R, H1, H2)
    W1[2, :] = 0
    b1[2] = 0  # unit 2 of layer 1 is 0 for every input
    W2[4, :] = 0
    b2[4] = 0  # unit 4 of layer 2 likewise
    batch = make_batch(rng, shape, 40)
    for mode in MODES:
        _, out, _ = check_update(ok, shape, st, batch, 4096, True, "sum", mode, None)
        g = G_.split(out["grad"], R, H1, H2)
        assert (g[1][2] == 0).all() and g[2][2] == 0 and (g[3][4] == 0).all() and g[4][4] == 0
        assert np.abs(g[3]).max() > 0
    # a saturated sample (t = +-1 exactly, u = 0, c = 0): in REFERENCE mode only log_std's -1 is left, loss finite
    st = fresh_state(rng, shape, 0.3, (2.5, 2.5))
    batch = make_batch(rng, shape, 1)
    batch["eps"][:] = (3.0, -3.0)
    batch["ret"][:] = 2.0
    _, out, _ = check_update(ok, shape, st, batch, 1, True, "sum", "reference", None)
    g = G_.split(out["grad"], R, H1, H2)
    assert (g[0] == 2.0).all() and all((a == 0).all() for a in g[1:]) and np.isfinite(out["loss"][0])


def test_recomputed_logp_equals_the_recorded_one_in_a_closed_loop(ok, oracle):
    """200 steps of act -> step with the oracle's step; afterwards REFERENCE mode's forward reproduces every recorded logp before the
    first optimiser step: the loss of the one-sample batch with G = 1 is -logp, bit for bit."""
    N, steps, seed, base = 24, 200, 17, 500
    fan = np.array([-70, -30, 0, 30, 70], dtype=f32)
    shape = (5, 128, 128)
    t = oracle.Track("Silverstone")
    env = oracle.OracleEnv(t.segments, N, fan.size, fan, (t.x, t.y, t.heading))
    env.set_lane_bounds(t.li, t.ri)
    env.reset_random(None, 1, seed, 0, base)
    env.step(1)
    rng = np.random.default_rng(4)
    st = fresh_state(rng, shape, 0.1, (0.0, -1.0))
    cfg = ok.capi.gauss_config(128, 128, seed=seed, agent_base=base)
    rec = []
    for k in range(steps):
        out = ok.gauss_act_host(cfg, st["params"], env.get(oracle.F_DIST), env.get(oracle.F_CRASHED), 1 + k)
        rec.append(out)
        env.set(oracle.F_THR, out["throttle"])
        env.set(oracle.F_STEER, out["steer"])
        env.step(1)
    M = steps * N
    batch = {"state": np.concatenate([r["state"] for r in rec]), "eps": np.concatenate([r["eps"] for r in rec]),
             "pre": np.concatenate([r["pre"] for r in rec]), "ret": np.ones(M, f32)}
    logp = np.concatenate([r["logp"] for r in rec])
    assert np.unique(logp).size > M // 4 and np.unique(batch["state"], axis=0).shape[0] > M // 4
    _, want = G_.update(st, shape + (2,), batch, 8192, mode=0, **HP)
    assert np.array_equal(bits(want["logp"]), bits(logp))
    lp = ok.capi.learner_params(clip=0.0, **HP)
    for k in range(0, M, 7):
        one = {name: v[k:k + 1] for name, v in batch.items()}
        _, out = ok.gauss_update_host(lp, shape, st, one, 1, want=("loss",))
        assert bits(out["loss"])[0] == bits(-logp[k:k + 1])[0], k


# ---- against autograd in float64 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape,scale", [((5, 128, 128), 0.12), ((6, 9, 13), 0.5), ((64, 64, 64), 0.1), ((5, 33, 31), 0.3)])
def test_first_step_against_torch_float64(ok, shape, scale, mode):
    """The first step's loss and gradient against autograd in float64.  REFERENCE is written exactly as the reference writes it
    (ReinforceAgent.hpp:70-83, 120-128): pre = mu + std * eps stays in the graph, log_prob = sum(-0.5 ((pre - mu) / std)^2 - log(std) -
    0.5 log(2 pi)) - sum log(1 - tanh(pre)^2 + 1e-6), loss = sum -(log_prob * G).  SCORE is the same with pre.detach() (the recorded pre).
    torch's own float32 run of the same graph must meet the same bounds.

    The bound, to first order in u = 2^-24 and then doubled; abs() of everything is taken from the float64 run.  It is written for any
    summation order (torch's matmul has its own), so every sum of n terms is charged n u times the sum of the terms' magnitudes:
      forward   habs1 = |b1| + |W1||x|, habs2 = |b2| + |W2| habs1, Z = |b3| + |W3| habs2 bound |pre1|, |pre2|, |mu|;
                e_h1 = (R + 2) u habs1, e_h2 = (R + H1 + 4) u habs2, e_mu = (R + H1 + H2 + 6) u Z.
      REFERENCE std, se = std eps and pre = mu + se: e_se = 3 u |se| (exp within 2 u), e_pre = e_mu + e_se + u |pre|;
                t = tanh(pre): e_t = (1 - t^2) e_pre + 2 u |t|;  w = 1 - t t: e_w = 2 |t| e_t + 2 u  (an ABSOLUTE error: near
                saturation w is a few multiples of 2^-24 and c below is coarse in either precision);
                c = 2 t w / (w + d), d = 1e-6: dc/dt = 2 w / (w + d) <= 2 and dc/dw = 2 t d / (w + d)^2, which decreases in w, so by the
                mean value theorem e_c = 2 e_t + 2 |t| d e_w / (max(w - e_w, 0) + d)^2 + 5 u |c|;
                seeds: E_mu = |G| (e_c + u |c|), E_ls = |G| (e_c |se| + |c| e_se + 2 u (|c se| + 1)).
      SCORE     z = (pre - mu) / std: e_z = e_mu / std + 4 u |z|;  E_mu = |G| (e_z + 4 u |z|) / std,  E_ls = |G| (2 |z| e_z + 2 u (z^2 + 1)).
      backward  D = |seed on mu|: d2 = (D |W3|) [pre2 > 0], E_d2 = (E_mu |W3|) [..] + (A + 1) u d2;  d1 = (d2 |W2|) [pre1 > 0],
                E_d1 = (E_d2 |W2|) [..] + (H2 + 1) u d1.
      terms     a b with errors E_a, e_b: E_a |b| + |a| e_b + u |a| |b|, summed over the samples; the sum over the M samples adds
                (M + 1) u sum |a| |b|.
      loss      n_k = -0.5 z^2 - log_std - 0.919: e_n = |z| e_z + 4 u (z^2 / 2 + |log_std| + 1);  l_k = log(w + d):
                e_l = e_w / (max(w - e_w, 0) + d) + 3 u (|l| + 1);  per sample |G| (sum_k (e_n + e_l) + 5 u sum_k (|n| + |l|)), and the sum
                over the samples adds (M + 1) u sum |G log_prob|.
    No pre-activation lies within 1e-6 of 0 (asserted), where the two precisions could take different sides of a ReLU."""
    import torch
    R, H1, H2 = shape
    A, M, d = 2, 200, 1e-6
    rng = np.random.default_rng(R + H1 + len(mode))
    st = fresh_state(rng, shape, scale, (0.0, -0.5))
    batch = make_batch(rng, shape, M)
    _, out = ok.gauss_update_host(ok.capi.learner_params(clip=0.0, **HP), shape, st, batch, 4096, grad=mode)
    parts64 = [a.astype(np.float64) for a in G_.split(st["params"], R, H1, H2)]
    results = {}
    for dtype in (torch.float64, torch.float32):
        ls, W1, b1, W2, b2, W3, b3 = prm = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in parts64]
        x, G = torch.tensor(batch["state"], dtype=dtype), torch.tensor(batch["ret"], dtype=dtype)
        p1 = x @ W1.T + b1
        p2 = torch.relu(p1) @ W2.T + b2
        mu = torch.relu(p2) @ W3.T + b3
        std = torch.exp(ls)
        pre = mu + std * torch.tensor(batch["eps"], dtype=dtype) if mode == "reference" else torch.tensor(batch["pre"], dtype=dtype)
        logp = (-0.5 * ((pre - mu) / std) ** 2 - torch.log(std) - 0.5 * np.log(2 * np.pi)).sum(1) - torch.log(1 - torch.tanh(pre) ** 2 + d).sum(1)
        loss = (-(logp * G)).sum()
        loss.backward()
        results[dtype] = (torch.cat([q.grad.reshape(-1) for q in prm]).double().numpy(), float(loss.detach()),
                          [v.detach().double().numpy() for v in (p1, p2, mu, pre, logp)])
    want, loss64, (p1, p2, mu, pre, logp) = results[torch.float64]
    assert np.abs(p1).min() > 1e-6 and np.abs(p2).min() > 1e-6
    ls, W1, b1, W2, b2, W3, b3 = (np.abs(a) for a in parts64)
    x, G = np.abs(batch["state"].astype(np.float64)), np.abs(batch["ret"].astype(np.float64))[:, None]
    habs1 = b1[None, :] + x @ W1.T
    habs2 = b2[None, :] + habs1 @ W2.T
    Z = b3[None, :] + habs2 @ W3.T
    e_h1, e_h2, e_mu = (R + 2) * U * habs1, (R + H1 + 4) * U * habs2, (R + H1 + H2 + 6) * U * Z
    std = np.exp(parts64[0])[None, :]
    t = np.tanh(pre)
    w = 1 - t * t
    if mode == "reference":
        eps = batch["eps"].astype(np.float64)
        se = np.abs(std * eps)
        z, e_z = np.abs(eps), 0.0
        e_se = 3 * U * se
        e_pre = e_mu + e_se + U * np.abs(pre)
        e_t = w * e_pre + 2 * U * np.abs(t)
        e_w = 2 * np.abs(t) * e_t + 2 * U
        c = np.abs(2 * t * w / (w + d))
        e_c = 2 * e_t + 2 * np.abs(t) * d * e_w / (np.maximum(w - e_w, 0) + d) ** 2 + 5 * U * c
        D, E_mu, E_ls = G * c, G * (e_c + U * c), G * (e_c * se + c * e_se + 2 * U * (c * se + 1))
    else:
        z = np.abs((pre - mu) / std)
        e_z = e_mu / std + 4 * U * z
        e_w = 2 * np.abs(t) * 2 * U * np.abs(t) + 2 * U
        D, E_mu, E_ls = G * z / std, G * (e_z + 4 * U * z) / std, G * (2 * z * e_z + 2 * U * (z * z + 1))
    m1, m2 = p1 > 0, p2 > 0
    d2 = (D @ W3) * m2
    E_d2 = (E_mu @ W3) * m2 + (A + 1) * U * d2
    d1 = (d2 @ W2) * m1
    E_d1 = (E_d2 @ W2) * m1 + (H2 + 1) * U * d1

    def outer(a, E_a, b, e_b):  # (sum of the terms' error bounds, sum of the terms' magnitudes) per parameter
        err = E_a.T @ b + a.T @ e_b + U * (a.T @ b)
        return err.reshape(-1), (a.T @ b).reshape(-1)

    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    h1b, h2b = habs1 * m1, habs2 * m2
    pieces = [(E_ls.sum(0), (G * (np.abs(c * se) + 1) if mode == "reference" else G * (z * z + 1)).sum(0)), outer(d1, E_d1, x, 0 * x), outer(d1, E_d1, one, zero),
              outer(d2, E_d2, h1b, e_h1 * m1), outer(d2, E_d2, one, zero), outer(D, E_mu, h2b, e_h2 * m2), outer(D, E_mu, one, zero)]
    err_terms, mags = np.concatenate([a for a, _ in pieces]), np.concatenate([b for _, b in pieces])
    bound = 2.0 * (err_terms + (M + 1) * U * mags) + 1e-300
    err, err32 = np.abs(out["grad"].astype(np.float64) - want), np.abs(results[torch.float32][0] - want)
    print("%s %s: max |g - g64| / bound = %.3g (torch fp32: %.3g), max |g| = %.3g, max bound = %.3g, median bound / |g| = %.3g" % (
        shape, mode, (err / bound).max(), (err32 / bound).max(), np.abs(want).max(), bound.max(), np.median(bound / (np.abs(want) + 1e-30))))
    assert (err <= bound).all() and (err32 <= bound).all()
    lsv = ls[None, :]
    n_abs = z * z / 2 + lsv + 0.919
    l_abs = np.abs(np.log(w + d))
    e_n = z * e_z + 4 * U * (z * z / 2 + lsv + 1)
    e_l = e_w / (np.maximum(w - e_w, 0) + d) + 3 * U * (l_abs + 1)
    per = G[:, 0] * ((e_n + e_l).sum(1) + 5 * U * (n_abs + l_abs).sum(1))
    lb = 2.0 * (per.sum() + (M + 1) * U * (G[:, 0] * np.abs(logp)).sum())
    print("    loss: |ours - f64| = %.3g (torch fp32: %.3g), bound %.3g, |loss| = %.3g" % (
        abs(float(out["loss"][0]) - loss64), abs(results[torch.float32][1] - loss64), lb, abs(loss64)))
    assert abs(float(out["loss"][0]) - loss64) <= lb and abs(results[torch.float32][1] - loss64) <= lb


# ---- validation ----------------------------------------------------------------------------------------------------------------------

def test_lds_budget(ok):
    budget = ok.capi.GAUSS_LDS_BUDGET
    for shape in ((5, 128, 128), (15, 128, 128), (64, 64, 64)):
        assert 0 < ok.capi.gauss_lds_bytes(*shape) <= budget, shape
    assert ok.capi.gauss_lds_bytes(64, 128, 128) > budget
    assert ok.capi.gauss_lds_bytes(5, 129, 128) == 0 and ok.capi.gauss_lds_bytes(0, 8, 8) == 0 and ok.capi.gauss_lds_bytes(5, 8, 8, 9) == 0
    # the pieces: the staged network with odd row strides, then 32 samples' rows and terms
    R, H1, H2, A = 5, 128, 128, 2
    net = H1 * (R | 1) + H1 + H2 * (H1 | 1) + H2 + A * H2 + 2 * A
    assert ok.capi.gauss_lds_bytes(R, H1, H2) == 4 * (net + 32 * ((R | 1) + 2 * (H1 + 8) + 2 * (H2 + 8) + 16) + 32)


def test_validation(ok):
    L, capi = ok.capi.load(), ok.capi
    rng = np.random.default_rng(3)
    shape = (5, 8, 7)
    st, batch = fresh_state(rng, shape, 0.3), make_batch(rng, shape, 10)
    lp = capi.learner_params(clip=0.0, **HP)

    def refused(fn, *a, **kw):
        with pytest.raises(capi.OkenvError) as e:
            fn(*a, **kw)
        assert e.value.code == -1, e.value

    dist = np.ones((3, 5), f32)
    refused(ok.gauss_act_host, None, st["params"], dist)
    refused(ok.gauss_act_host, capi.gauss_config(8, 7), None, dist)
    for bad in (dict(hidden1=0), dict(hidden1=129), dict(hidden2=0), dict(hidden2=129), dict(greedy=2), dict(scale=(np.inf, 1.0)), dict(bias=(0.0, np.nan))):
        cfg = capi.gauss_config(**dict(dict(hidden1=8, hidden2=7), **bad))
        assert L.okenv_gauss_act_host(C.byref(cfg), capi.ptr(st["params"]), 5, 3, capi.ptr(dist), None, 0, *(None,) * 8) == -1, bad
    cfg = capi.gauss_config(8, 7)
    assert L.okenv_gauss_act_host(C.byref(cfg), capi.ptr(st["params"]), 5, -1, capi.ptr(dist), None, 0, *(None,) * 8) == -1
    assert L.okenv_gauss_act_host(C.byref(cfg), capi.ptr(st["params"]), 5, 3, None, None, 0, *(None,) * 8) == -1
    assert L.okenv_gauss_act_host(C.byref(cfg), capi.ptr(st["params"]), 65, 3, capi.ptr(dist), None, 0, *(None,) * 8) == -1
    big = capi.gauss_config(128, 128)  # (64, 128, 128) does not fit the LDS: refused, never shrunk
    assert L.okenv_gauss_act_host(C.byref(big), capi.ptr(np.zeros(capi.gauss_num_params(64, 128, 128), f32)), 64, 1, capi.ptr(np.ones((1, 64), f32)), None, 0,
                                  *(None,) * 8) == -1
    assert L.okenv_gauss_act_host(C.byref(cfg), capi.ptr(st["params"]), 5, 3, capi.ptr(dist), None, 0, *(None,) * 8) == 0  # every output NULL

    refused(ok.gauss_update_host, None, shape, st, batch, 4)
    refused(ok.gauss_update_host, lp, shape, st, batch, 4, reduce=None)
    refused(ok.gauss_update_host, lp, shape, st, batch, 0)
    refused(ok.gauss_update_host, lp, shape, st, batch, 4, reduce=2)
    refused(ok.gauss_update_host, lp, shape, st, batch, 4, grad=2)
    refused(ok.gauss_update_host, lp, shape, st, dict(batch, eps=None), 4, grad="reference")
    refused(ok.gauss_update_host, lp, shape, st, dict(batch, pre=None), 4, grad="score")
    refused(ok.gauss_update_host, lp, shape, st, dict(batch, state=None), 4)
    refused(ok.gauss_update_host, lp, shape, dict(st, m=None), batch, 4)
    refused(ok.gauss_update_host, lp, shape, dict(st, t=-1), batch, 4)
    for bad in ((0, 8, 7), (65, 8, 7), (5, 0, 7), (5, 129, 7), (5, 8, 0), (5, 8, 129), (5, 8, 7, 0), (5, 8, 7, 9), (64, 128, 128)):
        refused(ok.gauss_update_host, lp, bad, st, batch, 4)
    refused(ok.gauss_update_host, capi.learner_params(lr=0.0), shape, st, batch, 4)
    # the field the mode does not read may be missing
    ok.gauss_update_host(lp, shape, st, dict(batch, pre=None), 4, grad="reference")
    ok.gauss_update_host(lp, shape, st, dict(batch, eps=None), 4, grad="score")
    assert L.okenv_debug_normal(capi.DEBUG_ON_HOST, None, None, None, None, 1) == -1
    assert L.okenv_gauss_create(None, C.byref(cfg)) != 0 and L.okenv_gauss_act(None, None) != 0 and L.okenv_gauss_learner_create(None, C.byref(lp)) != 0
    assert L.okenv_gauss_update(None, None, None, 1, 1, None, None) != 0
