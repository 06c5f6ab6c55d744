"""Guided cost learning's rule on the CPU (include/okenv_gcl.h; okenv_gcl_act_host, okenv_gcl_cost_host, okenv_gcl_cost_update_host,
okenv_gcl_policy_update_host, okenv_gcl_lds_bytes): the parameter order, the state, acting and the three updates against an independent
numpy restatement (tests/_gcl_numpy.py) bit for bit, constructed cases, a closed loop with the oracle's step, the first step of each loss
against autograd in float64 with a derived bound, and validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _gcl_numpy as N_

f32 = np.float32
U = 2.0 ** -24
HP = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
CLIP = 0.2
# (R, H1, H2): the policy's and the value's widths; the cost network takes the same two widths on R + 2 inputs
SHAPES = [(7, 64, 64), (1, 1, 1), (6, 9, 13), (5, 33, 31), (62, 64, 64)]
MS = (1, 31, 32, 33, 1000)
BS = (1, 32, 33, 1000, 4096)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def fresh(rng, which, shape, scale, log_std=(0.0, 0.0), moments=False):
    par = (rng.standard_normal(N_.num_params(which, *shape)) * scale).astype(f32)
    if which == N_.POLICY:
        par[:2] = np.asarray(log_std, dtype=f32)
    st = {"params": par, "m": np.zeros_like(par), "v": np.zeros_like(par), "t": 0}
    if moments:
        st["t"] = 3
        st["m"] = (rng.standard_normal(par.size) * 0.01).astype(f32)
        st["v"] = (rng.random(par.size) * 0.01).astype(f32)
    return st


def rel_of(rng, n, R):
    """Hits up to 200 m away in every direction."""
    ang, d = rng.random((n, R)) * 2 * np.pi, rng.random((n, R)) * 200
    return np.stack([d * np.cos(ang), d * np.sin(ang)], axis=-1).astype(f32)


def make_batch(rng, shape, M):
    R = shape[0]
    return {"state": rng.random((M, R)).astype(f32), "pre": (rng.standard_normal((M, 2)) * 0.7).astype(f32),
            "logp": (-2.0 - rng.random(M) * 2).astype(f32), "ret": rng.standard_normal(M).astype(f32)}


def recorded_batch(ok, rng, shape, policy, M, seed=5):
    """A batch whose pre and logp were recorded by the host entry's act with `policy`: its ratios are exactly 1 under `policy`."""
    out = ok.gcl_act_host(ok.capi.gcl_config(shape[1], shape[2], 1, 1, seed=seed), policy, rel_of(rng, M, shape[0]), None, 9)
    return {"state": out["state"], "pre": out["pre"], "logp": out["logp"], "ret": rng.standard_normal(M).astype(f32)}


# ---- the parameter order and the state --------------------------------------------------------------------------------------------

def _modules(R, H1, H2):
    import torch

    class PolicyNet(torch.nn.Module):  # built like RLRacers/GuidedCostLearning/Networks.hpp: log_std registered last, listed first
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = torch.nn.Linear(R, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, 2)
            self.log_std = torch.nn.Parameter(torch.zeros(2))

        def forward(self, x):
            return torch.tanh(self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x)))))), self.log_std

    class ValueNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = torch.nn.Linear(R, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, 1)

        def forward(self, x):
            return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x))))).squeeze(1)

    class CostNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = torch.nn.Linear(R + 2, H1), torch.nn.Linear(H1, H2), torch.nn.Linear(H2, 1)
            self.fc3.weight.data.mul_(0.1)
            self.fc3.bias.data.mul_(0.0)

        def forward(self, s, a):
            return self.fc3(torch.tanh(self.fc2(torch.tanh(self.fc1(torch.cat([s, a], 1)))))).squeeze(1)

    torch.manual_seed(0)
    return PolicyNet(), ValueNet(), CostNet()


def test_parameter_order_is_torchs(ok):
    import torch
    R, H1, H2 = 6, 9, 13
    pol, val, cost = _modules(R, H1, H2)
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([0.25, -0.5]))
    assert [n for n, _ in pol.named_parameters()] == ["log_std", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
    for which, mod in ((N_.POLICY, pol), (N_.VALUE, val), (N_.COST, cost)):
        if which != N_.POLICY:
            assert [n for n, _ in mod.named_parameters()] == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
        flat = torch.cat([p.detach().reshape(-1) for p in mod.parameters()]).numpy()
        assert flat.size == ok.capi.gcl_num_params(which, R, H1, H2) == N_.num_params(which, R, H1, H2)
        pieces = N_.split(flat, which, R, H1, H2)
        theirs = ([mod.log_std] if which == N_.POLICY else [torch.zeros(0)]) + [mod.fc1.weight, mod.fc1.bias, mod.fc2.weight, mod.fc2.bias, mod.fc3.weight,
                                                                                  mod.fc3.bias]
        for ours, t in zip(pieces, theirs):
            assert np.array_equal(ours, t.detach().numpy())
    # the host entries read those layouts
    rng = np.random.default_rng(0)
    rel = rel_of(rng, 4, R)
    flat = {w: torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy() for w, m in ((N_.POLICY, pol), (N_.VALUE, val), (N_.COST, cost))}
    out = ok.gcl_act_host(ok.capi.gcl_config(H1, H2, H1, H2, greedy=True), flat[N_.POLICY], rel)
    x = torch.tensor(out["state"])
    assert np.allclose(out["pre"], pol(x)[0].detach().numpy(), rtol=0, atol=1e-5)
    a = torch.tensor(out["squashed"])
    assert np.allclose(ok.gcl_cost_host(flat[N_.COST], (R, H1, H2), out["state"], out["squashed"]), cost(x, a).detach().numpy(), rtol=0, atol=1e-5)


def test_state_formula_and_bank_rows(ok):
    """x = (rel_x^2 + rel_y^2) / 40000 of the recorded hits: the act record's state and the bank row made from a demonstration record's
    rel_xy by the same float32 expression in numpy and in torch agree bit for bit; so do the bank's action formulas."""
    import torch
    rng = np.random.default_rng(1)
    R = 7
    rel = rel_of(rng, 65, R)
    rel[0, 0] = (200.0, 0.0)
    rel[0, 1] = (0.0, 0.0)
    st = fresh(rng, N_.POLICY, (R, 8, 8), 0.3)
    out = ok.gcl_act_host(ok.capi.gcl_config(8, 8, 1, 1), st["params"], rel)
    want = N_.state_of(rel)
    assert np.array_equal(bits(out["state"]), bits(want)) and out["state"][0, 0] == 1.0 and out["state"][0, 1] == 0.0
    t = torch.tensor(rel)
    row = ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) / 40000.0).numpy()  # what a bank row is made with
    assert np.array_equal(bits(row), bits(out["state"]))
    dist = np.hypot(rel[..., 0].astype(np.float64), rel[..., 1].astype(np.float64))
    assert np.abs(out["state"] - (dist / 200.0) ** 2).max() < 1e-6  # the squared ratio, not the other actors' dist / 200


# ---- acting --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_act_host_entry_equals_the_numpy_restatement(ok, shape):
    R, H1, H2 = shape
    rng = np.random.default_rng(R * 1000 + H1)
    for N, log_std, greedy in itertools.product((1, 63, 65), (-3.0, 0.0, 1.0), (False, True)):
        st = fresh(rng, N_.POLICY, shape, 0.3, (log_std, log_std))
        rel = rel_of(rng, N, R)
        crashed = (rng.random(N) < 0.3).astype(np.uint8)
        seed, base, draw = int(rng.integers(1 << 32)), int(rng.integers(1 << 31)), int(rng.integers(1 << 32))
        scale, bias = (50.0, 10.0), (50.0, 0.0)
        got = ok.gcl_act_host(ok.capi.gcl_config(H1, H2, 1, 1, scale, bias, greedy, seed, base), st["params"], rel, crashed, draw)
        want = N_.act(st["params"], shape, rel, seed, base, draw, greedy, scale, bias)
        for k in ("state", "pre", "squashed", "action", "logp", "throttle", "steer"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (k, N, log_std, greedy)
        if greedy:
            assert np.isnan(got["eps"]).all()  # nothing drawn, nothing recorded
        else:
            assert np.array_equal(bits(got["eps"]), bits(want["eps"]))
        assert np.array_equal(got["alive"], 1 - crashed)  # crashed agents are acted for like the others
        assert (np.abs(got["squashed"]) <= 1).all() and (got["throttle"] >= 0).all() and (got["throttle"] <= 100).all() and (np.abs(got["steer"]) <= 10).all()
        if N == 65 and not greedy:  # a sharded population draws the unsharded streams
            lo = ok.gcl_act_host(ok.capi.gcl_config(H1, H2, 1, 1, scale, bias, greedy, seed, base + 40), st["params"], rel[40:], crashed[40:], draw)
            for k in ("eps", "pre", "squashed", "action", "logp"):
                assert np.array_equal(bits(lo[k]), bits(got[k][40:]))


def test_act_draws_stream_11(ok):
    """The normal draws are Philox stream 11's, not the Gaussian actor's stream 10."""
    import _gauss_numpy as G_
    rng = np.random.default_rng(2)
    st = fresh(rng, N_.POLICY, (5, 8, 8), 0.3)
    got = ok.gcl_act_host(ok.capi.gcl_config(8, 8, 1, 1, seed=3, agent_base=10), st["params"], rel_of(rng, 16, 5), None, 4)
    assert np.array_equal(bits(got["eps"]), bits(N_.draw_eps(3, np.arange(16) + 10, 4)))
    assert not np.array_equal(bits(got["eps"]), bits(G_.draw_eps(3, np.arange(16) + 10, 4)))


# ---- the cost network --------------------------------------------------------------------------------------------------------------

def check_cost(ok, shape, st, bank, batch, Me, seed):
    lp = ok.capi.learner_params(clip=0.0, **HP)
    new, out = ok.gcl_cost_update_host(lp, seed, shape, st, bank, batch, Me)
    want_new, want = N_.cost_update(st, shape, bank, batch, Me, seed, **HP)
    tag = (shape, len(batch["state"]), Me, len(bank["state"]))
    assert new["t"] == want_new["t"] == st["t"] + 1, tag
    for k in ("params", "m", "v"):
        assert np.array_equal(bits(new[k]), bits(want_new[k])), (k,) + tag
    assert np.array_equal(bits(out["loss"]), bits(want["loss"])) and np.array_equal(bits(out["grad"]), bits(want["grad"])), tag
    return new, out, want


@pytest.mark.parametrize("shape", SHAPES)
def test_cost_forward_and_update_host_entries_equal_the_numpy_restatement(ok, shape):
    R = shape[0]
    rng = np.random.default_rng(R * 31 + shape[1])
    st = fresh(rng, N_.COST, shape, 0.3, moments=True)
    for E in (1, 33, 5000):
        bank = {"state": rng.random((E, R)).astype(f32), "action": (rng.random((E, 2)) * 2 - 1).astype(f32)}
        for Mp, Me in ((1, 1), (31, 33), (32, 32), (33, 1), (1000, 31), (33, 1000)):
            batch = {"state": rng.random((Mp, R)).astype(f32), "squashed": (rng.random((Mp, 2)) * 2 - 1).astype(f32)}
            got = ok.gcl_cost_host(st["params"], shape, batch["state"], batch["squashed"])
            assert np.array_equal(bits(got), bits(N_.cost(st["params"], shape, batch["state"], batch["squashed"])))
            _, _, want = check_cost(ok, shape, st, bank, batch, Me, seed=E + Mp)
            assert want["rows"].min() >= 0 and want["rows"].max() < E
            if E == 5000 and Me == 1000:
                assert np.unique(want["rows"]).size > 800  # uniform with replacement


def test_cost_two_calls_continue_one_run_and_draw_anew(ok):
    rng = np.random.default_rng(3)
    shape = (5, 9, 13)
    st = fresh(rng, N_.COST, shape, 0.3)
    bank = {"state": rng.random((200, 5)).astype(f32), "action": (rng.random((200, 2)) * 2 - 1).astype(f32)}
    batch = {"state": rng.random((40, 5)).astype(f32), "squashed": (rng.random((40, 2)) * 2 - 1).astype(f32)}
    a, _, w1 = check_cost(ok, shape, st, bank, batch, 40, 7)
    b, _, w2 = check_cost(ok, shape, a, bank, batch, 40, 7)
    assert b["t"] == 2 and not np.array_equal(w1["rows"], w2["rows"])  # update number d = t: other rows


def test_cost_constructed_cases(ok):
    """Logits 0, +-20 and +-120 (e = exp(-|c|) underflows to 0 at 120), in both sets, and saturated units with h = +-1."""
    rng = np.random.default_rng(4)
    shape = (5, 8, 7)
    R, H1, H2 = shape
    st = fresh(rng, N_.COST, shape, 0.3)
    _, W1, b1, W2, b2, W3, b3 = N_.split(st["params"], N_.COST, *shape)
    # the logit is b3 + W3[0, 0] * tanh(b2[0]) with everything else cut: c = logit * tanh(40) = logit exactly (tanh(40) is 1.0f)
    W3[:] = 0
    W2[0, :] = 0
    b2[0] = 40.0
    W1[1, :] = 0
    b1[1] = -40.0  # a saturated unit of the first layer, h = -1
    lp = ok.capi.learner_params(clip=0.0, **HP)
    for logit in (0.0, 20.0, -20.0, 120.0, -120.0):
        W3[0, 0] = logit
        b3[0] = 0.0
        bank = {"state": rng.random((3, R)).astype(f32), "action": (rng.random((3, 2)) * 2 - 1).astype(f32)}
        batch = {"state": rng.random((5, R)).astype(f32), "squashed": (rng.random((5, 2)) * 2 - 1).astype(f32)}
        h1, h2, z3 = N_.forward(st["params"], N_.COST, shape, np.concatenate([batch["state"], batch["squashed"]], 1))
        assert (z3[:, 0] == f32(logit)).all() and (h2[:, 0] == 1).all() and (h1[:, 1] == -1).all()  # present, not merely allowed
        _, out, want = check_cost(ok, shape, st, bank, batch, 4, 1)
        assert np.isfinite(out["loss"]).all() and np.isfinite(out["grad"]).all()
        e = np.exp(-abs(np.float64(logit)))
        softplus = lambda c: max(c, 0.0) + np.log1p(np.exp(-abs(c)))  # noqa: E731
        assert abs(float(out["loss"][0]) - (softplus(logit) + softplus(-logit))) <= 1e-5 * max(1.0, abs(logit))
        g = N_.split(out["grad"], N_.COST, *shape)
        sig = 1 / (1 + e) if logit >= 0 else e / (1 + e)
        assert abs(float(g[6][0]) - (sig + sig - 1)) < 1e-6  # db3 = mean sigmoid + mean (sigmoid - 1)
        assert (g[3][0] == 0).all() and g[4][0] == 0 and (g[1][1] == 0).all()  # through h = +-1 nothing flows: 1 - h h = 0
        if abs(logit) == 120:
            assert N_.expf(f32(-120.0)) == 0  # e underflows; the loss is |c| exactly
            assert out["loss"][0] == f32(120.0)


# ---- the policy / value update -----------------------------------------------------------------------------------------------------

def check_policy(ok, shape, pol, val, batch, B, accumulate, reduce, order):
    lp = ok.capi.learner_params(clip=CLIP, **HP)
    newp, newv, out = ok.gcl_policy_update_host(lp, shape, pol, val, batch, B, accumulate, reduce, order)
    wantp, wantv, want = N_.policy_update(pol, val, shape, batch, B, accumulate, reduce, order, CLIP, **HP)
    tag = (shape, len(batch["ret"]), B, accumulate, reduce, order is not None)
    assert newp["t"] == newv["t"] == wantp["t"] == wantv["t"], tag
    for new, wanted in ((newp, wantp), (newv, wantv)):
        for k in ("params", "m", "v"):
            assert np.array_equal(bits(new[k]), bits(wanted[k])), (k,) + tag
    for k in ("policy_loss", "value_loss", "grad_policy", "grad_value", "adv"):
        assert np.array_equal(bits(out[k]), bits(want[k])), (k,) + tag
    assert np.array_equal(out["clipped"], want["clipped"]), tag
    return newp, newv, out, want


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("shape", SHAPES)
def test_policy_update_host_entry_equals_the_numpy_restatement(ok, shape, M):
    """Every M, B, accumulate, reduce and order of the issue's lists, crossed in full; only at M = 1000 with B = 1 (a thousand slices in
    numpy) two of the eight combinations of (accumulate, reduce, order) run, which between them still hold every value of each."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1] + M)
    pol, val = fresh(rng, N_.POLICY, shape, 0.3, (0.0, -0.5), moments=True), fresh(rng, N_.VALUE, shape, 0.3, moments=True)
    batch = make_batch(rng, shape, M)
    # logp_old near the recomputed logp, so that ratios fall below, inside and above the range
    batch["logp"] = (N_.policy_update(pol, val, shape, batch, 4096)[2]["logp"] + rng.standard_normal(M) * 0.3).astype(f32)
    perm = rng.permutation(M).astype(np.int32)
    perm[0] = -5 if M > 1 else 0  # an index outside 0 .. M-1 counts as the nearest valid one
    clipped = 0
    for B, accumulate, reduce, order in itertools.product(BS, (True, False), ("sum", "mean"), (None, perm)):
        if M == 1000 and B == 1 and (accumulate, reduce, order is None) not in ((True, "sum", True), (False, "mean", False)):
            continue
        out = check_policy(ok, shape, pol, val, batch, B, accumulate, reduce, order)[2]
        clipped += int(out["clipped"].sum())
    assert M < 31 or clipped > 0


def test_policy_two_calls_continue_one_run(ok):
    """With accumulate = 0 the slices of one call equal as many calls of one slice each, as long as the advantages are the same: a
    batch of which every slice has the statistics of the whole is not to be had, so the second run is handed the advantages' inputs
    unchanged and must reproduce t, and the first slice's step bit for bit."""
    rng = np.random.default_rng(6)
    shape = (5, 33, 31)
    pol, val = fresh(rng, N_.POLICY, shape, 0.3), fresh(rng, N_.VALUE, shape, 0.3)
    batch = recorded_batch(ok, rng, shape, pol["params"], 96)
    lp = ok.capi.learner_params(clip=CLIP, **HP)
    one = ok.gcl_policy_update_host(lp, shape, pol, val, batch, 96, True, "mean")
    again = ok.gcl_policy_update_host(lp, shape, pol, val, batch, 96, True, "mean")
    for a, b in zip(one[:2], again[:2]):
        assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("params", "m", "v"))
    # two calls: the second continues t and the moments of the first
    two = ok.gcl_policy_update_host(lp, shape, one[0], one[1], batch, 96, True, "mean")
    wantp, wantv, _ = N_.policy_update(one[0], one[1], shape, batch, 96, True, "mean", None, CLIP, **HP)
    assert two[0]["t"] == two[1]["t"] == 2
    for got, want in ((two[0], wantp), (two[1], wantv)):
        assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in ("params", "m", "v"))


def test_policy_constructed_cases(ok):
    rng = np.random.default_rng(9)
    shape = (5, 8, 7)
    pol, val = fresh(rng, N_.POLICY, shape, 0.3, (0.0, -0.5)), fresh(rng, N_.VALUE, shape, 0.3)
    M = 64
    batch = recorded_batch(ok, rng, shape, pol["params"], M)
    base = N_.policy_update(pol, val, shape, batch, 4096, clip=CLIP, **HP)[2]
    assert (base["r"] == 1).all()  # recorded by the same rule: r is exactly 1 before any step
    # r < lo, r > hi, inside the range, and exactly 1; advantages of both signs on every kind; a tie s1 == s2 with adv = 0
    batch["logp"][0:16] += f32(0.5)
    batch["logp"][16:32] -= f32(0.5)
    batch["logp"][32:40] += f32(0.05)
    lo, hi = f32(1.0 - float(f32(CLIP))), f32(1.0 + float(f32(CLIP)))
    _, _, out, want = check_policy(ok, shape, pol, val, batch, 4096, True, "mean", None)
    r, adv = want["r"], want["adv"]
    below, above, inside, one = r < lo, r > hi, (r >= lo) & (r <= hi) & (r != 1), r == 1
    for kind in (below, above, inside, one):
        assert (kind & (adv > 0)).any() and (kind & (adv < 0)).any()
    assert out["clipped"][0] == int(below.sum() + above.sum()) == 32
    # adv = 0 exactly: M = 1 has std = 0 and adv = (raw - raw) / 1e-8 = 0, a tie s1 == s2 = 0 whatever r is; no NaN anywhere
    for shift in (0.0, 0.5, -0.5):
        single = {k: v[:1].copy() for k, v in batch.items()}
        single["logp"] = (base["logp"][:1] + f32(shift)).astype(f32)
        newp, newv, o, w = check_policy(ok, shape, pol, val, single, 1, True, "mean", None)
        assert o["adv"][0] == 0 and o["policy_loss"][0] == 0 and (o["grad_policy"] == 0).all() and np.array_equal(bits(newp["params"]), bits(pol["params"]))
        assert np.isfinite(o["value_loss"]).all() and np.isfinite(newv["params"]).all() and (o["grad_value"] != 0).any()
    # a pre-activation of exactly 0 in either ReLU layer, in both networks: ReLU's derivative there is 0
    for which, st in ((N_.POLICY, pol), (N_.VALUE, val)):
        _, W1, b1, W2, b2, _, _ = N_.split(st["params"], which, *shape)
        W1[2, :] = 0
        b1[2] = 0
        W2[4, :] = 0
        b2[4] = 0
    _, _, out, _ = check_policy(ok, shape, pol, val, batch, 4096, True, "mean", None)
    for which, key in ((N_.POLICY, "grad_policy"), (N_.VALUE, "grad_value")):
        g = N_.split(out[key], which, *shape)
        assert (g[1][2] == 0).all() and g[2][2] == 0 and (g[3][4] == 0).all() and g[4][4] == 0 and np.abs(g[3]).max() > 0


def test_closed_loop_recomputed_logp_equals_the_recorded_one(ok, oracle):
    """200 steps of act -> step with the oracle's step: afterwards the update's forward reproduces every recorded logp before the first
    optimiser step, so every ratio is exactly 1.  With r = 1 the surrogate is adv itself, so the loss is -mean(adv) bit for bit."""
    N, steps, seed, base = 24, 200, 17, 500
    fan = np.array([-90, -60, -30, 0, 30, 60, 90], dtype=f32)
    shape = (7, 64, 64)
    t = oracle.Track("Silverstone")
    env = oracle.OracleEnv(t.segments, N, fan.size, fan, (t.x, t.y, t.heading))
    env.set_lane_bounds(t.li, t.ri)
    env.reset_random(None, 1, seed, 0, base)
    env.step(1)
    rng = np.random.default_rng(4)
    pol, val = fresh(rng, N_.POLICY, shape, 0.1, (0.0, -1.0)), fresh(rng, N_.VALUE, shape, 0.1)
    cfg = ok.capi.gcl_config(64, 64, 1, 1, seed=seed, agent_base=base)
    rec = []
    for k in range(steps):
        rel = np.stack([env.get(oracle.F_REL_X), env.get(oracle.F_REL_Y)], axis=-1).reshape(N, fan.size, 2)
        out = ok.gcl_act_host(cfg, pol["params"], rel, env.get(oracle.F_CRASHED), 1 + k)
        rec.append(out)
        env.set(oracle.F_THR, out["throttle"])
        env.set(oracle.F_STEER, out["steer"])
        env.step(1)
    M = steps * N
    batch = {k: np.concatenate([r[k] for r in rec]) for k in ("state", "pre", "logp")}
    batch["ret"] = rng.standard_normal(M).astype(f32)
    # (crashed agents stand still and repeat their state; their draws, and so their logp, go on changing)
    assert np.unique(batch["logp"]).size > M // 4 and np.unique(batch["state"], axis=0).shape[0] > M // 8
    want = N_.policy_update(pol, val, shape, batch, 8192, clip=CLIP, **HP)[2]
    assert np.array_equal(bits(want["logp"]), bits(batch["logp"])) and (want["r"] == 1).all()
    _, _, out = ok.gcl_policy_update_host(ok.capi.learner_params(clip=CLIP, **HP), shape, pol, val, batch, 8192, True, "sum")
    assert out["clipped"][0] == 0
    import _gauss_numpy as G_
    cols = N_.chunk_columns(np.zeros((M, 0), f32), (-out["adv"]).astype(f32))
    assert bits(out["policy_loss"])[0] == bits(G_.tree(cols)[-1:])[0]


# ---- against autograd in float64 -----------------------------------------------------------------------------------------------------

def _mlp_bounds(pieces64, x, tanh_layers):
    """Error bounds of a float32 forward of in -> H1 -> H2 -> out written for any summation order: a sum of n terms is charged (n + 2) u
    times the sum of the terms' magnitudes (the products' roundings and the bias included), an activation with slope <= 1 passes its
    input's error on (tanh adds 2 u |h| of its own).  Returns (h1, h2, z3) of the float64 run and (e_h1, e_h2, e_z3)."""
    _, W1, b1, W2, b2, W3, b3 = pieces64
    act = np.tanh if tanh_layers else (lambda s: np.maximum(s, 0))
    p1 = x @ W1.T + b1
    h1 = act(p1)
    p2 = h1 @ W2.T + b2
    h2 = act(p2)
    z3 = h2 @ W3.T + b3
    aW1, aW2, aW3 = np.abs(W1), np.abs(W2), np.abs(W3)
    own = 2 * U if tanh_layers else 0.0
    e_h1 = (x.shape[1] + 2) * U * (np.abs(b1) + np.abs(x) @ aW1.T) + own * np.abs(h1)
    e_h2 = e_h1 @ aW2.T + (W2.shape[1] + 2) * U * (np.abs(b2) + np.abs(h1) @ aW2.T) + own * np.abs(h2)
    e_z3 = e_h2 @ aW3.T + (W3.shape[1] + 2) * U * (np.abs(b3) + np.abs(h2) @ aW3.T)
    return (p1, p2, h1, h2, z3), (e_h1, e_h2, e_z3)


def _grad_bounds(pieces64, x, fwd, errs, dz, E_dz, tanh_layers, extra=None):
    """Bounds on every parameter's summed gradient from the output seeds dz (float64 run) and their error bounds E_dz, to first order in
    u: dh = W^T d charged (n + 1) u, the activation's slope (exactly 0 / 1 for ReLU away from 0; 1 - h^2 for tanh, in error by
    2 |h| e_h + 2 u), every term a * b charged E_a |b| + |a| e_b + u |a b|, the sum over the M samples (M + 1) u times the magnitudes.
    Returns (bound, magnitude) per parameter in parameter order, before the division by the count."""
    _, W1, b1, W2, b2, W3, b3 = pieces64
    p1, p2, h1, h2, _ = fwd
    e_h1, e_h2, _ = errs
    M = x.shape[0]
    aW2, aW3 = np.abs(W2), np.abs(W3)

    def slope(p, h, e_h):
        if tanh_layers:
            return 1 - h * h, 2 * np.abs(h) * e_h + 2 * U
        return (p > 0).astype(np.float64), 0.0

    adz = np.abs(dz)
    dh2, E_dh2 = adz @ aW3, E_dz @ aW3 + (W3.shape[0] + 1) * U * (adz @ aW3)
    s2, e_s2 = slope(p2, h2, e_h2)
    d2, E_d2 = dh2 * s2, E_dh2 * s2 + dh2 * e_s2 + U * dh2 * s2
    dh1, E_dh1 = d2 @ aW2, E_d2 @ aW2 + (W2.shape[0] + 1) * U * (d2 @ aW2)
    s1, e_s1 = slope(p1, h1, e_h1)
    d1, E_d1 = dh1 * s1, E_dh1 * s1 + dh1 * e_s1 + U * dh1 * s1

    def outer(a, E_a, b, e_b):
        return (E_a.T @ b + a.T @ e_b + U * (a.T @ b)).reshape(-1), (a.T @ b).reshape(-1)

    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    pieces = ([extra] if extra is not None else []) + [outer(d1, E_d1, np.abs(x), 0 * x), outer(d1, E_d1, one, zero), outer(d2, E_d2, np.abs(h1), e_h1),
                                                      outer(d2, E_d2, one, zero), outer(adz, E_dz, np.abs(h2), e_h2), outer(adz, E_dz, one, zero)]
    err, mag = np.concatenate([a for a, _ in pieces]), np.concatenate([b for _, b in pieces])
    return err + (M + 1) * U * mag, mag


def _torch_pieces(pieces64, dtype):
    import torch
    return [torch.tensor(a, dtype=dtype, requires_grad=True) for a in pieces64]


def _flat_grad(prm):
    import torch
    return torch.cat([q.grad.reshape(-1) for q in prm if q.numel()]).double().numpy()


@pytest.mark.parametrize("shape,scale", [((7, 64, 64), 0.15), ((6, 9, 13), 0.5), ((62, 64, 64), 0.1), ((5, 33, 31), 0.3)])
def test_first_cost_step_against_torch_float64(ok, shape, scale):
    """BCEWithLogits(c_expert, 0) + BCEWithLogits(c_policy, 1), each a mean over its own set, against autograd in float64 on a module
    built like CostNet; torch's own float32 run must meet the same bound.  The bound: _mlp_bounds / _grad_bounds; the seed sigmoid(c)
    (or sigmoid(c) - 1) has slope <= 1/4 in c and is itself evaluated within 4 u (exp, 1 + e, one division: absolute, since it is at
    most 1), so E_seed = e_c / 4 + 4 u; softplus has slope <= 1: e_term = e_c + 4 u (|term| + 1).  Each set's sum is divided by its
    count (one more u); the whole is doubled."""
    import torch
    R, C1, C2 = shape
    rng = np.random.default_rng(R + C1)
    st = fresh(rng, N_.COST, shape, scale)
    E, Mp, Me = 300, 150, 170
    bank = {"state": rng.random((E, R)).astype(f32), "action": (rng.random((E, 2)) * 2 - 1).astype(f32)}
    batch = {"state": rng.random((Mp, R)).astype(f32), "squashed": (rng.random((Mp, 2)) * 2 - 1).astype(f32)}
    _, out = ok.gcl_cost_update_host(ok.capi.learner_params(clip=0.0, **HP), 11, shape, st, bank, batch, Me)
    rows = N_.expert_rows(11, np.arange(Me), 0, E)
    xe = np.concatenate([bank["state"][rows], bank["action"][rows]], 1).astype(np.float64)
    xp = np.concatenate([batch["state"], batch["squashed"]], 1).astype(np.float64)
    pieces64 = [a.astype(np.float64) for a in N_.split(st["params"], N_.COST, *shape)]
    results = {}
    for dtype in (torch.float64, torch.float32):
        prm = _torch_pieces(pieces64, dtype)
        _, W1, b1, W2, b2, W3, b3 = prm
        net = lambda x: (torch.tanh(torch.tanh(x @ W1.T + b1) @ W2.T + b2) @ W3.T + b3)[:, 0]  # noqa: E731
        ce, cp = net(torch.tensor(xe, dtype=dtype)), net(torch.tensor(xp, dtype=dtype))
        loss = torch.nn.functional.binary_cross_entropy_with_logits(ce, torch.zeros_like(ce)) + \
            torch.nn.functional.binary_cross_entropy_with_logits(cp, torch.ones_like(cp))
        loss.backward()
        results[dtype] = (_flat_grad(prm), float(loss.detach()))
    want, loss64 = results[torch.float64]
    bound, lbound = 0.0, 0.0
    for x, count, policy in ((xe, Me, False), (xp, Mp, True)):
        fwd, errs = _mlp_bounds(pieces64, x, True)
        c = fwd[4]
        sig = 1 / (1 + np.exp(-c))
        dz = sig - 1 if policy else sig
        E_dz = errs[2] / 4 + 4 * U
        b, mag = _grad_bounds(pieces64, x, fwd, errs, dz, E_dz, True)
        bound = bound + (b + U * mag) / count
        term = np.logaddexp(0, -c if policy else c)
        lbound += ((errs[2] + 4 * U * (term + 1)).sum() + (count + 2) * U * term.sum()) / count
    bound, lbound = 2.0 * bound + 1e-300, 2.0 * lbound
    err, err32 = np.abs(out["grad"].astype(np.float64) - want), np.abs(results[torch.float32][0] - want)
    print("cost %s: max |g - g64| / bound = %.3g (torch fp32: %.3g), max |g| = %.3g; loss |ours - f64| = %.3g (torch fp32: %.3g), bound %.3g" % (
        shape, (err / bound).max(), (err32 / bound).max(), np.abs(want).max(), abs(float(out["loss"][0]) - loss64), abs(results[torch.float32][1] - loss64), lbound))
    assert (err <= bound).all() and (err32 <= bound).all()
    assert abs(float(out["loss"][0]) - loss64) <= lbound and abs(results[torch.float32][1] - loss64) <= lbound


@pytest.mark.parametrize("shape,scale", [((7, 64, 64), 0.15), ((6, 9, 13), 0.5), ((62, 64, 64), 0.1), ((5, 33, 31), 0.3)])
def test_first_policy_and_value_step_against_torch_float64(ok, shape, scale):
    """updatePolicy's two losses (GCLAgent.hpp:146-168) against autograd in float64 on modules built like PolicyNet and ValueNet, with
    the recorded pre a constant; torch's own float32 run must meet the same bounds.  logp_old is the recorded logp shifted by up to
    +-0.1, so that the ratios are inside (0.8, 1.2) and well away from its ends (asserted): min and clamp then pass adv on whole.
      value     e = v - G: e_e = e_v + u |e|;  seed 2 e: E = 2 e_e;  term e^2: 2 |e| e_e + u e^2.
      adv       raw = G - v: e_raw = e_v + u |raw|.  Mean and std are formed in fp64 from the fp32 raws, so they move by at most
                mean(e_raw) and max(e_raw):  e_adv = (e_raw + mean(e_raw)) / std + |adv| max(e_raw) / std + 4 u |adv|  (x 1.01 for M / (M-1)).
      policy    mu = tanh(z3): e_mu = e_z3 + 2 u |mu|;  z = (pre - mu) / std with exp within 2 u: e_z = e_mu / std + 4 u |z|;
                n_k: e_n = |z| e_z + 4 u (z^2 / 2 + |log_std| + 1);  d = logp - logp_old: e_d = sum_k e_n + u (|logp| + |d|);
                r = exp(d): e_r = r (e_d + 2 u);  g = -adv r: E_g = |adv| e_r + r e_adv + u |adv| r;
                dmu = g z / std: (E_g |z| + |g| e_z) / std + 4 u |g z| / std;  dls = g (z^2 - 1): E_g |z^2 - 1| + 2 |g z| e_z + 3 u |g| (z^2 + 1);
                dz3 = dmu (1 - mu^2): E_dmu (1 - mu^2) + |dmu| (2 |mu| e_mu + 2 u) + u |dz3|;  term r adv: |adv| e_r + r e_adv + u |r adv|.
    _mlp_bounds / _grad_bounds carry these through the layers; the mean's division adds one u; the whole is doubled.  No
    pre-activation lies within 1e-6 of 0 (asserted)."""
    import torch
    R, H1, H2 = shape
    M = 200
    rng = np.random.default_rng(R + H1 + 1)
    pol, val = fresh(rng, N_.POLICY, shape, scale, (0.0, -0.5)), fresh(rng, N_.VALUE, shape, scale)
    batch = recorded_batch(ok, rng, shape, pol["params"], M)
    batch["logp"] = (batch["logp"] + (rng.random(M) * 0.2 - 0.1)).astype(f32)
    _, _, out = ok.gcl_policy_update_host(ok.capi.learner_params(clip=CLIP, **HP), shape, pol, val, batch, 4096, True, "mean")
    pp64 = [a.astype(np.float64) for a in N_.split(pol["params"], N_.POLICY, *shape)]
    vp64 = [a.astype(np.float64) for a in N_.split(val["params"], N_.VALUE, *shape)]
    x64, G64, pre64, old64 = (batch[k].astype(np.float64) for k in ("state", "ret", "pre", "logp"))
    results = {}
    for dtype in (torch.float64, torch.float32):
        pprm, vprm = _torch_pieces(pp64, dtype), _torch_pieces(vp64, dtype)
        x, G, pre, old = (torch.tensor(a, dtype=dtype) for a in (x64, G64, pre64, old64))
        mlp = lambda p, inp: torch.relu(torch.relu(inp @ p[1].T + p[2]) @ p[3].T + p[4]) @ p[5].T + p[6]  # noqa: E731
        v = mlp(vprm, x)[:, 0]
        adv = G - v.detach()
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        mu, std = torch.tanh(mlp(pprm, x)), torch.exp(pprm[0])
        eps = (pre - mu) / std
        logp = -0.5 * ((eps ** 2).sum(1) + 2 * pprm[0].sum() + 2 * np.log(2 * np.pi))
        ratio = torch.exp(logp - old)
        loss_pi = -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
        loss_v = torch.nn.functional.mse_loss(v, G)
        loss_pi.backward()
        loss_v.backward()
        results[dtype] = (_flat_grad(pprm), _flat_grad(vprm), float(loss_pi.detach()), float(loss_v.detach()), adv.double().numpy(),
                          ratio.detach().double().numpy())
    gp64, gv64, lp64, lv64, adv64, r64 = results[torch.float64]
    assert r64.min() > 0.85 and r64.max() < 1.15
    # the value network
    vf, ve = _mlp_bounds(vp64, x64, False)
    assert np.abs(vf[0]).min() > 1e-6 and np.abs(vf[1]).min() > 1e-6
    v64 = vf[4][:, 0]
    e_v = ve[2][:, 0]
    e = v64 - G64
    e_e = e_v + U * np.abs(e)
    vb, vmag = _grad_bounds(vp64, x64, vf, ve, (2 * e)[:, None], (2 * e_e)[:, None], False)
    vbound = 2.0 * (vb + U * vmag) / M + 1e-300
    lvb = 2.0 * ((2 * np.abs(e) * e_e + U * e * e).sum() + (M + 2) * U * (e * e).sum()) / M
    # the advantages
    raw = G64 - v64
    e_raw = e_v + U * np.abs(raw)
    sd = raw.std(ddof=1)
    e_adv = 1.01 * ((e_raw + e_raw.mean()) / sd + np.abs(adv64) * e_raw.max() / sd) + 4 * U * np.abs(adv64)
    for name, a in (("ours", out["adv"].astype(np.float64)), ("torch fp32", results[torch.float32][4])):
        assert (np.abs(a - adv64) <= 2.0 * e_adv).all(), name
    # the policy network
    pf, pe = _mlp_bounds(pp64, x64, False)
    assert np.abs(pf[0]).min() > 1e-6 and np.abs(pf[1]).min() > 1e-6
    ls = pp64[0][None, :]
    std = np.exp(ls)
    mu = np.tanh(pf[4])
    e_mu = pe[2] + 2 * U * np.abs(mu)
    z = (pre64 - mu) / std
    az = np.abs(z)
    e_z = e_mu / std + 4 * U * az
    e_n = az * e_z + 4 * U * (z * z / 2 + np.abs(ls) + 1)
    logp = (-0.5 * z * z - ls - 0.5 * np.log(2 * np.pi)).sum(1)
    d = logp - old64
    e_d = e_n.sum(1) + U * (np.abs(logp) + np.abs(d))
    r = np.exp(d)
    e_r = r * (e_d + 2 * U)
    aadv = np.abs(adv64)
    g = aadv * r
    E_g = (aadv * e_r + r * e_adv + U * g)[:, None]
    g = g[:, None]
    dmu = g * az / std
    E_dmu = (E_g * az + g * e_z) / std + 4 * U * dmu
    dls = g * np.abs(z * z - 1)
    E_dls = E_g * np.abs(z * z - 1) + 2 * g * az * e_z + 3 * U * g * (z * z + 1)
    dz3 = dmu * (1 - mu * mu)
    E_dz3 = E_dmu * (1 - mu * mu) + dmu * (2 * np.abs(mu) * e_mu + 2 * U) + U * dz3
    pb, pmag = _grad_bounds(pp64, x64, pf, pe, dz3, E_dz3, False, extra=(E_dls.sum(0), dls.sum(0)))
    pbound = 2.0 * (pb + U * pmag) / M + 1e-300
    lpb = 2.0 * ((aadv * e_r + r * e_adv + U * aadv * r).sum() + (M + 2) * U * (aadv * r).sum()) / M
    for name, gp, gv, lp_, lv in (("ours", out["grad_policy"].astype(np.float64), out["grad_value"].astype(np.float64), float(out["policy_loss"][0]),
                                   float(out["value_loss"][0])), ("torch fp32",) + results[torch.float32][:4]):
        ep, ev = np.abs(gp - gp64), np.abs(gv - gv64)
        print("%s %s: policy max err / bound = %.3g (max |g| %.3g), value %.3g (max |g| %.3g); losses |d| = %.3g / %.3g, bounds %.3g / %.3g" % (
            shape, name, (ep / pbound).max(), np.abs(gp64).max(), (ev / vbound).max(), np.abs(gv64).max(), abs(lp_ - lp64), abs(lv - lv64), lpb, lvb))
        assert (ep <= pbound).all() and (ev <= vbound).all(), name
        assert abs(lp_ - lp64) <= lpb and abs(lv - lv64) <= lvb, name


# ---- validation ----------------------------------------------------------------------------------------------------------------------

def test_lds_budget(ok):
    capi = ok.capi
    assert 0 < capi.gcl_lds_bytes(7, 64, 64, 64, 64) <= capi.GCL_LDS_BUDGET
    # the pieces of the largest kernel at the reference's shape, the cost network's: the staged network with odd row strides (and one
    # unused log_std slot per output), 32 samples' rows, terms and clip flags
    inp, H1, H2, A = 9, 64, 64, 1
    net = H1 * (inp | 1) + H1 + H2 * (H1 | 1) + H2 + A * H2 + 2 * A
    assert capi.gcl_lds_bytes(7, 64, 64, 64, 64) == 4 * (net + 32 * ((inp | 1) + 2 * (H1 + 8) + 2 * (H2 + 8) + 16) + 32 + 32)
    assert capi.gcl_lds_bytes(62, 128, 128, 128, 128) > capi.GCL_LDS_BUDGET  # refused, never shrunk
    for bad in ((63, 8, 8, 8, 8), (0, 8, 8, 8, 8), (5, 129, 8, 8, 8), (5, 8, 0, 8, 8), (5, 8, 8, 129, 8), (5, 8, 8, 8, 0)):
        assert capi.gcl_lds_bytes(*bad) == 0, bad


def test_validation(ok):
    L, capi = ok.capi.load(), ok.capi
    rng = np.random.default_rng(3)
    shape = (5, 8, 7)
    pol, val, cost = fresh(rng, N_.POLICY, shape, 0.3), fresh(rng, N_.VALUE, shape, 0.3), fresh(rng, N_.COST, shape, 0.3)
    batch = make_batch(rng, shape, 10)
    lp = capi.learner_params(clip=CLIP, **HP)

    def refused(fn, *a, **kw):
        with pytest.raises(capi.OkenvError) as e:
            fn(*a, **kw)
        assert e.value.code == -1, e.value

    rel = rel_of(rng, 3, 5)
    refused(ok.gcl_act_host, None, pol["params"], rel)
    refused(ok.gcl_act_host, capi.gcl_config(8, 7, 8, 7), None, rel)
    for bad in (dict(hidden1=0), dict(hidden1=129), dict(hidden2=0), dict(cost_hidden1=129), dict(cost_hidden2=0), dict(greedy=2), dict(scale=(np.inf, 1.0)),
                dict(bias=(0.0, np.nan))):
        cfg = capi.gcl_config(**dict(dict(hidden1=8, hidden2=7, cost_hidden1=8, cost_hidden2=7), **bad))
        refused(ok.gcl_act_host, cfg, np.zeros(capi.gcl_num_params("policy", 5, cfg.hidden1, cfg.hidden2), f32), rel)
    wide = rel_of(rng, 2, 63)  # R + 2 > 64
    refused(ok.gcl_act_host, capi.gcl_config(8, 7, 8, 7), np.zeros(capi.gcl_num_params("policy", 63, 8, 7), f32), wide)
    refused(ok.gcl_cost_host, np.zeros(capi.gcl_num_params("cost", 63, 8, 7), f32), (63, 8, 7), np.zeros((2, 63), f32), np.zeros((2, 2), f32))
    refused(ok.gcl_cost_host, None, shape, np.zeros((2, 5), f32), np.zeros((2, 2), f32))
    bank = {"state": rng.random((4, 5)).astype(f32), "action": rng.random((4, 2)).astype(f32)}
    cb = {"state": batch["state"], "squashed": batch["pre"]}
    ok.gcl_cost_update_host(lp, 0, shape, cost, bank, cb, 3)
    refused(ok.gcl_cost_update_host, None, 0, shape, cost, bank, cb, 3)
    refused(ok.gcl_cost_update_host, lp, 0, shape, cost, bank, cb, 0)  # Me < 1
    refused(ok.gcl_cost_update_host, lp, 0, shape, cost, {"state": np.zeros((0, 5), f32), "action": np.zeros((0, 2), f32)}, cb, 3)  # an empty bank
    refused(ok.gcl_cost_update_host, lp, 0, shape, cost, {"state": None, "action": None}, cb, 3)
    refused(ok.gcl_cost_update_host, lp, 0, shape, cost, bank, dict(cb, squashed=None), 3)
    refused(ok.gcl_cost_update_host, lp, 0, shape, dict(cost, v=None), bank, cb, 3)
    refused(ok.gcl_cost_update_host, lp, 0, (63, 8, 7), cost, bank, cb, 3)
    ok.gcl_policy_update_host(lp, shape, pol, val, batch, 4)
    refused(ok.gcl_policy_update_host, None, shape, pol, val, batch, 4)
    refused(ok.gcl_policy_update_host, lp, shape, pol, val, batch, 4, reduce=None)
    refused(ok.gcl_policy_update_host, lp, shape, pol, val, batch, 0)
    refused(ok.gcl_policy_update_host, lp, shape, pol, val, batch, 4, reduce=2)
    for field in ("state", "pre", "logp"):
        refused(ok.gcl_policy_update_host, lp, shape, pol, val, dict(batch, **{field: None}), 4)
    refused(ok.gcl_policy_update_host, lp, shape, dict(pol, m=None), val, batch, 4)
    refused(ok.gcl_policy_update_host, lp, shape, pol, dict(val, params=None), batch, 4)
    refused(ok.gcl_policy_update_host, lp, shape, dict(pol, t=-1), val, batch, 4)
    for bad in ((0, 8, 7), (63, 8, 7), (5, 0, 7), (5, 129, 7), (5, 8, 0), (5, 8, 129)):
        refused(ok.gcl_policy_update_host, lp, bad, pol, val, batch, 4)
    refused(ok.gcl_policy_update_host, capi.learner_params(lr=0.0), shape, pol, val, batch, 4)
    cfg = capi.gcl_config(8, 7, 8, 7)
    assert L.okenv_gcl_create(None, C.byref(cfg)) != 0 and L.okenv_gcl_act(None, None) != 0 and L.okenv_gcl_learner_create(None, C.byref(lp), C.byref(lp)) != 0
    assert L.okenv_gcl_cost_update(None, None, 1, 1, None) != 0 and L.okenv_gcl_policy_update(None, None, None, 1, 1, None, None) != 0
    assert L.okenv_gcl_set_expert(None, None, None, 1) != 0 and L.okenv_gcl_cost(None, None, None, 1, None) != 0
