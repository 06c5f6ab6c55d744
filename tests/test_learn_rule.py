"""PPO's update on the CPU (include/okenv_learn.h, okenv_ppo_update_host): the host entry against an independent numpy restatement
(tests/_learn_numpy.py) bit for bit, the continuation across calls, the first minibatch of a recorded episode, constructed ties and
edges, the gradients against torch autograd in float64 on the reference's expressions and Adam against torch.optim.Adam in float64,
both with derived bounds, and validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _learn_numpy as L_

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32
HP = dict(lr=3e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8)
SHAPES = [(5, 128, 3, 128), (1, 1, 2, 1), (7, 9, 4, 16), (64, 256, 8, 256), (6, 9, 4, 13), (8, 131, 3, 9)]
TABLE8 = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(8))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def fresh_state(rng, shape, scale=0.3):
    R, H, A, Hv = shape
    st = {"policy": (rng.standard_normal(L_.n_params(R, H, A)) * scale).astype(f32), "t": 0}
    st["policy_m"], st["policy_v"] = np.zeros_like(st["policy"]), np.zeros_like(st["policy"])
    if Hv:
        st["value"] = (rng.standard_normal(L_.n_params(R, Hv, 1)) * scale).astype(f32)
        st["value_m"], st["value_v"] = np.zeros_like(st["value"]), np.zeros_like(st["value"])
    return st


def random_batch(rng, shape, M, with_adv):
    R, H, A, Hv = shape
    b = {"state": rng.random((M, R)).astype(f32), "action": rng.integers(0, A, M).astype(np.int64),
         "prob": (0.05 + 0.9 * rng.random(M)).astype(f32), "ret": rng.standard_normal(M).astype(f32)}
    if with_adv:
        b["adv"] = rng.standard_normal(M).astype(f32)
    return b


def assert_same(got_state, got_out, want_state, want_out, what):
    assert got_state["t"] == want_state["t"], what
    for k in want_state:
        if k != "t":
            assert np.array_equal(bits(got_state[k]), bits(want_state[k])), (k,) + what
    for k in ("actor_loss", "critic_loss", "grad_policy", "grad_value"):
        if k in want_out and k in got_out:
            assert np.array_equal(bits(got_out[k]), bits(want_out[k])), (k,) + what
    assert np.array_equal(got_out["clipped"], want_out["clipped"]), what


# ---- host entry against the numpy restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_host_entry_equals_the_numpy_restatement(ok, shape):
    rng = np.random.default_rng(sum(shape))
    lp = ok.capi.learner_params(**HP)
    clipped_seen = 0
    for M, B, epochs, permuted, with_adv in itertools.product([1, 31, 32, 33, 1000], [1, 32, 100, 4096], [1, 3], [False, True], [True, False]):
        st = fresh_state(rng, shape)
        batch = random_batch(rng, shape, M, with_adv)
        order = np.stack([rng.permutation(M) for _ in range(epochs)]).astype(np.int32) if permuted else None
        got_state, got_out = ok.ppo_update_host(lp, shape, st, batch, B, epochs, order)
        want_state, want_out = L_.update(ok.debug_expf, HP, shape, st, batch, B, epochs, order)
        assert_same(got_state, got_out, want_state, want_out, (shape, M, B, epochs, permuted, with_adv))
        assert got_state["t"] == epochs * ((M + B - 1) // B)
        clipped_seen += int(got_out["clipped"].sum())
    assert clipped_seen > 0


@pytest.mark.parametrize("B", [513, 1500, 4096])
def test_host_entry_equals_the_numpy_restatement_above_seven_chunks(ok, B):
    """ok_learn_tree in the host entry at C = 17, 47 and 128 chunks (the cases above stop at C = 7: M = 1000 in minibatches of 4096
    is never run as one, B = 100 gives four): padded widths 32, 64 and 128, the guard `i + h < n` false at the first level for
    C = 17 and 47 and never for 128.  M = B + 40 adds a partial second minibatch (two chunks) to each of the two epochs.  These are
    the B of tests/test_gpu_update_geometry.py, whose device results are compared with this host entry."""
    shape = (7, 9, 4, 16)
    rng = np.random.default_rng(B)
    lp = ok.capi.learner_params(**HP)
    for permuted, with_adv in ((False, True), (True, False)):
        M = B + 40
        st = fresh_state(rng, shape)
        batch = random_batch(rng, shape, M, with_adv)
        order = np.stack([rng.permutation(M) for _ in range(2)]).astype(np.int32) if permuted else None
        got_state, got_out = ok.ppo_update_host(lp, shape, st, batch, B, 2, order)
        want_state, want_out = L_.update(ok.debug_expf, HP, shape, st, batch, B, 2, order)
        assert_same(got_state, got_out, want_state, want_out, (shape, M, B, permuted, with_adv))
        assert got_state["t"] == 4 and got_out["actor_loss"].size == 4


def test_two_calls_continue_one_run(ok):
    shape = (5, 128, 3, 128)
    rng = np.random.default_rng(3)
    lp = ok.capi.learner_params(**HP)
    st = fresh_state(rng, shape)
    batch = random_batch(rng, shape, 333, False)
    order = np.stack([rng.permutation(333) for _ in range(4)]).astype(np.int32)
    whole, out_whole = ok.ppo_update_host(lp, shape, st, batch, 100, 4, order)
    first, out_a = ok.ppo_update_host(lp, shape, st, batch, 100, 2, order[:2])
    assert first["t"] == 8
    second, out_b = ok.ppo_update_host(lp, shape, first, batch, 100, 2, order[2:])
    assert second["t"] == whole["t"] == 16
    for k in whole:
        if k != "t":
            assert np.array_equal(bits(whole[k]), bits(second[k])), k
    assert np.array_equal(bits(np.concatenate([out_a["actor_loss"], out_b["actor_loss"]])), bits(out_whole["actor_loss"]))
    restarted, _ = ok.ppo_update_host(lp, shape, dict(first, t=0), batch, 100, 2, order[2:])
    assert not np.array_equal(bits(restarted["policy"]), bits(whole["policy"]))  # t matters


# ---- a recorded episode's first minibatch --------------------------------------------------------------------------------------------

def recorded(ok, rng, shape, n, scale=0.3, prepare=None):
    R, H, A, Hv = shape
    st = fresh_state(rng, shape, scale)
    if prepare is not None:
        prepare(st)
    dist = (rng.random((n, R)) * 200.0).astype(f32)
    ap = ok.capi.actor_params(H, TABLE8[:A], Hv, "sample", 0.0, 11, 0)
    rec = ok.actor_act_host(ap, st["policy"], st.get("value"), dist, draw_index=5)
    return st, {"state": rec["state"], "action": rec["action"].astype(np.int64), "prob": rec["prob"], "ret": rng.standard_normal(n).astype(f32)}


@pytest.mark.parametrize("shape", [(5, 128, 3, 128), (7, 9, 4, 16)])
@pytest.mark.parametrize("with_adv", [True, False])
def test_first_minibatch_of_a_recorded_episode(ok, shape, with_adv):
    rng = np.random.default_rng(8)
    st, batch = recorded(ok, rng, shape, 333)
    if with_adv:
        batch["adv"] = rng.standard_normal(333).astype(f32)
        adv = batch["adv"]
    else:
        adv = batch["ret"] - L_.forward(st["value"], shape[0], shape[3], 1, batch["state"])[0][:, 0]
    _, out = ok.ppo_update_host(ok.capi.learner_params(**HP), shape, st, batch, 100, 1)
    assert out["clipped"][0] == 0  # the ratio is exactly 1: the forward reproduces the recorded probability bit for bit
    assert bits(out["actor_loss"][:1])[0] == bits(np.array([L_.rule_mean(-adv[:100])]))[0]


def test_constructed_ties_edges_clamps_and_zero_preactivations(ok):
    """One minibatch with r == 1 (a tie of the min), r exactly on each clip edge, a clamped probability and hidden pre-activations
    of exactly 0; the restatement agrees bit for bit, and the conventions show in the gradient."""
    shape = (5, 16, 3, 16)
    R, H, A, Hv = shape
    rng = np.random.default_rng(21)
    st, batch = recorded(ok, rng, shape, 64)
    st["policy"][:R] = 0.0          # hidden unit 0: weights and bias 0, so its pre-activation is exactly 0 for every sample
    st["policy"][H * R] = 0.0
    ap = ok.capi.actor_params(H, TABLE8[:A], Hv, "sample", 0.0, 11, 0)
    rec = ok.actor_act_host(ap, st["policy"], st["value"], batch["state"] * f32(200.0), draw_index=5)
    assert np.array_equal(bits(rec["state"]), bits(batch["state"]))
    batch["action"], batch["prob"] = rec["action"].astype(np.int64), rec["prob"].copy()
    batch["adv"] = rng.standard_normal(64).astype(f32)
    lo, hi = f32(1.0 - float(f32(0.2))), f32(1.0 + float(f32(0.2)))
    on_edge = {}
    for s, edge in ((1, lo), (2, hi), (3, lo), (4, hi)):  # p_old with p_new / p_old == edge exactly
        p_new = rec["prob"][s]
        cand = f32(p_new / edge)
        for _ in range(64):
            if f32(p_new / cand) == edge:
                break
            cand = np.nextafter(cand, f32(0) if f32(p_new / cand) < edge else f32(2))
        assert f32(p_new / cand) == edge
        batch["prob"][s] = cand
        on_edge[s] = edge
    batch["adv"][1], batch["adv"][2], batch["adv"][3], batch["adv"][4] = 1.0, 1.0, -1.0, -1.0
    batch["prob"][5] = f32(rec["prob"][5] * f32(2.0))   # r = 0.5: clipped
    batch["prob"][6] = f32(rec["prob"][6] * f32(0.5))   # r = 2: clipped
    lp = ok.capi.learner_params(**HP)
    got_state, got_out = ok.ppo_update_host(lp, shape, st, batch, 64, 1)
    want_state, want_out = L_.update(ok.debug_expf, HP, shape, st, batch, 64, 1)
    assert_same(got_state, got_out, want_state, want_out, ("constructed",))
    assert got_out["clipped"][0] == 2  # an edge is inside the closed range
    g = got_out["grad_policy"]
    assert (g[:R] == 0).all() and g[H * R] == 0  # ReLU's derivative at 0 is 0
    # a saturated softmax: the recorded action's probability clamps to 1.0f exactly (passes, closed range) and the others to 1e-8f
    sat = fresh_state(rng, shape)
    sat["policy"][H * R + H + A * H:] = np.array([90.0, -90.0, -90.0], dtype=f32)
    b2 = {k: v[:8].copy() for k, v in batch.items()}
    rec = ok.actor_act_host(ap, sat["policy"], sat["value"], b2["state"] * f32(200.0), draw_index=1)
    b2["prob"] = rec["prob"]
    b2["action"] = np.array([1, 2, 1, 2, 1, 2, 1, 2], dtype=np.int64)  # actions whose probability is below the clamp
    b2["prob"][:] = f32(1e-8)
    got_state, got_out = ok.ppo_update_host(lp, shape, sat, b2, 8, 1)
    want_state, want_out = L_.update(ok.debug_expf, HP, shape, sat, b2, 8, 1)
    assert_same(got_state, got_out, want_state, want_out, ("clamped",))
    assert (got_out["grad_policy"] == 0).all() and got_out["clipped"][0] == 0  # a clamped probability contributes no policy gradient
    assert np.array_equal(bits(got_state["policy"]), bits(sat["policy"]))


# ---- gradients against torch autograd in float64 -----------------------------------------------------------------------------------

def torch_nets(shape, st, dtype):
    import torch
    R, H, A, Hv = shape

    def build(params, hidden, out):
        w1, b1, w2, b2 = L_.split(params, R, hidden, out)
        return [torch.tensor(np.array(a), dtype=dtype, requires_grad=True) for a in (w1, b1, w2, b2)]
    return build(st["policy"], H, A), build(st["value"], Hv, 1)


def torch_losses(nets, x, action, logp_old, ret, clip):
    """The reference's expressions (PPOAgent.hpp:122-141)."""
    import torch
    (w1, b1, w2, b2), (v1, c1, v2, c2) = nets
    values = torch.relu(x @ v1.T + c1) @ v2.T + c2
    adv = ret - values.detach()
    probs = torch.clamp(torch.softmax(torch.relu(x @ w1.T + b1) @ w2.T + b2, dim=1), 1e-8, 1.0 - 1e-8)
    ratio = torch.exp(torch.log(probs).gather(1, action) - logp_old)
    actor_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    critic_loss = torch.nn.functional.mse_loss(values, ret)
    return actor_loss, critic_loss, probs.gather(1, action).detach(), values.detach()


def torch_ratio(nets, x, action, logp_old):
    import torch
    w1, b1, w2, b2 = nets[0]
    with torch.no_grad():
        probs = torch.clamp(torch.softmax(torch.relu(x @ w1.T + b1) @ w2.T + b2, dim=1), 1e-8, 1.0 - 1e-8)
        return torch.exp(torch.log(probs).gather(1, action) - logp_old)


def magnitudes(shape, policy, value, x, ret):
    """The float64 sums of absolute terms behind a minibatch and the relative errors the docstring of
    test_gradients_against_torch_float64 derives from them."""
    R, H, A, Hv = shape
    x = np.asarray(x, dtype=np.float64)

    def forward_abs(params, hidden, outs):
        w1, b1, w2, b2 = (a.astype(np.float64) for a in L_.split(params, R, hidden, outs))
        pre = x @ w1.T + b1
        Z = np.abs(b2) + (np.abs(b1) + np.abs(x) @ np.abs(w1).T) @ np.abs(w2).T  # [B, outs]
        return w2, pre, np.maximum(pre, 0.0) @ w2.T + b2, Z

    m = {}
    m["w2v"], m["prev"], _, Zv = forward_abs(value, Hv, 1)
    m["w2p"], m["prep"], z64, Zp = forward_abs(policy, H, A)
    m["k_lin"] = (R + Hv / 8.0 + 10.0) * U                       # a value, or v - ret, relative to Zv + |ret|
    b2p = np.abs(L_.split(policy, R, H, A)[3].astype(np.float64))
    e_zp = ((R + H / 8.0 + 8.0) * U * (Zp - b2p).max() + 2 * U * Zp.max())  # a logit, absolute (its bias enters in one addition)
    m["k_soft"] = 3.0 * (2.0 * e_zp + (A + 6) * U) + 10.0 * U    # a policy seed beyond its advantage
    m["adv_abs"] = Zv[:, 0] + np.abs(np.asarray(ret, dtype=np.float64))
    y = np.exp(z64 - z64.max(axis=1, keepdims=True))
    m["y"] = y / y.sum(axis=1, keepdims=True)
    m["sums"] = (32 + np.log2(max((x.shape[0] + 31) // 32, 1)) + 3) * U
    return m


def loss_bounds(m, factor):
    """Rounding bounds of the two losses of a minibatch: means of B terms, each within its relative error of the magnitudes."""
    la = 2.0 * (m["sums"] + m["k_lin"] + m["k_soft"]) * (m["adv_abs"] * np.maximum(factor, 1.2)).mean()
    lc = 2.0 * (m["sums"] + 2.0 * m["k_lin"] + 2 * U) * (m["adv_abs"] ** 2).mean()
    return la, lc


@pytest.mark.parametrize("shape,scale", [((5, 128, 3, 128), 0.3), ((7, 9, 4, 16), 0.5), ((64, 256, 8, 256), 0.05)])
def test_gradients_against_torch_float64(ok, shape, scale):
    """The first minibatch's gradients against autograd in float64 on the reference's expressions, exp(log - log) included.

    The bound, per parameter: the gradient is a sum of B terms a_s * b_s / B (a: a seed ds or dz, b: x or h).  With the float64 sum
    of absolute terms T = sum |a_s b_s| / B, the fp32 summation (a chunk of 32 in sequence, log2 of the chunk count in the tree, one
    multiplication per term, the division) contributes (32 + log2 C + 3) u T, and each term carries the relative error of its seed
    and of its hidden value.  Those come from the forward pass: a logit or value is a sum of R + 1 and H / 8 + 4 terms, so its error is
    at most e_z = (R + H / 8 + 8) u Z with Z the float64 sum of absolute terms behind it (|b2| + |w2| (|b1| + |w1| |x|)); the softmax
    turns e_z into a relative error 2 e_z + (A + 6) u of every probability (as in tests/test_actor_rule.py) and the ratio, the
    surrogate's derivative and the seed take eight more roundings; a hidden seed is a sum of A products of seeds, a hidden value a
    sum of R + 1 terms.  To first order the relative error of a term is at most k = 3 (2 e_z + (A + 6) u) + (R + A + 16) u with
    e_z the largest over the minibatch, and the bound is (32 + log2 C + 3 + R + A + 16) u T + 3 (2 e_z + (A + 6) u) T, doubled for
    the second-order terms; the advantage ret - v and the critic's seed 2 (v - ret) are differences, so their error is taken relative
    to Zv + |ret|, the float64 sum of absolute terms behind them.  torch's own float32 backward must meet the same bound.

    Constructed samples, so that the conventions themselves are compared with autograd's and not only with the restatement's:
    r == 1 on every other sample (each side divides by its own forward's probability: a tie of the min); four samples whose ratio
    lies exactly on a clip edge on every side (p_old, or torch's log p_old, is moved by single ulps until the side's own ratio equals
    its own edge: there the min ties AND the clamp must pass the gradient, so the sample counts in full; a clamp that is open at its
    ends would halve it); samples whose action has a probability below 1e-8 on every side (the last logit's bias is lowered by 20;
    their terms are left out of T, so a gradient through the clamp would break the bound); and hidden unit 0 of the policy with
    weights and bias 0, whose pre-activation is exactly 0 on every side (its T is 0: any derivative other than 0 breaks the bound)."""
    import torch
    R, H, A, Hv = shape
    B = 200
    rng = np.random.default_rng(R + H)

    def prepare(st):
        st["policy"][:R] = 0.0
        st["policy"][H * R] = 0.0
        st["policy"][-1] -= f32(20.0)

    st, batch = recorded(ok, rng, shape, B, scale, prepare)
    m = magnitudes(shape, st["policy"], st["value"], batch["state"], batch["ret"])
    rows = np.arange(B)
    low = list(np.nonzero((m["y"][:, A - 1] > 1e-10) & (m["y"][:, A - 1] < 5e-9))[0][:8])
    assert len(low) >= 3, "no sample has a probability just below the clamp"
    action = batch["action"].copy()
    action[low] = A - 1
    # our side: the rule's own clamped probabilities of the chosen actions (the restatement's forward is the library's bit for bit)
    z32, _, _ = L_.forward(st["policy"], R, H, A, batch["state"])
    e32 = ok.debug_expf((z32 - z32.max(axis=1, keepdims=True)).astype(f32)).reshape(z32.shape)
    s32 = e32[:, 0].copy()
    for k in range(1, A):
        s32 = s32 + e32[:, k]
    own32 = np.minimum(np.maximum((e32 / s32[:, None]).astype(f32), f32(1e-8)), f32(1.0))[rows, action]
    assert (own32[low] == f32(1e-8)).all()
    lo32, hi32 = f32(1.0 - float(f32(0.2))), f32(1.0 + float(f32(0.2)))
    sides = {}
    for dtype in (torch.float64, torch.float32):
        nets = torch_nets(shape, st, dtype)
        x = torch.tensor(batch["state"], dtype=dtype)
        act = torch.tensor(action).reshape(-1, 1)
        ret = torch.tensor(batch["ret"], dtype=dtype).reshape(-1, 1)
        with torch.no_grad():
            own = torch_losses(nets, x, act, torch.zeros(B, 1, dtype=dtype), ret, 0.2)[2]  # this side's own forward
        assert (own[low] == 1e-8).all()
        sides[dtype] = (nets, x, act, ret, own)

    def our_edge(s, which):
        """p_old with own32 / p_old == the edge exactly, or None."""
        edge = lo32 if which == "lo" else hi32
        cand = f32(own32[s] / edge)
        for _ in range(16):
            if f32(own32[s] / cand) == edge:
                return cand
            cand = np.nextafter(cand, f32(0) if f32(own32[s] / cand) < edge else f32(2))
        return None

    def torch_edge(dtype, s, which):
        """log p_old, moved by single ulps, with which this side's ratio is this side's edge exactly, or None."""
        nets, x, act, ret, own = sides[dtype]
        edge = torch.tensor(0.8 if which == "lo" else 1.2, dtype=dtype)
        logp = torch.log(own / edge)
        for _ in range(16):
            r = torch_ratio(nets, x, act, logp)[s, 0]
            if r == edge:
                return logp[s, 0].clone()
            logp[s, 0] = torch.nextafter(logp[s, 0], torch.tensor(-np.inf if r < edge else np.inf, dtype=dtype))
        return None

    # the exponential does not reach every number (its argument's spacing is that of log p, coarser than the ratio's where p is
    # small), so the edge samples are the first candidates for which all three sides find an exact edge
    edges, found = {}, {"lo": 0, "hi": 0}
    for s in range(1, B, 2):
        which = "lo" if found["lo"] <= found["hi"] else "hi"
        if s in low or found[which] >= 2:
            continue
        hit = (our_edge(s, which), torch_edge(torch.float64, s, which), torch_edge(torch.float32, s, which))
        if all(h is not None for h in hit):
            edges[s] = (which,) + hit
            found[which] += 1
        if found == {"lo": 2, "hi": 2}:
            break
    # (with eight nearly uniform actions log p is near -2 and no candidate has an exact edge on all three sides: that shape runs
    # with the ties, the clamped probabilities and the zero pre-activations only)
    assert found == {"lo": 2, "hi": 2} or A == 8, found
    print("%s: samples on a clip edge %s" % (shape, {k: v[0] for k, v in edges.items()}))
    # every second sample keeps its recorded probability; the others are moved off by up to 15 %, inside the clip range, and a
    # tenth of them far outside it
    factor = np.where(rows % 2 == 0, 1.0, 1.0 + rng.uniform(-0.15, 0.15, B))
    far = (rows % 20 == 11)
    far[low] = False
    far[list(edges)] = False
    factor[far] = np.where(rng.random(int(far.sum())) < 0.5, 0.5, 2.0)
    factor[low] = 1.0
    p_old = (own32 * factor).astype(f32)
    for s, (which, ours, _, _) in edges.items():
        factor[s] = 1.0 / (0.8 if which == "lo" else 1.2)
        p_old[s] = ours
    _, out = ok.ppo_update_host(ok.capi.learner_params(**HP), shape, st, dict(batch, action=action, prob=p_old), B, 1)
    assert out["clipped"][0] == int(far.sum())  # the edges are inside
    results = {}
    for i, dtype in enumerate((torch.float64, torch.float32)):
        nets, x, act, ret, own = sides[dtype]
        logp_old = torch.log(own * torch.tensor(factor, dtype=dtype).reshape(-1, 1))
        for s, hit in edges.items():
            logp_old[s, 0] = hit[2 + i]
            assert torch_ratio(nets, x, act, logp_old)[s, 0] == (0.8 if hit[0] == "lo" else 1.2), (dtype, s)
        actor_loss, critic_loss, _, _ = torch_losses(nets, x, act, logp_old, ret, 0.2)
        actor_loss.backward()
        critic_loss.backward()
        assert (nets[0][0].grad[0] == 0).all() and nets[0][1].grad[0] == 0  # autograd's ReLU'(0) is 0
        results[dtype] = (torch.cat([p.grad.reshape(-1) for p in nets[0]]).double().numpy(), torch.cat([p.grad.reshape(-1) for p in nets[1]]).double().numpy(),
                          float(actor_loss.detach()), float(critic_loss.detach()))
    x = batch["state"].astype(np.float64)

    def term_sums(w2, pre, seed_abs):
        ds = (seed_abs @ np.abs(w2)) * (pre > 0)
        h = np.maximum(pre, 0.0)
        return np.concatenate([(ds[:, :, None] * np.abs(x)[:, None, :]).reshape(B, -1).sum(0), ds.sum(0),
                               (seed_abs[:, :, None] * h[:, None, :]).reshape(B, -1).sum(0), seed_abs.sum(0)]) / B

    onehot = np.zeros_like(m["y"])
    onehot[rows, action] = 1.0
    seed_p = (m["adv_abs"] / factor)[:, None] * (onehot + m["y"])
    seed_p[low] = 0.0  # a clamped probability contributes no policy gradient
    Tv = term_sums(m["w2v"], m["prev"], 2.0 * m["adv_abs"][:, None])
    Tp = term_sums(m["w2p"], m["prep"], seed_p)
    assert (Tp[:R] == 0).all() and Tp[H * R] == 0
    for name, T, k, outs, got, idx in (("policy", Tp, m["k_lin"] + m["k_soft"], A, out["grad_policy"], 0), ("value", Tv, m["k_lin"], 1, out["grad_value"], 1)):
        bound = 2.0 * (m["sums"] + (R + outs + 16) * U + k) * T + 1e-300
        want, t32 = results[torch.float64][idx], results[torch.float32][idx]
        err, err32 = np.abs(got.astype(np.float64) - want), np.abs(t32 - want)
        print("%s %s: max |g - g64| / bound = %.3g (torch fp32: %.3g), max |g| = %.3g, max bound = %.3g" % (
            shape, name, (err / bound).max(), (err32 / bound).max(), np.abs(want).max(), bound.max()))
        assert (err <= bound).all(), name
        assert (err32 <= bound).all(), name
    la, lc = loss_bounds(m, factor)
    print("    losses: |actor - f64| = %.3g (bound %.3g), |critic - f64| = %.3g (bound %.3g)" % (
        abs(float(out["actor_loss"][0]) - results[torch.float64][2]), la, abs(float(out["critic_loss"][0]) - results[torch.float64][3]), lc))
    assert abs(float(out["actor_loss"][0]) - results[torch.float64][2]) <= la and abs(results[torch.float32][2] - results[torch.float64][2]) <= la
    assert abs(float(out["critic_loss"][0]) - results[torch.float64][3]) <= lc and abs(results[torch.float32][3] - results[torch.float64][3]) <= lc


def test_three_minibatches_against_torch_float64(ok):
    """Three whole minibatches (M = 300, B = 100, the buffer's order) against the reference's loop in torch float64: both losses of
    every minibatch within a derived bound, which torch's own float32 loop meets too; the parameters' largest deviation is printed as
    a fraction of steps * lr and recorded in docs/HISTORY.md section 20, not asserted (Adam amplifies rounding where a gradient is
    near eps; the gradient and Adam bounds above are the hard assertions).

    The bound of minibatch k (k steps taken before it) is the rounding bound of its losses at equal parameters (loss_bounds) plus
    what the parameters' deviation can do.  One Adam step moves a parameter by at most lr c_t with
    c_t = (1 - b1) / (1 - b1^t) * sqrt((1 - b2^t) / (1 - b2)) * sqrt(sum_{j < t} (b1^2 / b2)^j)
    (Cauchy-Schwarz on m_t = (1 - b1) sum b1^(t-i) g_i against v_t = (1 - b2) sum b2^(t-i) g_i^2; eps only shortens the step), in
    fp32 as in float64, so two runs are at most d_k = 2 (1 + 1e-3) lr (c_1 + .. + c_k) apart in any parameter -- the case of a
    gradient whose sign differs between them.  To first order a loss then moves by at most d_k times the 1-norm of its gradient with
    respect to ALL parameters it depends on (the actor loss depends on the critic's through the advantage, so that gradient is taken
    without the detach), doubled for the second-order terms."""
    import torch
    shape = (5, 128, 3, 128)
    R, H, A, Hv = shape
    M, B = 300, 100
    rng = np.random.default_rng(77)
    st, batch = recorded(ok, rng, shape, M)
    lp = ok.capi.learner_params(**HP)
    got_state, out = ok.ppo_update_host(lp, shape, st, batch, B, 1, want=("actor_loss", "critic_loss", "clipped"))
    lr, b1, b2 = float(f32(HP["lr"])), float(f32(0.9)), float(f32(0.999))
    c = [(1 - b1) / (1 - b1 ** t) * np.sqrt((1 - b2 ** t) / (1 - b2)) * np.sqrt(sum((b1 * b1 / b2) ** j for j in range(t))) for t in (1, 2, 3)]
    finals = {}
    for dtype in (torch.float64, torch.float32):
        nets = torch_nets(shape, st, dtype)
        opt_a = torch.optim.Adam(nets[0], lr=lr, betas=(b1, b2), eps=float(f32(1e-8)))
        opt_c = torch.optim.Adam(nets[1], lr=lr, betas=(b1, b2), eps=float(f32(1e-8)))
        x_all = torch.tensor(batch["state"], dtype=dtype)
        act_all = torch.tensor(batch["action"]).reshape(-1, 1)
        ret_all = torch.tensor(batch["ret"], dtype=dtype).reshape(-1, 1)
        with torch.no_grad():  # this side's own recorded log-probabilities
            logp_all = torch.log(torch_losses(nets, x_all, act_all, torch.zeros(M, 1, dtype=dtype), ret_all, 0.2)[2])
        for k in range(3):
            sl = slice(k * B, (k + 1) * B)
            x, act, ret, logp_old = x_all[sl], act_all[sl], ret_all[sl], logp_all[sl]
            actor_loss, critic_loss, _, _ = torch_losses(nets, x, act, logp_old, ret, 0.2)
            if dtype == torch.float64:
                (w1, bb1, w2, bb2), (v1, c1, v2, c2) = nets
                values = torch.relu(x @ v1.T + c1) @ v2.T + c2
                probs = torch.clamp(torch.softmax(torch.relu(x @ w1.T + bb1) @ w2.T + bb2, dim=1), 1e-8, 1.0 - 1e-8)
                ratio = torch.exp(torch.log(probs).gather(1, act) - logp_old)
                adv = ret - values  # no detach: everything the actor loss depends on
                loss_nd = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean()
                n1_actor = sum(float(g.abs().sum()) for g in torch.autograd.grad(loss_nd, nets[0] + nets[1]))
                n1_critic = sum(float(g.abs().sum()) for g in torch.autograd.grad(critic_loss, nets[1], retain_graph=True))
                m = magnitudes(shape, torch.cat([p.detach().reshape(-1) for p in nets[0]]).numpy(), torch.cat([p.detach().reshape(-1) for p in nets[1]]).numpy(),
                               batch["state"][sl], batch["ret"][sl])
                la, lc = loss_bounds(m, np.ones(B))
                d_k = 2.0 * (1 + 1e-3) * lr * sum(c[:k])
                bounds = (la + 2.0 * d_k * n1_actor, lc + 2.0 * d_k * n1_critic)
                finals.setdefault("bounds", []).append(bounds)
                finals.setdefault("ref", []).append((float(actor_loss.detach()), float(critic_loss.detach())))
                ea, ec = abs(float(out["actor_loss"][k]) - finals["ref"][k][0]), abs(float(out["critic_loss"][k]) - finals["ref"][k][1])
                print("minibatch %d: |actor - f64| = %.3g (bound %.3g), |critic - f64| = %.3g (bound %.3g)" % (k, ea, bounds[0], ec, bounds[1]))
                assert ea <= bounds[0] and ec <= bounds[1], k
            else:
                ref, bounds = finals["ref"][k], finals["bounds"][k]
                assert abs(float(actor_loss.detach()) - ref[0]) <= bounds[0] and abs(float(critic_loss.detach()) - ref[1]) <= bounds[1], k
            opt_a.zero_grad()
            actor_loss.backward()
            opt_a.step()
            opt_c.zero_grad()
            critic_loss.backward()
            opt_c.step()
        finals[dtype] = (torch.cat([p.detach().reshape(-1) for p in nets[0]]).double().numpy(), torch.cat([p.detach().reshape(-1) for p in nets[1]]).double().numpy())
    assert out["clipped"][0] == 0 and got_state["t"] == 3
    for name, got, idx in (("policy", got_state["policy"], 0), ("value", got_state["value"], 1)):
        dev = np.abs(got.astype(np.float64) - finals[torch.float64][idx]).max() / (3 * lr)
        dev32 = np.abs(finals[torch.float32][idx] - finals[torch.float64][idx]).max() / (3 * lr)
        moved = np.abs(finals[torch.float64][idx] - st[name].astype(np.float64)).max() / (3 * lr)
        print("%s: largest parameter deviation from float64 = %.3g of steps * lr (torch fp32: %.3g); largest movement %.3g of steps * lr" % (name, dev, dev32, moved))
        assert np.isfinite(got).all()


# ---- Adam against torch.optim.Adam in float64 ----------------------------------------------------------------------------------------

def test_adam_against_torch_float64(ok):
    """ok_learn_adam (through okenv_debug_adam) over 50 steps of given gradients with magnitudes from 1e-6 to 1e2, against
    torch.optim.Adam in float64; the restatement's Adam gives the library's bits.  The bound per step, relative to lr: m and v are recurrences of
    three and four roundings per step, so their errors obey e_m <- beta1 e_m + 4 u M (M the same recurrence on |g|) and
    e_v <- beta2 e_v + 5 u v; the update lr' m / (sqrt(v) / c + eps) then deviates by at most lr' (e_m + |m| (e_v / (2 v) + 8 u)) /
    (sqrt(v) / c + eps) (the square root halves a relative error; step size, correction, root, two divisions, sum and product round
    once each), and the subtraction adds u |p|."""
    import torch
    rng = np.random.default_rng(50)
    n, steps = 512, 50
    mag = 10.0 ** rng.uniform(-6, 2, n)
    grads = (mag[None, :] * rng.standard_normal((steps, n)) * np.where(rng.random((steps, n)) < 0.1, 0.01, 1.0)).astype(f32)
    p0 = rng.standard_normal(n).astype(f32)
    p64 = torch.tensor(p0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([p64], lr=float(f32(HP["lr"])), betas=(float(f32(0.9)), float(f32(0.999))), eps=float(f32(1e-8)))
    p, m, v = p0.copy(), np.zeros(n, f32), np.zeros(n, f32)
    e_m, e_v, e_p, M = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    m64, v64 = np.zeros(n), np.zeros(n)
    b1, b2, lr = float(f32(0.9)), float(f32(0.999)), float(f32(HP["lr"]))
    worst = 0.0
    lp = ok.capi.learner_params(**HP)
    for t in range(1, steps + 1):
        g = grads[t - 1]
        restated = L_.adam(p, m, v, g, HP, t)
        p, m, v = ok.debug_adam(lp, t, p, m, v, g)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((p, m, v), restated)), t
        p64.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        g64 = np.abs(g.astype(np.float64))
        m64 = b1 * m64 + (1 - b1) * g.astype(np.float64)
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        M = b1 * M + (1 - b1) * g64
        e_m = b1 * e_m + 4 * U * M
        e_v = b2 * e_v + 5 * U * v64
        step, c = lr / (1 - b1 ** t), np.sqrt(1 - b2 ** t)
        den = np.sqrt(v64) / c + 1e-8
        e_p = e_p + step * (e_m + np.abs(m64) * (e_v / (2 * v64) + 8 * U)) / den * (1 + 1e-3) + U * (np.abs(p64.detach().numpy()) + lr)
        err = np.abs(p.astype(np.float64) - p64.detach().numpy())
        worst = max(worst, float((err / e_p).max()))
        assert (err <= e_p).all(), t
        assert (e_p <= t * lr * 1e-4 + U * t * (np.abs(p0) + 1)).all()  # the bound itself is small against the steps taken
    print("Adam: largest error / bound over 50 steps = %.3g" % worst)


def test_host_adam_is_the_restatements(ok):
    """The host entry's Adam with every gradient magnitude: one-sample minibatches whose returns span eight decades."""
    shape = (1, 1, 2, 1)
    rng = np.random.default_rng(4)
    st = fresh_state(rng, shape, 1.0)
    st["policy"], st["value"] = np.abs(st["policy"]), np.abs(st["value"])
    batch = random_batch(rng, shape, 50, False)
    batch["ret"] = (10.0 ** rng.uniform(-6, 2, 50) * rng.choice([-1.0, 1.0], 50)).astype(f32)
    got_state, got_out = ok.ppo_update_host(ok.capi.learner_params(**HP), shape, st, batch, 1, 1)
    want_state, want_out = L_.update(ok.debug_expf, HP, shape, st, batch, 1, 1)
    assert_same(got_state, got_out, want_state, want_out, ("adam",))


# ---- validation ------------------------------------------------------------------------------------------------------------------------

def test_validation(ok):
    L = ok.capi.load()
    shape = (5, 8, 3, 4)
    rng = np.random.default_rng(1)
    st = fresh_state(rng, shape)
    batch = random_batch(rng, shape, 10, False)
    keep = []

    def call(lp=HP, shape=shape, state=st, b=batch, M=10, B=4, epochs=1, drop=(), null_state=False, null_batch=False):
        params = ok.capi.learner_params(**lp) if lp is not None else None
        s = ok.capi.fill_pointers(ok.capi.OkenvLearnerState(), {k: v for k, v in state.items() if k != "t" and k not in drop}, "state")
        s.t = state["t"]
        pb = ok.capi.fill_pointers(ok.capi.OkenvPpoBatch(), {k: v for k, v in b.items() if k not in drop}, "batch")
        keep.extend([s, pb])
        return L.okenv_ppo_update_host(C.byref(params) if params is not None else None, *shape, None if null_state else C.byref(s),
                                       None if null_batch else C.byref(pb), M, B, epochs, None, None)

    assert call(state={k: (v.copy() if k != "t" else v) for k, v in st.items()}) == 0
    assert call(lp=None) == -1 and b"NULL" in L.okenv_last_error(None)
    assert call(null_state=True) == -1 and call(null_batch=True) == -1
    for k in ("state", "action", "prob", "ret", "policy", "policy_m", "policy_v", "value", "value_m", "value_v"):
        assert call(drop=(k,)) == -1, k
    assert call(B=2 ** 31 - 1, state={k: (v.copy() if k != "t" else v) for k, v in st.items()}) == 0  # ceil(M / B) does not leave int32
    assert L.okenv_debug_adam(None, 1, None, None, None, None, 0) == -1
    assert call(M=0) == -1 and call(B=0) == -1 and call(epochs=0) == -1 and call(M=-1) == -1
    assert call(state=dict(st, t=-1)) == -1
    for bad in (dict(lr=0.0), dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(clip=-0.1), dict(clip=1.0), dict(clip=float("nan")),
                dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=0.0), dict(eps=float("nan"))):
        assert call(lp=dict(HP, **bad)) == -1, bad
    for bad_shape in ((0, 8, 3, 4), (65, 8, 3, 4), (5, 0, 3, 4), (5, 257, 3, 4), (5, 8, 1, 4), (5, 8, 9, 4), (5, 8, 3, -1), (5, 8, 3, 257)):
        assert call(shape=bad_shape) == -1, bad_shape
    # neither adv nor a value network
    no_value = {k: v for k, v in fresh_state(rng, (5, 8, 3, 0)).items()}
    assert call(shape=(5, 8, 3, 0), state=no_value) == -1
    assert b"value network" in L.okenv_last_error(None)
    assert call(shape=(5, 8, 3, 0), state=no_value, b=dict(batch, adv=batch["ret"])) == 0
    # a NULL handle is refused, not dereferenced
    lp = ok.capi.learner_params(**HP)
    assert L.okenv_learner_create(None, C.byref(lp)) == -1 and L.okenv_learner_reset(None) != 0
    assert L.okenv_ppo_update(None, None, 1, 1, 1, None, None) == -1
    assert L.okenv_actor_get_params(None, None, None) != 0 and L.okenv_learner_get_state(None, None, None, None, None, None) != 0
    assert L.okenv_debug_update_timing(None, None) == -1
