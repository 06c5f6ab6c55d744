"""REINFORCE's rule on the CPU (include/okenv_reinforce.h, ok_logf of include/okenv_math.h; okenv_actor_act_dropout_host,
okenv_reinforce_update_host): ok_logf against fp64, the dropout mask's layout and share, acting and the update against an independent
numpy restatement (tests/_reinforce_numpy.py) bit for bit, constructed cases, the first step against autograd in float64 with a derived
bound, a closed loop with the oracle's step, and validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _actor_numpy as A_
import _learn_numpy as L_
import _reinforce_numpy as R_

f32 = np.float32
U = 2.0 ** -24
PPO_ACTIONS = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0))
TABLE8 = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(8))
HP = dict(lr=0.01, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8)
SHAPES = [(1, 1, 2), (5, 128, 3), (6, 9, 4), (5, 31, 3), (5, 32, 3), (5, 33, 3), (64, 256, 8)]  # the second Philox block starts at unit 32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- ok_logf -----------------------------------------------------------------------------------------------------------------------

def test_logf_against_fp64(ok):
    rng = np.random.default_rng(2025)
    parts = [rng.uniform(1e-8, 1.0, 500_000), np.exp(rng.uniform(np.log(1e-8), 0.0, 500_000)), 1.0 - rng.random(50_000) ** 3 * 0.3]
    unit = np.concatenate(parts).astype(f32)
    unit = unit[(unit >= f32(1e-8)) & (unit <= 1)]
    assert unit.size >= 1_000_000
    # every binade of the positive normal floats: its ends, the neighbours of sqrt 2 (where the split changes) and random mantissas
    mant = np.concatenate([[0, 1, 2, 0x7FFFFF, 0x7FFFFE], 0x3504F3 + np.arange(-8, 9), rng.integers(0, 1 << 23, 230)]).astype(np.uint32)
    binades = ((np.arange(1, 255, dtype=np.uint32)[:, None] << np.uint32(23)) | mant[None, :]).reshape(-1).view(f32)
    for name, x in (("[1e-8, 1]", unit), ("binades", binades)):
        got = ok.debug_logf(x)
        want = np.log(x.astype(np.float64)).astype(f32)
        diff = got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)
        differing = int((diff != 0).sum())
        print("ok_logf %s: %d of %d arguments differ from the rounded fp64 log (share %.3g)" % (name, differing, x.size, differing / x.size))
        assert np.abs(diff).max() <= 1
        assert differing <= 1e-5 * x.size  # the cap tests/test_actor_rule.py puts on ok_expf
    special = ok.debug_logf(np.array([1.0, 1e-8, 2.0, 1e-45], dtype=f32))
    assert special[0] == 0 and special[1] == f32(np.log(np.float64(f32(1e-8)))) and special[2] == f32(np.log(2.0))
    assert special[3] == f32(np.log(np.float64(f32(1e-45))))  # a subnormal argument


# ---- the mask ------------------------------------------------------------------------------------------------------------------------

def test_philox_restatements_agree_and_match_the_known_answer():
    assert R_.philox_int((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)  # Random123's kat_vectors
    assert R_.philox_int((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, (4, 50), dtype=np.uint64)
    got = np.stack(A_.philox4x32(c[0], c[1], c[2], c[3], 77, R_.OKEN), axis=1)
    for i in range(50):
        assert tuple(int(v) for v in got[i]) == R_.philox_int(c[:, i], (77, R_.OKEN))


def test_mask_layout_and_kept_share(ok):
    for p, seed, agent, draw in ((0.25, 3, 0, 0), (0.6, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF), (0.6, 9, 1234, 77)):
        got = ok.debug_reinforce_mask(p, seed, agent, draw, 256)
        want = np.array([R_.kept_int(p, seed, agent, draw, j) for j in range(256)])
        assert np.array_equal(got.astype(bool), want)
        assert np.array_equal(R_.mask(p, seed, [agent], [draw], 256)[0], want)
        assert np.array_equal(ok.debug_reinforce_mask(p, seed, agent, draw, 33), got[:33])  # depends on j only, not on H
    assert ok.debug_reinforce_mask(0.0, 1, 2, 3, 64).all()
    for p in (0.25, 0.6):  # 2^16 (agent, draw, unit) triples: 32 agents x 16 draws x 128 units
        kept = np.stack([ok.debug_reinforce_mask(p, 5, 1000 + a, d, 128) for a in range(32) for d in range(16)])
        n = kept.size
        assert n == 1 << 16
        share, sigma = kept.mean(), np.sqrt(p * (1 - p) / n)
        print("p = %.2f: kept share %.5f of %d, expected %.5f, sigma %.5f" % (p, share, n, 1 - p, sigma))
        assert abs(share - (1 - p)) <= 5 * sigma


# ---- acting with dropout -----------------------------------------------------------------------------------------------------------

def make_net(rng, R, H, A, scale):
    return (rng.standard_normal(L_.n_params(R, H, A)) * scale).astype(f32)


@pytest.mark.parametrize("shape", SHAPES)
def test_act_host_entry_equals_the_numpy_restatement(ok, shape):
    R, H, A = shape
    rng = np.random.default_rng(R * 1000 + H)
    for i, (N, p) in enumerate(itertools.product((1, 63, 65), (0.0, 0.25, 0.6))):
        Hv = (0, 7)[i % 2]
        policy, value = make_net(rng, R, H, A, 0.7), (make_net(rng, R, Hv, 1, 0.5) if Hv else None)
        dist = (rng.random((N, R)) * 200.0).astype(f32)
        dist[0] = 0.0
        crashed = (rng.random(N) < 0.3).astype(np.uint8)
        base, seed, dseed, draw = (0, 4000000000)[i % 2] + 17 * i, 5 + i, 900 + i, (3, 0xFFFFFFF0)[i % 2] + i
        ap = ok.capi.actor_params(H, TABLE8[:A], Hv, "sample", 0.0, seed, base)
        got = ok.actor_act_dropout_host(ap, p, dseed, policy, value, dist, crashed=crashed, draw_index=draw)
        want = R_.act(ok.debug_expf, seed, base, TABLE8[:A], policy, value, R, H, A, Hv, dist, draw, p, dseed)
        assert np.array_equal(got["action"], want["action"]), (shape, N, p)
        for k in ("prob", "throttle", "steer", "state") + (("value",) if Hv else ()):
            assert np.array_equal(bits(got[k]), bits(want[k])), (k, shape, N, p)
        assert np.array_equal(got["alive"], 1 - crashed)
        if p == 0.0:  # section 14's entry, bit for bit
            plain = ok.actor_act_host(ap, policy, value, dist, crashed=crashed, draw_index=draw)
            for k in plain:
                assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(plain[k]).view(np.uint8)), k
        elif H >= 9 and N > 1:
            other = ok.actor_act_dropout_host(ap, p, dseed, policy, value, dist, crashed=crashed, draw_index=draw + 1)
            assert not np.array_equal(bits(other["prob"]), bits(got["prob"]))  # another draw index, other masks


def test_a_sharded_population_draws_the_unsharded_masks(ok):
    rng = np.random.default_rng(5)
    R, H, A, n = 5, 128, 3, 130
    policy = make_net(rng, R, H, A, 0.3)
    dist = (rng.random((n, R)) * 200.0).astype(f32)
    whole = ok.actor_act_dropout_host(ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample", 0, 9, 0), 0.6, 21, policy, None, dist, draw_index=4)
    for lo, hi in ((0, 65), (65, 130)):
        part = ok.actor_act_dropout_host(ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample", 0, 9, lo), 0.6, 21, policy, None, dist[lo:hi], draw_index=4)
        assert np.array_equal(part["action"], whole["action"][lo:hi]) and np.array_equal(bits(part["prob"]), bits(whole["prob"][lo:hi]))


# ---- the update ----------------------------------------------------------------------------------------------------------------------

def fresh_state(rng, shape, scale=0.5):
    R, H, A = shape
    P = L_.n_params(R, H, A)
    return {"policy": make_net(rng, R, H, A, scale), "policy_m": np.zeros(P, f32), "policy_v": np.zeros(P, f32), "t": 0}


def make_batch(rng, shape, M, N=7):
    R, H, A = shape
    T = (M + N - 1) // N + 2
    index = np.sort(rng.choice(T * N, M, replace=False)).astype(np.int32)
    return {"state": rng.random((M, R)).astype(f32), "action": rng.integers(0, A, M).astype(np.int64), "ret": rng.standard_normal(M).astype(f32),
            "index": index}, N


def compare_update(ok, shape, st, batch, B, N, **kw):
    got_st, got = ok.reinforce_update_host(ok.capi.learner_params(**HP), shape, st, batch, B, num_agents=N, **kw)
    want_st, want = R_.update(ok.debug_expf, ok.debug_logf, HP, shape, st, batch, B, num_agents=N, **kw)
    what = (shape, batch["ret"].shape[0], B, kw)
    assert got_st["t"] == want_st["t"], what
    for k in ("policy", "policy_m", "policy_v"):
        assert np.array_equal(bits(got_st[k]), bits(want_st[k])), (k,) + what
    assert np.array_equal(bits(got["loss"]), bits(want["loss"])), what
    assert np.array_equal(bits(got["grad_policy"]), bits(want["grad_policy"])), what
    return got_st, got, want


VARIANTS = list(itertools.product((1, 0), ("sum", "mean"), (False, True), (0.0, 0.6)))  # accumulate, reduce, order, p


@pytest.mark.parametrize("shape", SHAPES)
def test_update_host_entry_equals_the_numpy_restatement(ok, shape):
    """The whole product on every shape: M in {1, 31, 32, 33, 1000} x B in {1, 32, 33, 1000, 4096} x accumulate x reduce x order NULL /
    given x p in {0, 0.6}, 400 cases a shape.  One batch and one state per (M, B) pair serve its sixteen variants."""
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    for i, (M, B) in enumerate(itertools.product((1, 31, 32, 33, 1000), (1, 32, 33, 1000, 4096))):
        batch, N = make_batch(rng, shape, M)
        st = fresh_state(rng, shape)
        perm = rng.permutation(M).astype(np.int32)
        for acc, reduce, with_order, p in VARIANTS:
            compare_update(ok, shape, st, batch, B, N, accumulate=bool(acc), reduce=reduce, order=perm if with_order else None, p=p, dropout_seed=11 + i,
                           agent_base=1000 * i, draw_first=(5, 0xFFFFFFFA)[i % 2])


def test_two_calls_continue_one_run(ok):
    rng = np.random.default_rng(8)
    shape = (5, 33, 3)
    batch, N = make_batch(rng, shape, 70)
    st0 = fresh_state(rng, shape)
    lp = ok.capi.learner_params(**HP)
    kw = dict(accumulate=False, reduce="mean", p=0.6, dropout_seed=3, agent_base=50, num_agents=N, draw_first=9)
    half = {k: v[:64] for k, v in batch.items()}
    rest = {k: v[64:] for k, v in batch.items()}
    st1, _ = ok.reinforce_update_host(lp, shape, st0, half, 32, **kw)
    st2, out2 = ok.reinforce_update_host(lp, shape, st1, rest, 32, **kw)
    one, out = ok.reinforce_update_host(lp, shape, st0, batch, 32, **kw)
    assert st1["t"] == 2 and st2["t"] == 3 == one["t"]
    for k in ("policy", "policy_m", "policy_v"):
        assert np.array_equal(bits(st2[k]), bits(one[k])), k
    assert bits(out2["loss"])[0] == bits(out["loss"])[2]


def test_constructed_cases(ok):
    shape = R, H, A = (5, 16, 3)
    rng = np.random.default_rng(77)
    lp = ok.capi.learner_params(**HP)
    st = fresh_state(rng, shape)
    P = L_.n_params(R, H, A)
    # a clamped probability: the last logit's bias far down, its action recorded: a zero seed and a finite loss
    low = dict(st, policy=st["policy"].copy())
    low["policy"][-1] = f32(-60.0)
    one = {"state": rng.random((1, R)).astype(f32), "action": np.array([A - 1]), "ret": np.array([1.5], f32), "index": np.array([0], np.int32)}
    new, out = ok.reinforce_update_host(lp, shape, low, one, 8, num_agents=1)
    assert (bits(out["grad_policy"]) == 0).all()  # +0 everywhere
    assert out["loss"][0] == -(ok.debug_logf(np.array([1e-8], f32))[0] * f32(1.5)) and np.isfinite(out["loss"][0])
    assert np.array_equal(bits(new["policy"]), bits(low["policy"]))  # Adam on a zero gradient from zero moments moves nothing
    compare_update(ok, shape, low, one, 8, 1)
    # a pre-activation of exactly 0 (unit 0: weights and bias 0) has derivative 0; G = 0 on sample 3; a unit dropped in every
    # sample gets +0 on its first-layer row
    zero = dict(st, policy=st["policy"].copy())
    zero["policy"][:R] = 0.0
    zero["policy"][H * R] = 0.0
    M, N = 40, 4
    batch, _ = make_batch(rng, shape, M, N)
    batch["ret"][3] = 0.0
    kw = dict(p=0.6, dropout_seed=1, agent_base=0, draw_first=0)
    kept = R_.mask(0.6, 1, batch["index"] % N, batch["index"] // N, H)
    never = np.nonzero(~kept.any(axis=0))[0]
    if never.size == 0:  # make one: keep only the samples in which unit 5 is dropped
        rows = np.nonzero(~kept[:, 5])[0]
        batch = {k: v[rows] for k, v in batch.items()}
        never = np.array([5])
        batch["ret"][min(3, rows.size - 1)] = 0.0
    _, out, _ = compare_update(ok, shape, zero, batch, 16, N, **kw)
    g = out["grad_policy"]
    assert (bits(g[:R]) == 0).all() and bits(g[H * R:H * R + 1])[0] == 0
    for j in never:
        assert (bits(g[j * R:(j + 1) * R]) == 0).all() and bits(g[H * R + j:H * R + j + 1])[0] == 0, j
        assert (bits(g[H * R + H + np.arange(A) * H + j]) == 0).all()  # and its second-layer column: h is 0 in every sample
    assert np.abs(g).max() > 0


def test_recomputed_probability_equals_the_recorded_one_in_a_closed_loop(ok, oracle):
    """200 steps of the loop with the oracle's step and dropout 0.6; afterwards the update's forward reproduces every recorded
    probability: the loss of the one-sample batch (G = 1) is -ok_logf(recorded), and the restatement's q agrees on the whole batch."""
    N, steps, p, dseed, seed, base = 24, 200, 0.6, 33, 17, 500
    fan = np.array([-70, -30, 0, 30, 70], dtype=f32)
    shape = R, H, A = (5, 128, 3)
    t = oracle.Track("Silverstone")
    env = oracle.OracleEnv(t.segments, N, fan.size, fan, (t.x, t.y, t.heading))
    env.set_lane_bounds(t.li, t.ri)
    env.reset_random(None, 1, seed, 0, base)
    env.step(1)
    rng = np.random.default_rng(4)
    st = fresh_state(rng, shape, 0.4)
    ap = ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample", 0.0, seed, base)
    rec, first = [], 1
    for k in range(steps):
        out = ok.actor_act_dropout_host(ap, p, dseed, st["policy"], None, env.get(oracle.F_DIST), crashed=env.get(oracle.F_CRASHED), draw_index=first + k)
        rec.append(out)
        env.set(oracle.F_THR, out["throttle"])
        env.set(oracle.F_STEER, out["steer"])
        env.step(1)
    M = steps * N
    batch = {"state": np.concatenate([r["state"] for r in rec]), "action": np.concatenate([r["action"] for r in rec]),
             "ret": np.ones(M, f32), "index": np.arange(M, dtype=np.int32)}
    prob = np.concatenate([r["prob"] for r in rec])
    assert np.unique(prob).size > M // 4
    kw = dict(p=p, dropout_seed=dseed, agent_base=base, num_agents=N, draw_first=first)
    _, want = R_.update(ok.debug_expf, ok.debug_logf, HP, shape, st, batch, 4096, **kw)
    assert np.array_equal(bits(want["q"]), bits(prob))
    lp = ok.capi.learner_params(**HP)
    expect = -ok.debug_logf(prob)
    for k in range(M):
        one = {name: v[k:k + 1] for name, v in batch.items()}
        _, out = ok.reinforce_update_host(lp, shape, st, one, 1, want=("loss",), **kw)
        assert bits(out["loss"])[0] == bits(expect[k:k + 1])[0], k
    # the wrong draw index does not reproduce them
    _, other = R_.update(ok.debug_expf, ok.debug_logf, HP, shape, st, batch, 4096, **dict(kw, draw_first=first + 1))
    assert not np.array_equal(bits(other["q"]), bits(prob))


# ---- against autograd in float64 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,scale,p", [((5, 128, 3), 0.3, 0.6), ((6, 9, 4), 0.5, 0.25), ((64, 256, 8), 0.05, 0.6), ((5, 33, 3), 0.4, 0.0)])
def test_first_step_against_torch_float64(ok, shape, scale, p):
    """The first step's loss and gradient against autograd in float64 on the reference's expressions (Policy.hpp:22-29,
    ReinforceAgent.hpp:109-113): affine1 -> mask * s -> relu -> affine2 -> softmax, loss += -log p * G, the mask from the restatement.

    The bound, per parameter (section 16's derivation, tests/test_learn_rule.py): the gradient is a sum of M terms a_s * b_s (a: a seed
    dpre or dz, b: x or h).  With T = sum |a_s b_s| in float64, the fp32 summation (32 in sequence in a chunk, log2 C in the tree, one
    multiplication per term) contributes (32 + log2 C + 3) u T.  Each term carries the relative error of its seed and of its hidden
    value: a logit is a sum of R + 2 and H / 8 + 4 terms (the scale s is one more multiplication, and s itself is rounded twice), so
    its error is at most e_z = (R + H / 8 + 11) u Z with Z = |b2| + |w2| (s kept (|b1| + |w1| |x|)); the softmax turns e_z into a
    relative error 2 e_z + (A + 6) u of every probability (tests/test_actor_rule.py), the seed -(G * (ind - q)) takes two more
    roundings relative to |G| (ind + q), a hidden seed is a sum of A products times s, a hidden value a sum of R + 1 terms times s.  To
    first order the relative error of a term is at most k = 3 (2 e_z + (A + 6) u) + (R + A + 19) u, and the bound is
    (32 + log2 C + 3) u T + k T, doubled for the second-order terms.  The loss likewise: each term -log(q_a) G errs by at most
    |G| (2 e_z + (A + 6) u) through q (d log q = dq / q) plus 3 u |G log q_a| (ok_logf's ulp, the product, the sum's own), and the
    summation adds (32 + log2 C) u sum |G log q_a|; doubled.  torch's own float32 backward must meet the same bounds.

    No probability lies near the clamp here (asserted): the clamp is the shared actor's and not the reference's, and
    test_constructed_cases covers it.  No kept pre-activation lies within 1e-6 of 0 (asserted), where the two precisions could take
    different sides of the ReLU."""
    import torch
    R, H, A = shape
    M, N = 200, 8
    rng = np.random.default_rng(R + H)
    st = fresh_state(rng, shape, scale)
    batch, _ = make_batch(rng, shape, M, N)
    kw = dict(p=p, dropout_seed=4, agent_base=10, num_agents=N, draw_first=2)
    _, out = ok.reinforce_update_host(ok.capi.learner_params(**HP), shape, st, batch, 4096, **kw)
    kept = R_.mask(p, 4, 10 + batch["index"] % N, 2 + batch["index"] // N, H)
    s32 = R_.scale(p) if p > 0 else f32(1)
    w1, b1, w2, b2 = (a.astype(np.float64) for a in L_.split(st["policy"], R, H, A))
    x64 = batch["state"].astype(np.float64)
    pre64 = b1[None, :] + x64 @ w1.T
    assert np.abs(pre64[kept]).min() > 1e-6
    results = {}
    for dtype in (torch.float64, torch.float32):
        prm = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in (w1, b1, w2, b2)]
        x = torch.tensor(batch["state"], dtype=dtype)
        scaled = torch.tensor(kept, dtype=dtype) * (float(s32) if dtype == torch.float32 else 1.0 / (1.0 - p))
        hid = torch.relu((x @ prm[0].T + prm[1]) * scaled)
        probs = torch.softmax(hid @ prm[2].T + prm[3], dim=1)
        qa = probs.gather(1, torch.tensor(batch["action"]).reshape(-1, 1))[:, 0]
        loss = (-torch.log(qa) * torch.tensor(batch["ret"], dtype=dtype)).sum()
        loss.backward()
        results[dtype] = (torch.cat([q.grad.reshape(-1) for q in prm]).double().numpy(), float(loss.detach()), probs.detach().double().numpy())
    want, loss64, q64 = results[torch.float64]
    rows = np.arange(M)
    assert q64[rows, batch["action"]].min() > 1e-6
    s = 1.0 / (1.0 - p)
    habs = s * kept * (np.abs(b1)[None, :] + np.abs(x64) @ np.abs(w1).T)
    Z = (np.abs(b2)[None, :] + habs @ np.abs(w2).T).max()
    e_z = (R + H / 8 + 11) * U * Z
    k_soft = 2 * e_z + (A + 6) * U
    onehot = np.zeros((M, A))
    onehot[rows, batch["action"]] = 1.0
    G = np.abs(batch["ret"].astype(np.float64))
    seed_abs = G[:, None] * (onehot + q64)
    ds = s * (seed_abs @ np.abs(w2)) * (kept & (pre64 > 0))
    h = s * np.maximum(pre64, 0.0) * kept
    T = np.concatenate([(ds[:, :, None] * np.abs(x64)[:, None, :]).reshape(M, -1).sum(0), ds.sum(0), (seed_abs[:, :, None] * h[:, None, :]).reshape(M, -1).sum(0),
                        seed_abs.sum(0)])
    sums = (32 + np.log2((M + 31) // 32) + 3) * U
    bound = 2.0 * (sums + 3 * k_soft + (R + A + 19) * U) * T + 1e-300
    err, err32 = np.abs(out["grad_policy"].astype(np.float64) - want), np.abs(results[torch.float32][0] - want)
    print("%s p=%.2f: max |g - g64| / bound = %.3g (torch fp32: %.3g), max |g| = %.3g, max bound = %.3g" % (
        shape, p, (err / bound).max(), (err32 / bound).max(), np.abs(want).max(), bound.max()))
    assert (err <= bound).all() and (err32 <= bound).all()
    logs = G * np.abs(np.log(q64[rows, batch["action"]]))
    lb = 2.0 * (k_soft * G.sum() + (sums + 3 * U) * logs.sum())
    print("    loss: |ours - f64| = %.3g (torch fp32: %.3g), bound %.3g" % (abs(float(out["loss"][0]) - loss64), abs(results[torch.float32][1] - loss64), lb))
    assert abs(float(out["loss"][0]) - loss64) <= lb and abs(results[torch.float32][1] - loss64) <= lb


# ---- validation ----------------------------------------------------------------------------------------------------------------------

def test_validation(ok):
    L = ok.capi.load()
    shape = R, H, A = (5, 8, 3)
    rng = np.random.default_rng(0)
    st = fresh_state(rng, shape)
    batch, N = make_batch(rng, shape, 10)
    lp = ok.capi.learner_params(**HP)

    def call(params=lp, cfg="default", p=0.0, shape=shape, state=st, batch=batch, M=10, B=4, drop=()):
        cfg = ok.capi.reinforce_config(True, "sum", N, 0) if cfg == "default" else cfg
        b = ok.capi.fill_pointers(ok.capi.OkenvReinforceBatch(), {k: v for k, v in batch.items() if k not in drop}, "b") if batch is not None else None
        new = {k: np.array(v, dtype=f32) for k, v in state.items() if k != "t"} if state is not None else None
        s = ok.capi.fill_pointers(ok.capi.OkenvLearnerState(), new, "s") if new is not None else None
        return L.okenv_reinforce_update_host(None if params is None else C.byref(params), None if cfg is None else C.byref(cfg), p, 1, 0, shape[0],
                                             shape[1], shape[2], None if s is None else C.byref(s), None if b is None else C.byref(b), M, B, None, None)

    assert call() == 0 and call(p=0.6) == 0
    assert call(params=None) == -1 and call(cfg=None) == -1 and call(state=None) == -1 and call(batch=None) == -1
    assert b"NULL" in L.okenv_last_error(None)
    for drop in ("state", "action", "ret"):
        assert call(drop=(drop,)) == -1, drop
    assert call(drop=("index",)) == 0 and call(drop=("index",), p=0.6) == -1  # index may be NULL only while dropout is off
    assert call(M=0) == -1 and call(B=0) == -1 and call(M=-1) == -1
    assert call(cfg=ok.capi.reinforce_config(True, 2, N, 0)) == -1 and call(cfg=ok.capi.reinforce_config(True, -1, N, 0)) == -1
    assert call(cfg=ok.capi.reinforce_config(True, "sum", 0, 0), p=0.6) == -1 and call(cfg=ok.capi.reinforce_config(True, "sum", 0, 0)) == 0
    for bad in (-0.1, 1.0, float("nan")):
        assert call(p=bad) == -1, bad
    assert call(shape=(0, 8, 3)) == -1 and call(shape=(5, 257, 3)) == -1 and call(shape=(5, 8, 9)) == -1
    assert call(state={k: v for k, v in st.items() if k != "policy_m"}) == -1
    assert call(params=ok.capi.learner_params(lr=0.0)) == -1
    # the acting entry
    ap = ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample")
    pol, dist = st["policy"], np.zeros((2, R), f32)

    def act(p, params=ap, policy=pol):
        return L.okenv_actor_act_dropout_host(None if params is None else C.byref(params), p, 0, ok.capi.ptr(policy), None, R, 2, ok.capi.ptr(dist), None, 0,
                                              None, None, None, None, None, None, None)

    assert act(0.0) == 0 and act(0.6) == 0
    for bad in (-0.1, 1.0, float("nan")):
        assert act(bad) == -1, bad
    assert act(0.6, params=None) == -1 and act(0.6, policy=None) == -1
    assert L.okenv_debug_logf(None, None, 1) == -1 and L.okenv_debug_reinforce_mask(1.0, 0, 0, 0, 4, ok.capi.ptr(np.zeros(4, np.uint8))) == -1
    # a NULL handle is refused, not dereferenced
    assert L.okenv_actor_set_dropout(None, 0.5, 0) == -1
    assert L.okenv_reinforce_update(None, None, None, 1, 1, None, None) == -1 and L.okenv_debug_reinforce_timing(None, None) == -1
