"""DDPG on the CPU (include/okenv_ddpg.h; okenv_ddpg_act_host, okenv_ddpg_replay_push_host, okenv_ddpg_update_host): the host entries
against an independent numpy restatement (tests/_ddpg_numpy.py) bit for bit, constructed edges, the order of the two steps, the first
iteration against torch autograd in float64 on the reference's expressions with a derived bound, validation, and a closed loop with
the oracle's step."""
import ctypes as C

import numpy as np
import pytest

import _ddpg_numpy as G_
import _learn_numpy as L_

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32
BASE = dict(scale=(50.0, 5.0), bias=(50.0, 0.0), noise=(0.0, 0.0), seed=0, agent_base=0, gamma=0.99, tau=0.005, lr_actor=1e-4, lr_critic=1e-3,
            beta1=0.9, beta2=0.999, eps=1e-8, sample_seed=0)
RING_FIELDS = ("state", "next_state", "action", "reward", "done")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


@pytest.fixture(scope="module")
def tanhf(oracle):
    """ok_tanhf as the oracle exports it: the one function the restatement shares with the library."""
    def f(x):
        x = np.ascontiguousarray(x, dtype=f32).ravel()
        out = np.zeros_like(x)
        oracle.lib().oracle_tanhf(x, out, x.size)
        return out
    return f


def config(H, Hc, **kw):
    return dict(BASE, hidden=H, critic_hidden=Hc, **kw)


def cfg_of(ok, cfg):
    return ok.capi.ddpg_config(**cfg)


def fresh_state(rng, R, H, Hc, scale=0.3, moments=False):
    st = {"actor": (rng.standard_normal(G_.n_actor(R, H)) * scale).astype(f32), "critic": (rng.standard_normal(G_.n_critic(R, Hc)) * scale).astype(f32), "t": 0}
    st["actor_target"] = (st["actor"] + (rng.standard_normal(st["actor"].size) * 0.02).astype(f32)).astype(f32)
    st["critic_target"] = (st["critic"] + (rng.standard_normal(st["critic"].size) * 0.02).astype(f32)).astype(f32)
    for net in ("actor", "critic"):
        n = st[net].size
        st[net + "_m"] = (rng.standard_normal(n) * 1e-3).astype(f32) if moments else np.zeros(n, f32)
        st[net + "_v"] = (rng.random(n) * 1e-4).astype(f32) if moments else np.zeros(n, f32)
    if moments:
        st["t"] = 5
    return st


def filled_ring(rng, R, capacity, size, cfg=BASE):
    rg = G_.ring(capacity, R)
    rg["state"][:] = rng.random((capacity, R)).astype(f32)
    rg["next_state"][:] = rng.random((capacity, R)).astype(f32)
    s, b = np.asarray(cfg["scale"], f32), np.asarray(cfg["bias"], f32)
    rg["action"][:] = (b + s * (rng.random((capacity, 2)) * 2 - 1)).astype(f32)
    rg["reward"][:] = np.where(rng.random(capacity) < 0.3, rng.standard_normal(capacity), 1.0).astype(f32)
    rg["done"][:] = (rng.random(capacity) < 0.2).astype(f32)
    rg["pushed"] = size
    return rg


def assert_same_update(got_state, got_out, want_state, want_out, what):
    assert got_state["t"] == want_state["t"], what
    for k in G_.VECTORS:
        assert np.array_equal(bits(got_state[k]), bits(want_state[k])), (k,) + tuple(what)
    for k in ("critic_loss", "actor_loss", "grad_critic", "grad_actor"):
        assert np.array_equal(bits(got_out[k]), bits(want_out[k])), (k,) + tuple(what)
    assert np.array_equal(got_out["index"], want_out["index"]), what


# ---- acting --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,H", [(1, 1), (5, 128), (7, 9), (62, 256), (6, 9)])
def test_act_host_equals_the_numpy_restatement(ok, tanhf, R, H):
    for n in (1, 63, 65):
        rng = np.random.default_rng(R * 1000 + n)
        actor = (rng.standard_normal(G_.n_actor(R, H)) * 0.5).astype(f32)
        dist = (rng.random((n, R)) * 220.0).astype(f32)
        crashed = (rng.random(n) < 0.3).astype(np.uint8)
        quiet = None
        for noise, draw in (((0.0, 0.0), 3), ((20.0, 2.0), 3), ((0.0, 2.0), 4), ((400.0, 0.0), 5)):
            cfg = config(H, 1, noise=noise, seed=77, agent_base=1000)
            got = ok.ddpg_act_host(cfg_of(ok, cfg), actor, dist, crashed, draw)
            want_a, want_x = G_.act(cfg, actor, R, dist, draw, tanhf)
            what = (R, H, n, noise)
            assert np.array_equal(bits(got["action"]), bits(want_a)), what
            assert np.array_equal(bits(got["state"]), bits(want_x)), what
            assert np.array_equal(bits(got["throttle"]), bits(want_a[:, 0])) and np.array_equal(bits(got["steer"]), bits(want_a[:, 1])), what
            assert np.array_equal(got["alive"], 1 - crashed), what
            lo, hi = f32(50.0 - 50.0), f32(50.0 + 50.0)
            assert (got["action"][:, 0] >= lo).all() and (got["action"][:, 0] <= hi).all() and (np.abs(got["action"][:, 1]) <= f32(5.0)).all(), what
            if noise == (0.0, 0.0):
                quiet = got["action"]
            else:  # a component without noise is the no-draw path bit for bit, one with noise moves (n agents: some do)
                for k in range(2):
                    same = np.array_equal(bits(got["action"][:, k]), bits(quiet[:, k]))
                    assert same == (noise[k] == 0.0) or n == 1, what + (k,)
        if n == 65 and H > 1:
            assert (got["action"][:, 0] == lo).any() and (got["action"][:, 0] == hi).any()  # noise 400 reaches both clamps


def test_act_global_ids_shard_and_saturated_tanh(ok, tanhf):
    R, H = 5, 16
    rng = np.random.default_rng(5)
    actor = (rng.standard_normal(G_.n_actor(R, H)) * 0.5).astype(f32)
    dist = (rng.random((40, R)) * 200.0).astype(f32)
    cfg = config(H, 1, noise=(10.0, 1.0), seed=3)
    whole = ok.ddpg_act_host(cfg_of(ok, cfg), actor, dist, None, 9)["action"]
    parts = [ok.ddpg_act_host(cfg_of(ok, dict(cfg, agent_base=b)), actor, dist[b:b + 20], None, 9)["action"] for b in (0, 20)]
    assert np.array_equal(bits(whole), bits(np.concatenate(parts)))
    # the output biases alone saturate tanh to exactly +1 and -1: a = bias + scale and bias - scale exactly
    w1, b1, w2, b2 = L_.split(actor, R, H, 2)
    w2[:], b2[0], b2[1] = 0.0, 30.0, -30.0
    got = ok.ddpg_act_host(cfg_of(ok, config(H, 1)), actor, dist, None, 0)["action"]
    assert (got[:, 0] == f32(100.0)).all() and (got[:, 1] == f32(-5.0)).all()
    assert np.array_equal(bits(got), bits(G_.act(config(H, 1), actor, R, dist, 0, tanhf)[0]))


# ---- the push ------------------------------------------------------------------------------------------------------------------------

def step_data(rng, n, R, mask):
    state = rng.random((n, R)).astype(f32)
    action = (rng.standard_normal((n, 2)) * 30).astype(f32)
    dist = (rng.random((n, R)) * 250.0).astype(f32)
    crashed = (rng.random(n) < 0.3).astype(np.uint8)
    alive = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
             "random": (rng.random(n) < 0.6).astype(np.uint8)}[mask]
    return state, action, alive, dist, crashed


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_push_host_equals_the_numpy_restatement(ok, n):
    R = 5
    for capacity in (1, 7, 64, 100, 1000):
        for mask in ("all", "none", "alternating", "random"):
            for push_all, own_reward in ((False, False), (True, False), (False, True)):
                rng = np.random.default_rng(n * 7919 + capacity)
                got, want = ok.ddpg_ring(capacity, R), G_.ring(capacity, R)
                for call in range(3):
                    state, action, alive, dist, crashed = step_data(rng, n, R, mask)
                    reward = rng.standard_normal(n).astype(f32) if own_reward else None
                    ok.ddpg_replay_push_host(got, state, action, alive, dist, crashed, reward, push_all)
                    G_.push(want, state, action, alive, dist, crashed, reward, push_all)
                    assert got["pushed"] == want["pushed"]
                    for k in RING_FIELDS:
                        assert np.array_equal(bits(got[k]), bits(want[k])), (k, n, capacity, mask, push_all, own_reward, call)
                if not own_reward and got["pushed"]:
                    assert (got["reward"][:min(got["pushed"], capacity)] == 1.0).all()  # ddpg_sim.cpp:73


# ---- the update against the numpy restatement -----------------------------------------------------------------------------------------

# (size, B, iterations, resample, tau): every value of every factor, each shape runs all rows
CASES = [(1, 1, 1, False, 0.005), (31, 32, 3, True, 0.005), (33, 33, 1, False, 1.0), (1000, 250, 3, False, 0.0), (1000, 33, 3, True, 0.005),
         (31, 250, 1, False, 0.005)]


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 128, 128), (7, 9, 13), (62, 256, 256), (6, 9, 131), (8, 131, 13), (5, 1, 256), (5, 256, 1)])
def test_update_host_equals_the_numpy_restatement(ok, tanhf, shape):
    R, H, Hc = shape
    rng = np.random.default_rng(sum(shape))
    for size, B, iterations, resample, tau in CASES:
        cfg = config(H, Hc, tau=tau, sample_seed=R)
        rg = filled_ring(rng, R, max(size, 40), size)
        st = fresh_state(rng, R, H, Hc, 0.3 if R < 62 else 0.05, moments=True)
        got = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, B, iterations, resample, draw_base=7)
        want = G_.update(cfg, R, st, rg, B, tanhf, iterations, resample, draw_base=7)
        what = (shape, size, B, iterations, resample, tau)
        assert_same_update(*got, *want, what)
        assert np.isfinite(got[1]["critic_loss"]).all() and got[1]["actor_loss"].size == iterations
        new = got[0]
        if tau == 1.0:
            assert np.array_equal(bits(new["actor_target"]), bits(new["actor"])) and np.array_equal(bits(new["critic_target"]), bits(new["critic"])), what
        elif tau == 0.0:
            assert np.array_equal(bits(new["actor_target"]), bits(st["actor_target"])) and np.array_equal(bits(new["critic_target"]), bits(st["critic_target"])), what
        else:
            assert not np.array_equal(new["actor_target"], st["actor_target"]) and not np.array_equal(new["actor_target"], new["actor"]), what


@pytest.mark.parametrize("B", [513, 1500, 4096])
def test_update_host_equals_the_numpy_restatement_above_eight_chunks(ok, tanhf, B):
    """ok_learn_tree in the host entry (okDdpgStepHost) at C = 17, 47 and 128 chunks (CASES stops at B = 250, eight chunks): padded
    widths 32, 64 and 128, the guard `i + h < n` false at the first level for C = 17 and 47 and never for 128.  These are the B of
    tests/test_gpu_update_geometry.py, whose device results are compared with this host entry."""
    R, H, Hc = 7, 9, 13
    rng = np.random.default_rng(B)
    for iterations, resample, tau in ((1, False, 0.005), (3, True, 1.0)):
        cfg = config(H, Hc, tau=tau, sample_seed=B)
        rg = filled_ring(rng, R, 1000, 1000)
        st = fresh_state(rng, R, H, Hc, moments=True)
        got = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, B, iterations, resample, draw_base=7)
        want = G_.update(cfg, R, st, rg, B, tanhf, iterations, resample, draw_base=7)
        assert_same_update(*got, *want, ((R, H, Hc), B, iterations, resample, tau))
        assert np.isfinite(got[1]["critic_loss"]).all() and got[1]["actor_loss"].size == iterations and got[1]["index"].size == B


def test_two_calls_continue_one_run(ok):
    R, H, Hc = 5, 32, 24
    rng = np.random.default_rng(21)
    rg, st, cfg = filled_ring(rng, R, 200, 200), fresh_state(rng, R, H, Hc), cfg_of(ok, config(H, Hc, sample_seed=2))
    for resample in (False, True):
        whole, out = ok.ddpg_update_host(cfg, R, st, rg, 33, 5, resample, draw_base=10)
        a, out_a = ok.ddpg_update_host(cfg, R, st, rg, 33, 2, resample, draw_base=10)
        b, out_b = ok.ddpg_update_host(cfg, R, a, rg, 33, 3, resample, draw_base=12 if resample else 10)
        assert b["t"] == whole["t"] == 5
        for k in G_.VECTORS:
            assert np.array_equal(bits(b[k]), bits(whole[k])), (k, resample)
        for k in ("critic_loss", "actor_loss"):
            assert np.array_equal(bits(np.concatenate([out_a[k], out_b[k]])), bits(out[k]))
        assert np.array_equal(bits(out_b["grad_actor"]), bits(out["grad_actor"])) and np.array_equal(out_b["index"], out["index"])


def test_an_empty_ring_leaves_fresh_online_parameters_alone(ok, tanhf):
    for R, H, Hc in ((1, 1, 1), (5, 128, 128), (7, 9, 13)):
        rng = np.random.default_rng(H)
        st = fresh_state(rng, R, H, Hc)
        rg = ok.ddpg_ring(16, R)
        rg["state"][:] = np.nan  # nothing may read the slots
        cfg = config(H, Hc)
        new, out = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, 33, 3)
        assert new["t"] == 3
        for net in ("actor", "critic"):
            assert np.array_equal(bits(new[net]), bits(st[net])) and not new[net + "_m"].any() and not new[net + "_v"].any()
            assert not np.array_equal(new[net + "_target"], st[net + "_target"])  # the soft update still runs
        assert not out["critic_loss"].any() and not out["actor_loss"].any() and not out["grad_critic"].any() and not out["grad_actor"].any()
        assert_same_update(new, out, *G_.update(cfg, R, st, rg, 33, tanhf, 3), (R, H, Hc))


def test_constructed_zero_preactivation_saturation_done_and_zero_error(ok, tanhf):
    R, H, Hc, B = 5, 16, 16, 64
    rng = np.random.default_rng(8)
    cfg = config(H, Hc, sample_seed=1)
    st = fresh_state(rng, R, H, Hc)
    rg = filled_ring(rng, R, B, B)
    # critic unit 0: weights and bias 0, so its pre-activation is exactly 0 and ReLU's derivative 0
    w1c, b1c, w2c, b2c = L_.split(st["critic"], R + 2, Hc, 1)
    w1c[0], b1c[0] = 0.0, 0.0
    # actor output 0 saturates: t_0 = 1 exactly, so dz_0 = 0 and nothing reaches row 0 of the second layer or its bias
    w1a, b1a, w2a, b2a = L_.split(st["actor"], R, H, 2)
    w2a[0], b2a[0] = 0.0, 40.0
    rg["done"][:] = 1.0
    got = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, B, 1)
    assert_same_update(*got, *G_.update(cfg, R, st, rg, B, tanhf, 1), ("constructed",))
    gc, ga = got[1]["grad_critic"], got[1]["grad_actor"]
    assert not gc[:R + 2].any() and gc[Hc * (R + 2)] == 0
    assert not ga[H * R + H:H * R + 2 * H].any() and ga[H * R + 3 * H] == 0 and ga[H * R + 3 * H + 1] != 0
    # done = 1 everywhere: y = r exactly, whatever the targets say
    idx = got[1]["index"]
    q, _, _ = L_.forward(st["critic"], R + 2, Hc, 1, np.concatenate([rg["state"][idx], rg["action"][idx]], axis=1))
    e = (q[:, 0] - rg["reward"][idx]).astype(f32)
    assert got[1]["critic_loss"][0] == L_.rule_sum((e * e)[:, None])[0] / f32(B)
    other = dict(st, actor_target=st["actor"] * f32(2), critic_target=st["critic"] * f32(3))
    assert np.array_equal(bits(ok.ddpg_update_host(cfg_of(ok, cfg), R, other, rg, B, 1)[1]["grad_critic"]), bits(gc))
    # e = 0: with done = 1 and r = q(s, a) the critic's loss, gradient and step are 0
    q, _, _ = L_.forward(st["critic"], R + 2, Hc, 1, np.concatenate([rg["state"], rg["action"]], axis=1))
    rg["reward"][:] = q[:, 0]
    new, out = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, B, 2)
    assert not out["critic_loss"].any() and not out["grad_critic"].any() and np.array_equal(bits(new["critic"]), bits(st["critic"]))
    assert out["grad_actor"].any()


def test_the_actor_step_reads_the_stepped_critic(ok, tanhf):
    """A large lr_critic makes the critic from before and after its step differ visibly: the restatement with the stale critic gives
    another actor gradient, and the host entry equals the right one."""
    R, H, Hc, B = 5, 16, 16, 64
    rng = np.random.default_rng(13)
    cfg = config(H, Hc, lr_critic=0.05, sample_seed=4)
    st, rg = fresh_state(rng, R, H, Hc), filled_ring(rng, R, 100, 100)
    got = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, B, 1)
    right = G_.update(cfg, R, st, rg, B, tanhf, 1)
    wrong = G_.update(cfg, R, st, rg, B, tanhf, 1, stale_critic=True)
    assert not np.array_equal(bits(right[1]["grad_actor"]), bits(wrong[1]["grad_actor"])) and right[1]["actor_loss"][0] != wrong[1]["actor_loss"][0]
    assert_same_update(*got, *right, ("stepped critic",))


# ---- against the reference's expressions in torch float64 ----------------------------------------------------------------------------

def torch_iteration(st, cfg, R, H, Hc, batch, dtype):
    """DDPGAgent::update (DDPGAgent.hpp:127-170) restated: mse_loss, -critic(s, actor(s)).mean(), Adam, the soft-update line."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    nets = {k: [t(a).requires_grad_(k in ("actor", "critic")) for a in L_.split(st[k], *(((R, H, 2)) if "actor" in k else (R + 2, Hc, 1)))]
            for k in ("actor", "critic", "actor_target", "critic_target")}
    scale, bias = t(np.asarray(cfg["scale"], f32)), t(np.asarray(cfg["bias"], f32))
    mlp = lambda n, x: torch.relu(x @ n[0].T + n[1]) @ n[2].T + n[3]
    actor = lambda n, x: torch.tanh(mlp(n, x)) * scale + bias
    critic = lambda n, s, a: mlp(n, torch.cat([s, a], 1))
    s, a, r, s2, d = (t(batch[k]) for k in ("state", "action", "reward", "next_state", "done"))
    f = lambda v: float(f32(v))
    opt_c = torch.optim.Adam(nets["critic"], lr=f(cfg["lr_critic"]), betas=(f(cfg["beta1"]), f(cfg["beta2"])), eps=f(cfg["eps"]))
    opt_a = torch.optim.Adam(nets["actor"], lr=f(cfg["lr_actor"]), betas=(f(cfg["beta1"]), f(cfg["beta2"])), eps=f(cfg["eps"]))
    with torch.no_grad():
        y = r[:, None] + (1 - d[:, None]) * f(cfg["gamma"]) * critic(nets["critic_target"], s2, actor(nets["actor_target"], s2))
    critic_loss = torch.nn.functional.mse_loss(critic(nets["critic"], s, a), y)
    opt_c.zero_grad()
    critic_loss.backward()
    gc = torch.cat([p.grad.reshape(-1) for p in nets["critic"]]).double().numpy().copy()
    opt_c.step()
    actor_loss = -critic(nets["critic"], s, actor(nets["actor"], s)).mean()
    opt_a.zero_grad()
    actor_loss.backward()
    ga = torch.cat([p.grad.reshape(-1) for p in nets["actor"]]).double().numpy().copy()
    opt_a.step()
    tau, out = f(cfg["tau"]), {}
    with torch.no_grad():
        for net in ("actor", "critic"):
            for p, q in zip(nets[net], nets[net + "_target"]):
                q.copy_(tau * p + (1 - tau) * q)
            out[net] = torch.cat([p.reshape(-1) for p in nets[net]]).double().numpy()
            out[net + "_target"] = torch.cat([p.reshape(-1) for p in nets[net + "_target"]]).double().numpy()
    out.update(grad_critic=gc, grad_actor=ga, critic_loss=float(critic_loss.detach()), actor_loss=float(actor_loss.detach()))
    return out


@pytest.mark.parametrize("shape,scale", [((5, 128, 128), 0.3), ((7, 9, 13), 0.5), ((62, 256, 256), 0.05)])
def test_first_iteration_against_torch_float64(ok, shape, scale):
    """The first iteration's two losses and two gradients, and the four networks after it, against autograd in float64.

    Notation: u = 2^-24; for a network, hid_j = |b1_j| + |w1_j| |x| and Z = |b2| + |w2| hid are the float64 sums of absolute terms behind
    a hidden unit and an output.  A hidden value is a sum of in + 1 terms: |h - h64| <= (in + 2) u hid.  An output is within
    k_out u Z of its float64 value, k_out = in + H / 8 + 8 (tests/test_dqn_rule.py).  The rule's sums of B terms (chunk of 32, log2 C
    tree levels, a product per term, scale and division) cost k_sum = 32 + log2 C + 3 roundings relative to the sum of absolute terms.

    Critic.  a' = tanh(z') scale + bias: tanh is 1-Lipschitz and ok_tanhf within 1 ulp, so
        Da'_k = |scale_k| (k_out u Za'_k + 2u) + 2u (|scale_k| + |bias_k|).
    The critic is Lipschitz in the action with L_k = sum_j |w2_j| |w1_j,R+k|, so with S = Zc(s, a) + |r| + g Zc'(s', a') (g = gamma (1 - done))
        |e - e64| <= De = (k_out + 4) u S + g sum_k L'_k Da'_k.
    The gradient is (2 / B) sum_b e_b c_b with c an input, a hidden value, or w2_j (hidden seed); exactly tests/test_dqn_rule.py's
    derivation with S in place of |e| and the extra absolute seed error De:
        |gc - gc64| <= 2 (T[(k_sum + in + 17) u S + De] + E[S]),
    T[w]_p = (2 / B) sum_b w_b |c_bp| over units that are active or within their rounding error of 0, E[w] the hidden values' absolute
    error (in + 2) u hid on the second layer's weights.  loss: 2 (k_sum + 2) u sum S^2 / B + 2 sum_b (2 S_b De_b) / B.

    Adam's first step from zero moments is p - lr g / (|g| + eps) up to 8 roundings, whose derivative in g is lr eps / (|g| + eps)^2:
        |p_new - p_new64| <= Dp = u |p| + lr (8u + min(2, bg eps / (max(|g64| - bg, 0) + eps)^2)),    bg the gradient's bound.
    Actor.  Its step reads the stepped critic, so the critic's Dp enters: with the unit set A_b (active, or within
    thr_j = (in + 2) u hid_j + |Dw1_j| |x| + |Db1_j| + sum_k |w1_j,R+k| Da_k of 0, which may flip and then changes da by its whole term)
        Dda_k = sum_{j in A} ((Hc / 8 + 6) u |w1 w2| + |Dw1| |w2| + |w1| |Dw2| + |Dw1| |Dw2|) + sum_{j flips} |w1_j,R+k w2_j|
        Ddz_k = |scale_k| ((1 - t^2) Dda_k + |da_k| (2 |t| (k_out u Za_k + 2u) + 2u)) + 3u |dz_k|
    and the actor's gradient -(1 / B) sum_b sum_k dz_bk c_bk is bounded as the critic's:
        |ga - ga64| <= 2 (T[Ddz + (k_sum + R + 18) u (|dz| + Ddz)] + E[|dz| + Ddz]).
    actor loss: q's error k_out u Zc + sum_k L_k Da_k + the stepped parameters' (|Dw2| h + |w2| (|Dw1| |x| + |Db1|) + |Db2|), averaged,
    plus (k_sum + 2) u mean Zc.  Targets: tau Dp + 3u (|p| + |target|).  torch's own float32 run must meet every bound too."""
    R, H, Hc = shape
    B, inn = 200, R + 2
    rng = np.random.default_rng(R * H)
    cfg = config(H, Hc, sample_seed=4)
    st = fresh_state(rng, R, H, Hc, scale)
    w1c, b1c, w2c, b2c = L_.split(st["critic"], inn, Hc, 1)
    w1c[0], b1c[0] = 0.0, 0.0  # a pre-activation of exactly 0 on every side: any derivative other than 0 breaks the bound
    rg = filled_ring(rng, R, 500, 500)
    new, out = ok.ddpg_update_host(cfg_of(ok, cfg), R, st, rg, B, 1)
    idx = out["index"]
    batch = {k: rg[k][idx] for k in RING_FIELDS}
    ref = torch_iteration(st, cfg, R, H, Hc, batch, __import__("torch").float64)
    t32 = torch_iteration(st, cfg, R, H, Hc, batch, __import__("torch").float32)
    d64 = lambda a: np.asarray(a, dtype=np.float64)
    sc, bi = d64(f32(cfg["scale"])), d64(f32(cfg["bias"]))
    gamma, tau = float(f32(cfg["gamma"])), float(f32(cfg["tau"]))
    k_sum = (32 + np.log2((B + 31) // 32) + 3) * U

    def net64(p, n_in, hid, n_out):
        return [d64(a) for a in L_.split(p, n_in, hid, n_out)]

    def absnet(net, x):
        hid = np.abs(net[1]) + np.abs(x) @ np.abs(net[0]).T
        return hid, np.abs(net[3]) + hid @ np.abs(net[2]).T

    def fwd(net, x):
        pre = x @ net[0].T + net[1]
        return pre, np.maximum(pre, 0) @ net[2].T + net[3]

    def T_of(w, net, x, pre, active):
        """per-parameter (1 / B) sum_b of the absolute terms with output weights w [B, out]"""
        ds = (w @ np.abs(net[2])) * active
        return np.concatenate([(ds[:, :, None] * np.abs(x)[:, None, :]).reshape(B, -1).sum(0), ds.sum(0),
                               (w[:, :, None] * np.maximum(pre, 0)[:, None, :]).reshape(B, -1).sum(0), w.sum(0)]) / B

    def E_of(w, hid_abs, active, n_in, hid, n_out):
        e = np.zeros(hid * n_in + hid + n_out * hid + n_out)
        e[hid * n_in + hid:hid * n_in + hid + n_out * hid] = (w[:, :, None] * ((n_in + 2) * U * hid_abs * active)[:, None, :]).reshape(B, -1).sum(0) / B
        return e

    def adam_dev(p, g64, bg, lr, eps=float(f32(cfg["eps"]))):
        return U * np.abs(p) + lr * (8 * U + np.minimum(2.0, bg * eps / (np.maximum(np.abs(g64) - bg, 0.0) + eps) ** 2))

    x, xn, a, r, d = (d64(batch[k]) for k in ("state", "next_state", "action", "reward", "done"))
    A, At, Cn, Ct = net64(st["actor"], R, H, 2), net64(st["actor_target"], R, H, 2), net64(st["critic"], inn, Hc, 1), net64(st["critic_target"], inn, Hc, 1)
    k_a, k_c = (R + H / 8.0 + 8.0) * U, (inn + Hc / 8.0 + 8.0) * U
    # the critic
    _, Zat = absnet(At, xn)
    an = np.tanh(fwd(At, xn)[1]) * sc + bi
    Dan = np.abs(sc) * (k_a * Zat + 2 * U) + 2 * U * (np.abs(sc) + np.abs(bi))
    xcn, xc = np.concatenate([xn, an], 1), np.concatenate([x, a], 1)
    _, Zct = absnet(Ct, xcn)
    hid_c, Zc = absnet(Cn, xc)
    g = gamma * (1 - d)
    Lt = (np.abs(Ct[2][0])[:, None] * np.abs(Ct[0][:, R:])).sum(0)
    S = Zc[:, 0] + np.abs(r) + g * Zct[:, 0]
    De = (k_c + 4 * U) * S + g * (Dan @ Lt)
    pre_c, _ = fwd(Cn, xc)
    act_c = pre_c > -(inn + 2) * U * hid_c
    act_c[:, 0] = False
    w = (k_sum + (inn + 17) * U) * S + De
    bound_gc = 2.0 * (2.0 * T_of(w[:, None], Cn, xc, pre_c, act_c) + 2.0 * E_of(S[:, None], hid_c, act_c, inn, Hc, 1)) + 1e-300
    bound_lc = 2.0 * (k_sum + 2 * U) * (S ** 2).sum() / B + 2.0 * (2 * S * De).sum() / B
    Dpc = adam_dev(d64(st["critic"]), ref["grad_critic"], bound_gc, float(f32(cfg["lr_critic"])))
    # the actor, through the stepped critic
    Cs = net64(ref["critic"], inn, Hc, 1)
    Dw1, Db1, Dw2, Db2 = Dpc[:Hc * inn].reshape(Hc, inn), Dpc[Hc * inn:Hc * inn + Hc], Dpc[Hc * inn + Hc:Hc * inn + 2 * Hc].reshape(1, Hc), Dpc[-1:]
    hid_a, Za = absnet(A, x)
    pre_a, za = fwd(A, x)
    th = np.tanh(za)
    act = th * sc + bi
    Da = np.abs(sc) * (k_a * Za + 2 * U) + 2 * U * (np.abs(sc) + np.abs(bi))
    xs = np.concatenate([x, act], 1)
    hid_s, Zs = absnet(Cs, xs)
    pre_s, q64 = fwd(Cs, xs)
    thr = (inn + 2) * U * hid_s + np.abs(xs) @ Dw1.T + Db1 + Da @ np.abs(Cs[0][:, R:]).T
    on, flips = pre_s > -thr, np.abs(pre_s) <= thr
    w12 = np.abs(Cs[0][:, R:]) * np.abs(Cs[2][0])[:, None]  # [Hc, 2]
    per_unit = (Hc / 8.0 + 6) * U * w12 + Dw1[:, R:] * np.abs(Cs[2][0])[:, None] + np.abs(Cs[0][:, R:]) * Dw2[0][:, None] + Dw1[:, R:] * Dw2[0][:, None]
    Dda = on @ per_unit + flips @ w12
    da = (pre_s > 0) @ (Cs[0][:, R:] * Cs[2][0][:, None])
    dz = da * sc * (1 - th ** 2)
    Ddz = np.abs(sc) * ((1 - th ** 2) * Dda + np.abs(da) * (2 * np.abs(th) * (k_a * Za + 2 * U) + 2 * U)) + 3 * U * np.abs(dz)
    act_a = pre_a > -(R + 2) * U * hid_a
    mz = np.abs(dz) + Ddz
    bound_ga = 2.0 * (T_of(Ddz + (k_sum + (R + 18) * U) * mz, A, x, pre_a, act_a) + E_of(mz, hid_a, act_a, R, H, 2)) + 1e-300
    Ls = (np.abs(Cs[2][0])[:, None] * np.abs(Cs[0][:, R:])).sum(0)
    Dq = k_c * Zs[:, 0] + Da @ Ls + np.maximum(pre_s, 0) @ Dw2[0] + (np.abs(xs) @ Dw1.T + Db1) @ np.abs(Cs[2][0]) + Db2[0]
    bound_la = 2.0 * (Dq.mean() + (k_sum + 2 * U) * Zs[:, 0].mean())
    Dpa = adam_dev(d64(st["actor"]), ref["grad_actor"], bound_ga, float(f32(cfg["lr_actor"])))
    bounds = {"grad_critic": bound_gc, "grad_actor": bound_ga, "critic_loss": bound_lc, "actor_loss": bound_la, "critic": Dpc, "actor": Dpa,
              "critic_target": tau * Dpc + 3 * U * (np.abs(ref["critic"]) + np.abs(ref["critic_target"])),
              "actor_target": tau * Dpa + 3 * U * (np.abs(ref["actor"]) + np.abs(ref["actor_target"]))}
    ours = dict(out, **{k: new[k] for k in ("actor", "critic", "actor_target", "critic_target")})
    ours["critic_loss"], ours["actor_loss"] = out["critic_loss"][0], out["actor_loss"][0]
    for k, bnd in bounds.items():
        err, err32 = np.abs(d64(ours[k]) - ref[k]), np.abs(d64(t32[k]) - ref[k])
        print("%s %-13s max err / bound = %.3g (torch fp32: %.3g), max |value| = %.3g, max bound = %.3g" % (
            shape, k, np.max(err / bnd), np.max(err32 / bnd), np.max(np.abs(ref[k])), np.max(bnd)))
        assert np.all(err <= bnd), k
        assert np.all(err32 <= bnd), k + " (torch float32)"


# ---- validation ----------------------------------------------------------------------------------------------------------------------

def test_validation(ok):
    L = ok.capi.load()
    R, H, Hc = 5, 8, 8
    rng = np.random.default_rng(1)
    st, rg = fresh_state(rng, R, H, Hc), filled_ring(rng, R, 16, 16)

    def update(B=4, iterations=1, state=st, ring=rg, size=None, rays=R, **kw):
        with pytest.raises(ok.capi.OkenvError) as e:
            ok.ddpg_update_host(cfg_of(ok, config(kw.pop("hidden", H), kw.pop("critic_hidden", Hc), **kw)), rays, state, ring, B, iterations, size=size)
        assert e.value.code == -1, e.value
        return str(e.value)

    assert "B and iterations" in update(B=0) and "B and iterations" in update(iterations=0)
    for bad in (1.5, -0.1, float("nan")):
        assert "gamma" in update(gamma=bad) and "tau" in update(tau=bad)
    assert "noise" in update(noise=(-1.0, 0.0)) and "noise" in update(noise=(0.0, float("nan")))
    assert "width" in update(hidden=300) and "width" in update(critic_hidden=0) and "size" in update(size=-1)
    assert "learning rate" in update(lr_actor=0.0) and "learning rate" in update(lr_critic=-1.0) and "beta" in update(beta1=1.0) and "eps" in update(eps=0.0)
    big = fresh_state(rng, 63, H, Hc)
    assert "62 rays" in update(rays=63, state=big, ring=filled_ring(rng, 63, 16, 16))
    cfg = cfg_of(ok, config(H, Hc))
    ring_s = ok.capi.fill_pointers(ok.capi.OkenvDdpgRing(), {k: rg[k] for k in RING_FIELDS}, "ring")
    no_reward = ok.capi.fill_pointers(ok.capi.OkenvDdpgRing(), {k: rg[k] for k in RING_FIELDS if k != "reward"}, "ring")
    vec = {k: st[k].copy() for k in G_.VECTORS}
    full = ok.capi.fill_pointers(ok.capi.OkenvDdpgState(), vec, "state")
    part = ok.capi.fill_pointers(ok.capi.OkenvDdpgState(), {k: v for k, v in vec.items() if k != "critic_v"}, "state")
    assert L.okenv_ddpg_update_host(C.byref(cfg), R, C.byref(full), C.byref(ring_s), 16, 4, 1, 0, 0, None) == 0
    assert L.okenv_ddpg_update_host(None, R, C.byref(full), C.byref(ring_s), 16, 4, 1, 0, 0, None) == -1
    assert L.okenv_ddpg_update_host(C.byref(cfg), R, None, C.byref(ring_s), 16, 4, 1, 0, 0, None) == -1
    assert L.okenv_ddpg_update_host(C.byref(cfg), R, C.byref(part), C.byref(ring_s), 16, 4, 1, 0, 0, None) == -1
    assert L.okenv_ddpg_update_host(C.byref(cfg), R, C.byref(full), C.byref(no_reward), 16, 4, 1, 0, 0, None) == -1
    assert L.okenv_ddpg_update_host(C.byref(cfg), R, C.byref(full), None, 16, 4, 1, 0, 0, None) == -1
    # acting
    dist = np.ones((2, R), f32)
    p = ok.capi.ptr
    assert L.okenv_ddpg_act_host(C.byref(cfg), p(vec["actor"]), R, 2, p(dist), None, 0, None, None, None, None, None) == 0
    assert L.okenv_ddpg_act_host(None, p(vec["actor"]), R, 2, p(dist), None, 0, None, None, None, None, None) == -1
    assert L.okenv_ddpg_act_host(C.byref(cfg), None, R, 2, p(dist), None, 0, None, None, None, None, None) == -1
    assert L.okenv_ddpg_act_host(C.byref(cfg), p(vec["actor"]), R, 2, None, None, 0, None, None, None, None, None) == -1
    assert L.okenv_ddpg_act_host(C.byref(cfg), p(vec["actor"]), 63, 2, p(dist), None, 0, None, None, None, None, None) == -1
    assert L.okenv_ddpg_act_host(C.byref(cfg), p(vec["actor"]), R, -1, p(dist), None, 0, None, None, None, None, None) == -1
    # the push
    n = 4
    state, action, alive, dist, crashed = step_data(rng, n, R, "all")
    pushed = C.c_uint64(0)

    def push(ring=ring_s, capacity=16, rays=R, flags=0, n=n, state=state, action=action, alive=alive, dist=dist, crashed=crashed, counter=pushed):
        return L.okenv_ddpg_replay_push_host(C.byref(ring) if ring is not None else None, capacity, rays, C.byref(counter) if counter is not None else None,
                                             flags, n, p(state), p(action), p(alive), p(dist), p(crashed), None)

    assert push() == 0 and pushed.value == 4
    assert push(capacity=0) == -1 and b"capacity" in L.okenv_last_error(None)
    assert push(flags=2) == -1 and b"unknown flags" in L.okenv_last_error(None)
    assert push(ring=None) == -1 and push(ring=no_reward) == -1 and push(counter=None) == -1
    assert push(state=None) == -1 and push(action=None) == -1
    assert push(alive=None) == -1 and b"alive" in L.okenv_last_error(None)
    assert push(alive=None, flags=ok.capi.REPLAY_PUSH_ALL) == 0
    assert push(dist=None) == -1 and push(crashed=None) == -1 and push(rays=63) == -1 and push(n=-1) == -1
    assert pushed.value == 8
    # entries that take the handle refuse a NULL one
    assert L.okenv_ddpg_create(None, C.byref(cfg)) == -1 and L.okenv_ddpg_act(None, None) == -1 and L.okenv_ddpg_update(None, 4, 1, 0, 0, None) == -1
    assert L.okenv_ddpg_replay_create(None, 8, 0) == -1 and L.okenv_ddpg_replay_push(None, None, None) == -1 and L.okenv_ddpg_replay_get(None, None) == -1
    assert L.okenv_ddpg_set_params(None, None, None) == -5 and L.okenv_ddpg_replay_reset(None) == -5 and L.okenv_ddpg_replay_size(None, None, None) == -5
    assert L.okenv_ddpg_get_state(None, None) == -1 and L.okenv_ddpg_num_params(None, None, None) == -5 and L.okenv_debug_ddpg_timing(None, None) == -1


# ---- closed loop with the oracle's Environment::step ----------------------------------------------------------------------------

def test_closed_loop_on_the_cpu(ok, oracle, tanhf):
    """ddpg_sim.cpp:55-95 for 300 steps: act, the oracle's Environment::step, push -- the host entries against the restatement."""
    N, R, H, steps, capacity = 48, 5, 32, 300, 1000
    fan = np.array([-70, -30, 0, 30, 70], dtype=f32)
    t = oracle.Track("Silverstone")
    env = oracle.OracleEnv(t.segments, N, R, fan, (t.x, t.y, t.heading))
    env.set_lane_bounds(t.li, t.ri)
    env.reset_random(None, 1, 17, 0, 0)
    env.step(1)
    rng = np.random.default_rng(3)
    actor = (rng.standard_normal(G_.n_actor(R, H)) * 0.5).astype(f32)
    cfg = config(H, 1, noise=(10.0, 1.0), seed=17)
    got, want = ok.ddpg_ring(capacity, R), G_.ring(capacity, R)
    for count in range(1, steps + 1):
        dist, crashed = env.get(oracle.F_DIST), env.get(oracle.F_CRASHED)
        rec = ok.ddpg_act_host(cfg_of(ok, cfg), actor, dist, crashed, count)
        a, x = G_.act(cfg, actor, R, dist, count, tanhf)
        assert np.array_equal(bits(rec["action"]), bits(a)) and np.array_equal(bits(rec["state"]), bits(x)), count
        env.set(oracle.F_THR, rec["throttle"])
        env.set(oracle.F_STEER, rec["steer"])
        env.step(1)
        after, now = env.get(oracle.F_DIST), env.get(oracle.F_CRASHED)
        ok.ddpg_replay_push_host(got, rec["state"], rec["action"], rec["alive"], after, now)
        G_.push(want, x, a, 1 - crashed, after, now)
    assert got["pushed"] == want["pushed"] > capacity  # the ring wrapped
    for k in RING_FIELDS:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert got["done"].any() and not got["done"].all()
