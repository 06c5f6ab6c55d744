"""The shared-network actors' rule on the CPU (include/okenv_math.h ok_expf / ok_actor_*, okenv_actor_act_host): ok_expf against
fp64, the host entry against an independent numpy restatement (tests/_actor_numpy.py), the sampling as the inverse CDF of the recorded
probabilities, the networks against torch in float64 with a derived bound, a closed loop with the oracle's step, and validation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _actor_numpy as A_

f32 = np.float32
PPO_ACTIONS = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0))
TABLE8 = tuple((10.0 * k + 5.0, 2.5 * k - 9.0) for k in range(8))
U = 2.0 ** -24  # unit roundoff of fp32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def n_params(R, H, out):
    return H * R + H + out * H + out


# ---- ok_expf ---------------------------------------------------------------------------------------------------------------------

def expf_arguments():
    rng = np.random.default_rng(2024)
    parts = [-(rng.random(600_000) * 104.0), -(rng.random(200_000) ** 4) * 2.0, -np.exp(rng.uniform(np.log(1e-9), np.log(104.0), 100_000))]
    # around every power-of-two boundary of the result: x = -k ln 2 and 4096 neighbours on both sides (k = 0 .. 150 covers the
    # subnormal results down to underflow)
    for k in range(0, 151):
        centre = f32(-k * np.log(2.0))
        up = np.full(2048, centre, dtype=f32)
        down = up.copy()
        for i in range(1, 2048):
            up[i] = np.nextafter(up[i - 1], f32(0))
            down[i] = np.nextafter(down[i - 1], f32(-np.inf))
        parts += [up.astype(np.float64), down.astype(np.float64)]
    parts.append(-np.linspace(87.0, 104.0, 100_000))  # subnormal results
    x = np.concatenate(parts).astype(f32)
    return x[(x <= 0) & (x >= -104)]


def test_expf_against_fp64(ok):
    x = expf_arguments()
    assert x.size >= 1_000_000
    got = ok.debug_expf(x)
    with np.errstate(under="ignore"):
        want = np.exp(x.astype(np.float64)).astype(f32)
    diff = got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)
    differing = int((diff != 0).sum())
    print("ok_expf: %d of %d arguments differ from the rounded fp64 exp (share %.3g)" % (differing, x.size, differing / x.size))
    assert np.abs(diff).max() <= 1
    assert differing <= 1e-5 * x.size
    assert (want[x < -88] < 1.2e-38).any() and (got[x < -88] > 0).any()  # subnormal results are in the set
    special = ok.debug_expf(np.array([-np.inf, np.nan, 0.0, -0.0], dtype=f32))
    assert special[0] == 0 and np.isnan(special[1]) and special[2] == 1 and special[3] == 1


# ---- host entry against the numpy restatement ---------------------------------------------------------------------------------

def make_case(rng, R, H, A, Hv, scale, n, tied=False):
    policy = (rng.standard_normal(n_params(R, H, A)) * scale).astype(f32)
    if tied:  # exactly tied logits: no second-layer weights, equal biases
        policy[H * R + H:H * R + H + A * H] = 0
        policy[H * R + H + A * H:] = f32(0.25)
    value = (rng.standard_normal(n_params(R, Hv, 1)) * scale).astype(f32) if Hv else None
    dist = (rng.random((n, R)) * 200.0).astype(f32)
    dist[0, :] = 0.0
    dist[1 % n, :] = 200.0
    dist[2 % n, ::2] = 0.0
    return policy, value, dist


def check_against_numpy(ok, R, H, A, Hv, mode, eps, policy, value, dist, seed, base, draw):
    table = TABLE8[:A]
    ap = ok.capi.actor_params(H, table, Hv, mode, eps, seed, base)
    got = ok.actor_act_host(ap, policy, value, dist, draw_index=draw)
    want = A_.act(ok.debug_expf, mode, eps, seed, base, table, policy, value, R, H, A, Hv, dist, draw)
    what = (R, H, A, Hv, mode, eps)
    assert np.array_equal(got["action"], want["action"]), what
    for k in ("prob", "throttle", "steer", "state") + (("value",) if Hv else ()):
        assert np.array_equal(bits(got[k]), bits(want[k])), (k,) + what
    return got, want


@pytest.mark.parametrize("R", [1, 5, 15, 64])
def test_host_entry_equals_the_numpy_restatement(ok, R):
    rng = np.random.default_rng(100 + R)
    variants = [(A_.SAMPLE, 0.0), (A_.GREEDY, 0.0), (A_.EPS_GREEDY, 0.0), (A_.EPS_GREEDY, 0.3), (A_.EPS_GREEDY, 1.0)]
    clamped_low = clamped_high = ties = 0
    for i, (H, A) in enumerate(itertools.product([1, 16, 128, 256], [2, 3, 5, 8])):
        for with_value in (False, True):
            Hv = [1, 16, 128, 256][(i + 1) % 4] if with_value else 0
            scale = [0.1, 1.0, 30.0][(i + with_value) % 3]
            policy, value, dist = make_case(rng, R, H, A, Hv, scale, n=24)
            for mode, eps in variants:
                got, want = check_against_numpy(ok, R, H, A, Hv, mode, eps, policy, value, dist, seed=7 + i, base=1000 * i, draw=i * 13 + mode)
                if mode == A_.SAMPLE:
                    clamped_low += int((want["p"] < 1e-8).sum())
                    clamped_high += int((got["prob"] == 1.0).sum())
        policy, value, dist = make_case(rng, R, H, A, 0, 1.0, n=24, tied=True)
        for mode, eps in variants:
            got, _ = check_against_numpy(ok, R, H, A, 0, mode, eps, policy, value, dist, seed=3, base=0, draw=i)
            if mode == A_.GREEDY:
                assert (got["action"] == 0).all()  # lowest index wins the tie
                ties += 1
    if R > 1:  # (one weight times x <= 1: a single ray does not push the logits far enough apart)
        assert clamped_low > 0 and clamped_high > 0, "no case saturated the softmax into the clamp"
    assert ties == 16


def test_global_agent_ids_shard(ok):
    """agent_base + i is the id the draws see: two halves with their bases give the whole."""
    rng = np.random.default_rng(5)
    R, H, A, n = 5, 128, 3, 512
    policy, _, dist = make_case(rng, R, H, A, 0, 0.05, n)  # (a soft distribution: the draws matter)
    whole = ok.actor_act_host(ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample", 0, 9, 0), policy, None, dist, draw_index=4)
    for lo in (0, n // 2):
        half = ok.actor_act_host(ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample", 0, 9, lo), policy, None, dist[lo:lo + n // 2], draw_index=4)
        assert np.array_equal(half["action"], whole["action"][lo:lo + n // 2])
    other = ok.actor_act_host(ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample", 0, 9, 0), policy, None, dist, draw_index=5)
    assert not np.array_equal(other["action"], whole["action"])  # another draw index, other draws


# ---- sampling is the inverse CDF of the recorded probabilities -------------------------------------------------------------------

@pytest.mark.parametrize("A,scale", [(3, 1.0), (8, 0.6), (2, 2.0)])
def test_sampling_frequencies_follow_the_recorded_probabilities(ok, A, scale):
    R, H, n_draws = 5, 16, 2 ** 16
    rng = np.random.default_rng(40 + A)
    policy, _, _ = make_case(rng, R, H, A, 0, scale, 1)
    dist = np.array([[150.0, 60.0, 120.0, 30.0, 90.0]], dtype=f32)
    table = TABLE8[:A]
    ap = ok.capi.actor_params(H, table, 0, "sample", 0.0, 77, 12)
    p32 = A_.act(ok.debug_expf, A_.SAMPLE, 0.0, 77, 12, table, policy, None, R, H, A, 0, dist, 0)["p"][0]
    p = p32.astype(np.float64)
    L = ok.capi.load()
    action, prob = np.zeros(1, np.int64), np.zeros(1, f32)
    counts = np.zeros(A, np.int64)
    for draw in range(n_draws):
        ok.capi.check(L.okenv_actor_act_host(C.byref(ap), ok.capi.ptr(policy), None, R, 1, ok.capi.ptr(dist), None, draw, None, None,
                                             ok.capi.ptr(action), ok.capi.ptr(prob), None, None, None))
        counts[action[0]] += 1
        assert prob[0] == max(p32[action[0]], f32(1e-8))  # the recorded probability is the clamped p of the action
    freq = counts / n_draws
    sigma = np.sqrt(p * (1.0 - p) / n_draws)
    print("A=%d p=%s freq=%s" % (A, np.round(p, 4), np.round(freq, 4)))
    assert (np.abs(freq - p) <= 5.0 * sigma).all()


# ---- against the networks users hand in: torch in float64 ------------------------------------------------------------------------

def layer_bound(w, b, x, dx, terms):
    """|computed - exact| of b + sum w x for inputs x known to within dx, fp32 sums of `terms` terms in any order:
    (terms + 2) u (|b| + sum |w x|) for the roundings (one per multiplication and addition, the bound of a recursive sum of
    terms + 1 numbers, the input's own rounding in the + 2) plus the inputs' errors passed through |w|."""
    mag = np.abs(b)[None, :] + np.abs(x) @ np.abs(w).T
    return (terms + 2) * U * mag + dx @ np.abs(w).T


@pytest.mark.parametrize("R,H,A,Hv,scale", [(5, 128, 3, 128, 0.3), (15, 64, 5, 32, 0.5), (64, 256, 8, 256, 0.1), (1, 1, 2, 1, 1.0), (5, 16, 3, 0, 3.0)])
def test_networks_against_torch_float64(ok, R, H, A, Hv, scale):
    import torch
    torch.manual_seed(R * 1000 + H)
    rng = np.random.default_rng(R + H + A)
    n = 400
    actor = torch.nn.Sequential(torch.nn.Linear(R, H), torch.nn.ReLU(), torch.nn.Linear(H, A), torch.nn.Softmax(dim=1))
    critic = torch.nn.Sequential(torch.nn.Linear(R, Hv), torch.nn.ReLU(), torch.nn.Linear(Hv, 1)) if Hv else None
    with torch.no_grad():
        for net in (actor, critic):
            if net is not None:
                for prm in net.parameters():
                    prm.mul_(scale * 4.0)
    flat = lambda net: torch.cat([q.detach().reshape(-1) for q in net.parameters()]).numpy().astype(f32)  # noqa: E731
    policy, value = flat(actor), (flat(critic) if critic is not None else None)
    dist = (rng.random((n, R)) * 200.0).astype(f32)
    ap = ok.capi.actor_params(H, TABLE8[:A], Hv, "greedy", 0.0, 1, 0)
    got = ok.actor_act_host(ap, policy, value, dist, draw_index=0)
    ours = A_.act(ok.debug_expf, A_.GREEDY, 0.0, 1, 0, TABLE8[:A], policy, value, R, H, A, Hv, dist, 0)
    assert np.array_equal(bits(got["prob"]), bits(ours["prob"]))  # the restatement's unclamped p is the library's p
    x64 = torch.from_numpy(dist.astype(np.float64) / 200.0)
    x = x64.numpy()
    dx = np.abs(x) * U  # the fp32 division
    with torch.no_grad():
        p64 = actor.double()(x64).numpy()
        z64 = actor[:3](x64).numpy()
        v64 = critic.double()(x64).numpy()[:, 0] if critic is not None else None
        actor.float()
        p32 = actor(torch.from_numpy(dist) / 200.0).numpy().astype(np.float64)
        if critic is not None:
            critic.float()
            v32 = critic(torch.from_numpy(dist) / 200.0).numpy()[:, 0].astype(np.float64)

    def net_bound(params, hidden, out):
        w1, b1, w2, b2 = (a.astype(np.float64) for a in A_.split(params, R, hidden, out))
        dh = layer_bound(w1, b1, x, dx, R)
        h = np.maximum(b1[None, :] + x @ w1.T, 0.0) + dh  # relu is 1-Lipschitz; |h| bounded by exact + its error
        return layer_bound(w2, b2, h, dh, hidden)

    dz = net_bound(policy, H, A).max(axis=1, keepdims=True)
    # softmax: errors dz in every logit move p_k by a factor within exp(+-2 dz); z - m is one fp32 subtraction (u |z - m|), ok_expf
    # one ulp (2 u), the sum of A terms A u, the division u: relative, applied to p <= 1.
    spread = np.abs(z64 - z64.max(axis=1, keepdims=True))
    p_bound = p64 * (np.expm1(2.0 * dz + spread * U) + (A + 4) * U) + 2.0 ** -149
    err = np.abs(ours["p"].astype(np.float64) - p64)
    err32 = np.abs(p32 - p64)
    print("R=%d H=%d A=%d: max |p - p64| = %.3g (torch fp32: %.3g), smallest bound/error margin %.3g" % (
        R, H, A, err.max(), err32.max(), (p_bound / np.maximum(err, 1e-300)).min()))
    assert (err <= p_bound).all()
    assert (err32 <= p_bound).all()  # torch's own float32 forward lies inside the same bound: the bound is not vacuous
    if critic is not None:
        dv = net_bound(value, Hv, 1)[:, 0]
        ev, ev32 = np.abs(got["value"].astype(np.float64) - v64), np.abs(v32 - v64)
        print("    value: max |v - v64| = %.3g (torch fp32: %.3g), bound up to %.3g" % (ev.max(), ev32.max(), dv.max()))
        assert (ev <= dv).all() and (ev32 <= dv).all()


# ---- closed loop with the oracle's Environment::step ----------------------------------------------------------------------------

PPO_FAN = np.array([-70, -30, 0, 30, 70], dtype=f32)


def loop_networks(R=5, H=128, Hv=128, A=3, seed=123, scale=0.5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n_params(R, H, A)) * scale).astype(f32), (rng.standard_normal(n_params(R, Hv, 1)) * scale).astype(f32)


def cpu_loop(ok, oracle, track, N, steps, seed, mode="sample", eps=0.0, auto_reset=False, flags=1, agent_base=0, record=True, H=128, Hv=128):
    """ppo_sim.cpp:53-89 with the oracle's Environment::step and okenv_actor_act_host; the draw index is the step count."""
    t = oracle.Track(track)
    env = oracle.OracleEnv(t.segments, N, PPO_FAN.size, PPO_FAN, (t.x, t.y, t.heading))
    env.set_lane_bounds(t.li, t.ri)
    env.set_auto_reset(auto_reset, flags, seed, agent_base)
    env.reset_random(None, flags, seed, 0, agent_base)
    env.step(1)
    count = 1
    policy, value = loop_networks(H=H, Hv=Hv)
    ap = ok.capi.actor_params(H, PPO_ACTIONS, Hv, mode, eps, seed, agent_base)
    rec = []
    for _ in range(steps):
        out = ok.actor_act_host(ap, policy, value, env.get(oracle.F_DIST), crashed=env.get(oracle.F_CRASHED), draw_index=count)
        if record:
            rec.append(out)
        env.set(oracle.F_THR, out["throttle"])
        env.set(oracle.F_STEER, out["steer"])
        env.step(1)
        count += 1
    return env, rec


def test_closed_loop_on_the_cpu(ok, oracle):
    N, steps = 256, 600
    env, rec = cpu_loop(ok, oracle, "Silverstone", N, steps, seed=17)
    alive = np.stack([r["alive"] for r in rec])
    assert (np.diff(alive.astype(np.int8), axis=0) <= 0).all()  # nobody comes back without a reset
    lengths = alive.sum(axis=0)
    print("closed loop: %d of %d agents crashed within %d steps, %d different episode lengths, actions used %s" % (
        int((lengths < steps).sum()), N, steps, np.unique(lengths).size, np.bincount(np.concatenate([r["action"] for r in rec]), minlength=3)))
    assert np.unique(lengths).size > 10
    env2, rec2 = cpu_loop(ok, oracle, "Silverstone", N, 50, seed=17)
    assert all(np.array_equal(a["action"], b["action"]) for a, b in zip(rec[:50], rec2))


# ---- validation ------------------------------------------------------------------------------------------------------------------

def test_host_entry_validation(ok):
    L = ok.capi.load()
    R, H, A = 5, 8, 3
    policy = np.zeros(n_params(R, H, A), f32)
    value = np.zeros(n_params(R, 4, 1), f32)
    dist = np.zeros((2, R), f32)

    def call(ap, pol=policy, val=None, rays=R, n=2, d=dist):
        return L.okenv_actor_act_host(None if ap is None else C.byref(ap), ok.capi.ptr(pol), ok.capi.ptr(val), rays, n, ok.capi.ptr(d), None, 0,
                                      None, None, None, None, None, None, None)

    good = ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample")
    assert call(good) == 0
    assert call(None) == -1
    assert b"NULL" in L.okenv_last_error(None)
    for kwargs in (dict(hidden=0), dict(hidden=257), dict(value_hidden=-1), dict(value_hidden=257), dict(mode=3), dict(mode=-1),
                   dict(epsilon=-0.1), dict(epsilon=1.5), dict(epsilon=float("nan"))):
        args = dict(hidden=H, actions=PPO_ACTIONS, value_hidden=0, mode="sample", epsilon=0.0)
        args.update(kwargs)
        assert call(ok.capi.actor_params(**args)) == -1, kwargs
    bad = ok.capi.actor_params(H, PPO_ACTIONS, 0, "sample")
    for a in (1, 9):
        bad.num_actions = a
        assert call(bad) == -1
    assert call(good, rays=0) == -1 and call(good, rays=65) == -1
    assert call(good, pol=None) == -1 and call(good, d=None) == -1 and call(good, n=-1) == -1
    with_value = ok.capi.actor_params(H, PPO_ACTIONS, 4, "sample")
    assert call(with_value, val=None) == -1 and call(with_value, val=value) == 0
    assert L.okenv_debug_expf(None, None, 1) == -1
    # a NULL handle is refused, not dereferenced
    assert L.okenv_actor_create(None, C.byref(good)) == -1 and L.okenv_actor_act(None, None) == -1
    assert L.okenv_actor_set_params(None, None, None) != 0 and L.okenv_actor_num_params(None, None, None) != 0
    assert L.okenv_actor_set_epsilon(None, 0.5) != 0 and L.okenv_actor_set_draw_offset(None, None) != 0
