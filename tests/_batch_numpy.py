"""An independent numpy restatement of the episode-to-batch rule (include/okenv_batch.h), written from
the rule's text: float32 arithmetic for the walk (numpy float32 arrays over the agent axis: elementwise, so every agent sees the
scalar operations of the rule), float64 for the sums, its own tree.  Nothing here calls the library."""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = np.float32(np.finfo(np.float32).eps)


def tree(x):
    """The fixed tree over the agent index: pad with zeros to a power of two, then halve: x[i] + x[i + h]."""
    x = np.asarray(x, dtype=F64)
    p = 1
    while p < x.size:
        p *= 2
    x = np.concatenate([x, np.zeros(p - x.size, F64)])
    while x.size > 1:
        h = x.size // 2
        x = x[:h] + x[h:]
    return F64(x[0])


def finish(m, s, q):
    mean, sd = F64(0.0), F64(0.0)
    if m >= 1:
        mean = F64(s) / F64(m)
    if m >= 2:
        ss = F64(q) - F64(s) * mean
        if not ss > 0.0:
            ss = F64(0.0)
        sd = np.sqrt(ss / F64(m - 1))
    return F32(mean), F32(sd)


def normalize(x, mean, sd):
    den = F32(sd) + EPS
    return ((np.asarray(x, F32) - F32(mean)) / den).astype(F32)


def prepare(reward, alive, value=None, last_value=None, state=None, action=None, prob=None, num_agents=None, gamma=0.99, lam=1.0,
            normalize_ret=False, normalize_adv=False):
    """Every output of the rule for reward / alive / value [T, S] (the first num_agents slots of a row count) and the fields
    state [T, S', R], action [T, S'], prob [T, S']."""
    reward = np.asarray(reward, F32)
    T, S = reward.shape
    N = S if num_agents is None else num_agents
    reward = reward[:, :N]
    al = np.asarray(alive)[:, :N] != 0
    g = F32(gamma)
    gl = F32(F64(F32(gamma)) * F64(F32(lam)))
    has_value = value is not None
    c, a = np.zeros(N, F32), np.zeros(N, F32)
    v_next = np.zeros(N, F32) if (last_value is None or not has_value) else np.asarray(last_value, F32).copy()
    G, A = np.zeros((T, N), F32), np.zeros((T, N), F32)
    s_g, q_g, s_a, q_a = (np.zeros(N, F64) for _ in range(4))
    zero32, zero64 = np.zeros(N, F32), np.zeros(N, F64)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            live, r = al[t], reward[t]
            c = np.where(live, r + g * c, zero32)
            G[t] = c
            cd = c.astype(F64)
            s_g = s_g + np.where(live, cd, zero64)
            q_g = q_g + np.where(live, cd * cd, zero64)
            if has_value:
                v = np.asarray(value[t, :N], F32)
                delta = (r + g * v_next) - v
                a = np.where(live, delta + gl * a, zero32)
                A[t] = a
                ad = a.astype(F64)
                s_a = s_a + np.where(live, ad, zero64)
                q_a = q_a + np.where(live, ad * ad, zero64)
                v_next = np.where(live, v, zero32)
    M = int(al.sum())
    st = {"sum_ret": tree(s_g), "sumsq_ret": tree(q_g), "sum_adv": tree(s_a), "sumsq_adv": tree(q_a), "count": M}
    st["mean_ret"], st["std_ret"] = finish(M, st["sum_ret"], st["sumsq_ret"])
    st["mean_adv"], st["std_adv"] = finish(M if has_value else 0, st["sum_adv"], st["sumsq_adv"])
    flat = np.flatnonzero(al.reshape(-1))
    tt, ii = flat // N, flat % N
    out = {"M": M, "count": np.array([M], np.int32), "stats": st, "index": flat.astype(np.int32), "ret_plane": G}
    ret = G.reshape(-1)[flat]
    out["ret"] = normalize(ret, st["mean_ret"], st["std_ret"]) if normalize_ret else ret
    if has_value:
        out["adv_plane"] = A
        adv = A.reshape(-1)[flat]
        out["adv"] = normalize(adv, st["mean_adv"], st["std_adv"]) if normalize_adv else adv
    if state is not None:
        out["state"] = np.asarray(state, F32)[tt, ii]
    if action is not None:
        out["action"] = np.asarray(action, np.int64)[tt, ii]
    if prob is not None:
        out["prob"] = np.asarray(prob, F32)[tt, ii]
    return out


# ---- test records ------------------------------------------------------------------------------------------------------------

MASKS = ("monotone", "interior", "all_dead", "one_sample", "one_to_last")
REWARDS = ("step", "progress")


def make_mask(kind, T, N, rng):
    if kind == "monotone":  # no auto-reset: an agent drives for `length` rows; lengths 0 and T occur
        length = rng.integers(0, T + 1, size=N)
        length[rng.integers(0, N)] = T
        if N > 1:
            length[(int(np.argmax(length == T)) + 1) % N] = 0
        return np.arange(T)[:, None] < length[None, :]
    if kind == "interior":  # auto-reset: dead rows inside the columns, several episodes per column
        m = rng.random((T, N)) >= 0.03
        if T >= 3:
            m[T // 2, :] = False  # an interior boundary in every column ...
            m[T // 2 - 1, 0] = True
            m[T // 2 + 1, 0] = True  # ... with live rows on both sides in column 0
        return m
    m = np.zeros((T, N), bool)
    if kind == "one_sample":
        m[rng.integers(0, T), rng.integers(0, N)] = True
    elif kind == "one_to_last":
        m[:, rng.integers(0, N)] = True
    return m


def make_record(T, N, mask="monotone", reward="step", seed=0, with_value=True, pad=0, R=5):
    """A record with `pad` unused agent slots per row (filled with values that must never be read into an output)."""
    rng = np.random.default_rng(seed)
    S = N + pad
    rec = {"alive": np.zeros((T, S), np.uint8), "reward": np.full((T, S), 7.5, F32)}
    rec["alive"][:, :N] = make_mask(mask, T, N, rng)
    rec["alive"][:, N:] = 1
    rec["reward"][:, :N] = 1.0 if reward == "step" else (rng.standard_normal((T, N)) * 0.37).astype(F32)
    if with_value:
        rec["value"] = (rng.standard_normal((T, S)) * 3.0 + 1.0).astype(F32)
        rec["last_value"] = (rng.standard_normal(N) * 3.0).astype(F32)
    rec["state"] = rng.random((T, S, R)).astype(F32)
    rec["action"] = rng.integers(0, 3, size=(T, S)).astype(np.int64)
    rec["prob"] = np.log(rng.random((T, S)).astype(F32) * 0.9 + 0.05).astype(F32)
    return rec


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def assert_same(got, want, what=""):
    """Every output both sides carry, bit for bit (statistics included)."""
    for k, w in want.items():
        if k not in got:
            continue
        g = got[k]
        if k == "stats":
            for name, wv in w.items():
                gv = g[name]
                if name == "count":
                    assert int(gv) == int(wv), (what, name, gv, wv)
                else:
                    dt = F32 if name.startswith(("mean", "std")) else F64
                    assert bits(np.array([gv], dt))[0] == bits(np.array([wv], dt))[0], (what, name, gv, wv)
        elif k == "M":
            assert int(g) == int(w), (what, k, g, w)
        else:
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
            assert np.array_equal(bits(g), bits(w)), (what, k)


def normalized_bound(G, M, mean64, std64, sum_abs, sumsq):
    """Bound on |ours - float64| for the normalised values and the two statistics, from the operations the rule performs: the fp64
    accumulation (at most M * 2^-53 * sum|G| on S and M * 2^-53 * Q on Q, taken four times over for the mean's own rounding, the
    product S * mean and the difference), rounding mean and std to fp32, one fp32 subtraction, one fp32 addition of the epsilon and
    one division.  Returns (bound per element, bound on mean, bound on std)."""
    u, u64 = 2.0 ** -24, 2.0 ** -53
    e_mean = 4.0 * u64 * sum_abs + abs(mean64) * u
    if M >= 2 and std64 > 0.0:
        e_ss = 4.0 * M * u64 * sumsq
        e_std = e_ss / ((M - 1) * 2.0 * std64) + std64 * u
    else:
        e_std = 0.0
    den = std64 + float(EPS)
    G = np.asarray(G, F64)
    n64 = (G - mean64) / den
    num_err = e_mean + np.abs(G - mean64) * u
    den_err = e_std + den * u
    bound = 2.0 * (num_err / den + np.abs(n64) * (den_err / den + u))
    return bound, e_mean, e_std
