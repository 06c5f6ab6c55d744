"""The rule of PPO's update (include/okenv_learn.h) read again in numpy float32, written from the header's prose and not from its
code.  It shares with the library only ok_expf (through okenv_debug_expf).  Every fp32 operation is one numpy float32 operation on
arrays, so the bits are those of separate IEEE multiplications and additions.  Where the rule leaves terms out (a partial last chunk,
a tree that is not full, hidden units beyond H in the eight interleaved sums) this restatement adds +0.0 instead: a running sum
that starts from +0.0 is never -0.0, and x + 0.0 == x bit for bit."""
import numpy as np

f32 = np.float32
CHUNK = 32


def n_params(R, H, out):
    return H * R + H + out * H + out if H > 0 else 0


def split(params, R, H, A):
    params = np.asarray(params, dtype=f32)
    w1 = params[:H * R].reshape(H, R)
    b1 = params[H * R:H * R + H]
    w2 = params[H * R + H:H * R + H + A * H].reshape(A, H)
    b2 = params[H * R + H + A * H:]
    assert b2.size == A
    return w1, b1, w2, b2


def forward(params, R, H, A, x):
    """x [n, R] -> (z [n, A], s [n, H] the hidden pre-activations, h [n, H])."""
    w1, b1, w2, b2 = split(params, R, H, A)
    n = x.shape[0]
    s = np.broadcast_to(b1, (n, H)).astype(f32)
    for i in range(R):
        s = s + w1[None, :, i] * x[:, i, None]
    h = np.where(s > 0, s, f32(0))
    Hp = (H + 7) // 8 * 8
    hp = np.zeros((n, Hp), dtype=f32)
    hp[:, :H] = h
    wp = np.zeros((A, Hp), dtype=f32)
    wp[:, :H] = w2
    part = np.zeros((n, A, 8), dtype=f32)
    for t in range(Hp // 8):
        part = part + wp[None, :, 8 * t:8 * t + 8] * hp[:, None, 8 * t:8 * t + 8]
    tree = ((part[..., 0] + part[..., 4]) + (part[..., 2] + part[..., 6])) + ((part[..., 1] + part[..., 5]) + (part[..., 3] + part[..., 7]))
    return b2[None, :] + tree, s, h


def backward_terms(params, R, H, A, x, s, h, dz):
    """The per-sample terms of every parameter, [n, P] in parameter order."""
    _, _, w2, _ = split(params, R, H, A)
    n = x.shape[0]
    dh = w2[None, 0, :] * dz[:, 0, None]
    for k in range(1, A):
        dh = dh + w2[None, k, :] * dz[:, k, None]
    ds = np.where(s > 0, dh, f32(0))
    return np.concatenate([(ds[:, :, None] * x[:, None, :]).reshape(n, H * R), ds, (dz[:, :, None] * h[:, None, :]).reshape(n, A * H), dz], axis=1)


def tree(x):
    """The fixed tree over axis 0."""
    n = x.shape[0]
    w = 1
    while w < n:
        w *= 2
    y = np.zeros((w,) + x.shape[1:], dtype=f32)
    y[:n] = x
    hlf = w // 2
    while hlf >= 1:
        y[:hlf] = y[:hlf] + y[hlf:2 * hlf]
        hlf //= 2
    return y[0]


def rule_sum(terms):
    """[n, P] per-position terms -> [P]: ascending sums inside chunks of 32 positions from +0.0, then the tree over the chunks."""
    n = terms.shape[0]
    C = (n + CHUNK - 1) // CHUNK
    padded = np.zeros((C * CHUNK,) + terms.shape[1:], dtype=f32)
    padded[:n] = terms
    padded = padded.reshape((C, CHUNK) + terms.shape[1:])
    acc = np.zeros((C,) + terms.shape[1:], dtype=f32)
    for q in range(min(CHUNK, n)):
        acc = acc + padded[:, q]
    return tree(acc)


def rule_mean(values):
    """The rule's mean of per-position values [n]."""
    return rule_sum(np.asarray(values, dtype=f32)[:, None])[0] / f32(len(values))


def powi(b, t):
    r = 1.0
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def factors(lr, beta1, beta2, t):
    """(step, bc2) of step number t: fp64 from the fp32 constants, powers by repeated squaring, each rounded once."""
    lr, beta1, beta2 = float(f32(lr)), float(f32(beta1)), float(f32(beta2))
    return f32(lr / (1.0 - powi(beta1, t))), f32(np.sqrt(1.0 - powi(beta2, t)))


def adam(p, m, v, g, hp, t):
    """One step on arrays; hp = dict(lr, beta1, beta2, eps).  Returns (p, m, v)."""
    b1, b2, eps = f32(hp["beta1"]), f32(hp["beta2"]), f32(hp["eps"])
    omb1, omb2 = f32(1.0 - float(b1)), f32(1.0 - float(b2))
    step, bc2 = factors(hp["lr"], hp["beta1"], hp["beta2"], t)
    m = b1 * m + omb1 * g
    v = b2 * v + (omb2 * g) * g
    den = np.sqrt(v) / bc2 + eps
    return p - step * (m / den), m, v


def policy_seed(z, action, p_old, adv, lo, hi, expf):
    """-> (dz [n, A], surr [n], clipped [n])."""
    n, A = z.shape
    rows = np.arange(n)
    m = z.max(axis=1, keepdims=True)
    e = expf((z - m).astype(f32)).reshape(z.shape)
    s = e[:, 0].copy()
    for k in range(1, A):
        s = s + e[:, k]
    y = (e / s[:, None]).astype(f32)
    ya = y[rows, action]
    p_new = np.minimum(np.maximum(ya, f32(1e-8)), f32(1.0))
    r = p_new / p_old
    rc = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(f32)
    s1, s2 = r * adv, rc * adv
    surr = np.where(s1 < s2, s1, s2)
    clipped = (r < lo) | (r > hi)
    w1 = np.where(s1 < s2, f32(1), np.where(s2 < s1, f32(0), f32(0.5))).astype(f32)
    w2 = f32(1) - w1
    g_r = w1 * adv + w2 * np.where((r >= lo) & (r <= hi), adv, f32(0))
    g_p = np.where((ya >= f32(1e-8)) & (ya <= f32(1.0)), -g_r / p_old, f32(0)).astype(f32)
    t = g_p * ya
    onehot = np.zeros((n, A), dtype=f32)
    onehot[rows, action] = 1
    return t[:, None] * (onehot - y), surr.astype(f32), clipped


def update(expf, hp, shape, state, batch, B, epochs=1, order=None):
    """The whole rule.  hp = dict(lr, clip, beta1, beta2, eps); state as env.ppo_update_host takes it.  Returns (new state, outputs)."""
    R, H, A, Hv = shape
    st = {k: (np.array(v, dtype=f32, copy=True) if k != "t" else int(v)) for k, v in state.items() if v is not None}
    t = st.get("t", 0)
    M = batch["ret"].shape[0]
    lo, hi = f32(1.0 - float(f32(hp["clip"]))), f32(1.0 + float(f32(hp["clip"])))
    out = {"actor_loss": [], "critic_loss": [], "clipped": []}
    with np.errstate(all="ignore"):
        for e in range(epochs):
            for base in range(0, M, B):
                Bk = min(B, M - base)
                pos = np.arange(base, base + Bk)
                idx = np.clip(order[e][pos].astype(np.int64), 0, M - 1) if order is not None else pos
                x, ret, p_old = batch["state"][idx].astype(f32), batch["ret"][idx].astype(f32), batch["prob"][idx].astype(f32)
                action = np.clip(batch["action"][idx], 0, A - 1)
                adv = batch["adv"][idx].astype(f32) if batch.get("adv") is not None else None
                bk = f32(Bk)
                t += 1
                if Hv > 0:
                    zv, sv, hv = forward(st["value"], R, Hv, 1, x)
                    err = zv[:, 0] - ret
                    if adv is None:
                        adv = ret - zv[:, 0]
                    gv = rule_sum(backward_terms(st["value"], R, Hv, 1, x, sv, hv, (f32(2) * err)[:, None])) / bk
                    out["critic_loss"].append(rule_sum((err * err)[:, None])[0] / bk)
                    out["grad_value"] = gv
                else:
                    out["critic_loss"].append(f32(0))
                z, s, h = forward(st["policy"], R, H, A, x)
                dz, surr, clipped = policy_seed(z, action, p_old, adv, lo, hi, expf)
                gp = rule_sum(backward_terms(st["policy"], R, H, A, x, s, h, dz)) / bk
                out["actor_loss"].append(-(rule_sum(surr[:, None])[0] / bk))
                out["clipped"].append(int(clipped.sum()))
                out["grad_policy"] = gp
                st["policy"], st["policy_m"], st["policy_v"] = adam(st["policy"], st["policy_m"], st["policy_v"], gp, hp, t)
                if Hv > 0:
                    st["value"], st["value_m"], st["value_v"] = adam(st["value"], st["value_m"], st["value_v"], gv, hp, t)
    st["t"] = t
    out["actor_loss"] = np.array(out["actor_loss"], dtype=f32)
    out["critic_loss"] = np.array(out["critic_loss"], dtype=f32)
    out["clipped"] = np.array(out["clipped"], dtype=np.int32)
    return st, out
