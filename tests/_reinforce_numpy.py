"""The rule of REINFORCE's network and update (include/okenv_reinforce.h) read again in numpy float32, written from the header's prose
and not from its code.  It shares with the library only ok_expf, ok_logf (through okenv_debug_expf / okenv_debug_logf) and nothing
else: Philox4x32-10 is restated here in Python integers (philox_int; tests/_actor_numpy.py's array form is checked against it and
used where thousands of blocks are wanted), Adam, the chunk sums and the tree are those of tests/_learn_numpy.py, themselves
restatements.  Every fp32 operation is one numpy float32 operation."""
import numpy as np

import _actor_numpy as A_
import _learn_numpy as L_

f32 = np.float32
STREAM = 9
OKEN = 0x6F6B656E


def philox_int(counter, key):
    """Philox4x32-10 on Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> four words."""
    c0, c1, c2, c3 = (int(v) & 0xFFFFFFFF for v in counter)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def kept_int(p, seed, agent, draw, j):
    """Whether hidden unit j of (agent, draw) is kept, in Python integers."""
    word = philox_int((agent, draw, STREAM, (j % 8) + 8 * (j // 32)), (seed, OKEN))[(j // 8) % 4]
    return f32(word >> 8) * f32(2.0 ** -24) >= f32(p)


def mask(p, seed, agents, draws, H):
    """kept [n, H] (bool) for n (global agent id, draw index) pairs; all True for p == 0."""
    agents, draws = np.asarray(agents, dtype=np.uint64), np.asarray(draws, dtype=np.uint64)
    n = agents.shape[0]
    if not p > 0:
        return np.ones((n, H), dtype=bool)
    j = np.arange(H)
    block, word = (j % 8) + 8 * (j // 32), (j // 8) % 4
    blocks = np.arange(int(block.max()) + 1, dtype=np.uint64)
    w = np.stack(A_.philox4x32(agents[:, None] & np.uint64(0xFFFFFFFF), draws[:, None] & np.uint64(0xFFFFFFFF), STREAM, blocks[None, :], seed, OKEN), axis=2)
    return A_.u01(w[:, block, word]) >= f32(p)


def scale(p):
    return f32(1.0) / (f32(1.0) - f32(p))


def forward(params, R, H, A, x, kept, s):
    """x [n, R] -> (z [n, A], pre [n, H], h [n, H]) with the mask `kept` and the scale s on the hidden layer."""
    w1, b1, w2, b2 = L_.split(params, R, H, A)
    n = x.shape[0]
    pre = np.broadcast_to(b1, (n, H)).astype(f32)
    for i in range(R):
        pre = pre + w1[None, :, i] * x[:, i, None]
    v = pre * f32(s)
    h = np.where(kept & (v > 0), v, f32(0)).astype(f32)
    Hp = (H + 7) // 8 * 8
    hp = np.zeros((n, Hp), dtype=f32)
    hp[:, :H] = h
    wp = np.zeros((A, Hp), dtype=f32)
    wp[:, :H] = w2
    part = np.zeros((n, A, 8), dtype=f32)
    for t in range(Hp // 8):
        part = part + wp[None, :, 8 * t:8 * t + 8] * hp[:, None, 8 * t:8 * t + 8]
    tree = ((part[..., 0] + part[..., 4]) + (part[..., 2] + part[..., 6])) + ((part[..., 1] + part[..., 5]) + (part[..., 3] + part[..., 7]))
    return b2[None, :] + tree, pre, h


def act(expf, seed, agent_base, table, policy, value, R, H, A, Hv, dist, draw_index, p, dropout_seed):
    """OKENV_ACTOR_SAMPLE with dropout for n agents; returns dict(action, prob, value, throttle, steer, state, kept)."""
    with np.errstate(all="ignore"):
        dist = np.asarray(dist, dtype=f32)
        n = dist.shape[0]
        x = dist / f32(200.0)
        agents = (np.arange(n, dtype=np.uint64) + np.uint64(agent_base)) & np.uint64(0xFFFFFFFF)
        kept = mask(p, dropout_seed, agents, np.full(n, draw_index, dtype=np.uint64), H)
        z, _, _ = forward(policy, R, H, A, x, kept, scale(p))
        out = {"state": x, "kept": kept}
        if Hv > 0:
            out["value"] = A_.forward(value, R, Hv, 1, x)[:, 0]
        u = A_.u01(A_.philox4x32(agents, np.uint32(draw_index), 6, 0, seed, OKEN)[0])
        _, pc = A_.softmax_clamped(z, expf)
        action = np.full(n, A - 1, dtype=np.int64)
        found = np.zeros(n, dtype=bool)
        cum = pc[:, 0].copy()
        for k in range(A):
            if k > 0:
                cum = cum + pc[:, k]
            hit = ~found & (u < cum)
            action[hit] = k
            found |= hit
        table = np.asarray(table, dtype=f32)
        out.update(action=action, prob=pc[np.arange(n), action].astype(f32), throttle=table[action, 0], steer=table[action, 1])
        return out


def seed_terms(z, action, G, expf, logf):
    """-> (dz [n, A], term [n], q_a clamped [n])."""
    n, A = z.shape
    rows = np.arange(n)
    q, qc = A_.softmax_clamped(z, expf)
    qa = q[rows, action]
    term = -(logf(qc[rows, action].astype(f32)).reshape(n) * G)
    onehot = np.zeros((n, A), dtype=f32)
    onehot[rows, action] = 1
    dz = -(G[:, None] * (onehot - q))
    passes = (qa >= f32(1e-8)) & (qa <= f32(1.0))
    return np.where(passes[:, None], dz, f32(0)).astype(f32), term.astype(f32), qc[rows, action]


def sample_terms(params, R, H, A, x, kept, s, action, G, expf, logf):
    """The per-sample terms of every column [n, P + 1]: the parameters in order, then the loss term; and the recomputed q_a."""
    _, _, w2, _ = L_.split(params, R, H, A)
    n = x.shape[0]
    z, pre, h = forward(params, R, H, A, x, kept, s)
    dz, term, qa = seed_terms(z, action, G, expf, logf)
    dh = w2[None, 0, :] * dz[:, 0, None]
    for k in range(1, A):
        dh = dh + w2[None, k, :] * dz[:, k, None]
    ds = np.where(kept & (pre * f32(s) > 0), dh * f32(s), f32(0)).astype(f32)
    cols = [(ds[:, :, None] * x[:, None, :]).reshape(n, H * R), ds, (dz[:, :, None] * h[:, None, :]).reshape(n, A * H), dz, term[:, None]]
    return np.concatenate(cols, axis=1), qa


def update(expf, logf, hp, shape, state, batch, B, accumulate=True, reduce="sum", p=0.0, dropout_seed=0, agent_base=0, num_agents=0, draw_first=0,
           order=None):
    """The whole rule.  hp = dict(lr, beta1, beta2, eps); state: policy, policy_m, policy_v, t.  Returns (new state, outputs)."""
    R, H, A = shape
    st = {k: (np.array(v, dtype=f32, copy=True) if k != "t" else int(v)) for k, v in state.items() if v is not None}
    t = st.get("t", 0)
    M = batch["ret"].shape[0]
    P = L_.n_params(R, H, A)
    out = {"loss": [], "q": np.zeros(M, dtype=f32)}
    acc = np.zeros(P + 1, dtype=f32)
    s = scale(p) if p > 0 else f32(1)
    with np.errstate(all="ignore"):
        for base in range(0, M, B):
            Bk = min(B, M - base)
            pos = np.arange(base, base + Bk)
            idx = np.clip(order[pos].astype(np.int64), 0, M - 1) if order is not None else pos
            x, G = batch["state"][idx].astype(f32), batch["ret"][idx].astype(f32)
            action = np.clip(batch["action"][idx], 0, A - 1)
            if p > 0:
                flat = np.maximum(batch["index"][idx].astype(np.int64), 0)
                kept = mask(p, dropout_seed, agent_base + flat % num_agents, draw_first + flat // num_agents, H)
            else:
                kept = np.ones((Bk, H), dtype=bool)
            terms, qa = sample_terms(st["policy"], R, H, A, x, kept, s, action, G, expf, logf)
            out["q"][idx] = qa
            sums = L_.rule_sum(terms)
            last = base + Bk == M
            if accumulate:
                acc = acc + sums
                if not last:
                    continue
                total, count = acc, f32(M)
            else:
                total, count = sums, f32(Bk)
            g = total / count if reduce == "mean" else total
            t += 1
            out["loss"].append(g[P])
            out["grad_policy"] = g[:P].copy()
            st["policy"], st["policy_m"], st["policy_v"] = L_.adam(st["policy"], st["policy_m"], st["policy_v"], g[:P], hp, t)
    st["t"] = t
    out["loss"] = np.array(out["loss"], dtype=f32)
    return st, out
