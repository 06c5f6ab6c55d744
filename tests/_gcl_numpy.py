"""An independent numpy-float32 restatement of include/okenv_gcl.h for tests/test_gcl_rule.py and
tests/test_gpu_gcl.py: the state, the three networks' forward and backward, acting, the cost seed and its two-set update, the
advantages, the clipped-ratio seed, the chunked sums, slices, accumulate / reduce and Adam.  Philox, the layers' sums, the tree and Adam
are tests/_gauss_numpy.py's (numpy too); only ok_expf, ok_logf, ok_tanhf and ok_sincosf are the library's, through its debug entries on
the host."""
import numpy as np

import _gauss_numpy as G_

f32 = np.float32
CHUNK, LANES = G_.CHUNK, G_.LANES
ACT_STREAM, EXPERT_STREAM = 11, 12
POLICY, VALUE, COST = "policy", "value", "cost"
expf, logf, tanhf = G_.expf, G_.logf, G_.tanhf


def state_of(rel_xy):
    """x = (rel_x^2 + rel_y^2) / 40000 of rel_xy [..., 2]."""
    rel_xy = np.asarray(rel_xy, dtype=f32)
    xx, yy = rel_xy[..., 0] * rel_xy[..., 0], rel_xy[..., 1] * rel_xy[..., 1]
    return (xx + yy) / f32(40000.0)


def dims(which, R):
    """(inputs, outputs, floats of log_std) of a network."""
    return (R + 2 if which == COST else R), (2 if which == POLICY else 1), (2 if which == POLICY else 0)


def num_params(which, R, H1, H2):
    n_in, out, nls = dims(which, R)
    return nls + H1 * n_in + H1 + H2 * H1 + H2 + out * H2 + out


def split(par, which, R, H1, H2):
    """(log_std, W1, b1, W2, b2, W3, b3) as views of the parameter vector; log_std is empty for the value and the cost network."""
    n_in, out, nls = dims(which, R)
    par = np.asarray(par, dtype=f32)
    sizes = [nls, H1 * n_in, H1, H2 * H1, H2, out * H2, out]
    shapes = [(nls,), (H1, n_in), (H1,), (H2, H1), (H2,), (out, H2), (out,)]
    pieces, at = [], 0
    for n, shp in zip(sizes, shapes):
        pieces.append(par[at:at + n].reshape(shp))
        at += n
    assert at == par.size
    return pieces


def _act_fn(which, s):
    return tanhf(s) if which == COST else np.where(s > 0, s, f32(0))


def forward(par, which, shape, x):
    """h1, h2 and the third layer's outputs z3 [M, out] for the input rows x [M, in]."""
    R, H1, H2 = shape
    _, W1, b1, W2, b2, W3, b3 = split(par, which, R, H1, H2)
    x = np.asarray(x, dtype=f32)
    s = np.repeat(b1[None, :], x.shape[0], axis=0)
    for i in range(x.shape[1]):
        s = s + W1[None, :, i] * x[:, i, None]
    h1 = _act_fn(which, s)
    h2 = _act_fn(which, G_._layer(W2, b2, h1))
    return h1, h2, G_._layer(W3, b3, h2)


def draw_eps(seed, agents, draw):
    w = G_.philox4x32(np.asarray(agents, dtype=np.uint64), int(draw) & 0xFFFFFFFF, ACT_STREAM, 0, seed, G_.KEY1)
    e0, e1 = G_.normal_pair(w[0], w[1])
    return np.stack([e0, e1], axis=1)


def normal_term(z, ls):
    return ((f32(-0.5) * z) * z - ls) - f32(0.9189385)


def act(par, shape, rel_xy, seed=0, agent_base=0, draw=0, greedy=False, scale=(50.0, 10.0), bias=(50.0, 0.0)):
    R, H1, H2 = shape
    x = state_of(rel_xy)
    n = x.shape[0]
    mu = tanhf(forward(par, POLICY, shape, x)[2])
    ls = split(par, POLICY, R, H1, H2)[0][None, :]
    if greedy:
        eps, pre, z = None, mu, np.zeros_like(mu)
    else:
        eps = draw_eps(seed, (np.arange(n, dtype=np.uint64) + np.uint64(agent_base)) & G_.MASK, draw)
        std = expf(ls)
        pre = mu + std * eps
        z = (pre - mu) / std
    sq = tanhf(pre)
    action = sq * np.asarray(scale, dtype=f32)[None, :] + np.asarray(bias, dtype=f32)[None, :]
    nn = normal_term(z, ls)
    return {"state": x, "eps": eps, "pre": pre, "squashed": sq, "action": action, "logp": nn[:, 0] + nn[:, 1], "throttle": action[:, 0],
            "steer": action[:, 1]}


def cost(par, shape, state, squashed):
    """The cost network's logit of the rows [state | squashed]; shape: (R, C1, C2)."""
    x = np.concatenate([np.asarray(state, dtype=f32), np.asarray(squashed, dtype=f32)], axis=1)
    return forward(par, COST, shape, x)[2][:, 0]


def expert_rows(seed, positions, d, E):
    w = G_.philox4x32(np.asarray(positions, dtype=np.uint64), int(d) & 0xFFFFFFFF, EXPERT_STREAM, 0, seed, G_.KEY1)[0]
    return ((w * np.uint64(E)) >> np.uint64(32)).astype(np.int64)


def cost_seed(c, policy):
    """(term, seed) of cost rows with logits c; policy: label 1, else label 0."""
    c = np.asarray(c, dtype=f32)
    e = expf(-np.abs(c))
    ope = f32(1.0) + e
    l = logf(ope)
    sig = np.where(c >= 0, f32(1.0) / ope, e / ope)
    if policy:
        return np.where(c < 0, -c, f32(0)) + l, sig - f32(1.0)
    return np.where(c > 0, c, f32(0)) + l, sig


def ratio_seed(logp, logp_old, adv, lo, hi):
    """(surr, clipped, g = d loss / d logp, r) of samples."""
    r = expf(logp - logp_old)
    rc = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(f32)
    s1, s2 = r * adv, rc * adv
    surr = np.where(s1 < s2, s1, s2)
    w1 = np.where(s1 < s2, f32(1), np.where(s2 < s1, f32(0), f32(0.5))).astype(f32)
    w2 = f32(1.0) - w1
    in_range = np.where((r >= lo) & (r <= hi), adv, f32(0)).astype(f32)
    g_r = w1 * adv + w2 * in_range
    return surr, ((r < lo) | (r > hi)).astype(np.int64), (-g_r) * r, r


def backward_rows(par, which, shape, x, h1, h2, dz, dls):
    """Per-sample gradient rows [n, P] from the output seeds dz [n, out] (and dls [n, 2] for the policy)."""
    R, H1, H2 = shape
    _, W1, b1, W2, b2, W3, b3 = split(par, which, R, H1, H2)
    out = W3.shape[0]
    dh2 = W3[0][None, :] * dz[:, 0, None]
    for k in range(1, out):
        dh2 = dh2 + W3[k][None, :] * dz[:, k, None]
    gate = (lambda dh, h: dh * (f32(1.0) - h * h)) if which == COST else (lambda dh, h: np.where(h > 0, dh, f32(0)))
    d2 = gate(dh2, h2)
    parts = []
    for l in range(LANES):
        p = np.zeros_like(h1)
        for j in range(l, H2, LANES):
            p = p + W2[j][None, :] * d2[:, j, None]
        parts.append(p)
    d1 = gate(G_._tree8(parts), h1)
    n = x.shape[0]
    pieces = [(d1[:, :, None] * x[:, None, :]).reshape(n, -1), d1, (d2[:, :, None] * h1[:, None, :]).reshape(n, -1), d2,
              (dz[:, :, None] * h2[:, None, :]).reshape(n, -1), dz]
    if which == POLICY:
        pieces.insert(0, dls)
    return np.concatenate(pieces, axis=1).astype(f32)


def chunk_columns(rows, terms):
    """[C, P + 1]: every chunk's sums, ascending within the chunk."""
    n, P = rows.shape
    cols = []
    for c0 in range(0, n, CHUNK):
        col = np.zeros(P + 1, dtype=f32)
        for q in range(c0, min(n, c0 + CHUNK)):
            col[:P] = col[:P] + rows[q]
            col[P] = col[P] + terms[q]
        cols.append(col)
    return np.stack(cols)


def cost_rows(par, shape, x, policy):
    h1, h2, z3 = forward(par, COST, shape, x)
    term, seed = cost_seed(z3[:, 0], policy)
    return backward_rows(par, COST, shape, x, h1, h2, seed[:, None].astype(f32), None), term.astype(f32), z3[:, 0]


def cost_update(state, shape, bank, batch, Me, seed=0, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step of the cost network: returns (new state, {"loss", "grad", "rows": the bank rows drawn, "logits": (expert, policy)})."""
    par, m, v = (np.array(state[k], dtype=f32, copy=True) for k in ("params", "m", "v"))
    t = int(state.get("t", 0))
    E = np.asarray(bank["state"]).shape[0]
    rows = expert_rows(seed, np.arange(Me), t, E)
    xe = np.concatenate([np.asarray(bank["state"], dtype=f32)[rows], np.asarray(bank["action"], dtype=f32)[rows]], axis=1)
    xp = np.concatenate([np.asarray(batch["state"], dtype=f32), np.asarray(batch["squashed"], dtype=f32)], axis=1)
    Mp = xp.shape[0]
    re, te, ce = cost_rows(par, shape, xe, False)
    rp, tp, cp = cost_rows(par, shape, xp, True)
    g = G_.tree(chunk_columns(re, te)) / f32(Me) + G_.tree(chunk_columns(rp, tp)) / f32(Mp)
    t += 1
    grad = g[:-1].copy()
    par, m, v = G_.adam(par, m, v, grad, t, lr, beta1, beta2, eps)
    return {"params": par, "m": m, "v": v, "t": t}, {"loss": g[-1:].copy(), "grad": grad, "rows": rows, "logits": (ce, cp)}


def tree64(x):
    """ok_batch_tree over the float64 vector x."""
    x = np.array(x, dtype=np.float64, copy=True)
    n = x.shape[0]
    w = 1
    while w < n:
        w <<= 1
    h = w >> 1
    while h >= 1:
        cnt = max(0, min(h, n - h))
        if cnt:
            x[:cnt] = x[:cnt] + x[h:h + cnt]
        h >>= 1
    return x[0]


def advantages(value_par, shape, states, ret):
    """(adv, raw, mean, std): the value sweep, section 15's statistics over chunks of 32 sample indices, the normalisation."""
    v = forward(value_par, VALUE, shape, states)[2][:, 0]
    raw = (np.asarray(ret, dtype=f32) - v).astype(f32)
    M = raw.size
    S, Q = [], []
    for c0 in range(0, M, CHUNK):
        s = q = np.float64(0.0)
        for r in raw[c0:c0 + CHUNK].astype(np.float64):
            s = s + r
            q = q + r * r
        S.append(s)
        Q.append(q)
    s, q = tree64(S), tree64(Q)
    mean = s / M
    sd = np.sqrt(max(q - s * mean, 0.0) / (M - 1)) if M >= 2 else 0.0
    mean, sd = f32(mean), f32(sd)
    return ((raw - mean) / (sd + f32(1e-8))).astype(f32), raw, mean, sd


def logp_of(par, shape, x, pre):
    """The log-probability of the recorded pre under the policy `par`."""
    R, H1, H2 = shape
    mu = tanhf(forward(par, POLICY, shape, x)[2])
    ls = split(par, POLICY, R, H1, H2)[0][None, :]
    nn = normal_term((np.asarray(pre, dtype=f32) - mu) / expf(ls), ls)
    return nn[:, 0] + nn[:, 1]


def policy_rows(par, shape, x, pre, logp_old, adv, lo, hi):
    R, H1, H2 = shape
    h1, h2, z3 = forward(par, POLICY, shape, x)
    mu = tanhf(z3)
    ls = split(par, POLICY, R, H1, H2)[0][None, :]
    std = expf(ls)
    z = (np.asarray(pre, dtype=f32) - mu) / std
    nn = normal_term(z, ls)
    logp = nn[:, 0] + nn[:, 1]
    surr, clipped, g, r = ratio_seed(logp, np.asarray(logp_old, dtype=f32), np.asarray(adv, dtype=f32), lo, hi)
    dmu = g[:, None] * (z / std)
    dls = g[:, None] * (z * z - f32(1.0))
    dz = dmu * (f32(1.0) - mu * mu)
    return backward_rows(par, POLICY, shape, x, h1, h2, dz.astype(f32), dls.astype(f32)), (-surr).astype(f32), clipped, logp, r


def value_rows(par, shape, x, ret):
    h1, h2, z3 = forward(par, VALUE, shape, x)
    e = z3[:, 0] - np.asarray(ret, dtype=f32)
    return backward_rows(par, VALUE, shape, x, h1, h2, (f32(2.0) * e)[:, None].astype(f32), None), (e * e).astype(f32)


def _slices(state, M, B, accumulate, reduce, order, hp, rows_of):
    """The slice loop for one network: rows_of(par, idx) -> (rows, terms, clipped or None).  Returns (state, losses, grad, clips)."""
    par, m, v = (np.array(state[k], dtype=f32, copy=True) for k in ("params", "m", "v"))
    t = int(state.get("t", 0))
    P = par.size
    acc = np.zeros(P + 1, dtype=f32)
    losses, clips, grad, pending = [], [], None, 0
    n_slices = (M + B - 1) // B
    for k in range(n_slices):
        base, Bk = k * B, min(B, M - k * B)
        pos = np.arange(base, base + Bk)
        idx = np.clip(np.asarray(order, dtype=np.int64)[pos], 0, M - 1) if order is not None else pos
        rows, terms, clipped = rows_of(par, idx)
        pending += 0 if clipped is None else int(clipped.sum())
        s = G_.tree(chunk_columns(rows, terms))
        step = (not accumulate) or k + 1 == n_slices
        if not step:
            acc = acc + s
            continue
        total = acc + s if accumulate else s
        count = f32(M if accumulate else Bk)
        g = total / count if reduce == "mean" else total
        t += 1
        grad = g[:P].copy()
        losses.append(g[P])
        clips.append(pending)
        pending = 0
        par, m, v = G_.adam(par, m, v, grad, t, **hp)
    return {"params": par, "m": m, "v": v, "t": t}, np.array(losses, dtype=f32), grad, np.array(clips, dtype=np.int32)


def policy_update(policy, value, shape, batch, B, accumulate=True, reduce="mean", order=None, clip=0.2, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """The whole policy / value update: returns (new policy state, new value state, outputs) with the outputs of the host entry plus
    "r": the first slice's ratios at the parameters the call starts with."""
    hp = dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps)
    lo, hi = f32(1.0 - float(f32(clip))), f32(1.0 + float(f32(clip)))
    states, pre, logp_old, ret = (np.asarray(batch[k], dtype=f32) for k in ("state", "pre", "logp", "ret"))
    M = ret.size
    adv = advantages(value["params"], shape, states, ret)[0]
    first = {}

    def pol_rows(par, idx):
        rows, terms, clipped, logp, r = policy_rows(par, shape, states[idx], pre[idx], logp_old[idx], adv[idx], lo, hi)
        first.setdefault("r", r)
        first.setdefault("logp", logp)
        return rows, terms, clipped

    def val_rows(par, idx):
        rows, terms = value_rows(par, shape, states[idx], ret[idx])
        return rows, terms, None

    t0 = int(policy.get("t", 0))
    newp, pl, gp, clips = _slices(dict(policy, t=t0), M, B, accumulate, reduce, order, hp, pol_rows)
    newv, vl, gv, _ = _slices(dict(value, t=t0), M, B, accumulate, reduce, order, hp, val_rows)
    return newp, newv, {"policy_loss": pl, "value_loss": vl, "clipped": clips, "grad_policy": gp, "grad_value": gv, "adv": adv, "r": first["r"],
                        "logp": first["logp"]}
