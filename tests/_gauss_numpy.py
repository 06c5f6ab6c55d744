"""An independent numpy-float32 restatement of include/okenv_gauss.h for tests/test_gauss_rule.py and
tests/test_gpu_gauss.py: the normal draw, the two-hidden-layer forward and backward, the sample, the two gradient modes, the chunked
sums, slices, accumulate / reduce and Adam.  Philox is written in integers here; only ok_expf, ok_logf, ok_tanhf and ok_sincosf are the
library's, through its debug entries on the host."""
import math

import numpy as np

from openkitchen_amd import _capi as capi
from openkitchen_amd import env

f32 = np.float32
HOST = capi.DEBUG_ON_HOST
CHUNK, LANES, STREAM = 32, 8, 10
KEY1 = 0x6F6B656E
MASK = np.uint64(0xFFFFFFFF)


def _leaf(fn, x):
    x = np.asarray(x, dtype=f32)
    return env.debug_math(fn, np.ascontiguousarray(x).ravel(), device=HOST).reshape(x.shape)


def expf(x):
    return _leaf("exp", x)


def logf(x):
    return _leaf("log", x)


def tanhf(x):
    return _leaf("tanh", x)


def sincosf(x):
    x = np.asarray(x, dtype=f32)
    s, c = env.debug_math("sincos", np.ascontiguousarray(x).ravel(), device=HOST)
    return s.reshape(x.shape), c.reshape(x.shape)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on integer arrays (uint64 holding 32-bit words): the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u01(w):
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)


def normal_pair(w0, w1):
    """Box-Muller on two words: (r cos, r sin)."""
    u1 = f32(1.0) - u01(w0)
    r = np.sqrt((f32(-2.0) * logf(u1)).astype(np.float64)).astype(f32)
    s, c = sincosf(f32(6.2831855) * u01(w1))
    return r * c, r * s


def draw_eps(seed, agents, draw, A=2):
    """eps [n, A] of the global agent ids `agents` at draw index `draw`."""
    agents = np.asarray(agents, dtype=np.uint64)
    out = np.zeros((agents.size, A), dtype=f32)
    for b in range((A + 1) // 2):
        w = philox4x32(agents, int(draw) & 0xFFFFFFFF, STREAM, b, seed, KEY1)
        e0, e1 = normal_pair(w[0], w[1])
        out[:, 2 * b] = e0
        if 2 * b + 1 < A:
            out[:, 2 * b + 1] = e1
    return out


def num_params(R, H1, H2, A=2):
    return A + H1 * R + H1 + H2 * H1 + H2 + A * H2 + A


def split(par, R, H1, H2, A=2):
    """(log_std, W1, b1, W2, b2, W3, b3) as views of the parameter vector."""
    par = np.asarray(par, dtype=f32)
    sizes = [A, H1 * R, H1, H2 * H1, H2, A * H2, A]
    shapes = [(A,), (H1, R), (H1,), (H2, H1), (H2,), (A, H2), (A,)]
    out, at = [], 0
    for n, shp in zip(sizes, shapes):
        out.append(par[at:at + n].reshape(shp))
        at += n
    assert at == par.size
    return out


def _tree8(p):
    return ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]))


def _layer(W, b, h):
    """The output-layer rule: 8 interleaved partial sums over the inputs, the tree, then the bias.  W [out, n], h [M, n]."""
    M, n = h.shape
    parts = []
    for l in range(LANES):
        p = np.zeros((M, W.shape[0]), dtype=f32)
        for i in range(l, n, LANES):
            p = p + W[None, :, i] * h[:, i, None]
        parts.append(p)
    return b[None, :] + _tree8(parts)


def forward(par, shape, x):
    R, H1, H2, A = shape
    _, W1, b1, W2, b2, W3, b3 = split(par, R, H1, H2, A)
    x = np.asarray(x, dtype=f32)
    s = np.repeat(b1[None, :], x.shape[0], axis=0)
    for i in range(R):
        s = s + W1[None, :, i] * x[:, i, None]
    h1 = np.where(s > 0, s, f32(0))
    s2 = _layer(W2, b2, h1)
    h2 = np.where(s2 > 0, s2, f32(0))
    return h1, h2, _layer(W3, b3, h2)


def sample(mu, log_std, eps=None, pre=None, greedy=False):
    """The components of the sample: dict of std, se, pre, t, u, z, logp.  eps given: pre = mu + std * eps, z = eps; pre given:
    z = (pre - mu) / std; greedy: pre = mu, z = 0."""
    std = expf(log_std)[None, :]
    ls = np.asarray(log_std, dtype=f32)[None, :]
    if pre is not None:
        se = np.zeros_like(mu)
        pre = np.asarray(pre, dtype=f32)
        z = (pre - mu) / std
    elif greedy:
        se, pre, z = np.zeros_like(mu), mu, np.zeros_like(mu)
    else:
        eps = np.asarray(eps, dtype=f32)
        se = std * eps
        pre = mu + se
        z = eps
    t = tanhf(pre)
    u = f32(1.0) - t * t
    n = ((f32(-0.5) * z) * z - ls) - f32(0.9189385)
    l = logf(u + f32(1e-6))
    sn, sl = n[:, 0], l[:, 0]
    for k in range(1, mu.shape[1]):
        sn, sl = sn + n[:, k], sl + l[:, k]
    return {"std": std, "se": se, "pre": pre, "t": t, "u": u, "z": z, "logp": sn - sl}


def act(par, shape, dist, seed=0, agent_base=0, draw=0, greedy=False, scale=(50.0, 10.0), bias=(50.0, 0.0)):
    R, H1, H2, A = shape
    dist = np.asarray(dist, dtype=f32)
    x = dist / f32(200.0)
    mu = forward(par, shape, x)[2]
    ls = split(par, R, H1, H2, A)[0]
    eps = None if greedy else draw_eps(seed, (np.arange(dist.shape[0], dtype=np.uint64) + np.uint64(agent_base)) & MASK, draw, A)
    s = sample(mu, ls, eps=eps, greedy=greedy)
    action = s["t"] * np.asarray(scale, dtype=f32)[None, :] + np.asarray(bias, dtype=f32)[None, :]
    return {"state": x, "eps": eps, "pre": s["pre"], "action": action, "logp": s["logp"], "throttle": action[:, 0], "steer": action[:, 1]}


def sample_grads(par, shape, x, eps, pre, G, mode):
    """Per-sample gradient rows [n, P] (the terms of every parameter) and loss terms [n] at the parameters `par`."""
    R, H1, H2, A = shape
    ls, W1, b1, W2, b2, W3, b3 = split(par, R, H1, H2, A)
    h1, h2, mu = forward(par, shape, x)
    G = np.asarray(G, dtype=f32)[:, None]
    if mode == capi.GAUSS_GRAD_SCORE:
        s = sample(mu, ls, pre=pre)
        dz = -(G * (s["z"] / s["std"]))
        dls = -(G * (s["z"] * s["z"] - f32(1.0)))
    else:
        s = sample(mu, ls, eps=eps)
        c = ((f32(2.0) * s["t"]) * s["u"]) / (s["u"] + f32(1e-6))
        dz = -(G * c)
        dls = -(G * (c * s["se"] - f32(1.0)))
    term = -(s["logp"] * G[:, 0])
    dh2 = W3[0][None, :] * dz[:, 0, None]
    for k in range(1, A):
        dh2 = dh2 + W3[k][None, :] * dz[:, k, None]
    d2 = np.where(h2 > 0, dh2, f32(0))
    parts = []
    for l in range(LANES):
        p = np.zeros_like(h1)
        for j in range(l, H2, LANES):
            p = p + W2[j][None, :] * d2[:, j, None]
        parts.append(p)
    d1 = np.where(h1 > 0, _tree8(parts), f32(0))
    n = x.shape[0]
    x = np.asarray(x, dtype=f32)
    rows = np.concatenate([dls, (d1[:, :, None] * x[:, None, :]).reshape(n, -1), d1, (d2[:, :, None] * h1[:, None, :]).reshape(n, -1), d2,
                           (dz[:, :, None] * h2[:, None, :]).reshape(n, -1), dz], axis=1)
    return rows, term, s["logp"]


def tree(parts):
    """ok_learn_tree over the rows of parts [C, cols]."""
    x = np.array(parts, dtype=f32, copy=True)
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


def _powi(b, t):
    r = 1.0
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def adam(p, m, v, g, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    lr, beta1, beta2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    omb1, omb2 = f32(1.0 - float(beta1)), f32(1.0 - float(beta2))
    step = f32(float(lr) / (1.0 - _powi(float(beta1), t)))
    bc2 = f32(math.sqrt(1.0 - _powi(float(beta2), t)))
    mn = beta1 * m + omb1 * g
    vn = beta2 * v + (omb2 * g) * g
    root = np.sqrt(vn.astype(np.float64)).astype(f32)
    den = root / bc2 + eps
    return p - step * (mn / den), mn, vn


def update(state, shape, batch, B, accumulate=True, reduce="sum", mode=0, order=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The whole update: returns (new state, {"loss": one per optimiser step, "grad": the last step's, "logp": per position of the
    first slice})."""
    R, H1, H2, A = shape
    P = num_params(R, H1, H2, A)
    par, m, v = (np.array(state[k], dtype=f32, copy=True) for k in ("params", "m", "v"))
    t = int(state.get("t", 0))
    M = int(np.asarray(batch["ret"]).shape[0])
    acc = np.zeros(P + 1, dtype=f32)
    losses, grad, first_logp = [], None, None
    slices = (M + B - 1) // B
    for k in range(slices):
        base, Bk = k * B, min(B, M - k * B)
        pos = np.arange(base, base + Bk)
        idx = np.clip(np.asarray(order, dtype=np.int64)[pos], 0, M - 1) if order is not None else pos
        parts = []
        logps = []
        for c0 in range(0, Bk, CHUNK):
            ii = idx[c0:c0 + CHUNK]
            rows, term, logp = sample_grads(par, shape, np.asarray(batch["state"], dtype=f32)[ii],
                                            None if batch.get("eps") is None else np.asarray(batch["eps"], dtype=f32)[ii],
                                            None if batch.get("pre") is None else np.asarray(batch["pre"], dtype=f32)[ii],
                                            np.asarray(batch["ret"], dtype=f32)[ii], mode)
            col = np.zeros(P + 1, dtype=f32)
            for q in range(len(ii)):
                col[:P] = col[:P] + rows[q]
                col[P] = col[P] + term[q]
            parts.append(col)
            logps.append(logp)
        if first_logp is None:
            first_logp = np.concatenate(logps)
        s = tree(np.stack(parts))
        step = (not accumulate) or k + 1 == slices
        if not step:
            acc = acc + s
            continue
        total = acc + s if accumulate else s
        count = f32(M if accumulate else Bk)
        g = total / count if reduce in ("mean", capi.REINFORCE_MEAN) else total
        t += 1
        grad = g[:P].copy()
        losses.append(g[P])
        par, m, v = adam(par, m, v, grad, t, lr, beta1, beta2, eps)
    return {"params": par, "m": m, "v": v, "t": t}, {"loss": np.array(losses, dtype=f32), "grad": grad, "logp": first_logp}


def word_pairs():
    """2^16 random word pairs and the edges: w0 = 0 (u1 = 1, r = 0) and 0xFFFFFFFF (the largest r), w1 at the quadrant boundaries."""
    rng = np.random.default_rng(20)
    w0 = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    w1 = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    quad = [q * (1 << 30) + d for q in range(4) for d in (-256, -1, 0, 1, 255, 256)] + [0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFEFF]
    e0, e1 = np.meshgrid(np.array([0, 1, 255, 256, 0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFEFF, 0x80000000], dtype=np.uint64),
                         np.array([q & 0xFFFFFFFF for q in quad], dtype=np.uint64))
    return np.concatenate([w0, e0.ravel()]).astype(np.uint32), np.concatenate([w1, e1.ravel()]).astype(np.uint32)
