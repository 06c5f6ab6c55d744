"""The rule of the image transformer driver's head update (include/okenv_vithead.h) restated in numpy, bit for bit: every float32
operation of the rule as one numpy float32 operation, the fused chains through fma() below, sequential where the rule is sequential
(over k in a dot, over the positions of a chunk, over the chunks) and vectorised over everything the rule leaves independent.
Behind it the float64 error bounds of the comparison with autograd (tests/test_gcl_rule.py's _mlp_bounds / _grad_bounds, restated)."""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
CHUNK = 64
# (D, H1, H2): the smallest; a partial 64-column block; the reference; H2 > H1: a d1 chain longer than its row and more column tiles in
# layer 3 than in layer 2; the widest layer the LDS takes: 8 strides of the forward kernel's row loops, 387 gradient units; the widest
# embedding: 49 column tiles of layer 1.  ((16, 16, 2048) needs 265 KB of LDS and is refused.)
SHAPES = [(16, 16, 16), (48, 32, 16), (384, 128, 64), (32, 16, 48), (16, 2048, 16), (768, 16, 16)]
LDS_BUDGET = 160 * 1024


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def num_params(D, H1, H2):
    return H1 * D + H1 + H2 * H1 + H2 + H2 + 1


def lds_bytes(D, H1, H2):
    """okVitHeadLdsBytes restated: [e | h1 | h2 | d2] of 16 positions, rows padded by 4 floats, and the 16 output seeds."""
    if any(v < 16 or v % 16 for v in (D, H1, H2)) or D > 768 or H1 > 2048 or H2 > 2048:
        return 0
    return 4 * (16 * (D + 4 + H1 + 4 + 2 * (H2 + 4)) + 16)


def split(head, D, H1, H2):
    head = np.asarray(head)
    at, out = 0, []
    for shape in ((H1, D), (H1,), (H2, H1), (H2,), (1, H2), (1,)):
        n = int(np.prod(shape))
        out.append(head[at:at + n].reshape(shape))
        at += n
    assert at == head.size
    return out


def fma(a, b, c):
    """fmaf on float32 values: a * b is exact in float64 and the float64 sum s, rounded once more to float32, is the exact result's
    rounding unless s lies exactly half way between two float32 values and is itself inexact.  Where that can be (the pattern of a
    half-way point in s's low bits; or a result in float32's subnormal range, whose half-way points look otherwise) the sum is rounded
    to odd instead, which a single rounding to float32 always turns into the exact result's.  Returns float32."""
    p = np.asarray(a, f64) * np.asarray(b, f64)
    c = np.asarray(c, f64)
    s = p + c
    mag = np.abs(s)
    if ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000).any() or ((mag < 1e-37) & (mag > 0.0)).any():
        c = np.broadcast_to(c, p.shape)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        move = (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(move, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(f32)


def linear(x, W, b):
    """ok_lidar_dot for every row of x and every row of W: the chain from the bias, k ascending."""
    acc = np.broadcast_to(b.astype(f32), (x.shape[0], W.shape[0])).copy()
    for k in range(W.shape[1]):
        acc = fma(x[:, k, None], W[None, :, k], acc)
    return acc


def label_weight(steer, steer_scale, weight, threshold):
    y = np.asarray(steer, f32) / f32(steer_scale)
    y = np.where(y < f32(-1), f32(-1), np.where(y > f32(1), f32(1), y)).astype(f32)
    w = np.where(np.abs(y) > f32(threshold), f32(weight), f32(1)).astype(f32)
    return y, w


def positions(head, shape, e, steer, steer_scale, weight, threshold):
    """Every row of ok_vithead_position for the positions' embeddings e [Q][D]: dict of h1, h2, o, y, w, t, do, d2, d1."""
    D, H1, H2 = shape
    W1, b1, W2, b2, W3, b3 = split(np.asarray(head, f32), D, H1, H2)
    s1 = linear(e, W1, b1)
    h1 = np.where(s1 > 0, s1, f32(0)).astype(f32)
    s2 = linear(h1, W2, b2)
    h2 = np.where(s2 > 0, s2, f32(0)).astype(f32)
    o = linear(h2, W3, b3)[:, 0]
    y, w = label_weight(steer, steer_scale, weight, threshold)
    err = (o - y).astype(f32)
    t = (w * (err * err).astype(f32)).astype(f32)
    do = ((f32(2) * w).astype(f32) * err).astype(f32)
    d2 = np.where(s2 > 0, (W3[0][None, :] * do[:, None]).astype(f32), f32(0)).astype(f32)
    acc = np.zeros((e.shape[0], H1), f32)
    for k in range(H2):
        acc = fma(W2[k][None, :], d2[:, k, None], acc)
    d1 = np.where(s1 > 0, acc, f32(0)).astype(f32)
    return dict(s1=s1, s2=s2, h1=h1, h2=h2, o=o, y=y, w=w, t=t, do=do, d2=d2, d1=d1)


def minibatch(head, shape, e, steer, steer_scale, weight, threshold):
    """The joined sums of one minibatch (its positions' rows e, steer) divided by B_k: (grad [P], loss)."""
    r = positions(head, shape, e, steer, steer_scale, weight, threshold)
    Bk = e.shape[0]
    layers = [(r["d1"], e), (r["d2"], r["h1"]), (r["do"][:, None], r["h2"])]
    joined, l_joined = None, None
    for c0 in range(0, Bk, CHUNK):
        n = min(CHUNK, Bk - c0)
        part = [[np.zeros((d.shape[1], a.shape[1]), f32), np.zeros(d.shape[1], f32)] for d, a in layers]
        l_part = f32(0)
        for q in range(c0, c0 + n):
            for (d, a), pw in zip(layers, part):
                pw[0] = fma(d[q][:, None], a[q][None, :], pw[0])
                pw[1] = (pw[1] + d[q]).astype(f32)
            l_part = f32(l_part + r["t"][q])
        flat = np.concatenate([x.reshape(-1) for pw in part for x in pw])
        if n < CHUNK:  # the rule's ZERO TERMS
            flat = (flat + f32(0)).astype(f32)
            l_part = f32(l_part + f32(0))
        joined = flat if joined is None else (joined + flat).astype(f32)
        l_joined = l_part if l_joined is None else f32(l_joined + l_part)
    return (joined / f32(Bk)).astype(f32), f32(l_joined / f32(Bk)), r


def powi(b, t):
    r = 1.0
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def adam(p, m, v, g, t, lr, beta1, beta2, eps):
    """ok_learn_adam with ok_learn_factors' step and bc2 of step number t."""
    lr, beta1, beta2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    step = f32(f64(lr) / (1.0 - powi(float(beta1), t)))
    bc2 = f32(np.sqrt(f64(1.0 - powi(float(beta2), t))))
    omb1, omb2 = f32(1.0 - f64(beta1)), f32(1.0 - f64(beta2))
    mn = ((beta1 * m).astype(f32) + (omb1 * g).astype(f32)).astype(f32)
    vn = ((beta2 * v).astype(f32) + ((omb2 * g).astype(f32) * g).astype(f32)).astype(f32)
    den = ((np.sqrt(vn).astype(f32) / bc2).astype(f32) + eps).astype(f32)
    return (p - (step * (mn / den).astype(f32)).astype(f32)).astype(f32), mn, vn


def sample_of(order_row, at, M):
    idx = np.arange(at[0], at[1]) if order_row is None else np.asarray(order_row[at[0]:at[1]], np.int64)
    return np.clip(idx, 0, M - 1)


def update(hp, shape, steer_scale, state, embedding, steer, B, epochs=1, order=None):
    """okenv_vit_head_update_host restated.  hp: dict(lr, beta1, beta2, eps, weight, threshold).  Returns (new state, losses, grad)."""
    embedding, steer = np.asarray(embedding, f32), np.asarray(steer, f32)
    M = steer.shape[0]
    p, m, v = (np.array(state[k], f32) for k in ("params", "m", "v"))
    t = int(state["t"])
    losses, grad = [], None
    for e in range(epochs):
        for base in range(0, M, B):
            s = sample_of(None if order is None else np.asarray(order).reshape(epochs, M)[e], (base, min(base + B, M)), M)
            grad, loss, _ = minibatch(p, shape, embedding[s], steer[s], steer_scale, hp["weight"], hp["threshold"])
            t += 1
            p, m, v = adam(p, m, v, grad, t, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"])
            losses.append(loss)
    return dict(params=p, m=m, v=v, t=t), np.array(losses, f32), grad


def evaluate(hp, shape, steer_scale, head, embedding, steer, B):
    embedding, steer = np.asarray(embedding, f32), np.asarray(steer, f32)
    M = steer.shape[0]
    return np.array([minibatch(head, shape, embedding[b:b + B], steer[b:b + B], steer_scale, hp["weight"], hp["threshold"])[1] for b in range(0, M, B)], f32)


# ---- data ---------------------------------------------------------------------------------------------------------------------------

HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight=5.0, threshold=0.1)
STEER_SCALE = 10.0
# (name, M, B, epochs, permuted): the geometries of the launch and of the rule's chunks
GEOMETRIES = [("less_than_a_tile", 13, 5, 1, False),  # B no multiple of 4, last minibatch of 3
              ("second_chunk_of_one", 65, 65, 1, False),
              ("reference_batch", 600, 512, 1, False),  # a partial minibatch of 88: one full chunk and 24 positions
              ("batch_beyond_M", 13, 20, 1, False),
              ("two_epochs_permuted", 13, 5, 2, True),  # an order with a repeated and an out-of-range index
              ("whole_chunk_then_one", 65, 64, 1, False),  # a minibatch of exactly one chunk (no filler term), then one of a single position
              ("permuted_across_chunks", 150, 70, 2, True)]  # minibatches of 70, 70 and 10: the order read past a chunk and in later minibatches


def random_head(shape, rng, scale=1.0):
    """torch's nn.Linear magnitudes: uniform in +-scale / sqrt(fan_in)."""
    D, H1, H2 = shape
    out = []
    for rows, cols in ((H1, D), (H2, H1), (1, H2)):
        bound = scale / np.sqrt(cols)
        out += [rng.uniform(-bound, bound, rows * cols), rng.uniform(-bound, bound, rows)]
    return np.concatenate(out).astype(f32)


def random_data(shape, M, rng):
    """Embeddings like a LayerNorm's output; steering on both sides of the threshold and beyond the clamp."""
    emb = rng.standard_normal((M, shape[0])).astype(f32)
    steer = (rng.uniform(-1.3, 1.3, M) * STEER_SCALE).astype(f32)
    steer[::4] = (rng.uniform(-0.1, 0.1, M)[::4] * STEER_SCALE).astype(f32)
    return emb, steer


def fresh_state(head):
    return dict(params=np.array(head, f32), m=np.zeros(head.size, f32), v=np.zeros(head.size, f32), t=0)


def case(shape, geometry, seed=0):
    """(state, embedding, steer, B, epochs, order) of one geometry; the state has already taken steps: m, v and t are not zero."""
    name, M, B, epochs, permuted = geometry
    rng = np.random.default_rng(1000 * seed + 7 * M + B + shape[0])
    head = random_head(shape, rng)
    emb, steer = random_data(shape, M, rng)
    st = fresh_state(head)
    st["m"] = (1e-3 * rng.standard_normal(head.size)).astype(f32)
    st["v"] = (1e-6 * rng.uniform(0, 1, head.size)).astype(f32)
    st["t"] = 3
    order = None
    if permuted:
        order = np.stack([rng.permutation(M) for _ in range(epochs)]).astype(np.int32)
        order[0, 1] = order[0, 0]  # a repeated index
        order[0, 3] = M + 5        # out of range: counts as M - 1
        order[1, 2] = -2           # ... as 0
    return st, emb, steer, B, epochs, order


# ---- float64 error bounds -----------------------------------------------------------------------------------------------------------

def mlp_bounds(pieces64, x):
    """Error bounds of a float32 forward of D -> H1 -> H2 -> 1 with ReLU, written for any summation order: a sum of n terms is charged
    (n + 2) u times the sum of the terms' magnitudes (the products' roundings and the bias included), ReLU (slope <= 1) passes its
    input's error on.  Returns (p1, p2, h1, h2, z3) of the float64 run and (e_h1, e_h2, e_z3)."""
    W1, b1, W2, b2, W3, b3 = pieces64
    p1 = x @ W1.T + b1
    h1 = np.maximum(p1, 0)
    p2 = h1 @ W2.T + b2
    h2 = np.maximum(p2, 0)
    z3 = h2 @ W3.T + b3
    aW1, aW2, aW3 = np.abs(W1), np.abs(W2), np.abs(W3)
    e_h1 = (x.shape[1] + 2) * U * (np.abs(b1) + np.abs(x) @ aW1.T)
    e_h2 = e_h1 @ aW2.T + (W2.shape[1] + 2) * U * (np.abs(b2) + np.abs(h1) @ aW2.T)
    e_z3 = e_h2 @ aW3.T + (W3.shape[1] + 2) * U * (np.abs(b3) + np.abs(h2) @ aW3.T)
    return (p1, p2, h1, h2, z3), (e_h1, e_h2, e_z3)


def grad_bounds(pieces64, x, fwd, errs, dz, E_dz):
    """Bounds on every parameter's summed gradient from the output seeds dz (float64 run) and their error bounds E_dz, to first order
    in u: dh = W^T d charged (n + 1) u, ReLU's slope exactly 0 / 1 away from 0, every term a * b charged E_a |b| + |a| e_b + u |a b|,
    the sum over the M samples (M + 1) u times the magnitudes.  Returns (bound, magnitude) per parameter in parameter order, before
    the division by the count."""
    W1, b1, W2, b2, W3, b3 = pieces64
    p1, p2, h1, h2, _ = fwd
    e_h1, e_h2, _ = errs
    M = x.shape[0]
    aW2, aW3 = np.abs(W2), np.abs(W3)
    adz = np.abs(dz)
    dh2, E_dh2 = adz @ aW3, E_dz @ aW3 + (W3.shape[0] + 1) * U * (adz @ aW3)
    s2 = (p2 > 0).astype(f64)
    d2, E_d2 = dh2 * s2, E_dh2 * s2 + U * dh2 * s2
    dh1, E_dh1 = d2 @ aW2, E_d2 @ aW2 + (W2.shape[0] + 1) * U * (d2 @ aW2)
    s1 = (p1 > 0).astype(f64)
    d1, E_d1 = dh1 * s1, E_dh1 * s1 + U * dh1 * s1

    def outer(a, E_a, b, e_b):
        return (E_a.T @ b + a.T @ e_b + U * (a.T @ b)).reshape(-1), (a.T @ b).reshape(-1)

    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    pieces = [outer(d1, E_d1, np.abs(x), 0 * x), outer(d1, E_d1, one, zero), outer(d2, E_d2, np.abs(h1), e_h1), outer(d2, E_d2, one, zero),
              outer(adz, E_dz, np.abs(h2), e_h2), outer(adz, E_dz, one, zero)]
    err, mag = np.concatenate([a for a, _ in pieces]), np.concatenate([b for _, b in pieces])
    return err + (M + 1) * U * mag, mag
