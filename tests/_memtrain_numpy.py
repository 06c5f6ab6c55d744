"""A numpy mirror of the training of the world-model racers' memory (include/okenv_memtrain.h), written from the header's prose
independently of the C code: the windows and their normalised inputs and targets, the forward through _memory_numpy's blocked chains
(dot) and the project's tanh, the seeds, the backward through every cell with each operation rounded once, the parameter sums as
chains over the step-major positions, the levelled sum of squares, the clip factor, AdamW and the step factors.  Also the grid of the
tests: SHAPES and GEOMETRIES, and the drawn data."""
import numpy as np

import _memory_numpy as mem
import _world_numpy as world

f32, f64 = np.float32, np.float64
BLOCK, MAX_SEQ = 64, 16

# name -> (Z, H, L)
SHAPES = {
    "16-16-1": (16, 16, 1),    # the smallest: one block everywhere, no layer above
    "48-48-2": (48, 48, 2),    # a partial column block, K blocks of 48, dx handed down one layer, 144 = 64 + 64 + 16 gate rows
    "128-96-2": (128, 96, 2),  # two K blocks in layer 0's input, a ragged chain over H (64 + 32), 288 gate rows
    "16-512-3": (16, 512, 3),  # the reference's width and depth: host and device only, at one small geometry
}
MIRRORED = ("16-16-1", "48-48-2", "128-96-2")
WIDE, WIDE_GEOMETRY = "16-512-3", "short_last_minibatch"  # 13 windows of 3 steps: 39 positions

# name -> (M, B, S, epochs, stride)
GEOMETRIES = {
    "one_position": (1, 1, 1, 1, 1),             # no recurrence
    "two_steps": (3, 3, 2, 1, 1),                # the smallest BPTT
    "second_block_of_one": (13, 13, 5, 1, 1),    # 65 positions
    "whole_block": (32, 32, 2, 1, 1),            # exactly 64 positions, no filler
    "second_row_workgroup": (129, 129, 1, 1, 1), # one window beyond 128 rows
    "short_last_minibatch": (13, 5, 3, 1, 1),    # minibatches of 5, 5 and 3
    "batch_beyond_M": (4, 9, 2, 1, 1),           # B larger than M
    "longest_window": (2, 2, 16, 1, 1),          # the largest S
    "two_epochs_strided": (13, 5, 3, 2, 7),      # seven interleaved agents, permuted orders, indices out of range, a clamped target row
}


def world_members(Z):
    """The members of capi.world_config for a latent width: the cheapest encoder shape (the training never runs the encoder)."""
    return dict(image_size=16, channels=(16, 16, 16, 16), latent=Z, hidden=2)


def draw_network(Z, H, L, seed):
    """The network vector at torch's default init with statistics of the size train_rnn.py finds."""
    rng = np.random.default_rng(4100 + seed)
    nn = mem.num_params(Z, H, L, 2)[0]
    net = np.empty(nn, f32)
    b = 1.0 / np.sqrt(H)
    for name, at, shape in mem.layout(Z, H, L):
        m = int(np.prod(shape))
        if name == "z_mean":
            net[at:at + m] = rng.uniform(-0.1, 0.5, m)
        elif name == "z_std":
            net[at:at + m] = rng.uniform(0.5, 1.5, m)
        elif name == "a_mean":
            net[at:at + m] = (90.0, 0.25)
        elif name == "a_std":
            net[at:at + m] = (20.0, 2.5)
        else:
            net[at:at + m] = rng.uniform(-b, b, m)
    return net


def trainable(Z, H, L):
    return mem.num_params(Z, H, L, 2)[0] - (2 * Z + 4)


def draw_data(Z, geometry, seed):
    """latent [rows][Z], action [rows][2], start [M] and the order [epochs][M] or None of a geometry.  The strided geometry's rows are
    [T][7] agents; its last windows' targets lie beyond the last row (clamped), its orders repeat an index and leave the range."""
    M, B, S, epochs, stride = GEOMETRIES[geometry]
    rng = np.random.default_rng(5200 + seed)
    if stride == 1:
        rows = M + S
        start = np.arange(M, dtype=np.int32)
        order = None
    else:
        T = 2 + S  # time steps: the windows start at t0 = 0 and 1; those at t0 = 2 have their last target beyond the end
        rows = T * stride
        start = np.array([t0 * stride + n for t0 in range(3) for n in range(stride)], np.int32)[:M]
        order = np.stack([rng.permutation(M) for _ in range(epochs)]).astype(np.int32)
        order[0, 1] = order[0, 0]      # a repeated index
        order[0, 2] = -3               # below the range: counts as 0
        order[epochs - 1, 4] = M + 5   # above it: counts as M - 1
    latent = rng.normal(0.2, 1.0, (rows, Z)).astype(f32)
    action = np.stack([rng.normal(90.0, 20.0, rows), rng.normal(0.25, 2.5, rows)], axis=1).astype(f32)
    return latent, action, start, order


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def chain(a, b):
    """a [n][K], b [M][K] -> [n][M]: the primitive from a +0.0f bias."""
    return mem.dot(a, b, np.zeros(b.shape[0], f32))


def clamp(i, n):
    return int(min(max(int(i), 0), n - 1))


def forward(Z, H, L, net, latent, action, first, S, stride):
    """The windows starting at rows `first` -> dict of what the backward needs, positions step-major: x0 [P][Z + 2], y [P][Z],
    zn [P][Z]; r, u, n, ghn, h, hprev [L][P][H]."""
    p = mem.split(Z, H, L, net)
    rows, Bk = latent.shape[0], len(first)
    P = Bk * S
    at = [clamp(int(f) + s * stride, rows) for s in range(S) for f in first]
    to = [clamp(int(f) + (s + 1) * stride, rows) for s in range(S) for f in first]
    x0 = np.concatenate([(latent[at] - p["z_mean"]) / p["z_std"], (action[at] - p["a_mean"]) / p["a_std"]], axis=1).astype(f32)
    y = ((latent[to] - p["z_mean"]) / p["z_std"]).astype(f32)
    keys = ("r", "u", "n", "ghn", "h", "hprev")
    out = {k: np.zeros((L, P, H), f32) for k in keys}
    for s in range(S):
        rows_s = slice(s * Bk, (s + 1) * Bk)
        x = x0[rows_s]
        for l in range(L):
            before = out["h"][l, (s - 1) * Bk:s * Bk] if s > 0 else np.zeros((Bk, H), f32)
            wih = p["gru.weight_ih_l%d" % l]
            if l == 0:
                gi = mem.dot(x[:, :Z], wih[:, :Z], p["gru.bias_ih_l0"]) + mem.dot(x[:, Z:], wih[:, Z:], np.zeros(3 * H, f32))
            else:
                gi = mem.dot(x, wih, p["gru.bias_ih_l%d" % l])
            gh = mem.dot(before, p["gru.weight_hh_l%d" % l], p["gru.bias_hh_l%d" % l])  # also at step 0: the chain over zeros
            r = mem.sig(gi[:, :H] + gh[:, :H])
            u = mem.sig(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = mem.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            x = ((f32(1.0) - u) * n + u * before).astype(f32)
            for k, v in zip(keys, (r, u, n, gh[:, 2 * H:], x, before)):
                out[k][l, rows_s] = v
    zn = mem.dot(out["h"][L - 1], p["head.weight"], p["head.bias"])
    out.update(x0=x0, y=y, zn=zn)
    return out


def minibatch(Z, H, L, net, latent, action, first, S, stride, want_grad=True):
    """(loss, the divided gradient [T] or None) of one minibatch."""
    p = mem.split(Z, H, L, net)
    f = forward(Z, H, L, net, latent, action, first, S, stride)
    Bk = len(first)
    P = Bk * S
    e = f["zn"] - f["y"]
    tt, dzn = e * e, f32(2.0) * e
    count = f32(Bk * S * Z)
    ones = np.ones((1, P), f32)
    lossj = chain(tt.T, ones)[:, 0]
    loss = chain(lossj[None], np.ones((1, Z), f32))[0, 0] / count
    if not want_grad:
        return loss, None
    grad = {}
    down = chain(dzn, p["head.weight"].T)  # [P][H]: over k < Z of dzn_k * head.w[k][j]
    one = f32(1.0)
    for l in range(L - 1, -1, -1):
        whh, wih = p["gru.weight_hh_l%d" % l], p["gru.weight_ih_l%d" % l]
        dgi, dgh = np.zeros((P, 3 * H), f32), np.zeros((P, 3 * H), f32)
        keep = back = np.zeros((Bk, H), f32)
        for s in range(S - 1, -1, -1):
            rows_s = slice(s * Bk, (s + 1) * Bk)
            r, u, n, ghn, hprev = (f[k][l, rows_s] for k in ("r", "u", "n", "ghn", "hprev"))
            dh = (down[rows_s] + keep) + back
            dn = dh * (one - u)
            du = dh * (hprev - n)
            keep = dh * u
            da_n = dn * (one - n * n)
            dr = da_n * ghn
            da_r = dr * (r * (one - r))
            da_u = du * (u * (one - u))
            dgi[rows_s] = np.concatenate([da_r, da_u, da_n], axis=1)
            dgh[rows_s] = np.concatenate([da_r, da_u, da_n * r], axis=1)
            if s > 0:
                back = chain(dgh[rows_s], whh.T)  # over the 3H gate rows i of dgh_i * Whh[i][j]
        x = f["x0"] if l == 0 else f["h"][l - 1]
        grad["gru.weight_ih_l%d" % l] = chain(dgi.T, x.T) / count
        grad["gru.weight_hh_l%d" % l] = chain(dgh.T, f["hprev"][l].T) / count
        grad["gru.bias_ih_l%d" % l] = chain(dgi.T, ones)[:, 0] / count
        grad["gru.bias_hh_l%d" % l] = chain(dgh.T, ones)[:, 0] / count
        if l > 0:
            down = chain(dgi, wih.T)
    grad["head.weight"] = chain(dzn.T, f["h"][L - 1].T) / count
    grad["head.bias"] = chain(dzn.T, ones)[:, 0] / count
    flat = np.concatenate([grad[name].astype(f32).ravel() for name, at, shape in mem.layout(Z, H, L) if name in grad])
    assert flat.size == trainable(Z, H, L)
    return loss, flat


def sumsq(g):
    """Level 0: blocks of 64, fmaf(g, g, part) from +0 ascending; further levels: groups of 64 summed by plain additions from +0."""
    g = np.asarray(g, f32)
    pad = (-g.size) % BLOCK
    v = np.concatenate([g, np.zeros(pad, f32)]).reshape(-1, BLOCK).astype(f64)  # (padding terms leave a chain from +0 as it is)
    part = np.zeros(v.shape[0], f64)
    for k in range(BLOCK):
        part = world.fma(v[:, k], v[:, k], part)
    level = part.astype(f32)
    while level.size > 1:
        pad = (-level.size) % BLOCK
        v = np.concatenate([level, np.zeros(pad, f32)]).reshape(-1, BLOCK)
        acc = np.zeros(v.shape[0], f32)
        for k in range(BLOCK):
            acc = acc + v[:, k]
        level = acc
    return level[0]


def clip(total, clip_grad):
    """(the pre-clip norm, the factor)."""
    norm = f32(np.sqrt(f64(total)))
    if not clip_grad > 0:
        return norm, f32(1.0)
    coef = f32(clip_grad) / (norm + f32(1e-6))
    return norm, (f32(1.0) if coef > f32(1.0) else coef)


def powi(b, t):
    r = 1.0
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def adamw(p, m, v, g, coef, lr, cfg, t):
    """One step of the trainable prefix; t: the step's number.  Returns (p, m, v, the clipped gradient)."""
    b1, b2, eps = f32(cfg["beta1"]), f32(cfg["beta2"]), f32(cfg["eps"])
    omb1, omb2 = f32(1.0 - f64(b1)), f32(1.0 - f64(b2))
    step = f32(f64(f32(lr)) / (1.0 - powi(float(b1), t)))
    bc2 = f32(np.sqrt(1.0 - powi(float(b2), t)))
    decay = f32(1.0 - f64(f32(lr)) * f64(f32(cfg["weight_decay"])))
    gc = (g * coef).astype(f32)
    p = p * decay
    mn = b1 * m + omb1 * gc
    vn = b2 * v + (omb2 * gc) * gc
    root = np.sqrt(vn.astype(f64)).astype(f32)
    p = p - step * (mn / (root / bc2 + eps))
    return p.astype(f32), mn.astype(f32), vn.astype(f32), gc


def update(Z, H, L, cfg, state, latent, action, start, M, B, S, epochs, stride, order=None, lr_schedule=None):
    """The whole call: (new state, dict(loss, norm, grad))."""
    T = trainable(Z, H, L)
    net, m, v, t = state["params"].copy(), state["m"].copy(), state["v"].copy(), int(state["t"])
    slices = -(-M // B)
    loss, norm = np.zeros(epochs * slices, f32), np.zeros(epochs * slices, f32)
    gc = None
    for e in range(epochs):
        for k in range(slices):
            Bk = min(B, M - k * B)
            idx = [clamp(order[e][k * B + q] if order is not None else k * B + q, M) for q in range(Bk)]
            l, g = minibatch(Z, H, L, net, latent, action, [start[i] for i in idx], S, stride)
            n, coef = clip(sumsq(g), cfg["clip_grad"])
            lr = cfg["lr"] if lr_schedule is None else lr_schedule[e * slices + k]
            t += 1
            net[:T], m, v, gc = adamw(net[:T], m, v, g, coef, lr, cfg, t)
            loss[e * slices + k], norm[e * slices + k] = l, n
    return dict(params=net, m=m, v=v, t=t), dict(loss=loss, norm=norm, grad=gc)


def evaluate(Z, H, L, net, latent, action, start, M, B, S, stride):
    slices = -(-M // B)
    return np.array([minibatch(Z, H, L, net, latent, action, [start[i] for i in range(k * B, min(M, k * B + B))], S, stride, False)[0]
                     for k in range(slices)], f32)


def lds_bytes():
    """The learner's kernels keep their operands in registers: no LDS."""
    return 0


def workspace_words(Z, H, L, S, B):
    """okMemTrainPlaces, restated: every piece rounded up to whole groups of 4 words."""
    T, P = trainable(Z, H, L), B * S
    r4 = lambda n: (n + 3) // 4 * 4
    words = r4(16) + 3 * r4(T) + r4(-(-T // 64)) + r4(-(-T // 4096)) + r4(P * (Z + 2)) + 3 * r4(P * Z) + r4(P * 3 * H) + r4(B * 3 * H)
    words += r4(P * H) + 2 * r4(B * H) + r4(Z)
    words += L * (4 * r4(P * H) + r4((B + P) * H) + 2 * r4(P * 3 * H))
    return words
