"""A numpy mirror of the world-model racers' memory (include/okenv_memory.h), written from the header's prose independently of the
C code: the network vector's layout, one act (the normalised input, the stacked GRU with every blocked chain's fmaf restated as exactly
rounded a * b + c through _world_numpy.fma, the head's prediction, the controller on [mu | h_top]) and the kernels' plan, LDS bytes and
workspace words (openkitchen_amd/csrc/ok_memory.h).  tanh is the project's own function and comes from the CPU oracle (oracle_tanhf);
the encoder's mu is _world_numpy's."""
import numpy as np

import _world_numpy as world

f32, f64 = np.float32, np.float64
LDS_BUDGET = 160 * 1024
ROWS, COLS, CHUNK, LDA = 128, 32, 64, 66  # of ok_memory.h: a workgroup's list slots and hidden units, a K block's k's, the A tile's pitch

# the world shapes the memories stand on: _world_numpy's cheap ones, and one with the widest latent on the narrowest encoder
WORLDS = dict(tiny=world.SHAPES["tiny"], odd=world.SHAPES["odd"], latent128=dict(image_size=16, channels=(16, 16, 16, 16), latent=128, hidden=2))

# name -> (world shape, the shape members of capi.memory_config)
SHAPES = {
    # the smallest memory: one column block whose second tile idles, one K block of 16 everywhere, one layer
    "h16": ("tiny", dict(hidden=16, layers=1, ctrl_hidden=2)),
    # H no multiple of a workgroup's 32 columns: two column blocks, the last with one live tile; K blocks of 48
    "h48": ("odd", dict(hidden=48, layers=2, ctrl_hidden=6)),
    # the limit of the width: sixteen column blocks, eight full K blocks; the reference's memory on the tiny encoder
    "h512": ("tiny", dict(hidden=512, layers=3, ctrl_hidden=16)),
    # the limit of the depth, the widest controller (560 inputs, 64 units)
    "l4": ("odd", dict(hidden=512, layers=4, ctrl_hidden=64)),
    # two K blocks in layer 0's input (Z = 128) and a chain over H whose last K block is shorter than the first (96 = 64 + 32); three
    # column blocks, all full
    "z128": ("latent128", dict(hidden=96, layers=2, ctrl_hidden=4)),
}
# okenv_memory_plan without its carry member: (column blocks, live tiles of the last, K blocks of layer 0's input, k's of the last, K
# blocks over H, k's of the last, layers)
PATHS = {
    "h16": (1, 1, 1, 16, 1, 16, 1),
    "h48": (2, 1, 1, 48, 1, 48, 2),
    "h512": (16, 2, 1, 16, 8, 64, 3),
    "l4": (16, 2, 1, 48, 8, 64, 4),
    "z128": (3, 2, 2, 64, 2, 32, 2),
}
COUNTS = (1, 17, 33)  # agents: a partial row tile, a full one and a partial one, several (every wave and a second and third row workgroup
#                       of the layer kernel: tests/_population_cases.py's MEMORY_COUNTS, in tests/test_gpu_image_populations.py)


def shape_of(name):
    """(world shape members, memory shape members, Z, H, L, h)."""
    wname, mem = SHAPES[name]
    w = WORLDS[wname]
    return w, mem, w["latent"], mem["hidden"], mem["layers"], mem["ctrl_hidden"]


def layout(Z, H, L):
    """(name, offset, shape) of every piece of the network vector: torch's state_dict of GRUDynamics, then the statistics."""
    pieces = []
    for l in range(L):
        pieces += [("gru.weight_ih_l%d" % l, (3 * H, Z + 2 if l == 0 else H)), ("gru.weight_hh_l%d" % l, (3 * H, H)),
                   ("gru.bias_ih_l%d" % l, (3 * H,)), ("gru.bias_hh_l%d" % l, (3 * H,))]
    pieces += [("head.weight", (Z, H)), ("head.bias", (Z,)), ("z_mean", (Z,)), ("z_std", (Z,)), ("a_mean", (2,)), ("a_std", (2,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def num_params(Z, H, L, h):
    """(floats of the network vector, floats of one controller)."""
    name, at, shape = layout(Z, H, L)[-1]
    i = Z + H
    return at + int(np.prod(shape)), (h * i + h) + ((h // 2) * h + h // 2) + (h // 2 + 1)


def split(Z, H, L, params):
    return {name: np.asarray(params[at:at + int(np.prod(shape))], f32).reshape(shape) for name, at, shape in layout(Z, H, L)}


def draw_params(name, seed, n):
    """Float32 vectors: the network at torch's default init (uniform in [-b, b], b = 1 / sqrt(H)), statistics of the size train_rnn.py
    finds for latents of the size the drawn encoders give (means in [-0.1, 0.5], spreads in [0.5, 1.5]; the throttle constant near 100, the steering within +-5), and n controllers uniform in
    [-b, b], b = 2 / sqrt(inputs), so that the wide first layer does not saturate."""
    w, mem, Z, H, L, h = shape_of(name)
    rng = np.random.default_rng(9000 + seed)
    nn, nc = num_params(Z, H, L, h)
    net = np.empty(nn, f32)
    b = 1.0 / np.sqrt(H)
    for pname, at, shape in layout(Z, H, L):
        m = int(np.prod(shape))
        if pname == "z_mean":
            net[at:at + m] = rng.uniform(-0.1, 0.5, m)
        elif pname == "z_std":
            net[at:at + m] = rng.uniform(0.5, 1.5, m)
        elif pname == "a_mean":
            net[at:at + m] = (90.0, 0.25)
        elif pname == "a_std":
            net[at:at + m] = (20.0, 2.5)
        else:
            net[at:at + m] = rng.uniform(-b, b, m)
    return net, rng.uniform(-1.0, 1.0, (n, nc)).astype(f32) * f32(2.0 / np.sqrt(Z + H))


def tanh(v):
    import _oracle as O
    v = np.ascontiguousarray(v, f32)
    out = np.empty(v.size, f32)
    O.lib().oracle_tanhf(v.reshape(-1), out, v.size)
    return out.reshape(v.shape)


BLOCK = 64  # the rule's block of k's


def dot(x, w, b):
    """x [n][K], w [M][K], b [M] -> [n][M] float32: from the bias, per block of 64 k's a fused chain from +0, added on in order."""
    acc = np.tile(np.asarray(b, f32)[None], (x.shape[0], 1))
    x, w = np.asarray(x, f64), np.asarray(w, f64)
    for k0 in range(0, x.shape[1], BLOCK):
        part = np.zeros(acc.shape, f64)
        for k in range(k0, min(k0 + BLOCK, x.shape[1])):
            part = world.fma(x[:, k, None], w[None, :, k], part)
        acc = acc + part.astype(f32)
    return acc


def sig(v):
    return f32(0.5) * tanh(f32(0.5) * v) + f32(0.5)


def step(Z, H, L, carry, net, mu, action, hidden):
    """mu [n][Z], action [n][2] (as stored), hidden [n][L][H] -> (the new hidden [n][L][H], the prediction [n][Z])."""
    p = split(Z, H, L, net)
    mu, action, hidden = np.asarray(mu, f32), np.asarray(action, f32), np.asarray(hidden, f32)
    n = mu.shape[0]
    x = np.concatenate([(mu - p["z_mean"]) / p["z_std"], (action - p["a_mean"]) / p["a_std"]], axis=1).astype(f32)
    out = np.empty((n, L, H), f32)
    for l in range(L):
        before = hidden[:, l] if carry else np.zeros((n, H), f32)
        wih = p["gru.weight_ih_l%d" % l]
        if l == 0:  # the latent columns in their blocks, the two action columns as a last block of their own
            gi = dot(x[:, :Z], wih[:, :Z], p["gru.bias_ih_l0"]) + dot(x[:, Z:], wih[:, Z:], np.zeros(3 * H, f32))
        else:
            gi = dot(x, wih, p["gru.bias_ih_l%d" % l])
        if carry:
            gh = dot(before, p["gru.weight_hh_l%d" % l], p["gru.bias_hh_l%d" % l])
        else:
            gh = np.tile(p["gru.bias_hh_l%d" % l][None], (n, 1))  # the rule leaves the chain out
        r = sig(gi[:, :H] + gh[:, :H])
        u = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        cand = tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        x = ((f32(1.0) - u) * cand + u * before).astype(f32)
        out[:, l] = x
    prediction = dot(x, p["head.weight"], p["head.bias"]) * p["z_std"] + p["z_mean"]
    return out, prediction.astype(f32)


def controller(n_in, h, ctrl, state):
    """ctrl [n][.], state [n][n_in] -> the output behind its tanh [n]: every unit from its bias, w * x added in ascending order, one
    multiply and one add per term."""
    x, at = np.asarray(state, f32), 0
    for a, b in ((n_in, h), (h, h // 2), (h // 2, 1)):
        w = ctrl[:, at:at + b * a].reshape(-1, b, a)
        at += b * a
        acc = ctrl[:, at:at + b].copy()
        at += b
        for k in range(a):
            acc = acc + w[:, :, k] * x[:, k, None]
        x = tanh(acc)
    assert at == ctrl.shape[1]
    return x[:, 0]


def act(name, carry, enc, net, ctrl, frames, hidden, throttle, steer, throttle_out=100.0, steer_scale=5.0):
    """One act of every frame's agent by the rule: the record's members, the new hidden_state [n][L][H], throttle and steer."""
    w, mem, Z, H, L, h = shape_of(name)
    mu = world.encode(w, enc, frames)
    new, prediction = step(Z, H, L, carry, net, mu, np.stack([throttle, steer], axis=1), hidden)
    state = np.concatenate([mu, new[:, L - 1]], axis=1)
    out = controller(Z + H, h, np.asarray(ctrl, f32), state)
    n = mu.shape[0]
    thr, st = np.full(n, throttle_out, f32), out * f32(steer_scale)
    return dict(mu=mu, hidden=new[:, L - 1].copy(), prediction=prediction, state=state, out=out, action=np.stack([thr, st], axis=1),
                alive=np.ones(n, np.uint8), hidden_state=new, throttle=thr, steer=st)


# ---- the plan, restated -----------------------------------------------------------------------------------------------------------------

def plan(Z, H, L, carry):
    blocks = -(-H // COLS)
    zb, hb = -(-Z // CHUNK), -(-H // CHUNK)
    return (blocks, (H - (blocks - 1) * COLS) // 16, zb, Z - (zb - 1) * CHUNK, hb, H - (hb - 1) * CHUNK, carry, L)


def lds_bytes():
    return 4 * (ROWS * LDA + 3 * COLS * CHUNK)


def workspace_words(Z, H, L, h, n):
    nn, nc = num_params(Z, H, L, h)
    pack = 3 * H * (Z + H) + (L - 1) * 3 * H * 2 * H
    words = (pack + n * nc + 3) // 4 * 4
    return words + n * Z + n * (Z + 4) + 2 * n * L * H + nn
