"""A numpy mirror of the world-model racers' rule (include/okenv_world.h): the parameter layouts, the forward pass with every fp32
operation of the rule restated (the fused chains as exactly rounded a * b + c), the score and the kernels' plan
(openkitchen_amd/csrc/ok_world.h: okWorldPlan), written independently for the tests.  sin / cos / tanh are the project's own
functions and come from the CPU oracle (oracle_sincosf, oracle_tanhf)."""
import numpy as np

f32, f64 = np.float32, np.float64
LDS_BUDGET = 160 * 1024
ROWS, COLS, CHUNK, LDA, AGENTS = 64, 128, 64, 66, 16  # of ok_world.h: a workgroup's tile, a K block's channels, the A tile's row pitch

# name -> the shape members of capi.world_config
SHAPES = {
    # sides 8 / 4 / 2 / 1: layers 2 and 3 have fewer than 16 rows per frame, so tiles span frames; a single position; 12 of 16 taps of
    # layer 3 in padding; one K block of 16 channels per tap; one 16-column tile, seven waves idle
    "tiny": dict(image_size=16, channels=(16, 16, 16, 16), latent=16, hidden=2),
    # sides 24 / 12 / 6 / 3: 36 and 9 rows per frame; channel counts that neither double nor are powers of two; K blocks of 16, 48 and
    # 32 channels; h / 2 odd
    "odd": dict(image_size=48, channels=(16, 48, 32, 80), latent=48, hidden=6),
    # the longest chain (K = 8192: eight K blocks per tap); the widest layer (four workgroups of columns), latent and controller
    "wide": dict(image_size=32, channels=(16, 16, 512, 512), latent=128, hidden=64),
    "reference": dict(image_size=128, channels=(64, 128, 256, 512), latent=32, hidden=16),
    # the paths of the plan the four above do not reach: a tap's last K block shorter than the others (80 = 64 + 16 input channels into
    # layer 2), a last workgroup of columns with idle waves behind full ones (144 = 128 + 16), and three-quarter blocks (112 = 64 + 48)
    "ragged": dict(image_size=16, channels=(80, 144, 112, 16), latent=32, hidden=4),
}
# okenv_world_plan: per layer (workgroups of columns, K blocks per tap, channels of a tap's last block)
PATHS = {
    "tiny": ((1, 0, 64), (1, 1, 16), (1, 1, 16), (1, 1, 16)),
    "odd": ((1, 0, 64), (1, 1, 16), (1, 1, 48), (1, 1, 32)),
    "wide": ((1, 0, 64), (1, 1, 16), (4, 1, 16), (4, 8, 64)),
    "reference": ((1, 0, 64), (1, 1, 64), (2, 2, 64), (4, 4, 64)),
    "ragged": ((1, 0, 64), (2, 2, 16), (1, 3, 16), (1, 2, 48)),
}


def cin(cfg, l):
    return 3 if l == 0 else cfg["channels"][l - 1]


def sides(cfg):
    return tuple(cfg["image_size"] >> (l + 1) for l in range(4))


def features(cfg):
    return cfg["channels"][3] * sides(cfg)[3] ** 2


CONVS = (0, 2, 5, 8)


def layout(cfg):
    """(name, offset, shape) of every piece of the encoder vector."""
    pieces = []
    for l in range(4):
        c = cfg["channels"][l]
        pieces += [("net.%d.weight" % CONVS[l], (c, cin(cfg, l), 4, 4)), ("net.%d.bias" % CONVS[l], (c,))]
    pieces += [("fc_mu.weight", (cfg["latent"], features(cfg))), ("fc_mu.bias", (cfg["latent"],))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def num_params(cfg):
    """(floats of the encoder vector, floats of one controller)."""
    name, at, shape = layout(cfg)[-1]
    i, h = cfg["latent"] + 2, cfg["hidden"]
    return at + int(np.prod(shape)), (h * i + h) + ((h // 2) * h + h // 2) + (h // 2 + 1)


def split(cfg, params):
    return {name: np.asarray(params[at:at + int(np.prod(shape))]).reshape(shape) for name, at, shape in layout(cfg)}


def draw_params(cfg, seed, n):
    """Float32 vectors: the encoder at torch's default init scale (weights uniform in [-b, b], b = 1 / sqrt(fan_in), the biases in
    [b / 2, b]: positive, so that the layers' outputs pass their ReLU), fc_mu's weights four times that, and n controllers uniform in
    [-1, 1] (CMA-ES candidates of sigma 0.5 are of that size)."""
    rng = np.random.default_rng(5000 + seed)
    ne, nc = num_params(cfg)
    enc = np.empty(ne, f32)
    for name, at, shape in layout(cfg):
        m = int(np.prod(shape))
        if name.endswith("weight"):
            bound = (4.0 if name == "fc_mu.weight" else 1.0) / np.sqrt(int(np.prod(shape[1:])))
            enc[at:at + m] = rng.uniform(-bound, bound, m)
        else:
            enc[at:at + m] = rng.uniform(0.5 * bound, bound, m)
    return enc, rng.uniform(-1.0, 1.0, (n, nc)).astype(f32)


def draw_frames(S, seed, n=2):
    return np.random.default_rng(7000 + seed).integers(0, 256, (n, S, S, 4), dtype=np.uint8)


def fma(a, b, c):
    """fmaf on arrays of float32 values (held as float32 or float64): a * b is exact in float64 and the float64 sum s, rounded once more
    to float32, is the exact result's rounding unless s lies exactly half way between two float32 values AND is itself inexact.  Where
    that can be (the pattern of a half-way point in s's low bits; or a result in float32's subnormal range, whose half-way points
    look otherwise) the sum is rounded to odd instead (moved to its odd neighbour on the side of what its rounding lost), which a
    single rounding to float32 always turns into the exact result's.  Returns float64 holding float32 values."""
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
    return s.astype(f32).astype(f64)


def conv(x, w, b):
    """x [n][Cin][side][side] float32, w [Cout][Cin][4][4], b [Cout]: kernel 4, stride 2, padding 1; the rule's chain, taps outside the
    input left out; the ReLU."""
    n, Cin, side_in, _ = x.shape
    side, Cout = side_in // 2, w.shape[0]
    x, w = x.astype(f64), w.astype(f64)
    acc = np.tile(b.astype(f64)[None, :, None, None], (n, 1, side, side))
    for ty in range(4):
        ys = [oy for oy in range(side) if 0 <= 2 * oy + ty - 1 < side_in]
        for tx in range(4):
            xs = [ox for ox in range(side) if 0 <= 2 * ox + tx - 1 < side_in]
            if not ys or not xs:
                continue  # (a tap that lies in the padding for every output)
            oy0, oy1, ox0, ox1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
            window = x[:, :, 2 * oy0 + ty - 1:2 * (oy1 - 1) + ty:2, 2 * ox0 + tx - 1:2 * (ox1 - 1) + tx:2]
            part = np.ascontiguousarray(acc[:, :, oy0:oy1, ox0:ox1])
            for ch in range(Cin):
                part = fma(window[:, ch][:, None], w[None, :, ch, ty, tx, None, None], part)
            acc[:, :, oy0:oy1, ox0:ox1] = part
    return np.maximum(acc, 0.0).astype(f32)


def encode(cfg, enc, frames):
    """frames [n][S][S][4] uint8 -> mu [n][Z] float32, by the rule."""
    p = split(cfg, np.asarray(enc, f32))
    x = np.asarray(frames)[..., :3].astype(f32).transpose(0, 3, 1, 2) / f32(255.0)
    for l in range(4):
        x = conv(np.ascontiguousarray(x), p["net.%d.weight" % CONVS[l]], p["net.%d.bias" % CONVS[l]])
    n, C, side, _ = x.shape
    P, Z = side * side, cfg["latent"]
    a = x.reshape(n, C, P)
    w = p["fc_mu.weight"].reshape(Z, C, P)  # torch's flatten: (ch, y, x)
    part = np.zeros((n, Z, P), f64)
    for ch in range(C):
        part = fma(a[:, None, ch, :], w[None, :, ch, :], part)
    part = part.astype(f32)
    mu = np.tile(p["fc_mu.bias"].astype(f32)[None], (n, 1))
    for q in range(P):
        mu = mu + part[:, :, q]
    return mu


def controller(cfg, ctrl, state):
    """ctrl [n][.], state [n][Z + 2] -> the output behind its tanh [n]: every unit from its bias, w * x added in ascending order, one
    multiply and one add per term."""
    import _oracle as O
    i, h = cfg["latent"] + 2, cfg["hidden"]
    x, at = np.asarray(state, f32), 0
    for n_in, n_out in ((i, h), (h, h // 2), (h // 2, 1)):
        w = ctrl[:, at:at + n_out * n_in].reshape(-1, n_out, n_in)
        at += n_out * n_in
        acc = ctrl[:, at:at + n_out].copy()
        at += n_out
        for k in range(n_in):
            acc = acc + w[:, :, k] * x[:, k, None]
        out = np.empty(acc.size, f32)
        O.lib().oracle_tanhf(np.ascontiguousarray(acc.reshape(-1)), out, acc.size)
        x = out.reshape(acc.shape)
    assert at == ctrl.shape[1]
    return x[:, 0]


def act(cfg, enc, ctrl, frames, rot, throttle=100.0, steer_scale=5.0):
    """dict(mu, state, out, throttle, steer) of every frame, by the rule."""
    import _oracle as O
    mu = encode(cfg, enc, frames)
    rot = np.ascontiguousarray(rot, f32)
    s, c = np.empty_like(rot), np.empty_like(rot)
    O.lib().oracle_sincosf(rot, s, c, rot.size)  # of the stored degrees, as the reference passes them
    state = np.concatenate([mu, s[:, None], c[:, None]], axis=1)
    out = controller(cfg, np.asarray(ctrl, f32), state)
    return dict(mu=mu, state=state, out=out, throttle=np.full(rot.size, throttle, f32), steer=out * f32(steer_scale))


def score(fitness, distance, crashed, timed_out):
    """One step of main.cpp:329-342 on float32 arrays; distance: RaceTrack::getDistanceToLaneCenter of every agent."""
    fitness = np.asarray(fitness, f32)
    crashed, timed_out = np.asarray(crashed) != 0, np.asarray(timed_out) != 0
    return np.where(~crashed, fitness + (f32(1.0) - np.asarray(distance, f32)), np.where(timed_out, f32(0.0), fitness)).astype(f32)


# ---- the plan, restated ----------------------------------------------------------------------------------------------------------------

def plan(cfg):
    out = []
    for l in range(4):
        blocks = 0 if l == 0 else -(-cin(cfg, l) // CHUNK)
        out.append((-(-cfg["channels"][l] // COLS), blocks, 64 if l == 0 else cin(cfg, l) - (blocks - 1) * CHUNK))
    return tuple(out)


def lds_bytes(cfg):
    return 4 * max(ROWS * LDA, AGENTS * (cfg["channels"][3] + 2))


def workspace_words(cfg, n):
    ne, nc = num_params(cfg)
    pack = 64 * cfg["channels"][0] + sum(16 * cin(cfg, l) * cfg["channels"][l] for l in (1, 2, 3)) + features(cfg) * cfg["latent"]
    words = (pack + n * nc + 3) // 4 * 4
    words += sum(n * sides(cfg)[l] ** 2 * cfg["channels"][l] for l in range(4)) + n * sides(cfg)[3] ** 2 * cfg["latent"]
    return words + n + n + 1 + ne
