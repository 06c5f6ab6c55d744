"""A float64 numpy mirror of the Deep-Q image racers' rule (include/okenv_qcnn.h): the parameter layout, the grey plane, the padded
forward pass, the frame ring's push and batch, and the kernels' LDS plan (openkitchen_amd/csrc/ok_qcnn.h: okQcnnPlaces), restated
independently for the tests."""
import numpy as np

LDS_BUDGET = 160 * 1024
WAVES, AGENTS, CHUNK = 8, 16, 256  # of the head kernel: its waves, the agents of a workgroup, the features staged at a time
GREY = (np.float32(0.2989), np.float32(0.5870), np.float32(0.1140))

# name -> the shape members of capi.qcnn_config
SHAPES = {
    # sides 8 / 8 / 8, F = 1024: the smallest of everything; 64 rows a layer
    "tiny": dict(image_size=16, kernel=(4, 3, 3), stride=(2, 1, 1), padding=(1, 1, 1), channels=(16, 16, 16), hidden=16, num_actions=2),
    # 7 / 5 / 4, F = 256: no border anywhere; row counts 49 and 25 are no multiple of 16
    "nopad": dict(image_size=16, kernel=(4, 3, 2), stride=(2, 1, 1), padding=(0, 0, 0), channels=(16, 16, 16), hidden=16, num_actions=3),
    # 9 / 4 / 4, F = 256: windows reach only part of the far border on layers 0 and 1 (remainders 1, 1, 0); S S is no multiple of 4
    "odd": dict(image_size=37, kernel=(8, 4, 3), stride=(4, 2, 1), padding=(2, 1, 1), channels=(16, 32, 16), hidden=32, num_actions=5),
    # 12 / 12 / 5, F = 3200: an unpadded pointwise layer between padded ones; stride 3 with a column left over; the widest H and A; the
    # widest against the narrowest channels
    "wide": dict(image_size=24, kernel=(5, 1, 3), stride=(2, 1, 3), padding=(2, 0, 2), channels=(64, 16, 128), hidden=512, num_actions=8),
    # 23 / 13 / 15, F = 3600: p = k - 1, corner windows see one real pixel; outputs larger than inputs
    "deep_pad": dict(image_size=20, kernel=(4, 4, 3), stride=(1, 2, 1), padding=(3, 3, 2), channels=(16, 16, 16), hidden=48, num_actions=4),
    # 24 / 12 / 12, F = 9216: the real shape; 137 KB of LDS
    "reference": dict(image_size=96, kernel=(8, 4, 3), stride=(4, 2, 1), padding=(2, 1, 1), channels=(32, 64, 64), hidden=512, num_actions=5),
    # the head kernel's two forms the shapes above do not reach: two and three column tiles a wave (the third on waves 0 .. 3 only)
    "two_tiles": dict(image_size=16, kernel=(4, 3, 3), stride=(2, 1, 1), padding=(1, 1, 1), channels=(16, 16, 16), hidden=256, num_actions=5),
    "three_tiles": dict(image_size=16, kernel=(4, 3, 2), stride=(2, 1, 1), padding=(0, 0, 0), channels=(16, 16, 32), hidden=320, num_actions=5),
}
# okenv_qcnn_plan: (tiles of 16 hidden units a wave of the head kernel owns; what sizes the conv kernel's first LDS region: 0 the grey
# plane, 1 layer 1's output; planes moved as 16-byte vectors)
PATHS = {"tiny": (1, 1, 1), "nopad": (1, 1, 1), "odd": (1, 0, 0), "wide": (4, 1, 1), "deep_pad": (1, 1, 1), "reference": (4, 1, 1),
         "two_tiles": (2, 1, 1), "three_tiles": (3, 1, 1)}
SIDES = {"tiny": (8, 8, 8), "nopad": (7, 5, 4), "odd": (9, 4, 4), "wide": (12, 12, 5), "deep_pad": (23, 13, 15), "reference": (24, 12, 12),
         "two_tiles": (8, 8, 8), "three_tiles": (7, 5, 4)}
FEATURES = {"tiny": 1024, "nopad": 256, "odd": 256, "wide": 3200, "deep_pad": 3600, "reference": 9216, "two_tiles": 1024, "three_tiles": 512}


def cin(cfg, l):
    return 1 if l == 0 else cfg["channels"][l - 1]


def sides(cfg):
    side, out = cfg["image_size"], []
    for k, s, p in zip(cfg["kernel"], cfg["stride"], cfg["padding"]):
        side = (side + 2 * p - k) // s + 1
        out.append(side)
    return tuple(out)


def features(cfg):
    return cfg["channels"][2] * sides(cfg)[2] ** 2


def layout(cfg):
    """(name, offset, shape) of every piece of the parameter vector, torch's parameters() order of the reference's CNN."""
    pieces = []
    for l in range(3):
        k, c = cfg["kernel"][l], cfg["channels"][l]
        pieces += [("conv%d.weight" % (l + 1), (c, cin(cfg, l), k, k)), ("conv%d.bias" % (l + 1), (c,))]
    H, A = cfg["hidden"], cfg["num_actions"]
    pieces += [("fc1.weight", (H, features(cfg))), ("fc1.bias", (H,)), ("fc2.weight", (A, H)), ("fc2.bias", (A,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def num_params(cfg):
    name, at, shape = layout(cfg)[-1]
    return at + int(np.prod(shape))


def split(cfg, params):
    return {name: np.asarray(params[at:at + int(np.prod(shape))]).reshape(shape) for name, at, shape in layout(cfg)}


def draw_params(cfg, seed):
    """A float32 parameter vector at torch's default init scale: weights uniform in [-b, b], b = 1 / sqrt(fan_in); the biases uniform
    in [b / 2, b] -- of torch's scale but positive, so that the layers' outputs pass their ReLU; fc2's weights twice torch's scale and
    its biases spread over [-b, b], which keeps the largest |q| between 0.01 and 3 and a frame's Q-values apart
    (tests/test_qcnn_rule.py asserts both)."""
    rng = np.random.default_rng(1000 + seed)
    out = np.empty(num_params(cfg), np.float32)
    for name, at, shape in layout(cfg):
        n = int(np.prod(shape))
        fan_in = int(np.prod(shape[1:])) if name.endswith("weight") else None
        if fan_in is None:  # the bias of the weight in front of it
            out[at:at + n] = rng.uniform(-bound, bound, n) if name == "fc2.bias" else rng.uniform(0.5 * bound, bound, n)
        else:
            bound = (2.0 if name == "fc2.weight" else 1.0) / np.sqrt(fan_in)
            out[at:at + n] = rng.uniform(-bound, bound, n)
    return out


def draw_frames(S, seed, n=2):
    """n frames of random bytes."""
    return np.random.default_rng(3000 + seed).integers(0, 256, (n, S, S, 4), dtype=np.uint8)


def grey32(frames):
    """The rule's grey in fp32, operation by operation: [n][S][S] float32."""
    x = np.asarray(frames)[..., :3].astype(np.float32) / np.float32(255.0)
    t = x[..., 0] * GREY[0]
    t = t + x[..., 1] * GREY[1]
    t = t + x[..., 2] * GREY[2]
    return t.astype(np.float32)


def grey64(frames):
    x = np.asarray(frames)[..., :3].astype(np.float64) / 255.0
    return x[..., 0] * float(GREY[0]) + x[..., 1] * float(GREY[1]) + x[..., 2] * float(GREY[2])


def conv(x, w, b, stride, pad):
    """x [n][Cin][side][side], w [Cout][Cin][k][k]: a zero-padded convolution, float64."""
    k = w.shape[2]
    x = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    side = (x.shape[2] - k) // stride + 1
    out = np.tile(b.astype(np.float64)[None, :, None, None], (x.shape[0], 1, side, side))
    for ty in range(k):
        for tx in range(k):
            window = x[:, :, ty:ty + stride * (side - 1) + 1:stride, tx:tx + stride * (side - 1) + 1:stride]
            out += np.einsum("ncyx,oc->noyx", window, w[:, :, ty, tx].astype(np.float64))
    return out


def forward_planes(cfg, params, planes):
    """planes [n][S][S] -> q [n][A] in float64."""
    p = split(cfg, np.asarray(params, np.float64))
    x = np.asarray(planes, np.float64)[:, None]
    for l in range(3):
        x = np.maximum(conv(x, p["conv%d.weight" % (l + 1)], p["conv%d.bias" % (l + 1)], cfg["stride"][l], cfg["padding"][l]), 0.0)
    h = np.maximum(x.reshape(x.shape[0], -1) @ p["fc1.weight"].T + p["fc1.bias"], 0.0)  # torch's flatten: (ch, y, x)
    return h @ p["fc2.weight"].T + p["fc2.bias"]


def forward(cfg, params, frames):
    """frames [n][S][S][4] uint8 -> q [n][A] in float64."""
    return forward_planes(cfg, params, grey64(frames))


# ---- the frame ring, restated ----------------------------------------------------------------------------------------------------------

def ring(capacity, S):
    return dict(state=np.zeros((capacity, S, S), np.float32), next_state=np.zeros((capacity, S, S), np.float32), action=np.zeros(capacity, np.int64),
                reward=np.zeros(capacity, np.float32), done=np.zeros(capacity, np.float32), pushed=0, capacity=capacity, image_size=S)


def clearance(crashed, dist):
    """ok_dqn_reward: -200 for a crashed agent, else the smallest distance, at most 200."""
    return np.float32(-200.0) if crashed else np.float32(min(200.0, float(np.min(dist))))


def push(r, action, alive, frames, next_frames, crashed, reward=None, dist=None, push_all=False):
    """One push, transition by transition as if pushed one at a time (the oldest of more than `capacity` are simply overwritten)."""
    state, nxt = grey32(frames), grey32(next_frames)
    for a in range(len(action)):
        if not (push_all or alive[a]):
            continue
        slot = r["pushed"] % r["capacity"]
        r["state"][slot], r["next_state"][slot], r["action"][slot] = state[a], nxt[a], action[a]
        r["done"][slot] = 1.0 if crashed[a] else 0.0
        r["reward"][slot] = reward[a] if reward is not None else clearance(crashed[a], dist[a])
        r["pushed"] += 1
    return r


def philox4x32(counter, key):
    """Philox4x32-10 on python ints."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def sample(seed, q, draw, size):
    """ok_dqn_sample: stream 7 of the project's Philox keying."""
    return (philox4x32((q, draw, 7, 0), (seed & 0xFFFFFFFF, 0x6F6B656E))[0] * size) >> 32


def batch(r, B, mode, start_or_draw=0, seed=0):
    C_, S = r["capacity"], r["image_size"]
    size = min(r["pushed"], C_)
    out = dict(state=np.zeros((B, S, S), np.float32), next_state=np.zeros((B, S, S), np.float32), action=np.zeros(B, np.int64),
               reward=np.zeros(B, np.float32), done=np.zeros(B, np.float32), index=np.zeros(B, np.int32))
    if size == 0:
        return out
    first = r["pushed"] - size
    for q in range(B):
        slot = sample(seed, q, start_or_draw, size) if mode == "uniform" else (first + (start_or_draw + q) % size) % C_
        for k in ("state", "next_state", "action", "reward", "done"):
            out[k][q] = r[k][slot]
        out["index"][q] = slot
    return out


# ---- the LDS plan, restated ------------------------------------------------------------------------------------------------------------

def _regions(cfg):
    s, p, c = sides(cfg), cfg["padding"], cfg["channels"]
    plane = (cfg["image_size"] + 2 * p[0]) ** 2                 # the grey plane inside its border
    out0 = (s[0] + 2 * p[1]) ** 2 * (c[0] + 1)                  # layer 0's output inside layer 1's border
    out1 = (s[1] + 2 * p[2]) ** 2 * (c[1] + 1)                  # layer 1's output inside layer 2's border
    return plane, out0, out1


def plan(cfg):
    plane, out0, out1 = _regions(cfg)
    return -(-(cfg["hidden"] // 16) // WAVES), 1 if out1 > plane else 0, 1 if cfg["image_size"] ** 2 % 4 == 0 else 0


def lds_bytes(cfg):
    plane, out0, out1 = _regions(cfg)
    conv_floats = max(plane, out1) + out0
    head_floats = AGENTS * (CHUNK + 4) + AGENTS * (cfg["hidden"] + 4)
    return 4 * max(conv_floats, head_floats)
