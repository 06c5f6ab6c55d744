"""A float64 numpy mirror of the behavioural-cloning image policy's rule (include/okenv_cnn.h): the parameter layout, the forward pass
and the kernels' LDS plan (openkitchen_amd/csrc/ok_cnn.h: okCnnPlaces), restated independently for the tests."""
import numpy as np

LDS_BUDGET = 160 * 1024
WAVES, AGENTS, CHUNK = 8, 16, 256  # of the head kernel: its waves, the agents of a workgroup, the features staged at a time

# name -> the shape members of capi.cnn_config
SHAPES = {
    # sides 7 / 5 / 4: F = 256; 49, 25 and 16 rows, of which 49 and 25 are no multiple of 16; one 16-column tile throughout
    "tiny": dict(image_size=16, kernel=(4, 3, 2), stride=(2, 1, 1), channels=(16, 16, 16), hidden=16),
    # 8 / 3 / 1: frame column and row 36 reached by no window; layer 1 with 9 rows; layer 2 a single position, F = c2
    "odd": dict(image_size=37, kernel=(8, 4, 3), stride=(4, 2, 1), channels=(16, 32, 16), hidden=32),
    # 20 / 20 / 6: stride 1 on the frame; a pointwise layer; stride = kernel with two columns dropped; the widest against the narrowest
    # channel count; the widest hidden layer; F = 4608
    "wide": dict(image_size=24, kernel=(5, 1, 3), stride=(1, 1, 3), channels=(64, 16, 128), hidden=512),
    "reference": dict(image_size=96, kernel=(8, 4, 3), stride=(4, 2, 1), channels=(32, 64, 64), hidden=256),  # 23 / 10 / 8, F = 4096
    # the head kernel's one form the four shapes above do not reach: three column tiles a wave, the last of them on waves 0 .. 3 only
    "three_tiles": dict(image_size=16, kernel=(4, 3, 2), stride=(2, 1, 1), channels=(16, 16, 32), hidden=320),
}
# okenv_cnn_plan: (tiles of 16 hidden units a wave of the head kernel owns -- its four forms; what sizes the conv kernel's first LDS
# region: 0 the frame, 1 layer 1's output)
PATHS = {"tiny": (1, 1), "odd": (1, 0), "wide": (4, 1), "reference": (2, 0), "three_tiles": (3, 1)}
SIDES = {"tiny": (7, 5, 4), "odd": (8, 3, 1), "wide": (20, 20, 6), "reference": (23, 10, 8), "three_tiles": (7, 5, 4)}


def cin(cfg, l):
    return 3 if l == 0 else cfg["channels"][l - 1]


def sides(cfg):
    side, out = cfg["image_size"], []
    for k, s in zip(cfg["kernel"], cfg["stride"]):
        side = (side - k) // s + 1
        out.append(side)
    return tuple(out)


def features(cfg):
    return cfg["channels"][2] * sides(cfg)[2] ** 2


def layout(cfg):
    """(name, offset, shape) of every piece of the parameter vector, torch's parameters() order of the reference's PolicyCNN."""
    pieces = []
    for l in range(3):
        k, c = cfg["kernel"][l], cfg["channels"][l]
        pieces += [("encoder.%d.weight" % (2 * l), (c, cin(cfg, l), k, k)), ("encoder.%d.bias" % (2 * l), (c,))]
    H = cfg["hidden"]
    pieces += [("steering_head.0.weight", (H, features(cfg))), ("steering_head.0.bias", (H,)), ("steering_head.2.weight", (1, H)),
               ("steering_head.2.bias", (1,))]
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
    in [b / 2, b] -- of torch's scale but positive, so that the layers' outputs pass their ReLU; the output layer's weights twice
    torch's scale, which keeps the output o between 0.01 and 3 in size (tests/test_cnn_rule.py asserts it)."""
    rng = np.random.default_rng(1000 + seed)
    out = np.empty(num_params(cfg), np.float32)
    for name, at, shape in layout(cfg):
        n = int(np.prod(shape))
        fan_in = int(np.prod(shape[1:])) if name.endswith("weight") else None
        if fan_in is None:  # the bias of the weight in front of it
            out[at:at + n] = rng.uniform(0.5 * bound, bound, n)
        else:
            bound = (2.0 if name == "steering_head.2.weight" else 1.0) / np.sqrt(fan_in)
            out[at:at + n] = rng.uniform(-bound, bound, n)
    return out


def draw_frames(S, seed, n=2):
    """n frames of random bytes."""
    return np.random.default_rng(3000 + seed).integers(0, 256, (n, S, S, 4), dtype=np.uint8)


def conv(x, w, b, stride):
    """x [n][Cin][side][side], w [Cout][Cin][k][k]: a valid convolution, float64."""
    k = w.shape[2]
    side = (x.shape[2] - k) // stride + 1
    out = np.tile(b.astype(np.float64)[None, :, None, None], (x.shape[0], 1, side, side))
    for ty in range(k):
        for tx in range(k):
            window = x[:, :, ty:ty + stride * (side - 1) + 1:stride, tx:tx + stride * (side - 1) + 1:stride]
            out += np.einsum("ncyx,oc->noyx", window, w[:, :, ty, tx].astype(np.float64))
    return out


def forward(cfg, params, frames):
    """frames [n][S][S][4] uint8 -> (o [n], tanh(o) [n]) in float64: the output layer's value and the policy's output."""
    p = split(cfg, np.asarray(params, np.float64))
    x = np.asarray(frames)[..., :3].astype(np.float64).transpose(0, 3, 1, 2) / 255.0
    for l in range(3):
        x = np.maximum(conv(x, p["encoder.%d.weight" % (2 * l)], p["encoder.%d.bias" % (2 * l)], cfg["stride"][l]), 0.0)
    h = np.maximum(x.reshape(x.shape[0], -1) @ p["steering_head.0.weight"].T + p["steering_head.0.bias"], 0.0)  # torch's flatten: (ch, y, x)
    o = (h @ p["steering_head.2.weight"].T + p["steering_head.2.bias"])[:, 0]
    return o, np.tanh(o)


# ---- the LDS plan, restated ----------------------------------------------------------------------------------------------------------

def plan(cfg):
    s = sides(cfg)
    frame, out1 = cfg["image_size"] ** 2, s[1] ** 2 * (cfg["channels"][1] + 1)
    return -(-(cfg["hidden"] // 16) // WAVES), 1 if out1 > frame else 0


def lds_bytes(cfg):
    s = sides(cfg)
    frame, out1 = cfg["image_size"] ** 2, s[1] ** 2 * (cfg["channels"][1] + 1)
    conv_floats = 256 + max(frame, out1) + s[0] ** 2 * (cfg["channels"][0] + 1)  # the pixel table, the frame or layer 1, layer 0
    head_floats = AGENTS * (CHUNK + 4) + AGENTS * (cfg["hidden"] + 4)
    return 4 * max(conv_floats, head_floats)
