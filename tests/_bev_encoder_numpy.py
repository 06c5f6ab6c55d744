"""A float64 numpy mirror of the image encoder's rule (include/okenv_bev.h): the parameter layout, the forward pass and the conv
kernels' LDS plan (openkitchen_amd/csrc/ok_bev.h: okBevPlaces), restated independently for the tests."""
import numpy as np

LDS_BUDGET = 160 * 1024

# name -> members of capi.bev_config; `tiles` is the path of the two conv kernels the shape reaches (okenv_bev_tiles): the side of
# the output tile of the front (layers 0 and 1) and of the back (layer 2) kernel
SHAPES = {
    "tiny": dict(image_size=16, kernel=(3, 3, 3), channels=(16, 16, 16), embed_dim=16),        # layer sides 8 / 4 / 2, below any tile
    "odd": dict(image_size=40, kernel=(5, 5, 5), channels=(16, 32, 48), embed_dim=32),         # 20 / 10 / 5: partial tiles everywhere
    "reference": dict(image_size=128, kernel=(5, 3, 3), channels=(32, 64, 128), embed_dim=128),
    "mixed": dict(image_size=24, kernel=(3, 5, 3), channels=(16, 128, 16), embed_dim=512),     # 12 / 6 / 3
    # the front kernel's 8 x 8 tile does not fit the LDS with 128 channels and k1 = 5 (19 x 19 x 129 floats), the back kernel's does
    "front4_back8": dict(image_size=48, kernel=(3, 5, 3), channels=(128, 16, 16), embed_dim=16),
}
PATHS = {"tiny": (4, 4), "odd": (8, 8), "reference": (8, 8), "mixed": (8, 4), "front4_back8": (4, 8)}


def cin(cfg, l):
    return 3 if l == 0 else cfg["channels"][l - 1]


def layout(cfg):
    """(name, offset, shape) of every piece of the parameter vector, torch's parameters() order of the reference's BEVEncoder."""
    out, at = [], 0
    pieces = []
    for l in range(3):
        k, c = cfg["kernel"][l], cfg["channels"][l]
        pieces += [("conv.%d.weight" % (2 * l), (c, cin(cfg, l), k, k)), ("conv.%d.bias" % (2 * l), (c,))]
    pieces += [("proj.weight", (cfg["embed_dim"], cfg["channels"][2])), ("proj.bias", (cfg["embed_dim"],))]
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
    in [b / 2, b] -- of torch's scale but positive, so that more than half of every layer's outputs pass its ReLU
    (test_bev_encoder_rule asserts it)."""
    rng = np.random.default_rng(1000 + seed)
    out = np.empty(num_params(cfg), np.float32)
    for name, at, shape in layout(cfg):
        n = int(np.prod(shape))
        fan_in = int(np.prod(shape[1:])) if name.endswith("weight") else None
        if fan_in is None:  # the bias of the weight in front of it
            out[at:at + n] = rng.uniform(0.5 * bound, bound, n)
        else:
            bound = 1.0 / np.sqrt(fan_in)
            out[at:at + n] = rng.uniform(-bound, bound, n)
    return out


def rendered_frame(S, seed):
    """A frame as the camera makes them: large regions of one colour (a background, a band of track, a car), alpha 255."""
    rng = np.random.default_rng(2000 + seed)
    f = np.empty((S, S, 4), np.uint8)
    f[...] = (34, 139, 34, 255)
    a, b = sorted(rng.integers(0, S, 2))
    f[:, a:max(b, a + 2)] = (90, 90, 90, 255)
    y, x = rng.integers(0, S - 4, 2)
    f[y:y + 4, x:x + 3] = (255, 0, 0, 255)
    return f


def draw_frames(S, seed, n=2):
    """n frames: random bytes, and from the second on rendered-looking ones."""
    rng = np.random.default_rng(3000 + seed)
    frames = rng.integers(0, 256, (n, S, S, 4), dtype=np.uint8)
    for i in range(1, n, 2):
        frames[i] = rendered_frame(S, seed + i)
    return frames


def conv(x, w, b):
    """x [n][Cin][side][side], w [Cout][Cin][k][k]: stride 2, padding k // 2, float64."""
    k, p = w.shape[2], w.shape[2] // 2
    side = x.shape[2] // 2
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    out = np.tile(b.astype(np.float64)[None, :, None, None], (x.shape[0], 1, side, side))
    for ty in range(k):
        for tx in range(k):
            out += np.einsum("ncyx,oc->noyx", xp[:, :, ty:ty + 2 * side:2, tx:tx + 2 * side:2], w[:, :, ty, tx].astype(np.float64))
    return out


def forward(cfg, params, frames, layers=False):
    """frames [n][S][S][4] uint8 -> [n][E] float64 (layers: and the three layers' outputs behind their ReLU)."""
    p = split(cfg, np.asarray(params, np.float64))
    x = np.asarray(frames)[..., :3].astype(np.float64).transpose(0, 3, 1, 2) / 255.0
    acts = []
    for l in range(3):
        x = np.maximum(conv(x, p["conv.%d.weight" % (2 * l)], p["conv.%d.bias" % (2 * l)]), 0.0)
        acts.append(x)
    pooled = x.reshape(x.shape[0], x.shape[1], -1).sum(axis=2) / float(x.shape[2] * x.shape[3])
    out = pooled @ p["proj.weight"].T + p["proj.bias"]
    return (out, acts) if layers else out


# ---- the LDS plan, restated ----------------------------------------------------------------------------------------------------------

def row_stride(side, ld):
    """Floats between the rows of an LDS tile: at least side * ld and 8 mod 16."""
    return (side * ld + 7) // 16 * 16 + 8


def front_floats(cfg, t):
    p1 = 2 * (t - 1) + cfg["kernel"][1]
    p0 = 2 * (p1 - 1) + cfg["kernel"][0]
    return 3 * p0 * p0 + p1 * row_stride(p1, cfg["channels"][0] + 1)


def back_floats(cfg, t):
    p2 = 2 * (t - 1) + cfg["kernel"][2]
    return p2 * row_stride(p2, cfg["channels"][1] + 1)


def tiles(cfg):
    S = cfg["image_size"]
    ta = 8 if S // 4 > 4 and 4 * front_floats(cfg, 8) <= LDS_BUDGET else 4
    tb = 8 if S // 8 > 4 and 4 * back_floats(cfg, 8) <= LDS_BUDGET else 4
    return ta, tb


def lds_bytes(cfg):
    ta, tb = tiles(cfg)
    return 4 * max(front_floats(cfg, ta), back_floats(cfg, tb))
