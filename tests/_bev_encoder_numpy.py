"""A float64 numpy mirror of the image encoder's rule (include/okenv_bev.h): the parameter layout, the forward pass, the conv
kernels' LDS plan (openkitchen_amd/csrc/ok_bev.h: okBevPlaces) and their launch geometry, restated independently for the tests, with
the predicate each shape of the table was chosen for."""
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
    # ---- the paths the five shapes above leave out (REACHES below has each one's predicate); all four have sides 20 / 10 / 5 but
    # back8_ragged's 40 / 20 / 10 ----
    # the front kernel on tiles of 4 with a partial last tile: three a side, 4, 4 and 2 wide; the back kernel on one tile of 8, 5 wide
    "front4_ragged": dict(image_size=40, kernel=(3, 5, 3), channels=(128, 16, 16), embed_dim=16),
    # the back kernel on tiles of 4 (128 channels with k2 = 5 leave no room for a tile of 8) with several tiles: two a side, 4 and 1 wide
    "back4_tiles": dict(image_size=40, kernel=(3, 3, 5), channels=(16, 128, 16), embed_dim=16),
    # tiles of 8 in both kernels, the last partial behind full ones: the front 8, 8 and 4 wide with tile (1, 1) reading no padding in
    # either of its patches, the back 8 and 2
    "back8_ragged": dict(image_size=80, kernel=(3, 3, 3), channels=(16, 16, 16), embed_dim=16),
    # tiles of 4 in both kernels, several of each: three a side in front, two behind
    "both4_tiles": dict(image_size=40, kernel=(5, 5, 5), channels=(128, 128, 32), embed_dim=48),
}
PATHS = {"tiny": (4, 4), "odd": (8, 8), "reference": (8, 8), "mixed": (8, 4), "front4_back8": (4, 8), "front4_ragged": (4, 8), "back4_tiles": (8, 4),
         "back8_ragged": (8, 8), "both4_tiles": (4, 4)}


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


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------------
# From the kernels' prose (openkitchen_amd/csrc/ok_bev.h, ok_conv.h), not by calling the library: tests/test_bev_encoder_rule.py pins
# the constants, the okConv instantiations and the two choices of okBevPlaces it rests on to the source text.

THREADS, WAVES = 256, 4  # kBevThreads, kBevWaves
LAYER0_ROW_TILES = 4     # the row tiles of 16 pixels a wave of layer 0 carries at a time: row blocks of 64 rows


def tile_geometry(side, T, patches):
    """A kernel whose workgroups each make one T x T tile of an output `side` wide.  patches: per patch of its input that the
    workgroup fills, (the side of the image it is cut from, origin(t) of the patch of tile t along one axis, the patch's side)."""
    n = -(-side // T)
    inside = [t for t in range(n) if all(0 <= origin(t) and origin(t) + p <= of for of, origin, p in patches)]
    return dict(T=T, tiles=n, last_width=side - (n - 1) * T, interior=bool(inside), interior_tiles=inside, row_tiles=T * T // 16)


def geometry(cfg, agents=1):
    """The front kernel (layers 0 and 1: a tile of layer 1's output, the region of layer 0's output under it with its halo, the frame's
    patch under that) and the back kernel (layer 2: a tile of its output, the patch of layer 1's output under it) at `agents` frames."""
    S, (k0, k1, k2), (ta, tb) = cfg["image_size"], cfg["kernel"], tiles(cfg)
    side0, side1, side2 = S // 2, S // 4, S // 8
    p1, p2 = 2 * (ta - 1) + k1, 2 * (tb - 1) + k2
    p0 = 2 * (p1 - 1) + k0
    front = tile_geometry(side1, ta, [(side0, lambda t: 2 * ta * t - k1 // 2, p1), (S, lambda t: 2 * (2 * ta * t - k1 // 2) - k0 // 2, p0)])
    back = tile_geometry(side2, tb, [(side1, lambda t: 2 * tb * t - k2 // 2, p2)])
    rows0 = p1 * p1
    return dict(front=front, back=back, front_blocks=agents * front["tiles"] ** 2, back_blocks=agents * back["tiles"] ** 2, layer0_rows=rows0,
                layer0_row_blocks=-(-rows0 // (16 * LAYER0_ROW_TILES)), layer0_last_rows=rows0 - (-(-rows0 // (16 * LAYER0_ROW_TILES)) - 1) * 16 * LAYER0_ROW_TILES,
                head_blocks=agents)


NEW_SHAPES = ("front4_ragged", "back4_tiles", "back8_ragged", "both4_tiles")
# The seeds of the host entry's comparison with forward() (tests/test_bev_encoder_rule.py), per shape the first four from 0 upward at
# which forward() alone passes at least half of every layer's outputs through its ReLU: a 16-channel layer 1 behind 128 channels clamps
# more at seeds 1 and 3 (0.36 .. 0.37 and 0.48 .. 0.49 of layer 1 for front4_back8 and front4_ragged), both4_tiles gives 0.470 of layer 1
# at seed 1 and 799 of layer 2's 1600 at seed 2, and back4_tiles just passes at seed 0 (402 of layer 2's 800).  (The two near counts do
# not hang on the order of a float64 sum: the smallest output that passes is 5.7e-5 and 5.1e-4 there.)  The test asserts the condition
# at the seeds listed and its failure at every seed skipped.
HOST_SEEDS = {"tiny": (0, 1, 2, 3), "odd": (0, 1, 2, 3), "reference": (0, 1, 2, 3), "mixed": (0, 1, 2, 3), "front4_back8": (0, 2, 4, 5),
              "front4_ragged": (0, 2, 4, 5), "back4_tiles": (0, 1, 2, 3), "back8_ragged": (0, 1, 2, 3), "both4_tiles": (0, 3, 4, 5)}


def passes_half(cfg, seed):
    """forward() alone on the test's draw of `seed`: does every layer pass at least half of its outputs through its ReLU?"""
    _, acts = forward(cfg, draw_params(cfg, seed), draw_frames(cfg["image_size"], seed), layers=True)
    return all(float((a > 0).mean()) >= 0.5 for a in acts)


def ft(g):
    return (g["front"]["T"], g["front"]["tiles"], g["front"]["last_width"])


def bt(g):
    return (g["back"]["T"], g["back"]["tiles"], g["back"]["last_width"])


# name: (the frames of its device case -- the first of them where it has several; the path the shape exists for, as a predicate on
# (shape, geometry(shape, frames))).  tests/test_bev_encoder_rule.py asserts every one, and every device case asserts its own first.
REACHES = {
    # every layer below a tile: one tile of 4 a frame in both kernels, 2 and 4 wide
    "tiny": (1, lambda s, g: ft(g) == (4, 1, 4) and bt(g) == (4, 1, 2) and (g["front"]["row_tiles"], g["back"]["row_tiles"]) == (1, 1)),
    # tiles of 8, partial at every edge: 8 and 2 in front, one of 5 behind; k = 5 throughout; no tile without padding
    "odd": (1, lambda s, g: ft(g) == (8, 2, 2) and bt(g) == (8, 1, 5) and set(s["kernel"]) == {5} and not g["front"]["interior"] and not g["back"]["interior"]),
    # exact tiles of 8: 4 x 4 in front, two of them a side without padding, 2 x 2 behind; four row tiles a unit
    "reference": (3, lambda s, g: ft(g) == (8, 4, 8) and bt(g) == (8, 2, 8) and g["front"]["interior_tiles"] == [1, 2] and g["front"]["row_tiles"] == 4),
    # the front on one tile of 8 (6 wide), the back on one tile of 4 (3 wide): 128 channels under k2 = 3 fit, but side 3 is below 5
    "mixed": (5, lambda s, g: ft(g) == (8, 1, 6) and bt(g) == (4, 1, 3) and s["channels"][1] == 128 and s["image_size"] // 8 <= 4),
    # the front on exact tiles of 4 because a tile of 8 does not fit, the back on one tile of 8
    "front4_back8": (2, lambda s, g: ft(g) == (4, 3, 4) and bt(g) == (8, 1, 6) and 4 * front_floats(s, 8) > LDS_BUDGET and s["image_size"] // 4 > 4),
    "front4_ragged": (2, lambda s, g: ft(g) == (4, 3, 2) and bt(g) == (8, 1, 5) and 4 * front_floats(s, 8) > LDS_BUDGET and g["front"]["row_tiles"] == 1
                      and (g["layer0_rows"], g["layer0_row_blocks"], g["layer0_last_rows"]) == (121, 2, 57)),
    "back4_tiles": (3, lambda s, g: ft(g) == (8, 2, 2) and bt(g) == (4, 2, 1) and 4 * back_floats(s, 8) == 186656 > LDS_BUDGET and s["image_size"] // 8 > 4
                    and g["back"]["row_tiles"] == 1 and g["back_blocks"] == 12),  # (three frames: a workgroup's frame is b / 4 of 0 .. 11)
    "back8_ragged": (2, lambda s, g: ft(g) == (8, 3, 4) and bt(g) == (8, 2, 2) and g["front"]["interior_tiles"] == [1] and not g["back"]["interior"]
                     and g["back"]["row_tiles"] == 4),
    "both4_tiles": (2, lambda s, g: ft(g) == (4, 3, 2) and bt(g) == (4, 2, 1) and 4 * front_floats(s, 8) > LDS_BUDGET and 4 * back_floats(s, 8) > LDS_BUDGET
                    and lds_bytes(s) == max(lds_bytes(SHAPES[n]) for n in NEW_SHAPES)),
}


def reaches(name, agents=None):
    """The shape's predicate at its case's population (or at `agents`)."""
    n, path = REACHES[name]
    return path(SHAPES[name], geometry(SHAPES[name], n if agents is None else agents))
