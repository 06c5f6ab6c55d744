"""A float64 numpy mirror of the behavioural-cloning image policy's rule (include/okenv_cnn.h): the parameter layout, the forward pass
the kernels' LDS plan (openkitchen_amd/csrc/ok_cnn.h: okCnnPlaces) and their launch geometry, restated independently for the tests,
with the predicate each shape of the table was chosen for."""
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
    # ---- the paths the five shapes above leave out (REACHES below has each one's predicate) ----
    # 7 / 5 / 5, F = 400 = 256 + 144: a partial chunk of 9 groups behind a full one; k0 = 3 (9 taps and 3 fillers); stride 3 on the
    # frame, whose row and column 21 no window reads; a pointwise layer 2; nine head tiles, the second of a wave on wave 0 alone
    "ragged_chunk": dict(image_size=22, kernel=(3, 3, 1), stride=(3, 1, 1), channels=(16, 16, 16), hidden=144),
    # 17 / 8 / 7, F = 784 = 3 x 256 + 16: the last chunk a single group; k0 = 1 (one tap, three fillers from the first advance on);
    # 128 channels into layer 1 (32 groups, the walk's channel wrap after eight); 289 rows of layer 0 in ten row blocks, one live row
    # in the last; eight head tiles on eight waves; the largest LDS of the table
    "one_group_tail": dict(image_size=17, kernel=(1, 2, 2), stride=(1, 2, 1), channels=(128, 16, 16), hidden=128),
    # 5 / 4 / 3, F = 288 = 256 + 32: k0 = 7 (13 groups, 3 fillers); 128 columns in layer 1, 128 channels into layer 2; a tail chunk of
    # two groups; 17 head tiles, the third of a wave on wave 0 alone
    "wide_inputs": dict(image_size=16, kernel=(7, 2, 2), stride=(2, 1, 1), channels=(16, 128, 32), hidden=272),
    # 14 / 7 / 1, F = 128: k0 = 6 (9 groups, no filler); a layer 1 of 64 taps; stride 4 under k = 4 in layer 2, onto one position; 128
    # columns in layer 2; one partial chunk of 8 groups; 24 head tiles, three a wave exactly
    "long_chains": dict(image_size=32, kernel=(6, 8, 4), stride=(2, 1, 4), channels=(16, 32, 128), hidden=384),
    # 8 / 2 / 1, F = 16: k0 = 2 (one group, no filler); stride 4 in layer 1; 25 head tiles, the fourth of a wave on wave 0 alone
    "four_tiles_one_wave": dict(image_size=16, kernel=(2, 4, 2), stride=(2, 4, 1), channels=(16, 16, 16), hidden=400),
}
# okenv_cnn_plan: (tiles of 16 hidden units a wave of the head kernel owns -- its four forms; what sizes the conv kernel's first LDS
# region: 0 the frame, 1 layer 1's output)
PATHS = {"tiny": (1, 1), "odd": (1, 0), "wide": (4, 1), "reference": (2, 0), "three_tiles": (3, 1), "ragged_chunk": (2, 0),
         "one_group_tail": (1, 1), "wide_inputs": (3, 1), "long_chains": (3, 1), "four_tiles_one_wave": (4, 0)}
SIDES = {"tiny": (7, 5, 4), "odd": (8, 3, 1), "wide": (20, 20, 6), "reference": (23, 10, 8), "three_tiles": (7, 5, 4), "ragged_chunk": (7, 5, 5),
         "one_group_tail": (17, 8, 7), "wide_inputs": (5, 4, 3), "long_chains": (14, 7, 1), "four_tiles_one_wave": (8, 2, 1)}


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


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------------
# From the kernels' prose (openkitchen_amd/csrc/ok_conv.h, ok_cnn.h), not by calling the library: tests/test_cnn_rule.py pins the
# constants and the okConv instantiations it rests on to the source text.

THREADS, ROW_BLOCK = 512, 2  # kConvThreads: WAVES waves of 64 lanes; kConvRowBlock: the row tiles of 16 pixels a wave carries at a time


def conv_geometry(cfg, l):
    """Layer l of the conv kernel, one frame per workgroup: a unit is 16 columns by a row block of 16 x ROW_BLOCK output pixels; wave w
    takes units w, w + WAVES, ...; a chain runs in groups of 16 k's (layer 0: four k's a tap -- R, G, B and the alpha slot -- and filler
    taps up to a whole group; layers 1 and 2: a tap's channels 16 at a time)."""
    M, rows = sides(cfg)[l] ** 2, 16 * ROW_BLOCK
    blocks = -(-M // rows)
    units = cfg["channels"][l] // 16 * blocks
    rounds = -(-units // WAVES)
    taps = cfg["kernel"][l] ** 2
    groups = -(-taps // 4) if l == 0 else taps * cin(cfg, l) // 16
    return dict(M=M, blocks=blocks, units=units, rounds=rounds, idle_waves=rounds * WAVES - units, last_rows=M - (blocks - 1) * rows, taps=taps,
                groups=groups, fillers=4 * groups - taps if l == 0 else 0, groups_a_tap=0 if l == 0 else cin(cfg, l) // 16)


def geometry(cfg, agents=1):
    """The two launches of an act of `agents` agents: the three layers of the conv kernel (conv_geometry), and the head kernel --
    AGENTS agents a workgroup, a wave owning tiles w, w + WAVES, ... of the H / 16 column tiles, the features staged CHUNK at a time."""
    tiles, F = cfg["hidden"] // 16, features(cfg)
    a_wave, chunks, blocks = -(-tiles // WAVES), -(-F // CHUNK), -(-agents // AGENTS)
    return dict(conv=[conv_geometry(cfg, l) for l in range(3)], conv_blocks=agents, tiles=tiles, tiles_a_wave=a_wave,
                last_tile_waves=tiles - (a_wave - 1) * WAVES, chunks=chunks, last_chunk_groups=(F - (chunks - 1) * CHUNK) // 16, head_blocks=blocks,
                last_block_agents=agents - (blocks - 1) * AGENTS)


NEW_SHAPES = ("ragged_chunk", "one_group_tail", "wide_inputs", "long_chains", "four_tiles_one_wave")
# name: (the agents of its device case -- the first of them where it has several; the path the shape exists for, as a predicate on
# (shape, geometry(shape, agents))).  tests/test_cnn_rule.py asserts every one, and every device case asserts its own first.
REACHES = {
    # one whole chunk, one tile a wave and four groups without a filler in layer 0; 49 and 25 rows: a last row block of 17 and 25 live rows
    "tiny": (1, lambda s, g: (g["chunks"], g["last_chunk_groups"], g["tiles_a_wave"]) == (1, 16, 1) and (g["conv"][0]["groups"], g["conv"][0]["fillers"]) == (4, 0)
             and [c["last_rows"] for c in g["conv"]] == [17, 25, 16]),
    # k0 = 8 under stride 4 with frame row 36 unread; layer 2 a single position: one lone partial chunk of one group; two tiles on two waves
    "odd": (1, lambda s, g: (s["image_size"] - s["kernel"][0]) % s["stride"][0] == 1 and g["conv"][2]["M"] == 1 and (g["chunks"], g["last_chunk_groups"]) == (1, 1)
            and (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (2, 1, 2) and g["conv"][0]["groups"] == 16),
    # 18 whole chunks; four tiles a wave on every wave; a pointwise layer 1; stride = kernel in layer 2; k0 = 5: 7 groups, 3 fillers
    "wide": (5, lambda s, g: (g["chunks"], g["last_chunk_groups"]) == (18, 16) and (g["tiles_a_wave"], g["last_tile_waves"]) == (4, 8) and g["conv"][1]["taps"] == 1
             and s["stride"][2] == s["kernel"][2] == 3 and (g["conv"][0]["groups"], g["conv"][0]["fillers"]) == (7, 3) and g["conv"][0]["groups_a_tap"] == 0),
    # 16 whole chunks; two tiles a wave on every wave; 529 rows of layer 0 in 17 row blocks
    "reference": (3, lambda s, g: (g["chunks"], g["last_chunk_groups"]) == (16, 16) and (g["tiles_a_wave"], g["last_tile_waves"]) == (2, 8)
                  and (g["conv"][0]["blocks"], g["conv"][0]["last_rows"]) == (17, 17)),
    # 20 tiles: three a wave, the last on waves 0 .. 3; two whole chunks
    "three_tiles": (2, lambda s, g: (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (20, 3, 4) and (g["chunks"], g["last_chunk_groups"]) == (2, 16)),
    "ragged_chunk": (17, lambda s, g: (g["chunks"], g["last_chunk_groups"]) == (2, 9) and (g["conv"][0]["groups"], g["conv"][0]["fillers"]) == (3, 3)
                     and s["stride"][0] == 3 and (s["image_size"] - s["kernel"][0]) % 3 == 1 and g["conv"][2]["taps"] == 1
                     and (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (9, 2, 1) and (g["head_blocks"], g["last_block_agents"]) == (2, 1)),
    "one_group_tail": (2, lambda s, g: g["chunks"] == 4 and g["last_chunk_groups"] == 1 and g["conv"][0]["groups"] == 1 and g["conv"][0]["fillers"] == 3
                       and (g["conv"][1]["groups_a_tap"], g["conv"][1]["groups"]) == (8, 32) and (g["conv"][0]["M"], g["conv"][0]["blocks"], g["conv"][0]["last_rows"]) == (289, 10, 1)
                       and (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (8, 1, 8) and lds_bytes(s) == max(lds_bytes(v) for v in SHAPES.values())),
    "wide_inputs": (3, lambda s, g: (g["conv"][0]["groups"], g["conv"][0]["fillers"]) == (13, 3) and s["channels"][1] == 128 and g["conv"][2]["groups_a_tap"] == 8
                    and (g["chunks"], g["last_chunk_groups"]) == (2, 2) and (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (17, 3, 1)),
    "long_chains": (2, lambda s, g: (g["conv"][0]["groups"], g["conv"][0]["fillers"]) == (9, 0) and g["conv"][1]["taps"] == 64 and (s["stride"][2], s["kernel"][2]) == (4, 4)
                    and g["conv"][2]["M"] == 1 and s["channels"][2] == 128 and (g["chunks"], g["last_chunk_groups"]) == (1, 8)
                    and (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (24, 3, 8)),
    "four_tiles_one_wave": (17, lambda s, g: (g["conv"][0]["groups"], g["conv"][0]["fillers"]) == (1, 0) and s["stride"][1] == 4
                            and (g["tiles"], g["tiles_a_wave"], g["last_tile_waves"]) == (25, 4, 1) and (g["chunks"], g["last_chunk_groups"]) == (1, 1)
                            and (g["head_blocks"], g["last_block_agents"]) == (2, 1)),
}


def reaches(name, agents=None):
    """The shape's predicate at its case's population (or at `agents`)."""
    n, path = REACHES[name]
    return path(SHAPES[name], geometry(SHAPES[name], n if agents is None else agents))
