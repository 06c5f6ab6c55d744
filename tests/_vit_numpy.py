"""Float64 mirror of the image transformer driver's rule (include/okenv_vit.h), in numpy: the same network on the same flat parameter
vector, every sum in double precision and in numpy's order.  It pins WHAT is computed (parameter order, pre-norm, the qkv split, GELU,
eps, the class token, the input's normalisation, the clamp); the fp32 summation orders are pinned by the device-against-host tests.
Behind it a restatement of the device's LDS plan, workspace and launch geometry (openkitchen_amd/csrc/ok_vit.h and the launches in
okenv_capi.hip), and the path each of the later shapes exists for (PATHS)."""
import math

import numpy as np

# S, P, D, heads, depth, feed-forward, head widths: what each shape is for is in the comments
SHAPES = {
    "tiny": dict(image_size=16, patch=8, dim=16, heads=1, depth=1, dim_feedforward=32, head_hidden1=16, head_hidden2=16),  # T 5: less than a tile
    "ten_tokens": dict(image_size=24, patch=8, dim=32, heads=2, depth=2, dim_feedforward=64, head_hidden1=16, head_hidden2=16),  # two heads, two blocks
    "second_tile": dict(image_size=32, patch=8, dim=48, heads=3, depth=1, dim_feedforward=96, head_hidden1=32, head_hidden2=16),  # T 17
    "patch4_dh64": dict(image_size=16, patch=4, dim=64, heads=1, depth=1, dim_feedforward=64, head_hidden1=16, head_hidden2=16),  # K 48; dh 64
    "long_rows": dict(image_size=224, patch=8, dim=16, heads=1, depth=1, dim_feedforward=16, head_hidden1=16, head_hidden2=16),  # T 785
    "reference_width": dict(image_size=32, patch=8, dim=384, heads=6, depth=1, dim_feedforward=1536, head_hidden1=128, head_hidden2=64),  # K 384, K 1536
    "reference_depth": dict(image_size=24, patch=8, dim=384, heads=6, depth=12, dim_feedforward=1536, head_hidden1=128, head_hidden2=64),  # 12 blocks, T 10
    # the paths the seven above never select; what each one reaches is in PATHS below and asserted by the tests that use it
    "dh32": dict(image_size=16, patch=8, dim=64, heads=2, depth=1, dim_feedforward=64, head_hidden1=16, head_hidden2=16),
    "dh48": dict(image_size=16, patch=8, dim=96, heads=2, depth=2, dim_feedforward=48, head_hidden1=16, head_hidden2=16),
    "patch16": dict(image_size=32, patch=16, dim=16, heads=1, depth=1, dim_feedforward=16, head_hidden1=16, head_hidden2=16),
    "grid_2d": dict(image_size=32, patch=8, dim=80, heads=5, depth=2, dim_feedforward=208, head_hidden1=16, head_hidden2=16),
    "wide_head": dict(image_size=16, patch=8, dim=16, heads=1, depth=1, dim_feedforward=16, head_hidden1=2048, head_hidden2=16),
    "head2_wider": dict(image_size=16, patch=8, dim=32, heads=2, depth=1, dim_feedforward=32, head_hidden1=16, head_hidden2=48),
    "most_tokens": dict(image_size=124, patch=4, dim=64, heads=1, depth=1, dim_feedforward=16, head_hidden1=16, head_hidden2=16),
}
TOKENS = {"tiny": 5, "ten_tokens": 10, "second_tile": 17, "patch4_dh64": 17, "long_rows": 785, "reference_width": 17, "reference_depth": 10,
          "dh32": 5, "dh48": 5, "patch16": 5, "grid_2d": 17, "wide_head": 5, "head2_wider": 5, "most_tokens": 962}
NEW_SHAPES = ("dh32", "dh48", "patch16", "grid_2d", "wide_head", "head2_wider", "most_tokens")

# ok_vit.h's constants
QUERIES, AGENTS, PAD, TILE, KBLOCK = 16, 16, 4, 64, 16
THREADS, LANES = 256, 8       # kVitThreads; OK_ACTOR_LANES: the lanes of a LayerNorm row
NORM_ROWS = THREADS // LANES  # kVitNormRows: the rows of a workgroup of okVitNormKernel and okVitEmbedKernel
LDS_BUDGET = 160 * 1024
DEFAULT_WORKSPACE = 1 << 30


def tokens(shape):
    return (shape["image_size"] // shape["patch"]) ** 2 + 1


def shape_bad(s):
    """ok_vit_shape_bad restated."""
    P, S, D = s["patch"], s["image_size"], s["dim"]
    if P not in (4, 8, 16) or S < P or S % P or tokens(s) > 1024:
        return True
    if D < 16 or D > 768 or D % 16 or s["heads"] < 1 or s["heads"] > D or D % s["heads"]:
        return True
    dh = D // s["heads"]
    if dh % 16 or dh > 64 or not 1 <= s["depth"] <= 12:
        return True
    if s["dim_feedforward"] < 16 or s["dim_feedforward"] > 4 * D or s["dim_feedforward"] % 16:
        return True
    return any(h < 16 or h > 2048 or h % 16 for h in (s["head_hidden1"], s["head_hidden2"]))


def lds_bytes(s):
    """okVitLdsBytes restated: the largest of the attention kernel's [q | softmax rows], the final kernel's [class tokens | hidden 1 |
    hidden 2] and the linear kernel's two staged tiles; 0 outside the limits."""
    if shape_bad(s):
        return 0
    T = tokens(s)
    Tp = (T + 15) // 16 * 16
    attend = QUERIES * (s["dim"] // s["heads"] + PAD + Tp + PAD)
    final = AGENTS * (s["dim"] + s["head_hidden1"] + s["head_hidden2"] + 3 * PAD)
    return 4 * max(attend, final, 2 * TILE * (KBLOCK + 4))


def linear_launch(rows, K, N):
    """One launch of okVitLinearKernel (vitLinear) of rows x K by K x N: its grid of 64 x 64 tiles, the ctiles of every column workgroup,
    the rows of the last row workgroup and how many of its four waves hold a row."""
    gx, gy = -(-rows // TILE), -(-N // TILE)
    last_rows = rows - (gx - 1) * TILE
    return dict(K=K, grid=(gx, gy), ctiles=[min(TILE // 16, (N - y * TILE) // 16) for y in range(gy)], last_rows=last_rows, last_live_waves=-(-last_rows // 16))


def geometry(s, count):
    """The launch geometry of one pass of `count` agents (vitBackbone, vitAct and vitEmbed in okenv_capi.hip) restated: every linear
    launch, the attention launch's workgroups, its dynamic LDS and the waves of its context phase, the workgroups of the norm, final
    and embed kernels and the final kernel's dynamic LDS."""
    T, D, F = tokens(s), s["dim"], s["dim_feedforward"]
    dh, M = D // s["heads"], count * T
    return dict(patch=linear_launch(count * (T - 1), 3 * s["patch"] ** 2, D), qkv=linear_launch(M, D, 3 * D), proj=linear_launch(M, D, D),
                fc1=linear_launch(M, D, F), fc2=linear_launch(M, F, D),
                attend_blocks=count * s["heads"] * (-(-T // QUERIES)), attend_lds=4 * QUERIES * (dh + PAD + -(-T // 16) * 16 + PAD), context_waves=dh // 16,
                norm_blocks=-(-M // NORM_ROWS), final_blocks=-(-count // AGENTS), embed_blocks=-(-count // NORM_ROWS),
                final_lds=4 * AGENTS * (D + s["head_hidden1"] + s["head_hidden2"] + 3 * PAD), final_last_agents=count - (-(-count // AGENTS) - 1) * AGENTS)


LINEARS = ("patch", "qkv", "proj", "fc1", "fc2")
# name: (the agents of the act case, the path the shape exists for as a predicate on (shape, geometry(shape, agents)))
PATHS = {
    "dh32": (2, lambda s, g: g["context_waves"] == 2 and s["heads"] == 2),  # the context on two waves, the second head starts at column 32
    "dh48": (2, lambda s, g: g["context_waves"] == 3 and s["heads"] == 2 and s["dim_feedforward"] < s["dim"]),  # three waves, a head at column 48
    # K 768 of the patch embedding's launch, the decode at P 16.  (geometry's K is held to the code elsewhere: test_launch_geometry_restated
    # has it equal the parameter layout's weight shape, test_plan_restated pins ok_vit_patch_k and the K vitBackbone passes to the source.)
    "patch16": (2, lambda s, g: s["patch"] == 16 and g["patch"]["K"] == 768),
    # several workgroups in x and in y in every linear launch; a short last column workgroup behind full ones; a last row workgroup of
    # 25 rows: wave 0 full, wave 1 partial, waves 2 and 3 dead
    "grid_2d": (9, lambda s, g: all(min(g[k]["grid"]) > 1 for k in LINEARS) and g["patch"]["grid"] == (3, 2) and g["qkv"]["grid"] == (3, 4)
                and g["qkv"]["ctiles"] == [4, 4, 4, 3] and g["fc1"]["ctiles"] == [4, 4, 4, 1] and g["proj"]["ctiles"] == g["fc2"]["ctiles"] == [4, 1]
                and g["qkv"]["last_rows"] == 25 and g["qkv"]["last_live_waves"] == 2),
    # okLidarLinear over 128 column tiles from the final kernel, its LDS the shape's largest; two workgroups, the second with one agent
    "wide_head": (17, lambda s, g: s["head_hidden1"] == 2048 and g["final_lds"] == lds_bytes(s) == 133888 and g["final_blocks"] == 2 and g["final_last_agents"] == 1),
    "head2_wider": (2, lambda s, g: s["head_hidden2"] > s["head_hidden1"]),
    "most_tokens": (1, lambda s, g: g["attend_lds"] == lds_bytes(s) == 67072 > 65536 and g["context_waves"] == 4),  # above 64 KB of dynamic LDS
}


def reaches(name, agents=None):
    """The shape's predicate at its case's population (or at `agents`)."""
    n, path = PATHS[name]
    return path(SHAPES[name], geometry(SHAPES[name], n if agents is None else agents))


def agent_floats(s):
    """ok_vit_agent_floats: x, n, ctx [T][D], qkv [T][3 D], hid [T][F]."""
    return tokens(s) * (6 * s["dim"] + s["dim_feedforward"])


def agents_per_pass(s, N, agents=0, workspace_bytes=0):
    """okVitAgentsPerPass restated."""
    if agents == 0:
        agents = max((workspace_bytes or DEFAULT_WORKSPACE) // (4 * agent_floats(s)), 1)
    return min(agents, max(N, 1))


def pieces(capi, cfg, params):
    params = np.asarray(params, dtype=np.float64).ravel()
    assert params.size == capi.vit_num_params(cfg)
    return {name: params[at:at + int(np.prod(shape))].reshape(shape) for name, at, shape in capi.vit_layout(cfg)}


def random_params(capi, cfg, rng, scale=1.0):
    """Torch-like magnitudes: weights uniform in +-scale / sqrt(fan_in), LayerNorm weights around 1, tokens of size 0.5."""
    out = np.empty(capi.vit_num_params(cfg), dtype=np.float64)
    for name, at, shape in capi.vit_layout(cfg):
        n = int(np.prod(shape))
        if "norm" in name and name.endswith("weight"):
            v = 1.0 + 0.1 * rng.standard_normal(n)
        elif "norm" in name:
            v = 0.1 * rng.standard_normal(n)
        elif name in ("cls_token", "pos_embed"):
            v = rng.uniform(-0.5, 0.5, n)
        elif name.endswith("bias"):
            v = rng.uniform(-0.1, 0.1, n)
        else:
            v = rng.uniform(-1.0, 1.0, n) * scale / np.sqrt(float(np.prod(shape[1:])))
        out[at:at + n] = v
    return out.astype(np.float32)


def layer_norm(v, g, b, eps):
    mean = v.mean(axis=-1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=-1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * g + b


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def frames_to_input(cfg, frames):
    """frames [n][S][S][4] uint8 -> [n][3][S][S] float64: (byte / 255 - mean) / std with the config's fp32 constants."""
    x = np.asarray(frames)[..., :3].astype(np.float64) / 255.0
    mean, std = np.array(list(cfg.mean), np.float64), np.array(list(cfg.std), np.float64)
    return ((x - mean) / std).transpose(0, 3, 1, 2)


def forward(capi, cfg, params, x):
    """x [n][3][S][S] -> (embedding [n][D], output [n]), float64."""
    p = pieces(capi, cfg, params)
    D, H, P = cfg.dim, cfg.heads, cfg.patch
    dh, side = D // H, cfg.image_size // cfg.patch
    n = x.shape[0]
    eps = float(np.float32(cfg.ln_eps))
    patches = x.reshape(n, 3, side, P, side, P).transpose(0, 2, 4, 1, 3, 5).reshape(n, side * side, 3 * P * P)
    tok = patches @ p["patch_embed.proj.weight"].reshape(D, -1).T + p["patch_embed.proj.bias"]
    h = np.concatenate([np.broadcast_to(p["cls_token"], (n, 1, D)), tok], axis=1) + p["pos_embed"]
    T = h.shape[1]
    for i in range(cfg.depth):
        pre = "blocks.%d." % i
        y = layer_norm(h, p[pre + "norm1.weight"], p[pre + "norm1.bias"], eps)
        qkv = (y @ p[pre + "attn.qkv.weight"].T + p[pre + "attn.qkv.bias"]).reshape(n, T, 3, H, dh).transpose(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(float(dh))
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        ctx = ((e / e.sum(axis=-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(n, T, D)
        h = h + ctx @ p[pre + "attn.proj.weight"].T + p[pre + "attn.proj.bias"]
        y = layer_norm(h, p[pre + "norm2.weight"], p[pre + "norm2.bias"], eps)
        f = gelu(y @ p[pre + "mlp.fc1.weight"].T + p[pre + "mlp.fc1.bias"])
        h = h + f @ p[pre + "mlp.fc2.weight"].T + p[pre + "mlp.fc2.bias"]
    emb = layer_norm(h[:, 0], p["norm.weight"], p["norm.bias"], eps)
    z = np.maximum(emb @ p["head.net.0.weight"].T + p["head.net.0.bias"], 0.0)
    z = np.maximum(z @ p["head.net.2.weight"].T + p["head.net.2.bias"], 0.0)
    return emb, (z @ p["head.output_layer.weight"].T + p["head.output_layer.bias"])[:, 0]


def attend(qkv, heads):
    """The attention piece in float64: qkv [seqs][T][3 D] -> ctx [seqs][T][D]."""
    qkv = np.asarray(qkv, np.float64)
    n, T, W = qkv.shape
    D = W // 3
    dh = D // heads
    q, k, v = qkv.reshape(n, T, 3, heads, dh).transpose(2, 0, 3, 1, 4)
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(float(dh))
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return ((e / e.sum(axis=-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(n, T, D)
