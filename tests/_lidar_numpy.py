"""Float64 mirror of the lidar transformer driver's rule (include/okenv_lidar.h), in numpy: the same network on the same flat
parameter vector, every sum in double precision and in numpy's order.  It pins WHAT is computed (parameter order, post-norm, the
head split, the scale, the positional table, the normalisations); the fp32 summation orders are pinned by the device-against-host
tests."""
import numpy as np

# the three shapes of the rule's tests: the reference's; one with dh = 8 (a scale that is no power of two) and a single layer; one in
# between with two layers.  Behind them the shapes chosen for the paths of the act kernel (openkitchen_amd/csrc/ok_lidar.h) that
# the first three never select; what each one reaches is in PATHS below and asserted by the tests that use it
SHAPES = {
    "reference": dict(num_points=7, d_model=128, nhead=8, num_layers=3, dim_feedforward=512, head_hidden1=256, head_hidden2=64),
    "tiny": dict(num_points=3, d_model=16, nhead=2, num_layers=1, dim_feedforward=16, head_hidden1=16, head_hidden2=16),
    "small": dict(num_points=7, d_model=32, nhead=2, num_layers=2, dim_feedforward=64, head_hidden1=32, head_hidden2=16),
    "unit_heads": dict(num_points=7, d_model=32, nhead=32, num_layers=1, dim_feedforward=64, head_hidden1=32, head_hidden2=16),
    "wide_group": dict(num_points=6, d_model=48, nhead=2, num_layers=2, dim_feedforward=80, head_hidden1=16, head_hidden2=96),
    "short_blocks": dict(num_points=5, d_model=80, nhead=5, num_layers=2, dim_feedforward=144, head_hidden1=48, head_hidden2=32),
    "two_tiles_a_head": dict(num_points=2, d_model=64, nhead=2, num_layers=1, dim_feedforward=16, head_hidden1=16, head_hidden2=16),
    "sixteen_points": dict(num_points=16, d_model=32, nhead=4, num_layers=1, dim_feedforward=64, head_hidden1=32, head_hidden2=16),
    "one_point": dict(num_points=1, d_model=16, nhead=1, num_layers=1, dim_feedforward=16, head_hidden1=256, head_hidden2=512),
}
OLD_SHAPES = ("reference", "tiny", "small")
NEW_SHAPES = tuple(name for name in SHAPES if name not in OLD_SHAPES)

# ok_lidar.h's constants; tests/test_lidar_rule.py keeps them in step with the header
AGENTS, THREADS, ROW_BLOCK, COL_BLOCK, PAD = 16, 256, 4, 64, 4


def blocks(n, size):
    """The pieces a loop `for (i = 0; i < n; i += size)` takes: full ones and a shorter last one."""
    return [min(size, n - i) for i in range(0, n, size)]


def plan(shape):
    """okLidarPlaces restated, with what the act kernel's loops make of the shape: the head group's width W and heads, the attention
    tasks of a group (dealt to THREADS threads), the row tiles a wave carries at a time, the column blocks of out_proj and of the
    feed-forward, which term sizes the LDS regions c and s, and the plan's bytes."""
    R, d, ff = shape["num_points"], shape["d_model"], shape["dim_feedforward"]
    dh = d // shape["nhead"]
    W = dh
    while W % 16 != 0:
        W += dh
    rows, ldx, ldq, ldb, ldp = R * AGENTS, d + PAD, W + PAD, COL_BLOCK + PAD, R | 1
    c_terms = {"activations": rows * ldx, "head1": AGENTS * (shape["head_hidden1"] + PAD)}
    s_terms = {"attention": 3 * rows * ldq + THREADS * ldp, "block": rows * ldb, "head2": AGENTS * (shape["head_hidden2"] + PAD),
               "inputs": 2 * rows}
    c_by, s_by = max(c_terms, key=c_terms.get), max(s_terms, key=s_terms.get)
    return dict(dh=dh, W=W, ff_under_d=ff < d, ldq=ldq, ldp=ldp, groups=d // W, heads=W // dh, tasks=AGENTS * (W // dh) * R, row_blocks=blocks(R, ROW_BLOCK),
                d_blocks=blocks(d, COL_BLOCK), ff_blocks=blocks(ff, COL_BLOCK), c_by=c_by, s_by=s_by,
                bytes=4 * (rows * ldx + c_terms[c_by] + s_terms[s_by]))


# What each new shape exists for, as a predicate on its plan: a later change of a constant that takes the path away fails the test
# that names the shape, before it compares anything
PATHS = {
    # d_head 1; a thread takes 7 attention tasks and reuses its softmax row; two head groups
    "unit_heads": lambda p: p["dh"] == 1 and p["heads"] == 16 and p["tasks"] == 1792 and p["tasks"] > 6 * THREADS and p["groups"] == 2,
    # three column tiles a group, head 1 starts inside the second; R even, so ldp != R; row blocks 4 + 2; a 16-wide block behind a full one
    "wide_group": lambda p: p["W"] == 48 and p["dh"] == 24 and p["dh"] % 16 != 0 and p["ldp"] == 7 and p["row_blocks"] == [4, 2]
    and p["ff_blocks"] == [64, 16],
    # out_proj 64 + 16; the feed-forward 64 + 64 + 16; okLidarUnit<1> as the tail of a row block
    "short_blocks": lambda p: p["d_blocks"] == [64, 16] and p["ff_blocks"] == [64, 64, 16] and p["row_blocks"] == [4, 1],
    # a head of two tiles; okLidarUnit<2> alone; a feed-forward narrower than d_model (the host entry keeps the context where the
    # hidden layer goes)
    "two_tiles_a_head": lambda p: p["dh"] == 32 and p["W"] == 32 and p["row_blocks"] == [2] and p["ff_under_d"],
    # R at its limit: four full row blocks, two passes of the attention loop, ldp 17, the plan just under the 160 KB
    "sixteen_points": lambda p: p["row_blocks"] == [4, 4, 4, 4] and p["tasks"] == 512 and p["ldp"] == 17 and 144 * 1024 < p["bytes"] <= 160 * 1024,
    # softmax over one key; the LDS regions sized by the head's hidden layers and not by the activations
    "one_point": lambda p: p["row_blocks"] == [1] and p["c_by"] == "head1" and p["s_by"] == "head2",
}


def pieces(capi, cfg, params):
    """{name: float64 array of its shape} of the flat vector."""
    params = np.asarray(params, dtype=np.float64).ravel()
    assert params.size == capi.lidar_num_params(cfg)
    return {name: params[at:at + int(np.prod(shape))].reshape(shape) for name, at, shape in capi.lidar_layout(cfg)}


def random_params(capi, cfg, rng, scale=1.0):
    """A parameter vector with torch-like magnitudes: weights uniform in +-scale / sqrt(fan_in), LayerNorm weights around 1, a
    token-dependent positional table."""
    out = np.empty(capi.lidar_num_params(cfg), dtype=np.float64)
    for name, at, shape in capi.lidar_layout(cfg):
        n = int(np.prod(shape))
        if ".norm" in name and name.endswith("weight"):
            v = 1.0 + 0.1 * rng.standard_normal(n)
        elif ".norm" in name:
            v = 0.1 * rng.standard_normal(n)
        elif name == "pos":
            v = rng.uniform(-1.0, 1.0, n)
        else:
            fan_in = shape[-1] if len(shape) == 2 else shape[0]
            v = rng.uniform(-1.0, 1.0, n) * scale / np.sqrt(fan_in if len(shape) == 2 else 4.0)
        out[at:at + n] = v
    return out.astype(np.float32)


def layer_norm(v, g, b):
    mean = v.mean(axis=-1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=-1, keepdims=True)
    return (v - mean) / np.sqrt(var + 1e-5) * g + b


def normalize_input(rel_xy, sensor_range=200.0):
    lo, hi = -sensor_range, sensor_range
    return 2.0 * (np.asarray(rel_xy, dtype=np.float64) - lo) / (hi - lo) - 1.0


def forward(capi, cfg, params, x):
    """x [n][R][2] normalised points -> o [n][2] normalised controls, float64."""
    p = pieces(capi, cfg, params)
    d, H = cfg.d_model, cfg.nhead
    dh = d // H
    x = np.asarray(x, dtype=np.float64)
    n, R = x.shape[0], x.shape[1]
    h = x @ p["point_embedding.weight"].T + p["point_embedding.bias"] + p["pos"]
    for i in range(cfg.num_layers):
        pre = "transformer_encoder.layers.%d." % i
        qkv = h @ p[pre + "self_attn.in_proj_weight"].T + p[pre + "self_attn.in_proj_bias"]
        q, k, v = (qkv[..., j * d:(j + 1) * d].reshape(n, R, H, dh).transpose(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(float(dh))
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        ctx = ((e / e.sum(axis=-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(n, R, d)
        y = ctx @ p[pre + "self_attn.out_proj.weight"].T + p[pre + "self_attn.out_proj.bias"]
        h = layer_norm(h + y, p[pre + "norm1.weight"], p[pre + "norm1.bias"])
        f = np.maximum(h @ p[pre + "linear1.weight"].T + p[pre + "linear1.bias"], 0.0)
        y = f @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"]
        h = layer_norm(h + y, p[pre + "norm2.weight"], p[pre + "norm2.bias"])
    z = h.reshape(n, R * d)
    z = np.maximum(z @ p["control_head.0.weight"].T + p["control_head.0.bias"], 0.0)
    z = np.maximum(z @ p["control_head.2.weight"].T + p["control_head.2.bias"], 0.0)
    return z @ p["control_head.4.weight"].T + p["control_head.4.bias"]


def normalized_outputs(cfg, throttle, steer):
    """The host entry's actions back to the network's outputs, in float64: o = 2 (a - lo) / (hi - lo) - 1."""
    a = np.stack([np.asarray(throttle, np.float64), np.asarray(steer, np.float64)], axis=1)
    lo, hi = np.array(list(cfg.action_lo), np.float64), np.array(list(cfg.action_hi), np.float64)
    return 2.0 * (a - lo) / (hi - lo) - 1.0
