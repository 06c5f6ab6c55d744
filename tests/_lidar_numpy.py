"""Float64 mirror of the lidar transformer driver's rule (include/okenv_lidar.h), in numpy: the same network on the same flat
parameter vector, every sum in double precision and in numpy's order.  It pins WHAT is computed (parameter order, post-norm, the
head split, the scale, the positional table, the normalisations); the fp32 summation orders are pinned by the device-against-host
tests."""
import numpy as np

# the three shapes of the rule's tests: the reference's; one with dh = 8 (a scale that is no power of two) and a single layer; one in
# between with two layers
SHAPES = {
    "reference": dict(num_points=7, d_model=128, nhead=8, num_layers=3, dim_feedforward=512, head_hidden1=256, head_hidden2=64),
    "tiny": dict(num_points=3, d_model=16, nhead=2, num_layers=1, dim_feedforward=16, head_hidden1=16, head_hidden2=16),
    "small": dict(num_points=7, d_model=32, nhead=2, num_layers=2, dim_feedforward=64, head_hidden1=32, head_hidden2=16),
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
