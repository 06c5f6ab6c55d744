"""Float64 mirror of the flow-matching driver's rule (include/okenv_flow.h), in numpy: the same sampler on the same flat parameter
vector -- the condition's share of layer 1 hoisted out of the loop and the embedding columns first, as the rule has them -- every sum
in double precision and in numpy's order.  It pins WHAT is computed (parameter order, the column order of layer 1, t and dt, the
clamps, the ranges, the draw); the fp32 summation orders are pinned by the device-against-host tests."""
import numpy as np

import _gauss_numpy as gauss

STREAM = 13
# the three shapes of the rule's tests: one tile wide in both widths and few steps; widths that are no power of two and an odd step
# count; the reference's.  Behind them the shapes at which the LDS's room, not kFlowStageCols, decides how many columns of W2 the act
# kernel (openkitchen_amd/csrc/ok_flow.h) stages at a time; what each one reaches is in PATHS below and asserted by the tests that use it
SHAPES = {
    "tiny": dict(cond_dim=16, hidden=16, steps=3),
    "small": dict(cond_dim=48, hidden=80, steps=5),
    "reference": dict(cond_dim=128, hidden=256, steps=32),
    "stage48": dict(cond_dim=16, hidden=352, steps=2),
    "stage32": dict(cond_dim=16, hidden=400, steps=2),
    "stage16": dict(cond_dim=512, hidden=448, steps=2),
    "stage16_full": dict(cond_dim=384, hidden=496, steps=2),
    "largest_plan": dict(cond_dim=464, hidden=480, steps=2),
}
OLD_SHAPES = ("tiny", "small", "reference")
NEW_SHAPES = tuple(name for name in SHAPES if name not in OLD_SHAPES)

# ok_flow.h's and ok_lidar.h's constants; tests/test_flow_rule.py keeps them in step with the headers
AGENTS, STAGE_COLS, PAD, LDS_BUDGET = 16, 64, 4, 160 * 1024


def plan(shape):
    """okFlowPlaces restated: the columns of W2 staged in LDS at a time (whole tiles that fit behind the rest, at most STAGE_COLS and at
    most H; 0: layer 2 reads W2 from global memory), the blocks an Euler step takes, whether the room decided, and the plan's bytes."""
    C, H = shape["cond_dim"], shape["hidden"]
    ldc, ldh = C + PAD, H + PAD
    w3s = AGENTS * ldc + 3 * AGENTS * ldh + 2 * AGENTS + 3 * H
    w2s = (w3s + 2 * ldh + 3) & ~3
    room = (LDS_BUDGET // 4 - w2s) // ldh
    room = 0 if room < 0 else room & ~15
    stage_cols = min(STAGE_COLS, H, room)
    return dict(stage_cols=stage_cols, room_limited=room < min(STAGE_COLS, H),
                blocks=[min(stage_cols, H - n0) for n0 in range(0, H, stage_cols)] if stage_cols else [], bytes=4 * (w2s + stage_cols * ldh))


# What each new shape exists for, as a predicate on (shape, plan): a later change of a constant that takes the path away fails the
# test that names the shape, before it compares anything
PATHS = {
    # three column tiles for four waves; a short block behind room-limited ones
    "stage48": lambda s, p: p["stage_cols"] == 48 and p["room_limited"] and p["blocks"] == [48] * 7 + [16],
    "stage32": lambda s, p: p["stage_cols"] == 32 and p["room_limited"] and s["hidden"] % 32 == 16 and p["blocks"] == [32] * 12 + [16],
    # one tile at a time with H > 16: many blocks per Euler step
    "stage16": lambda s, p: p["stage_cols"] == 16 and p["room_limited"] and s["hidden"] > 16 and p["blocks"] == [16] * 28,
    # ... at the widest H that still stages, the plan within 1 KB of the budget
    "stage16_full": lambda s, p: p["stage_cols"] == 16 and p["room_limited"] and p["blocks"] == [16] * 31 and LDS_BUDGET - 1024 < p["bytes"] <= LDS_BUDGET,
    # the largest plan any allowed shape has (tests/test_flow_rule.py walks the grid): the staged block ends 224 bytes under the budget
    "largest_plan": lambda s, p: p["stage_cols"] == 16 and p["room_limited"] and LDS_BUDGET - 256 < p["bytes"] <= LDS_BUDGET,
}


def pieces(capi, cfg, params):
    """{name: float64 array of its shape} of the flat vector."""
    params = np.asarray(params, dtype=np.float64).ravel()
    assert params.size == capi.flow_num_params(cfg)
    return {name: params[at:at + int(np.prod(shape))].reshape(shape) for name, at, shape in capi.flow_layout(cfg)}


def random_params(capi, cfg, rng, scale=1.0):
    """A parameter vector at torch's default init scale (uniform in +-scale / sqrt(fan_in), weights and biases alike), the biases
    moved by 0.2 sigma so that a swapped pair shows."""
    out = np.empty(capi.flow_num_params(cfg), dtype=np.float64)
    fan_in = None
    for name, at, shape in capi.flow_layout(cfg):
        n = int(np.prod(shape))
        if len(shape) == 2:
            fan_in = shape[1]
            v = rng.uniform(-1.0, 1.0, n) * scale / np.sqrt(fan_in)
        else:
            v = rng.uniform(-1.0, 1.0, n) * scale / np.sqrt(fan_in) + 0.2 * rng.standard_normal(n)
        out[at:at + n] = v
    return out.astype(np.float32)


def noise(seed, agents, draw):
    """x0 [n, 2] of the global agent ids `agents` at draw index `draw`: the rule's Box-Muller pair, in float32 as the rule has it."""
    w = gauss.philox4x32(np.asarray(agents, dtype=np.uint64), int(draw) & 0xFFFFFFFF, STREAM, 0, seed, gauss.KEY1)
    e0, e1 = gauss.normal_pair(w[0], w[1])
    return np.stack([e0, e1], axis=1)


def velocity(p, pre, x, t):
    h1 = np.maximum(pre + x @ p["net.0.weight"][:, :2].T + t * p["net.0.weight"][:, 2], 0.0)
    h2 = np.maximum(h1 @ p["net.2.weight"].T + p["net.2.bias"], 0.0)
    return h2 @ p["net.4.weight"].T + p["net.4.bias"]


def forward(capi, cfg, params, cond, x0, clamp=True):
    """cond [n][C], x0 [n][2] -> x [n][2], the (clamped) normalised sample, float64.  t and dt are the rule's fp32 values
    (float)i / (float)S and 1.0f / (float)S (exact quotients when S is a power of two)."""
    p = pieces(capi, cfg, params)
    S = np.float32(cfg.steps)
    x = np.asarray(x0, dtype=np.float64)
    pre = np.asarray(cond, dtype=np.float64) @ p["net.0.weight"][:, 3:].T + p["net.0.bias"]
    dt = float(np.float32(1.0) / S)
    for i in range(cfg.steps):
        x = x + dt * velocity(p, pre, x, float(np.float32(i) / S))
    return np.clip(x, -1.0, 1.0) if clamp else x


def actions(cfg, x):
    """The denormalised, clamped actions of normalised samples, float64."""
    lo, hi = np.array(list(cfg.action_lo), np.float64), np.array(list(cfg.action_hi), np.float64)
    return np.clip((np.asarray(x, np.float64) + 1.0) / 2.0 * (hi - lo) + lo, lo, hi)
