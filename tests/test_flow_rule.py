"""The flow-matching driver's rule (include/okenv_flow.h) without a GPU: the float64 mirror against the PyTorch trunk through the
exporter, the host entry's draw, the host entry okenv_flow_act_host against the mirror, the rule's edges and the limits of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _flow_numpy as mirror

f32 = np.float32
INVALID, STATE = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Item 3's bound on |host entry - float64 mirror| of the clamped normalised sample x, from the same fp32 x0, cond and parameters.
# Measured here over seeds 0 .. 3 and 33 agents a shape, cond uniform in [-1, 1], 23 .. 38 % of the outputs on the clamp: the largest
# deviation was 2.75e-7 (tiny C 16 H 16 S 3: 9.58e-8; small C 48 H 80 S 5: 9.61e-8; reference C 128 H 256 S 32: 2.75e-7); the bound is
# 4 x that, for seed-to-seed spread.
MEASURED_DEVIATION = 2.75e-7
HOST_VS_MIRROR_TOL = 4 * MEASURED_DEVIATION
# The shapes chosen for the act kernel's room-limited staging of W2 (tests/_flow_numpy.py: PATHS) are wider and take two Euler steps,
# so each has a bound of its own, found the same way: the largest deviation measured over seeds 0 .. 3 and 33 agents (23 .. 44 % of
# the outputs on the clamp), times 4
MEASURED_DEVIATION_BY_SHAPE = {
    "stage48": 2.19e-7,       # C 16 H 352
    "stage32": 1.96e-7,       # C 16 H 400
    "stage16": 3.40e-7,       # C 512 H 448
    "stage16_full": 1.46e-7,  # C 384 H 496
    "largest_plan": 2.28e-7,  # C 464 H 480
}
TOL = dict({name: HOST_VS_MIRROR_TOL for name in mirror.OLD_SHAPES}, **{name: 4 * v for name, v in MEASURED_DEVIATION_BY_SHAPE.items()})
# The action from x: x + 1 in [0, 2] rounds by at most 2^-24 * 2 / 2, the halving is exact, the product with hi - lo <= 100 carries that
# as 1.2e-5 and rounds by 3.8e-6, the sum with lo by 3.8e-6 again: 2^-15 = 3.1e-5 covers them
ACTION_TOL = 2.0 ** -15
SEEDS, AGENTS = (0, 1, 2, 3), 33


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def torch_trunk(shape, seed):
    from openkitchen_amd.flow import ActionFlowTrunk
    torch.manual_seed(seed)
    trunk = ActionFlowTrunk(bev_dim=shape["cond_dim"], hidden_dim=shape["hidden"]).double().eval()
    with torch.no_grad():  # move the biases, so that a swapped pair shows
        for name, p in trunk.named_parameters():
            if name.endswith("bias"):
                p.add_(0.2 * torch.randn_like(p))
    return trunk


def test_mirror_equals_torch_sampler(capi):
    """Item 1: reference shape, 33 agents, the PyTorch loop on cat([x, t, embedding]) in float64."""
    from openkitchen_amd import flow
    shape = mirror.SHAPES["reference"]
    trunk = torch_trunk(shape, 0)
    sd = trunk.state_dict()
    cfg = flow.flow_config_from_state_dict(sd, steps=shape["steps"])
    assert (cfg.cond_dim, cfg.hidden, cfg.steps) == (128, 256, 32)
    params = flow.flow_params_from_state_dict(sd, dtype=torch.float64).numpy()
    assert params.size == capi.flow_num_params(cfg) == 256 * 131 + 256 + 256 * 256 + 256 + 2 * 256 + 2
    # the whole policy's state dict gives the same vector
    from openkitchen_amd.flow import ConditionalFlowMatchingPolicy
    policy = ConditionalFlowMatchingPolicy().double()
    policy.action_flow_trunk.load_state_dict(sd)
    assert np.array_equal(flow.flow_params_from_state_dict(policy.state_dict(), dtype=torch.float64).numpy(), params)
    cond = torch.rand(33, 128, dtype=torch.float64) * 2 - 1
    x0 = torch.randn(33, 2, dtype=torch.float64)
    want = flow.sample(trunk, cond, x0, 32).numpy()
    got = mirror.forward(capi, cfg, params, cond.numpy(), x0.numpy())
    err = np.abs(got - want).max()
    on_clamp = float((np.abs(want) == 1.0).mean())
    print("mirror vs torch float64: max abs deviation %.3g, %.0f %% of the outputs on the clamp" % (err, 100 * on_clamp))
    assert on_clamp < 0.5
    assert err <= 1e-9


@pytest.mark.parametrize("draw", [0, 1, 2 ** 31])
def test_host_entry_draw(capi, draw):
    """Item 2: x0 is the mirror's Box-Muller pair of Philox stream 13, bit for bit; agents 0, 1 and agent_base + i."""
    shape = mirror.SHAPES["tiny"]
    rng = np.random.default_rng(3)
    cond = rng.uniform(-1.0, 1.0, (5, shape["cond_dim"])).astype(f32)
    for seed, base in ((0, 0), (7, 0), (7, 1000), (7, 2 ** 32 - 2)):
        cfg = capi.flow_config(seed=seed, agent_base=base, **shape)
        params = mirror.random_params(capi, cfg, rng)
        out = capi.flow_act_host(cfg, params, cond, draw_index=draw)
        want = mirror.noise(seed, (base + np.arange(5)) % 2 ** 32, draw)
        assert np.array_equal(out["x0"].view(np.uint32), want.view(np.uint32)), (seed, base)
    others = [mirror.noise(7, np.arange(5), d) for d in (0, 1, 2 ** 31) if d != draw]
    assert all(not np.array_equal(o, mirror.noise(7, np.arange(5), draw)) for o in others)
    quiet = capi.flow_act_host(capi.flow_config(noise=False, seed=7, **shape), params, cond, draw_index=draw)
    assert np.array_equal(quiet["x0"].view(np.uint32), np.zeros((5, 2), np.uint32))
    assert np.abs(quiet["x"] - mirror.forward(capi, cfg, params, cond, np.zeros((5, 2)))).max() <= HOST_VS_MIRROR_TOL


def host_vs_mirror(capi, name, seed):
    cfg = capi.flow_config(seed=seed, **mirror.SHAPES[name])
    rng = np.random.default_rng(100 * seed + len(name))
    params = mirror.random_params(capi, cfg, rng)
    cond = rng.uniform(-1.0, 1.0, (AGENTS, cfg.cond_dim)).astype(f32)
    out = capi.flow_act_host(cfg, params, cond, draw_index=seed)
    want = mirror.forward(capi, cfg, params, cond, out["x0"])  # from the same fp32 noise
    act = np.stack([out["throttle"], out["steer"]], axis=1)
    assert np.abs(act - mirror.actions(cfg, out["x"])).max() <= ACTION_TOL
    assert np.all(out["alive"] == 1)
    return np.abs(out["x"] - want).max(), float((np.abs(out["x"]) == 1.0).mean())


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_host_entry_against_mirror(capi, name):
    """Item 3; the shapes behind the first three have the widths at which the act kernel stages W2 in 48, 32 or 16 columns."""
    if name in mirror.PATHS:
        assert mirror.PATHS[name](mirror.SHAPES[name], mirror.plan(mirror.SHAPES[name])), name
    worst = 0.0
    for seed in SEEDS:
        err, on_clamp = host_vs_mirror(capi, name, seed)
        print("%s seed %d: max abs deviation %.3g, %.0f %% of the outputs on the clamp" % (name, seed, err, 100 * on_clamp))
        assert on_clamp < 0.5, "most outputs sit on the clamp: the comparison is one of constants"
        worst = max(worst, err)
    assert worst <= TOL[name]


WIDEST = dict(cond_dim=512, hidden=512, steps=2)  # tests/test_gpu_flow.py's shape without a staged block


@pytest.mark.parametrize("name", list(mirror.SHAPES) + ["widest"])
def test_lds_plan_restated(capi, name):
    """tests/_flow_numpy.py's plan() is okFlowPlaces: the same bytes as okenv_flow_lds_bytes, inside the budget; a new shape reaches
    the path it was chosen for, and no earlier shape did."""
    shape = WIDEST if name == "widest" else mirror.SHAPES[name]
    plan = mirror.plan(shape)
    print(name, plan)
    assert plan["bytes"] == capi.flow_lds_bytes(capi.flow_config(**shape)) <= capi.FLOW_LDS_BUDGET == mirror.LDS_BUDGET
    assert sum(plan["blocks"]) == (shape["hidden"] if plan["stage_cols"] else 0)
    assert (name in mirror.PATHS) == (name in mirror.NEW_SHAPES)
    if name in mirror.PATHS:
        assert mirror.PATHS[name](shape, plan), plan
    elif name == "widest":
        assert plan["stage_cols"] == 0 and plan["room_limited"]
    else:
        assert not plan["room_limited"] and set(plan["blocks"]) <= {16, 64}


def test_lds_plan_restated_over_the_grid(capi):
    """Every (C, H) of multiples of 16 the rule allows: the restatement's bytes are the library's, every plan fits, and none is
    larger than the shape's that bears that name."""
    largest, seen = 0, set()
    for Cd in range(16, 513, 16):
        for H in range(16, 513, 16):
            shape = dict(cond_dim=Cd, hidden=H, steps=2)
            plan = mirror.plan(shape)
            assert plan["bytes"] == capi.flow_lds_bytes(capi.flow_config(**shape)) <= capi.FLOW_LDS_BUDGET, shape
            assert plan["stage_cols"] % 16 == 0 and plan["stage_cols"] <= min(mirror.STAGE_COLS, H)
            seen.add(plan["stage_cols"])
            largest = max(largest, plan["bytes"])
    assert seen == {0, 16, 32, 48, 64}
    assert largest == mirror.plan(mirror.SHAPES["largest_plan"])["bytes"]


def test_rule_edges(capi):
    """Item 4."""
    shape = dict(mirror.SHAPES["small"], steps=1)
    cfg = capi.flow_config(seed=11, **shape)
    rng = np.random.default_rng(9)
    params = mirror.random_params(capi, cfg, rng, scale=0.5)
    cond = rng.uniform(-1.0, 1.0, (6, cfg.cond_dim)).astype(f32)
    crashed = np.array([0, 1, 0, 0, 5, 0], dtype=np.uint8)
    out = capi.flow_act_host(cfg, params, cond, crashed)
    # one step: x = x0 + v(x0, 0)
    p = mirror.pieces(capi, cfg, params)
    x0 = out["x0"].astype(np.float64)
    pre = cond.astype(np.float64) @ p["net.0.weight"][:, 3:].T + p["net.0.bias"]
    want = np.clip(x0 + mirror.velocity(p, pre, x0, 0.0), -1.0, 1.0)
    assert np.abs(out["x"] - want).max() <= HOST_VS_MIRROR_TOL
    assert np.any(np.abs(out["x"]) < 1.0)
    # a crashed agent is asked all the same
    assert list(out["alive"]) == [1, 0, 1, 1, 0, 1]
    free = capi.flow_act_host(cfg, params, cond)
    assert np.array_equal(free["throttle"].view(np.uint32), out["throttle"].view(np.uint32)) and np.all(free["alive"] == 1)
    # a velocity of (+50, -50) pushes x past both ends: exactly +-1, and exactly hi / lo behind the denormalisation
    at = {name: (a, int(np.prod(s))) for name, a, s in capi.flow_layout(cfg)}
    pushed = params.copy()
    a, n = at["net.4.weight"]
    pushed[a:a + n] = 0.0
    a, n = at["net.4.bias"]
    pushed[a:a + n] = (50.0, -50.0)
    for steps in (1, 5):
        cfg_s = capi.flow_config(seed=11, **dict(shape, steps=steps))
        out = capi.flow_act_host(cfg_s, pushed, cond)
        assert np.all(out["x"][:, 0] == 1.0) and np.all(out["x"][:, 1] == -1.0)
        assert np.all(out["throttle"] == cfg_s.action_hi[0]) and np.all(out["steer"] == cfg_s.action_lo[1])
    # outputs may be NULL
    thr = np.empty(6, dtype=f32)
    L = capi.load()
    assert L.okenv_flow_act_host(C.byref(cfg), capi.ptr(params), 6, capi.ptr(cond), None, 0, capi.ptr(thr), None, None, None, None) == 0
    assert np.array_equal(thr.view(np.uint32), free["throttle"].view(np.uint32))


BAD = [dict(cond_dim=8), dict(cond_dim=24), dict(cond_dim=528), dict(cond_dim=0), dict(hidden=8), dict(hidden=24), dict(hidden=528), dict(hidden=0),
       dict(steps=0), dict(steps=257), dict(steps=-1), dict(noise=2), dict(noise=-1), dict(action_lo=(float("nan"), 0.0)),
       dict(action_hi=(1.0, float("inf"))), dict(action_lo=(0.0, float("-inf")))]


def test_limits(capi):
    """Item 5 (the calls that need a handle are in tests/test_gpu_flow.py)."""
    L = capi.load()
    good = capi.flow_config()
    assert 0 < capi.flow_lds_bytes(good) <= capi.FLOW_LDS_BUDGET
    assert L.okenv_flow_lds_bytes(None) == 0
    sizes = [capi.flow_lds_bytes(capi.flow_config(hidden=H)) for H in (16, 64, 256, 512)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    tiny = capi.flow_config(**mirror.SHAPES["tiny"])
    params = np.zeros(capi.flow_num_params(capi.flow_config(cond_dim=512, hidden=512)), dtype=f32)
    cond = np.zeros((1, 528), dtype=f32)
    thr = np.zeros(1, dtype=f32)

    def act_host(cfg, p=params, c=cond, n=1):
        return L.okenv_flow_act_host(C.byref(cfg) if cfg is not None else None, capi.ptr(p), n, capi.ptr(c), None, 0, capi.ptr(thr), None, None, None, None)

    assert act_host(tiny) == 0
    assert act_host(capi.flow_config(cond_dim=512, hidden=512, steps=1)) == 0  # the limits themselves are inside
    for bad in BAD:
        cfg = capi.flow_config(**dict(mirror.SHAPES["tiny"], **bad))
        assert act_host(cfg) == INVALID, bad
        assert L.okenv_flow_create(None, C.byref(cfg)) == INVALID, bad
        if any(k in bad for k in ("cond_dim", "hidden", "steps")):
            assert capi.flow_lds_bytes(cfg) == 0, bad
    assert act_host(None) == INVALID and act_host(tiny, p=None) == INVALID and act_host(tiny, c=None) == INVALID and act_host(tiny, n=-1) == INVALID
    # NULL handles
    n = C.c_int32()
    assert L.okenv_flow_create(None, C.byref(good)) == INVALID
    assert L.okenv_flow_num_params(None, C.byref(n)) == INVALID
    assert L.okenv_flow_set_params(None, capi.ptr(params)) == INVALID
    assert L.okenv_flow_get_params(None, capi.ptr(params)) == INVALID
    assert L.okenv_flow_act(None, capi.ptr(cond), None) == INVALID
    assert L.okenv_flow_set_draw_offset(None, None) == STATE  # (okenv_gauss_set_draw_offset's answer)


def test_binding_constants_match_the_headers(capi):
    kernel = open(os.path.join(ROOT, "openkitchen_amd", "csrc", "ok_flow.h")).read()
    tiles = int(re.search(r"constexpr int kFlowTiles\s*=\s*(\d+);", kernel).group(1))
    assert capi.FLOW_AGENTS == 16 * tiles
    rule = open(os.path.join(ROOT, "include", "okenv_flow.h")).read()
    assert int(re.search(r"#define OK_FLOW_STREAM (\d+)u", rule).group(1)) == mirror.STREAM
    # what tests/_flow_numpy.py's plan() restates
    assert capi.FLOW_AGENTS == mirror.AGENTS
    assert int(re.search(r"constexpr int\s+kFlowStageCols\s*=\s*(\d+);", kernel).group(1)) == mirror.STAGE_COLS
    budget = re.search(r"constexpr size_t kFlowLdsBudget\s*=\s*(\d+)U \* (\d+)U;", kernel)
    assert int(budget.group(1)) * int(budget.group(2)) == mirror.LDS_BUDGET == capi.FLOW_LDS_BUDGET
    lidar = open(os.path.join(ROOT, "openkitchen_amd", "csrc", "ok_lidar.h")).read()
    assert int(re.search(r"constexpr int kLidarPad\s*=\s*(\d+);", lidar).group(1)) == mirror.PAD
