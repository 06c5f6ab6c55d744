"""The lidar transformer driver's rule (include/okenv_lidar.h) without a GPU: the float64 mirror against torch's own transformer
stack through the exporter, the positional table's two readings, the host entry okenv_lidar_act_host against the mirror, the linear
piece's fused bias-first chain, and the limits of the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _lidar_numpy as mirror

f32 = np.float32
INVALID, STATE = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Item 3's bound on |host entry - float64 mirror| of the normalised outputs, from the same fp32 points, default action ranges.
# Measured here over the seeds and agent counts below: the largest deviation was 2.07e-7 (reference shape 2.07e-7, tiny 1.51e-7,
# small 2.01e-7) at outputs of magnitude up to 0.56; the bound is 4 x that, for seed-to-seed spread.  It covers the fp32 network AND
# the rounding of the denormalised action (half an ulp of a throttle in 64 .. 100 is 3.8e-6, 7.6e-8 once normalised).
HOST_VS_MIRROR_TOL = 4 * 2.07e-7
# The shapes chosen for the act kernel's other paths (tests/_lidar_numpy.py: PATHS) have other depths and widths, so each has a bound
# of its own, found the same way: the largest deviation measured over seeds 0 .. 3 and 33 agents, times 4.  random_params' scale
# stays 1: the smallest of the outputs' maxima per seed is 0.098 (two_tiles_a_head, seed 0), above the guard of 0.05.  Measured, with
# the largest output over the seeds (one_point's head is 256 and 512 wide behind a single token, hence its longer chains):
MEASURED_DEVIATION = {
    "unit_heads": 1.88e-7,        # outputs up to 0.41
    "wide_group": 1.96e-7,        # 0.68
    "short_blocks": 2.26e-7,      # 0.71
    "two_tiles_a_head": 1.76e-7,  # 0.57
    "sixteen_points": 2.01e-7,    # 0.81
    "one_point": 5.08e-7,         # 0.58
}
TOL = dict({name: HOST_VS_MIRROR_TOL for name in mirror.OLD_SHAPES}, **{name: 4 * v for name, v in MEASURED_DEVIATION.items()})
SEEDS = dict({"reference": (0, 1), "tiny": (0, 1, 2, 3), "small": (0, 1, 2, 3)}, **{name: (0, 1, 2, 3) for name in mirror.NEW_SHAPES})
# (the host forward of the reference shape is 4.4 M fused operations per agent)
AGENTS = dict({"reference": 8, "tiny": 33, "small": 33}, **{name: 33 for name in mirror.NEW_SHAPES})


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def torch_model(shape, positional, seed):
    from openkitchen_amd.imitation import LidarTransformer
    torch.manual_seed(seed)
    kw = dict(shape)
    model = LidarTransformer(n_points=kw.pop("num_points"), positional=positional, **kw).double().eval()
    with torch.no_grad():  # LayerNorm starts at (1, 0) and biases small: move them, so that a swapped pair shows
        for name, p in model.named_parameters():
            if "norm" in name or name.endswith("bias"):
                p.add_(0.2 * torch.randn_like(p))
    return model


def mirror_vs_torch(capi, name, agents=33):
    from openkitchen_amd.imitation import lidar_params_from_state_dict
    shape = mirror.SHAPES[name]
    model = torch_model(shape, "token", 0)
    cfg = capi.lidar_config(**shape)
    params = lidar_params_from_state_dict(model.state_dict(), positional="token", dtype=torch.float64).numpy()
    assert params.size == capi.lidar_num_params(cfg)
    x = torch.rand(agents, shape["num_points"], 2, dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        want = model(x).numpy()
    got = mirror.forward(capi, cfg, params, x.numpy())
    err = np.abs(got - want).max()
    print("%s: mirror vs torch float64: max abs deviation %.3g, outputs up to %.3g" % (name, err, np.abs(want).max()))
    assert np.abs(want).max() > 0.05
    assert err <= 1e-9
    return params


def test_mirror_equals_torch_stack(capi):
    """Item 1: reference shape, 33 agents, a token-dependent positional table."""
    assert mirror_vs_torch(capi, "reference").size == 841410 + 896


@pytest.mark.parametrize("name", ["wide_group", "unit_heads"])
def test_mirror_equals_torch_stack_at_other_head_widths(capi, name):
    """The mirror's head split and scale at heads of 24 columns (no multiple of a tile, scale no power of two) and of one column."""
    assert mirror.PATHS[name](mirror.plan(mirror.SHAPES[name])) and mirror.SHAPES[name]["d_model"] // mirror.SHAPES[name]["nhead"] in (24, 1)
    mirror_vs_torch(capi, name)


@pytest.mark.parametrize("positional", ["reference", "token"])
def test_positional_table(capi, positional):
    """Item 2: with the state dict's own table (made random here, so that it is read and not recomputed), "reference" gives every
    token row 0 -- what the reference's module adds to a batch of one -- and "token" gives token t row t."""
    from openkitchen_amd.imitation import lidar_params_from_state_dict
    shape = mirror.SHAPES["small"]
    model = torch_model(shape, positional, 3)
    with torch.no_grad():
        model.pos_encoder.pe.copy_(torch.randn_like(model.pos_encoder.pe))
    sd = model.state_dict()
    cfg = capi.lidar_config(**shape)
    params = lidar_params_from_state_dict(sd, positional=positional, dtype=torch.float64).numpy()
    pos = mirror.pieces(capi, cfg, params)["pos"]
    pe = sd["pos_encoder.pe"][:, 0].numpy()
    for t in range(shape["num_points"]):
        assert np.array_equal(pos[t], pe[0] if positional == "reference" else pe[t])
    x = torch.rand(5, shape["num_points"], 2, dtype=torch.float64) * 2 - 1
    with torch.no_grad():  # one sample at a time: the C++ driver's batch of one
        want = torch.cat([model(x[i:i + 1]) for i in range(5)]).numpy()
        assert torch.equal(model.driven(x[:1]), model(x[:1]))
    assert np.abs(mirror.forward(capi, cfg, params, x.numpy()) - want).max() <= 1e-9
    # without a table in the state dict the sinusoid is used: row 0 is (0, 1, 0, 1, ...)
    bare = {k: v for k, v in sd.items() if k != "pos_encoder.pe"}
    pos = mirror.pieces(capi, cfg, lidar_params_from_state_dict(bare, positional=positional).numpy())["pos"]
    assert np.array_equal(pos[0], np.tile([0.0, 1.0], shape["d_model"] // 2))
    assert np.array_equal(pos[1], pos[0]) == (positional == "reference")


def host_vs_mirror(capi, name, seed):
    n = AGENTS[name]
    cfg = capi.lidar_config(**mirror.SHAPES[name])
    rng = np.random.default_rng(100 * seed + len(name))
    params = mirror.random_params(capi, cfg, rng)
    rel = rng.uniform(-200.0, 200.0, (n, cfg.num_points, 2)).astype(f32)
    out = capi.lidar_act_host(cfg, params, rel)
    # the normalised points: x - lo in [0, 400] rounds by at most 2^-16, which 2 / 400 scales to 7.6e-8; the quotient in [0, 2] and
    # the difference in [-1, 1] round by at most 6e-8 each: 2^-22 = 2.4e-7 covers the three
    assert np.abs(out["input"].astype(np.float64) - mirror.normalize_input(rel)).max() <= 2.0 ** -22
    want = mirror.forward(capi, cfg, params, out["input"])  # the network from the same fp32 points
    got = mirror.normalized_outputs(cfg, out["throttle"], out["steer"])
    assert np.all(out["alive"] == 1)
    return np.abs(got - want).max(), np.abs(want).max()


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_host_entry_against_mirror(capi, name):
    """Item 3; the shapes behind the first three reach, in the host entry too, the widths their names say."""
    if name in mirror.PATHS:
        assert mirror.PATHS[name](mirror.plan(mirror.SHAPES[name])), name
    worst = 0.0
    for seed in SEEDS[name]:
        err, size = host_vs_mirror(capi, name, seed)
        print("%s seed %d: max abs deviation %.3g, outputs up to %.3g" % (name, seed, err, size))
        assert size > 0.05, "the outputs are too small for an absolute bound to say anything"
        worst = max(worst, err)
    assert worst <= TOL[name]


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_lds_plan_restated(capi, name):
    """tests/_lidar_numpy.py's plan() is okLidarPlaces: the same bytes as okenv_lidar_lds_bytes, inside the budget; a new shape
    reaches the path it was chosen for."""
    shape = mirror.SHAPES[name]
    plan = mirror.plan(shape)
    print(name, plan)
    assert plan["bytes"] == capi.lidar_lds_bytes(capi.lidar_config(**shape)) <= capi.LIDAR_LDS_BUDGET
    assert (name in mirror.PATHS) == (name in mirror.NEW_SHAPES)
    if name in mirror.PATHS:
        assert mirror.PATHS[name](plan), plan
    else:  # what the first three shapes have in common, and the others are for
        assert plan["W"] == 16 and plan["tasks"] <= mirror.THREADS and plan["ldp"] == shape["num_points"] and plan["row_blocks"] in ([3], [4, 3])
        assert all(b == mirror.COL_BLOCK for b in plan["d_blocks"][:-1] + plan["ff_blocks"][:-1]) and plan["c_by"] == "activations"
        assert len(plan["d_blocks"]) == 1 or plan["d_blocks"][-1] == mirror.COL_BLOCK
        assert len(plan["ff_blocks"]) == 1 or plan["ff_blocks"][-1] == mirror.COL_BLOCK


def test_lds_plan_restated_over_a_grid(capi):
    """The restatement against the library wherever the rule's limits allow a shape, the ones over the budget included."""
    seen = set()
    for R in (1, 2, 5, 8, 16):
        for d, nhead in ((16, 1), (16, 16), (48, 2), (48, 3), (64, 2), (80, 5), (96, 4), (128, 8), (256, 8), (512, 1)):
            for ff, h1, h2 in ((16, 16, 16), (80, 2048, 16), (4096, 16, 2048), (144, 256, 512)):
                shape = dict(num_points=R, d_model=d, nhead=nhead, num_layers=1, dim_feedforward=ff, head_hidden1=h1, head_hidden2=h2)
                plan = mirror.plan(shape)
                assert plan["bytes"] == capi.lidar_lds_bytes(capi.lidar_config(**shape)), shape
                seen.add((plan["c_by"], plan["s_by"], plan["bytes"] <= capi.LIDAR_LDS_BUDGET))
    # (a column block never sizes s: 3 rows (W + 4) + 256 (R | 1) exceeds rows x 68 already at W = 16)
    assert {c for c, s, fits in seen} == {"activations", "head1"} and {s for c, s, fits in seen} == {"attention", "head2"}
    assert {fits for c, s, fits in seen} == {True, False}


def test_mirror_constants_match_the_header():
    kernel = open(os.path.join(ROOT, "openkitchen_amd", "csrc", "ok_lidar.h")).read()

    def constant(name):
        return int(re.search(r"constexpr int %s\s*=\s*(\d+);" % name, kernel).group(1))

    assert (constant("kLidarAgents"), constant("kLidarThreads")) == (mirror.AGENTS, mirror.THREADS)
    assert (constant("kLidarRowBlock"), constant("kLidarColBlock"), constant("kLidarPad")) == (mirror.ROW_BLOCK, mirror.COL_BLOCK, mirror.PAD)
    budget = re.search(r"constexpr size_t kLidarLdsBudget\s*=\s*(\d+)U \* (\d+)U;", kernel)
    assert int(budget.group(1)) * int(budget.group(2)) == 160 * 1024


def test_host_forwards_stay_inside_their_work_space(tmp_path):
    """The host forwards of both matrix-core drivers as a stand-alone program under AddressSanitizer and UBSan
    (tests/cpp/lidar_host_check.cpp), on work spaces of exactly ok_*_work_floats floats: every shape of the two mirrors and the corners
    of the limits -- a feed-forward narrower than d_model, which once let the attention's context run past the work space's end."""
    import _flow_numpy as flow_mirror
    exe = str(tmp_path / "lidar_host_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "lidar_host_check.cpp")], check=True)
    keys = ("num_points", "d_model", "dim_feedforward", "head_hidden1", "head_hidden2", "nhead", "num_layers")
    lidar = [tuple(shape[k] for k in keys) for name, shape in mirror.SHAPES.items() if name != "reference"]
    lidar += [(16, 512, 16, 16, 16, 1, 1), (16, 16, 16, 16, 16, 16, 8), (1, 16, 16, 2048, 16, 2, 1), (1, 16, 16, 16, 2048, 1, 1), (3, 64, 48, 32, 16, 4, 2)]
    assert any(ff < d for R, d, ff, h1, h2, nhead, layers in lidar)
    flow = [(shape["cond_dim"], shape["hidden"], 2) for shape in flow_mirror.SHAPES.values()] + [(512, 16, 1), (16, 512, 1)]
    args = [str(v) for shape in lidar for v in ("lidar",) + shape] + [str(v) for shape in flow for v in ("flow",) + shape]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(lidar) + len(flow))], r.stdout[-1000:] + r.stderr[-4000:]


def test_host_entry_crashed_and_null_outputs(capi):
    cfg = capi.lidar_config(**mirror.SHAPES["tiny"])
    rng = np.random.default_rng(5)
    params = mirror.random_params(capi, cfg, rng)
    rel = rng.uniform(-200.0, 200.0, (4, 3, 2)).astype(f32)
    crashed = np.array([0, 1, 0, 7], dtype=np.uint8)
    full = capi.lidar_act_host(cfg, params, rel, crashed)
    assert list(full["alive"]) == [1, 0, 1, 0]
    thr = np.empty(4, dtype=f32)
    L = capi.load()
    assert L.okenv_lidar_act_host(C.byref(cfg), capi.ptr(params), 4, capi.ptr(rel), None, capi.ptr(thr), None, None, None) == 0
    assert np.array_equal(thr.view(np.uint32), full["throttle"].view(np.uint32))  # crashed agents are asked all the same


def test_linear_chain_is_fused_and_starts_from_the_bias(capi):
    """Item 4."""
    K, N = 16, 16
    x = np.zeros((1, K), dtype=f32)
    w = np.zeros((N, K), dtype=f32)
    x[0, 0] = 1 + 2.0 ** -12
    w[:, 0] = 1 - 2.0 ** -12
    out = capi.debug_lidar_linear(x, w, np.full(N, -1.0, dtype=f32))
    assert np.all(out == f32(-2.0 ** -24))  # (1 + e)(1 - e) - 1 = -e^2 exactly; a rounded product is 1, and 1 - 1 = 0
    # small integers: exact; the weight matrix is not symmetric, so w read as [K][N] fails
    rng = np.random.default_rng(2)
    M, K, N = 5, 32, 16
    xi = rng.integers(-4, 5, (M, K)).astype(f32)
    wi = rng.integers(-4, 5, (N, K)).astype(f32)
    wi[3, 7], wi[7, 3] = 4.0, -4.0
    bi = rng.integers(-9, 10, N).astype(f32)
    want = xi.astype(np.int64) @ wi.astype(np.int64).T + bi.astype(np.int64)
    assert np.array_equal(capi.debug_lidar_linear(xi, wi, bi).astype(np.int64), want)
    assert np.array_equal(capi.debug_lidar_linear(xi, wi, bi, relu=True).astype(np.int64), np.maximum(want, 0))


BAD_SHAPES = [dict(num_points=0), dict(num_points=17), dict(d_model=0), dict(d_model=24), dict(d_model=528, nhead=8), dict(nhead=0), dict(nhead=3),
              dict(nhead=256), dict(num_layers=0), dict(num_layers=9), dict(dim_feedforward=0), dict(dim_feedforward=100), dict(dim_feedforward=4112),
              dict(head_hidden1=0), dict(head_hidden1=40), dict(head_hidden1=2064), dict(head_hidden2=0), dict(head_hidden2=8), dict(head_hidden2=2064),
              dict(action_lo=(float("nan"), 0.0)), dict(action_hi=(1.0, float("inf"))), dict(sensor_range=0.0), dict(sensor_range=-1.0),
              dict(sensor_range=float("nan")),
              dict(num_points=16, d_model=256, nhead=8)]  # in range, but the LDS plan does not fit


def test_limits(capi):
    """Item 5 (the calls that need a handle are in tests/test_gpu_lidar.py)."""
    L = capi.load()
    good = capi.lidar_config()
    assert 0 < capi.lidar_lds_bytes(good) <= capi.LIDAR_LDS_BUDGET
    assert L.okenv_lidar_lds_bytes(None) == 0
    params = np.zeros(capi.lidar_num_params(capi.lidar_config(**mirror.SHAPES["tiny"])), dtype=f32)
    rel = np.zeros((1, 16, 2), dtype=f32)
    thr = np.zeros(1, dtype=f32)

    def act_host(cfg, p=params, r=rel):
        return L.okenv_lidar_act_host(C.byref(cfg) if cfg is not None else None, capi.ptr(p), 1, capi.ptr(r), None, capi.ptr(thr), None, None, None)

    tiny = capi.lidar_config(**mirror.SHAPES["tiny"])
    assert act_host(tiny) == 0
    for bad in BAD_SHAPES:
        cfg = capi.lidar_config(**dict(mirror.SHAPES["tiny"], **bad))
        assert act_host(cfg) == INVALID, bad
        if not any(k.startswith(("action", "sensor")) for k in bad):
            assert capi.lidar_lds_bytes(cfg) == 0 or capi.lidar_lds_bytes(cfg) > capi.LIDAR_LDS_BUDGET, bad
    assert act_host(None) == INVALID and act_host(tiny, p=None) == INVALID and act_host(tiny, r=None) == INVALID
    assert L.okenv_lidar_act_host(C.byref(tiny), capi.ptr(params), -1, capi.ptr(rel), None, None, None, None, None) == INVALID
    # NULL handles
    n = C.c_int32()
    assert L.okenv_lidar_create(None, C.byref(good)) == INVALID
    assert L.okenv_lidar_num_params(None, C.byref(n)) == INVALID
    assert L.okenv_lidar_set_params(None, capi.ptr(params)) == INVALID
    assert L.okenv_lidar_get_params(None, capi.ptr(params)) == INVALID
    assert L.okenv_lidar_act(None, None) == INVALID
    # the debug entry
    x, w, b, out = (np.zeros(s, dtype=f32) for s in ((2, 16), (16, 16), (16,), (2, 16)))

    def linear(M=2, K=16, N=16, x=x, w=w, b=b, out=out):
        return L.okenv_debug_lidar_linear(-1, M, K, N, capi.ptr(x), capi.ptr(w), capi.ptr(b), 0, capi.ptr(out))

    assert linear() == 0
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(out=None), dict(M=-1), dict(K=0), dict(K=20), dict(K=4112), dict(N=0), dict(N=8),
               dict(N=4112)):
        assert linear(**kw) == INVALID, kw
