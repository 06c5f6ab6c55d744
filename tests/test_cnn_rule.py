"""The behavioural-cloning image policy's rule (include/okenv_cnn.h) without a GPU: the host entry okenv_cnn_act_host against the
float64 mirror, the parameter layout against the PyTorch module, the hidden layer's weight index, the limits of the shape, the plan
functions, the launch geometry restated and the path each shape was chosen for, the crashed flags and the host forward under the
sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _cnn_numpy as mirror

f32 = np.float32
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3)

# The bound on |host entry - float64 mirror| of the tanh output, from the same frames (two of random bytes a seed) and fp32 parameters
# (mirror.draw_params): the largest deviation measured here on the CPU per shape over seeds 0 .. 3, times 4, the project's margin for an
# fp32 chain against float64 (DESIGN.md sections 25 and 26).  Per seed the deviations were
#   tiny        5.09e-8, 2.16e-8, 6.47e-8, 6.86e-9        odd         7.03e-8, 4.93e-8, 6.91e-8, 9.56e-8
#   wide        3.53e-8, 6.07e-8, 9.07e-8, 1.24e-7        reference   4.07e-8, 3.56e-8, 8.96e-8, 1.01e-7
#   three_tiles 4.04e-8, 3.55e-8, 6.28e-8, 1.53e-7
#   ragged_chunk        7.46e-8, 4.30e-8, 4.99e-8, 5.07e-8        one_group_tail 7.05e-8, 4.08e-8, 7.83e-8, 6.24e-8
#   wide_inputs         5.61e-8, 9.87e-8, 2.53e-8, 7.75e-8        long_chains    6.60e-8, 7.77e-8, 9.96e-8, 3.15e-8
#   four_tiles_one_wave 1.68e-7, 5.55e-8, 4.74e-8, 9.12e-8
# with the output layer's largest |o| of a run between 0.014 (wide, seed 1) and 0.46 (the test holds it inside 0.01 .. 3, so that a
# wrong term shows behind the tanh); at the five shapes of the second block it lies between 0.037 (wide_inputs, seed 1) and 0.43.
MEASURED_DEVIATION = {"tiny": 6.47e-8, "odd": 9.56e-8, "wide": 1.24e-7, "reference": 1.02e-7, "three_tiles": 1.54e-7, "ragged_chunk": 7.46e-8,
                      "one_group_tail": 7.83e-8, "wide_inputs": 9.87e-8, "long_chains": 9.97e-8, "four_tiles_one_wave": 1.68e-7}
TOL = {name: 4 * v for name, v in MEASURED_DEVIATION.items()}


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def config(capi, name_or_members, **more):
    members = mirror.SHAPES[name_or_members] if isinstance(name_or_members, str) else name_or_members
    return capi.cnn_config(**dict(members, **more))


@pytest.fixture(scope="module")
def host_runs(capi):
    """Per shape and seed: (deviation of the host entry's output from the mirror's, the largest |o| of the mirror)."""
    runs = {}
    for name, cfg in mirror.SHAPES.items():
        assert mirror.sides(cfg) == mirror.SIDES[name] == capi.cnn_sides(config(capi, name))
        for seed in SEEDS:
            params, frames = mirror.draw_params(cfg, seed), mirror.draw_frames(cfg["image_size"], seed)
            o, want = mirror.forward(cfg, params, frames)
            got = capi.cnn_act_host(config(capi, name), params, frames)
            assert got["out"].dtype == f32 and got["out"].shape == want.shape and np.isfinite(got["out"]).all()
            assert np.array_equal(got["throttle"], np.full(2, 100.0, f32)) and np.array_equal(got["steer"], got["out"] * f32(10.0))
            assert np.array_equal(got["alive"], np.ones(2, np.uint8))
            runs[name, seed] = (float(np.abs(got["out"].astype(np.float64) - want).max()), float(np.abs(o).max()))
    return runs


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_host_entry_against_mirror(host_runs, name):
    for seed in SEEDS:
        dev, scale = host_runs[name, seed]
        print("%s seed %d: deviation %.3e, largest |o| %.3f" % (name, seed, dev, scale))
        assert 0.01 < scale < 3, "the draw saturates the tanh or gives nothing: a wrong term would not show"
    worst = max(host_runs[name, seed][0] for seed in SEEDS)
    assert worst <= TOL[name], (worst, TOL[name])


@pytest.mark.parametrize("S, sides", [(96, (23, 10, 8)), (48, (11, 4, 2))])
def test_layout_equals_the_pytorch_module(capi, S, sides):
    from openkitchen_amd import bc
    model = bc.PolicyCNN(S)
    sd = model.state_dict()
    cfg = bc.cnn_config_from_state_dict(sd, image_size=S)
    assert (cfg.image_size, tuple(cfg.kernel), tuple(cfg.stride), tuple(cfg.channels), cfg.hidden) == (S, (8, 4, 3), (4, 2, 1), (32, 64, 64), 256)
    assert (cfg.throttle, cfg.steer_scale) == (100.0, 10.0) and capi.cnn_sides(cfg) == sides
    members = dict(mirror.SHAPES["reference"], image_size=S)
    want = [(name, tuple(p.shape)) for name, p in model.named_parameters()]
    assert [(n, tuple(s)) for n, a, s in capi.cnn_layout(cfg)] == want == [(n, tuple(s)) for n, a, s in mirror.layout(members)]
    assert [a for n, a, s in capi.cnn_layout(cfg)] == [a for n, a, s in mirror.layout(members)]
    total = sum(p.numel() for p in model.parameters())
    assert capi.cnn_num_params(cfg) == mirror.num_params(members) == total
    params = bc.cnn_params_from_state_dict(sd, image_size=S)
    assert torch.equal(params, torch.cat([p.detach().reshape(-1) for p in model.parameters()]))


def test_hidden_layer_reads_torchs_weight_index(capi):
    """The hidden layer's chain runs over (y, x, channel) but reads the weight at torch's flatten index: with the weights of sixteen
    channels permuted among their positions in the module, torch's output and the host entry's change alike (fp32 against fp32: torch's moves by more than 1e-3, and agree to 1e-5, the rounding of chains of 256 terms of size below 1)."""
    from openkitchen_amd import bc
    S = 48
    torch.manual_seed(4)
    model = bc.PolicyCNN(S).eval()
    with torch.no_grad():
        model.steering_head[0].weight.mul_(8.0)  # (torch's init leaves the output near 0: a larger hidden layer, a larger change)
    frames = torch.from_numpy(mirror.draw_frames(S, 7, n=3))
    outs = []
    for permuted in (False, True):
        if permuted:
            with torch.no_grad():
                w = model.steering_head[0].weight  # [256][64 * 2 * 2]: the four positions of each of channels 0 .. 15 turned round
                w[:, :64] = w[:, :64].reshape(256, 16, 4).flip(2).reshape(256, 64).clone()
        sd = model.state_dict()
        with torch.no_grad():
            want = model(bc.frames_to_input(frames))[:, 0].numpy()
        got = capi.cnn_act_host(bc.cnn_config_from_state_dict(sd, image_size=S), bc.cnn_params_from_state_dict(sd, image_size=S).numpy(), frames.numpy())
        outs.append((want, got["out"]))
    (t0, h0), (t1, h1) = outs
    print("torch vs host: %.3e, %.3e; the permutation moves the output by %.3e" % (np.abs(t0 - h0).max(), np.abs(t1 - h1).max(), np.abs(t1 - t0).max()))
    assert np.abs(t1 - t0).max() > 1e-3
    assert np.abs(t0 - h0).max() <= 1e-5 and np.abs(t1 - h1).max() <= 1e-5


BAD_SHAPES = [dict(image_size=15), dict(image_size=129), dict(kernel=(0, 4, 3)), dict(kernel=(8, 9, 3)), dict(stride=(0, 2, 1)),
              dict(stride=(4, 5, 1), kernel=(8, 8, 3)), dict(stride=(4, 2, 4)), dict(image_size=32), dict(channels=(8, 64, 64)),
              dict(channels=(32, 64, 144)), dict(channels=(32, 24, 64)), dict(image_size=112, channels=(32, 64, 128)), dict(hidden=8),
              dict(hidden=520), dict(hidden=24)]


def test_shape_limits(capi):
    L = capi.load()
    ref = mirror.SHAPES["reference"]
    params, frames = np.zeros(mirror.num_params(ref), f32), np.zeros((1, 96, 96, 4), np.uint8)
    out = np.empty(1, f32)
    plan = (C.c_int32 * 2)()
    for bad in BAD_SHAPES:
        cfg = config(capi, ref, **bad)
        assert capi.cnn_lds_bytes(cfg) == 0, bad
        assert L.okenv_cnn_plan(C.byref(cfg), plan) == INVALID, bad
        assert b"okenv_cnn_plan: shape outside the limits" in L.okenv_last_error(None)
        rc = L.okenv_cnn_act_host(C.byref(cfg), capi.ptr(params), 1, capi.ptr(frames), None, None, None, capi.ptr(out), None)
        assert rc == INVALID and b"okenv_cnn_act_host: shape outside the limits" in L.okenv_last_error(None), bad
    # F = 128 x 10 x 10 = 12800 > 8192 is what refuses the frame of 112: with 64 channels (F = 6400) the same frame passes
    assert capi.cnn_lds_bytes(config(capi, ref, image_size=112)) > 0
    for bad in (dict(throttle=float("nan")), dict(throttle=float("inf")), dict(steer_scale=float("-inf")), dict(steer_scale=float("nan"))):
        cfg = config(capi, ref, **bad)
        rc = L.okenv_cnn_act_host(C.byref(cfg), capi.ptr(params), 1, capi.ptr(frames), None, None, None, capi.ptr(out), None)
        assert rc == INVALID and b"throttle / steer_scale must be finite" in L.okenv_last_error(None), bad
    # the corners of the limits are inside
    for good in (dict(image_size=16, kernel=(1, 1, 1), stride=(1, 1, 1), channels=(16, 16, 16), hidden=16),
                 dict(image_size=128, kernel=(8, 8, 6), stride=(4, 4, 4), channels=(128, 128, 128), hidden=512)):
        assert not_bad(capi, good), good


def not_bad(capi, members):
    """The shape check alone passes (the LDS may still refuse the shape)."""
    return capi.cnn_lds_bytes(config(capi, members)) > 0


def test_plan_functions_equal_the_mirror(capi):
    L = capi.load()
    for name, cfg in mirror.SHAPES.items():
        assert capi.cnn_lds_bytes(config(capi, name)) == mirror.lds_bytes(cfg) <= capi.CNN_LDS_BUDGET, name
        assert capi.cnn_plan(config(capi, name)) == mirror.plan(cfg) == mirror.PATHS[name], name
    assert {p[0] for p in mirror.PATHS.values()} == {1, 2, 3, 4} and {p[1] for p in mirror.PATHS.values()} == {0, 1}
    assert (mirror.WAVES, mirror.AGENTS) == (8, capi.CNN_AGENTS)
    # inside the shape's limits and outside the LDS: 128 x 128 pixels of 128 channels do not fit a workgroup
    big = dict(image_size=128, kernel=(1, 8, 8), stride=(1, 4, 4), channels=(128, 16, 16), hidden=16)
    assert capi.cnn_lds_bytes(config(capi, big)) == mirror.lds_bytes(big) > capi.CNN_LDS_BUDGET
    plan = (C.c_int32 * 2)()
    assert L.okenv_cnn_plan(C.byref(config(capi, big)), plan) == INVALID and b"does not fit 160 KB" in L.okenv_last_error(None)
    assert L.okenv_cnn_plan(None, plan) == INVALID and L.okenv_cnn_plan(C.byref(config(capi, "tiny")), None) == INVALID
    assert L.okenv_cnn_lds_bytes(None) == 0


# (F, LDS bytes, parameters) of the shapes that exist for a path of the kernels, as they were computed when the shapes were chosen
NEW_FIGURES = {"ragged_chunk": (400, 26112, 60929), "one_group_tail": (784, 154500, 110369), "wide_inputs": (288, 34304, 105985),
               "long_chains": (128, 41472, 150129), "four_tiles_one_wave": (16, 42496, 12561)}


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_launch_geometry_restated(capi, name):
    """mirror.geometry at every shape of the table against a count of the units, tiles and chunks one by one, and the predicate the
    shape was chosen for (mirror.REACHES)."""
    shape = mirror.SHAPES[name]
    assert set(mirror.REACHES) == set(mirror.SHAPES) == set(mirror.PATHS) == set(mirror.SIDES) and set(NEW_FIGURES) == set(mirror.NEW_SHAPES)
    for agents in (1, 2, 15, 16, 17, 33):
        g = mirror.geometry(shape, agents)
        for l, c in enumerate(g["conv"]):
            M = mirror.SIDES[name][l] ** 2
            units = sorted({(row // 32, col // 16) for row in range(M) for col in range(shape["channels"][l])})  # (row block, column tile)
            waves = [sum(1 for u in range(len(units)) if u % 8 == w) for w in range(8)]  # the units of wave w: w, w + 8, ...
            assert (c["M"], c["units"], c["blocks"]) == (M, len(units), units[-1][0] + 1)
            assert c["rounds"] == max(waves) and c["idle_waves"] == sum(1 for n in waves if n < max(waves))
            assert c["last_rows"] == sum(1 for row in range(M) if row // 32 == c["blocks"] - 1)
            k = shape["kernel"][l]
            if l == 0:  # four k's a tap; the chain ends on a whole group of 16
                assert c["taps"] == k * k and c["groups"] == len(range(0, 4 * k * k, 16)) and c["fillers"] == c["groups"] * 4 - k * k and 0 <= c["fillers"] < 4
            else:       # a tap's channels 16 at a time, tap after tap
                assert c["groups"] == len([(tap, c0) for tap in range(k * k) for c0 in range(0, shape["channels"][l - 1], 16)])
                assert c["groups_a_tap"] * 16 == shape["channels"][l - 1] and c["fillers"] == 0
        tiles = list(range(0, shape["hidden"], 16))
        owners = [[t for t in range(len(tiles)) if t % 8 == w] for w in range(8)]
        assert g["tiles"] == len(tiles) and g["tiles_a_wave"] == max(len(o) for o in owners)
        assert g["last_tile_waves"] == sum(1 for o in owners if len(o) == g["tiles_a_wave"]) and capi.cnn_plan(config(capi, name))[0] == g["tiles_a_wave"]
        F = mirror.features(shape)
        chunks = [min(256, F - k0) for k0 in range(0, F, 256)]
        assert g["chunks"] == len(chunks) and g["last_chunk_groups"] * 16 == chunks[-1] and all(c == 256 for c in chunks[:-1])
        blocks = [len(range(a0, min(a0 + 16, agents))) for a0 in range(0, agents, 16)]
        assert (g["conv_blocks"], g["head_blocks"], g["last_block_agents"]) == (agents, len(blocks), blocks[-1])
    assert mirror.reaches(name), (name, mirror.geometry(shape, mirror.REACHES[name][0]))
    if name in NEW_FIGURES:
        assert (mirror.features(shape), mirror.lds_bytes(shape), mirror.num_params(shape)) == NEW_FIGURES[name]
        assert capi.cnn_num_params(config(capi, name)) == NEW_FIGURES[name][2]
    # what the second block of shapes adds to the first, over the whole table: every k0 from 1 to 8, every tiles-a-wave form with its last
    # tile on wave 0 alone and on all eight, a last chunk of one group and of several behind whole ones
    geo = {n: mirror.geometry(s) for n, s in mirror.SHAPES.items()}
    assert {s["kernel"][0] for s in mirror.SHAPES.values()} == set(range(1, 9))
    assert {(g["tiles_a_wave"], g["last_tile_waves"]) for g in geo.values()} >= {(1, 8), (2, 1), (2, 8), (3, 1), (3, 8), (4, 1), (4, 8)}
    assert {(g["chunks"] > 1, g["last_chunk_groups"]) for g in geo.values()} >= {(True, 1), (True, 2), (True, 9), (True, 16), (False, 1), (False, 8)}
    assert {s["stride"][0] for s in mirror.SHAPES.values()} == {1, 2, 3, 4} and {s["stride"][l] for s in mirror.SHAPES.values() for l in (1, 2)} == {1, 2, 3, 4}


def squeezed(*path):
    return " ".join(open(os.path.join(ROOT, *path)).read().split())


def test_geometry_rests_on_the_source():
    """The constants, the okConv instantiations and the loops that mirror.geometry restates, pinned to the source text: a change to
    any of them fails here and not only in a device case."""
    conv, cnn, launch = squeezed("openkitchen_amd", "csrc", "ok_conv.h"), squeezed("openkitchen_amd", "csrc", "ok_cnn.h"), squeezed("openkitchen_amd", "csrc", "okenv_capi.hip")
    constant = lambda name: int(re.search(r"constexpr int %s\s*=\s*(\d+);" % name, conv).group(1))  # noqa: E731
    assert (constant("kConvThreads"), constant("kConvRowBlock"), constant("kConvAgents"), constant("kConvChunk")) == (512, 2, 16, 256)
    assert (mirror.THREADS, mirror.ROW_BLOCK, mirror.AGENTS, mirror.CHUNK, mirror.WAVES) == (512, 2, 16, 256, 512 // 64)
    assert "constexpr int kConvWaves = kConvThreads / 64;" in conv and "constexpr int kConvMaxColTiles = OK_CNN_MAX_HIDDEN / 16 / kConvWaves;" in conv
    # the unit loop of a convolution: row blocks of 16 RB rows, a unit per (row block, column tile), a wave every Waves-th unit
    for text in ("const int Nt = j.Cout >> 4, Mb = (j.M + 16 * RB - 1) / (16 * RB), units = Nt * Mb, groups = Taps::groups(j);",
                 "for (int u = wave; u < units; u += Waves)", "const int mb = u / Nt, n0 = (u - mb * Nt) << 4;",
                 "const int row = okLidarMin((mb * RB + m) * 16 + i, j.M - 1), oy = row / j.W, ox = row - oy * j.W;",
                 # the walk of layers 1 and 2 and its length
                 "return j.k * j.k * (j.Cin >> 4);", "c0 += 16; if (c0 == j.Cin) { c0 = 0; if (++tx == j.k) tx = 0, ++ty; }",
                 # the hidden layer's chunk loop, its staging split and its weight index; a wave's tiles
                 "for (int k0 = 0; k0 < F; k0 += kConvChunk)", "const int kc = okLidarMin(kConvChunk, F - k0), kc4 = kc >> 2;",
                 "for (int e = tid; e < kAgents * kc4; e += kConvThreads)", "const int r = e / kc4, c4 = e - r * kc4;",
                 "for (int grp = 0; grp < (kc >> 4); ++grp)", "okConvMfma(a, wp[((k0 >> 4) + grp) * gstride + t * 64], acc[c]);",
                 "const int t = okLidarMin(wave + kConvWaves * c, Nt - 1);", "const int t = wave + kConvWaves * c; if (t < Nt)",
                 "at.ct = (H / 16 + kConvWaves - 1) / kConvWaves;"):
        assert text in conv, text
    # the three convolutions of the conv kernel, and layer 0's chain
    assert len(re.findall(r"okConv<", cnn)) == 3
    assert cnn.count("okConv<OkCnnRgbaTaps, kConvRowBlock, kConvWaves, false>(j, to);") == 1
    assert cnn.count("okConv<OkConvWalk, kConvRowBlock, kConvWaves, false>(j, to);") == 2
    for text in ("return (j.k * j.k + 3) >> 2;", "if (ty != j.k - 1 || tx != j.k - 1) // (the filler taps stay on the last tap) if (++tx == j.k) tx = 0, ++ty;",
                 "okConvFc1<CT, 1>(p.feat, p.N, ok_cnn_features(sh), H, a0, p.pack + pl.pack[3], p.params + at.hb, pl.ldt, pl.ldh);",
                 "const long a0 = static_cast<long>(blockIdx.x) * kConvAgents;", "__global__ __launch_bounds__(kConvThreads) void okCnnConvKernel(",
                 "template <int CT> __global__ __launch_bounds__(kConvThreads) void okCnnHeadKernel("):
        assert text in cnn, text
    # the two launches: a frame a workgroup; kConvAgents agents a workgroup of the head form the plan selects
    for text in ("actLaunch(h, okCnnConvKernel, 1, kConvThreads, sizeof(float) * static_cast<size_t>(pl.conv_end), p)",
                 "{okCnnHeadKernel<1>, okCnnHeadKernel<2>, okCnnHeadKernel<3>, okCnnHeadKernel<4>};",
                 "return actLaunch(h, heads[pl.ct - 1], kConvAgents, kConvThreads, sizeof(float) * static_cast<size_t>(pl.head_end), p);"):
        assert text in launch, text


def test_crashed_only_sets_alive(capi):
    cfg = mirror.SHAPES["tiny"]
    params, frames = mirror.draw_params(cfg, 5), mirror.draw_frames(16, 5, n=4)
    plain = capi.cnn_act_host(config(capi, "tiny"), params, frames)
    crashed = np.array([0, 1, 0, 7], np.uint8)
    got = capi.cnn_act_host(config(capi, "tiny"), params, frames, crashed)
    assert np.array_equal(got["alive"], [1, 0, 1, 0]) and np.array_equal(plain["alive"], [1, 1, 1, 1])
    for k in ("out", "throttle", "steer"):
        assert np.array_equal(got[k], plain[k]) and np.isfinite(got[k]).all()
    assert len(set(got["out"].tolist())) == 4  # an action of its own for every agent, crashed or not
    L = capi.load()
    c = config(capi, "tiny")
    assert L.okenv_cnn_act_host(C.byref(c), capi.ptr(params), 4, capi.ptr(frames), None, None, None, None, None) == 0  # every output may be NULL
    assert L.okenv_cnn_act_host(C.byref(c), None, 4, capi.ptr(frames), None, None, None, None, None) == INVALID
    assert L.okenv_cnn_act_host(C.byref(c), capi.ptr(params), 4, None, None, None, None, None, None) == INVALID
    assert L.okenv_cnn_act_host(C.byref(c), capi.ptr(params), -1, capi.ptr(frames), None, None, None, None, None) == INVALID
    assert L.okenv_cnn_act_host(None, capi.ptr(params), 4, capi.ptr(frames), None, None, None, None, None) == INVALID


def test_host_forward_stays_inside_its_work_space(tmp_path):
    """The host forward as a stand-alone program under AddressSanitizer and UBSan (tests/cpp/cnn_host_check.cpp), on frames, parameter
    vectors and work spaces of exactly their sizes: every shape of the mirror and the corners of the limits."""
    exe = str(tmp_path / "cnn_host_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "cnn_host_check.cpp")], check=True)
    keys = ("kernel", "stride", "channels")
    shapes = [(s["image_size"],) + sum((tuple(s[k]) for k in keys), ()) + (s["hidden"],) for s in mirror.SHAPES.values()]
    shapes += [(16, 1, 1, 1, 1, 1, 1, 16, 16, 16, 16),           # the smallest frame, pointwise layers: F = 4096
               (16, 8, 8, 1, 1, 1, 1, 16, 16, 16, 512),          # sides 9 / 2 / 2, the widest hidden layer
               (128, 8, 8, 6, 4, 4, 4, 128, 128, 128, 16),       # the largest frame, strides and channels: sides 31 / 6 / 1
               (29, 8, 3, 2, 3, 2, 2, 16, 16, 128, 16),          # sides 8 / 3 / 1 with rows left over on every layer
               (32, 1, 1, 1, 4, 1, 1, 16, 16, 128, 16)]          # a stride without a kernel to match: s <= k refuses it
    args = [str(v) for shape in shapes[:-1] for v in shape]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(shapes) - 1)], r.stdout[-1000:] + r.stderr[-4000:]
    r = subprocess.run([exe] + [str(v) for v in shapes[-1]], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2  # the program refuses a shape outside the limits
