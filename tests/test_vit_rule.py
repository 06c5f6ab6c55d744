"""The image transformer driver's rule (include/okenv_vit.h) without a GPU: the float64 mirror against dino.ViT, the host entry against
the mirror at every shape, the fused bias-first chains, the limits and refusals, the LDS and workspace plan, and the host forward under
the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _vit_numpy as mirror

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
# |host entry - float64 mirror|, the largest over seeds 0 .. 3 (mirror.random_params, two frames of random bytes each), as measured when
# the rule was written: (embedding, output).  The host entry sums in fp32 in the rule's order, the mirror in float64.  The bound is 4 x
# the measured value, for the spread from seed to seed.
HOST_MEASURED = {
    "tiny": (3.834e-07, 4.978e-08),
    "ten_tokens": (5.745e-07, 5.154e-08),
    "second_tile": (6.004e-07, 6.745e-08),
    "patch4_dh64": (8.143e-07, 6.709e-08),
    "long_rows": (4.405e-07, 3.898e-08),
    "reference_width": (2.097e-06, 1.319e-07),
    "reference_depth": (3.233e-06, 7.693e-08),
    # the shapes of mirror.PATHS, by the same recipe
    "dh32": (6.884e-07, 2.470e-08),
    "dh48": (8.904e-07, 3.398e-08),
    "patch16": (4.856e-07, 3.358e-08),
    "grid_2d": (9.732e-07, 7.990e-08),
    "wide_head": (4.631e-07, 1.183e-07),
    "head2_wider": (5.137e-07, 2.672e-08),
    "most_tokens": (5.110e-07, 1.229e-08),
}


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


@pytest.mark.parametrize("name", ["ten_tokens", "second_tile"])
def test_mirror_equals_dino_vit(capi, name):
    """dino.ViT in float64 through the exporter: the parameter order, pre-norm, the qkv split, GELU, eps, the class token."""
    from openkitchen_amd import dino
    shape = mirror.SHAPES[name]
    torch.manual_seed(3)
    model = dino.ViT(**shape).double().eval()
    with torch.no_grad():  # (LayerNorm weights away from 1 and biases away from 0, so that a swap shows)
        for n, p in model.named_parameters():
            if "norm" in n:
                p.add_(0.2 * torch.randn_like(p))
    sd = model.state_dict()
    cfg = dino.vit_config_from_state_dict(sd, heads=shape["heads"])
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in capi.vit_layout(cfg)]
    assert all(getattr(cfg, k) == v for k, v in shape.items())
    params = dino.vit_params_from_state_dict(sd, heads=shape["heads"], dtype=torch.float64).numpy()
    assert params.size == capi.vit_num_params(cfg)
    frames = torch.randint(0, 256, (3, shape["image_size"], shape["image_size"], 4), dtype=torch.uint8)
    x = dino.frames_to_input(frames, mean=list(cfg.mean), std=list(cfg.std), dtype=torch.float64)
    assert np.abs(x.numpy() - mirror.frames_to_input(cfg, frames.numpy())).max() <= 1e-12
    with torch.no_grad():
        want, want_emb = model(x)[:, 0].numpy(), model.embed(x).numpy()
    emb, out = mirror.forward(capi, cfg, params, x.numpy())
    assert np.abs(out - want).max() <= 1e-9 and np.abs(emb - want_emb).max() <= 1e-9 and np.abs(want).max() > 1e-3


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_host_entry_against_the_mirror(capi, name):
    shape = mirror.SHAPES[name]
    cfg = capi.vit_config(**shape)
    assert capi.vit_tokens(cfg) == mirror.TOKENS[name] and (name in mirror.PATHS) == (name in mirror.NEW_SHAPES) and (name not in mirror.PATHS or mirror.reaches(name))
    worst_emb = worst_out = 0.0
    for seed in range(4):
        rng = np.random.default_rng(seed)
        params = mirror.random_params(capi, cfg, rng)
        frames = rng.integers(0, 256, (2, shape["image_size"], shape["image_size"], 4), dtype=np.uint8)
        got = capi.vit_act_host(cfg, params, frames)
        emb, out = mirror.forward(capi, cfg, params, mirror.frames_to_input(cfg, frames))
        worst_emb, worst_out = max(worst_emb, float(np.abs(got["embedding"] - emb).max())), max(worst_out, float(np.abs(got["output"] - out).max()))
        steer = np.clip(got["output"].astype(np.float64) * 10.0, -10.0, 10.0).astype(f32)
        assert np.array_equal(got["steer"], steer) and np.array_equal(got["throttle"], np.full(2, 100.0, f32)) and list(got["alive"]) == [1, 1]
    print("%s: host entry against float64: embedding %.3e, output %.3e" % (name, worst_emb, worst_out))
    assert worst_emb <= 4 * HOST_MEASURED[name][0] and worst_out <= 4 * HOST_MEASURED[name][1]


def witness_params(capi, cfg, layer):
    """A network whose head sees 1 + 2^-12 whatever the frame: all zero but LayerNorm-free biases.  layer 2: hidden 2's unit 0 is the
    chain bias 1, x (1 + 2^-12), w -(1 - 2^-12) -> 2^-24, handed on with weight 1; layer 3: the output is the chain bias -1,
    x (1 + 2^-12), w (1 - 2^-12) -> -2^-24.  A product rounded on its own is 1 and leaves 0."""
    at = {name: (o, shape) for name, o, shape in capi.vit_layout(cfg)}
    p = np.zeros(capi.vit_num_params(cfg), f32)
    e = 2.0 ** -12
    if layer == 2:
        p[at["head.net.0.bias"][0]] = 1 + e
        p[at["head.net.2.weight"][0]] = -(1 - e)
        p[at["head.net.2.bias"][0]] = 1.0
        p[at["head.output_layer.weight"][0]] = 1.0
    else:
        p[at["head.net.2.bias"][0]] = 1 + e
        p[at["head.output_layer.weight"][0]] = 1 - e
        p[at["head.output_layer.bias"][0]] = -1.0
    return p


def test_linear_chain_is_fused_and_starts_from_the_bias(capi):
    cfg = capi.vit_config(**mirror.SHAPES["tiny"])
    frames = np.random.default_rng(0).integers(0, 256, (1, 16, 16, 4), dtype=np.uint8)
    assert capi.vit_act_host(cfg, witness_params(capi, cfg, 2), frames)["output"][0] == f32(2.0 ** -24)
    assert capi.vit_act_host(cfg, witness_params(capi, cfg, 3), frames)["output"][0] == f32(-2.0 ** -24)


def test_gelu_order_and_steer_clamp(capi):
    """The output layer's weight large: the clamp at +-steer_scale; a NaN-free zero network gives 0."""
    cfg = capi.vit_config(steer_scale=7.0, **mirror.SHAPES["tiny"])
    at = {name: o for name, o, shape in capi.vit_layout(cfg)}
    frames = np.zeros((1, 16, 16, 4), np.uint8)
    p = np.zeros(capi.vit_num_params(cfg), f32)
    for bias, steer in ((0.0, 0.0), (0.5, 3.5), (3.0, 7.0), (-3.0, -7.0)):
        p[at["head.output_layer.bias"]] = bias
        got = capi.vit_act_host(cfg, p, frames)
        assert got["output"][0] == f32(bias) and got["steer"][0] == f32(steer)


BAD_SHAPES = [dict(patch=2), dict(patch=32, image_size=32), dict(image_size=20), dict(image_size=0), dict(image_size=256), dict(dim=0), dict(dim=24), dict(dim=784),
              dict(heads=0), dict(dim=32, heads=4), dict(dim=128, heads=1), dict(dim=48, heads=2), dict(depth=0), dict(depth=13), dict(dim_feedforward=0),
              dict(dim_feedforward=40), dict(dim_feedforward=80), dict(head_hidden1=0), dict(head_hidden1=24), dict(head_hidden1=2064), dict(head_hidden2=8),
              dict(head_hidden2=2064)]
BAD_CONSTS = [(dict(head_hidden1=2048, head_hidden2=2048), "the kernels' LDS (okenv_vit_lds_bytes) does not fit 160 KB"),
              (dict(std=(0.2, -1.0, 0.2)), "mean must be finite, std finite and > 0"), (dict(mean=(0.0, float("inf"), 0.0)), "mean must be finite, std finite and > 0"),
              (dict(ln_eps=float("nan")), "ln_eps must be finite and > 0"), (dict(throttle=float("nan")), "throttle must be finite, steer_scale finite and >= 0"),
              (dict(steer_scale=-1.0), "throttle must be finite, steer_scale finite and >= 0"),
              (dict(workspace_bytes=-5), "agents_per_pass and workspace_bytes must not be negative")]


def test_limits_and_refusals(capi):
    L = capi.load()
    shape = mirror.SHAPES["tiny"]
    good = capi.vit_config(**shape)
    params = np.zeros(capi.vit_num_params(good), f32)
    frames = np.zeros((1, 16, 16, 4), np.uint8)
    out = np.zeros(1, f32)
    assert L.okenv_vit_lds_bytes(None) == 0
    host = lambda cfg, p=params, fr=frames, n=1: L.okenv_vit_act_host(cfg, capi.ptr(p), n, capi.ptr(fr), None, None, None, capi.ptr(out), None, None)  # noqa: E731
    assert host(C.byref(good)) == 0
    for bad in BAD_SHAPES:
        cfg = capi.vit_config(**dict(shape, **bad))
        assert capi.vit_lds_bytes(cfg) == 0 == mirror.lds_bytes(dict(shape, **bad)), bad
        assert host(C.byref(cfg)) == INVALID and L.okenv_last_error(None).startswith(b"okenv_vit_act_host: shape outside the limits (patch 4, 8 or 16;"), bad
    for bad, text in BAD_CONSTS:
        assert host(C.byref(capi.vit_config(**dict(shape, **bad)))) == INVALID and L.okenv_last_error(None) == ("okenv_vit_act_host: " + text).encode(), bad
    assert host(None) == INVALID and L.okenv_last_error(None) == b"okenv_vit_act_host: config is NULL"
    for args in (dict(p=None), dict(fr=None), dict(n=-1)):
        assert host(C.byref(good), **args) == INVALID and L.okenv_last_error(None) == b"okenv_vit_act_host: bad argument"
    assert host(C.byref(good), n=0) == 0
    # every output of the host entry may be NULL, and crashed agents are asked all the same
    full = capi.vit_act_host(good, mirror.random_params(capi, good, np.random.default_rng(1)), np.repeat(frames, 3, axis=0), np.array([0, 1, 9], np.uint8))
    assert list(full["alive"]) == [1, 0, 0] and len(set(full["output"].tolist())) == 1
    # the attention piece
    qkv, ctx = np.zeros((1, 4, 48), f32), np.zeros((1, 4, 16), f32)
    attend = lambda T=4, heads=1, dh=16, q=qkv, c=ctx, seqs=1: L.okenv_debug_vit_attend(-1, seqs, T, heads, dh, capi.ptr(q), capi.ptr(c))  # noqa: E731
    assert attend() == 0
    for args in (dict(T=0), dict(T=1025), dict(heads=0), dict(dh=8), dict(dh=24), dict(dh=80), dict(heads=13, dh=64), dict(q=None), dict(c=None), dict(seqs=-1)):
        assert attend(**args) == INVALID, args
        assert L.okenv_last_error(None).startswith(b"okenv_debug_vit_attend: bad argument"), args
    # a handle's entries without a handle
    n = C.c_int32()
    assert L.okenv_vit_create(None, C.byref(good)) == INVALID and L.okenv_last_error(None) == b"okenv_vit_create: NULL handle"
    assert L.okenv_vit_act(None, None, 0, None) == INVALID and L.okenv_last_error(None) == b"okenv_vit_act: NULL handle"
    for call in (lambda: L.okenv_vit_num_params(None, C.byref(n)), lambda: L.okenv_vit_set_params(None, capi.ptr(params)), lambda: L.okenv_vit_get_params(None, capi.ptr(params))):
        assert call() == INVALID and L.okenv_last_error(None).endswith(b": NULL argument")


def test_attention_sum_is_eight_interleaved_partials(capi):
    """One query, 24 keys, v = 1: q = 0 makes every weight 1 / sum, and keys of very different size make the sum depend on its order:
    the host entry's context is the quotient by the tree of the 8 interleaved partials, not by the sequential sum."""
    T, dh = 24, 16
    rng = np.random.default_rng(4)
    qkv = np.zeros((1, T, 3 * dh), f32)
    qkv[0, :, dh] = rng.uniform(-12.0, 0.0, T)  # k's first column; q's first column is 4 for query 0: scores = k0 (scale 1/4)
    qkv[0, 0, 0] = 4.0
    qkv[0, :, 2 * dh:] = 1.0
    got = capi.debug_vit_attend(qkv, 1)[0, 0]
    s = (f32(4.0) * qkv[0, :, dh]) * f32(0.25)
    e = np.array([np.float32(np.exp(np.float64(v - s.max()))) for v in s], f32)  # (ok_expf is the rounded fp64 exp on all but rare arguments)
    part = [f32(0.0)] * 8
    for t in range(T):
        part[t % 8] = f32(part[t % 8] + e[t])
    tree = f32(f32(f32(part[0] + part[4]) + f32(part[2] + part[6])) + f32(f32(part[1] + part[5]) + f32(part[3] + part[7])))
    acc = f32(0.0)
    for t in range(T):
        acc = f32(np.float64(f32(e[t] / tree)) * 1.0 + np.float64(acc))
    assert got[0] == acc and np.all(got == got[0])


def test_plan_restated(capi):
    """okenv_vit_lds_bytes against the restatement over a grid of shapes, and the kernels' constants against the source."""
    for S, P in ((16, 8), (32, 8), (64, 4), (224, 8), (248, 8), (496, 16), (16, 16)):
        for D, heads in ((16, 1), (64, 1), (64, 4), (384, 6), (768, 12)):
            for h1, h2 in ((16, 16), (128, 64), (2048, 16), (1024, 1024), (2048, 2048)):
                shape = dict(image_size=S, patch=P, dim=D, heads=heads, depth=1, dim_feedforward=4 * D, head_hidden1=h1, head_hidden2=h2)
                assert capi.vit_lds_bytes(capi.vit_config(**shape)) == mirror.lds_bytes(shape) > 0, shape
    assert mirror.lds_bytes(dict(mirror.SHAPES["tiny"], head_hidden1=2048, head_hidden2=2048)) > mirror.LDS_BUDGET
    reference = dict(image_size=224, patch=8, dim=384, heads=6, depth=12, dim_feedforward=1536, head_hidden1=128, head_hidden2=64)
    assert mirror.tokens(reference) == 785 and mirror.lds_bytes(reference) == 4 * 16 * (64 + 4 + 800 + 4) <= mirror.LDS_BUDGET
    assert 4 * mirror.agent_floats(reference) == 785 * 3840 * 4 and mirror.agents_per_pass(reference, 1000) == (1 << 30) // (785 * 3840 * 4) == 89
    assert mirror.agents_per_pass(reference, 16) == 16 and mirror.agents_per_pass(reference, 64, workspace_bytes=1000) == 1
    kernel = open(os.path.join(ROOT, "openkitchen_amd", "csrc", "ok_vit.h")).read()
    constant = lambda name: int(re.search(r"constexpr int %s\s*=\s*(\d+);" % name, kernel).group(1))  # noqa: E731
    assert (constant("kVitTile"), constant("kVitKBlock"), constant("kVitQueries"), constant("kVitAgents")) == (mirror.TILE, mirror.KBLOCK, mirror.QUERIES, mirror.AGENTS)
    assert "kVitDefaultWorkspace = static_cast<size_t>(1) << 30" in kernel
    # ... and the launch geometry's: 256 threads, 8 lanes a LayerNorm row, so 32 rows a workgroup of the norm and embed kernels
    math_h = open(os.path.join(ROOT, "include", "okenv_math.h")).read()
    assert constant("kVitThreads") == mirror.THREADS and int(re.search(r"#define OK_ACTOR_LANES\s+(\d+)", math_h).group(1)) == mirror.LANES
    assert "constexpr int kVitNormRows = kVitThreads / OK_ACTOR_LANES;" in kernel and mirror.NORM_ROWS == mirror.THREADS // mirror.LANES == 32
    head = open(os.path.join(ROOT, "openkitchen_amd", "csrc", "ok_vithead.h")).read()
    assert "r_raw = static_cast<long>(blockIdx.x) * kVitNormRows + static_cast<int>(threadIdx.x) / OK_ACTOR_LANES;" in head
    # ... and what mirror.geometry restates of the launches themselves: every grid, the rows, K and columns of the five linear launches,
    # the ctiles of a column workgroup, the waves of the context phase, the K of the patch embedding
    launches = " ".join(open(os.path.join(ROOT, "openkitchen_amd", "csrc", "okenv_capi.hip")).read().split())
    u = "dim3(static_cast<unsigned>(%s))"
    for text in ("(okVitLinearKernel<kSrc, kEpi>), dim3(static_cast<unsigned>((M + kVitTile - 1) / kVitTile), static_cast<unsigned>((N + kVitTile - 1) / kVitTile)), "
                 "dim3(kVitThreads), 0,",
                 "const long M = static_cast<long>(count) * T;",
                 "const unsigned norm_blocks = static_cast<unsigned>((M + kVitNormRows - 1) / kVitNormRows);",
                 "okVitNormKernel, dim3(norm_blocks), dim3(kVitThreads), 0,",
                 "ap.qtiles = (T + kVitQueries - 1) / kVitQueries;",
                 "okVitAttendKernel, " + u % "count * s.heads * ap.qtiles" + ", dim3(kVitThreads), sizeof(float) * static_cast<size_t>(pl.attend),",
                 "okVitEmbedKernel, " + u % "(count + kVitNormRows - 1) / kVitNormRows" + ", dim3(kVitThreads), 0,",
                 "okVitFinalKernel, " + u % "(count + kVitAgents - 1) / kVitAgents" + ", dim3(kLidarThreads), sizeof(float) * static_cast<size_t>(pl.final),",
                 "vitLinear<kVitSrcPatch, kVitEpiPos>(h, lp, static_cast<long>(count) * (T - 1), ok_vit_patch_k(s), D,",
                 "vitLinear<kVitSrcPlain, kVitEpiNone>(h, lp, M, D, 3 * D,",
                 "vitLinear<kVitSrcPlain, kVitEpiResidual>(h, lp, M, D, D,",
                 "vitLinear<kVitSrcPlain, kVitEpiGelu>(h, lp, M, D, F,",
                 "vitLinear<kVitSrcPlain, kVitEpiResidual>(h, lp, M, F, D,"):
        assert text in launches, text
    assert "const int ctiles = okLidarMin(kVitTile / 16, (p.N - n0) >> 4);" in " ".join(kernel.split()) and "if (wave < dh / 16)" in kernel
    rule = " ".join(open(os.path.join(ROOT, "include", "okenv_vit.h")).read().split())
    assert "OK_HDI int ok_vit_patch_k(const ok_vit_shape s) { return 3 * s.P * s.P; }" in rule


# (rows of an agent, K, columns) of the five linear launches, from the parameter layout's own weight shapes (columns x K)
LINEAR_WEIGHTS = {"patch": "patch_embed.proj.weight", "qkv": "blocks.0.attn.qkv.weight", "proj": "blocks.0.attn.proj.weight", "fc1": "blocks.0.mlp.fc1.weight",
                  "fc2": "blocks.0.mlp.fc2.weight"}
LINEAR_SIZES = {"patch": lambda T, D, F: (T - 1, D), "qkv": lambda T, D, F: (T, 3 * D), "proj": lambda T, D, F: (T, D), "fc1": lambda T, D, F: (T, F),
                "fc2": lambda T, D, F: (T, D)}


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_launch_geometry_restated(capi, name):
    """mirror.geometry at every shape of the table: the LDS plan against okenv_vit_lds_bytes, the grids against a count of the tiles
    one by one, the figures the shapes were chosen for, and each new shape's predicate."""
    shape = mirror.SHAPES[name]
    T, D, F = mirror.tokens(shape), shape["dim"], shape["dim_feedforward"]
    assert not mirror.shape_bad(shape) and T == mirror.TOKENS[name]
    weights = {n: w for n, _, w in capi.vit_layout(capi.vit_config(**shape))}
    for agents in (1, 2, 9, 17, 33, 40):
        g = mirror.geometry(shape, agents)
        assert capi.vit_lds_bytes(capi.vit_config(**shape)) == mirror.lds_bytes(shape) == max(g["attend_lds"], g["final_lds"], 10240)
        for k in mirror.LINEARS:
            rows, N = LINEAR_SIZES[k](T, D, F)
            rows *= agents
            assert (N, g[k]["K"]) == (weights[LINEAR_WEIGHTS[k]][0], int(np.prod(weights[LINEAR_WEIGHTS[k]][1:])))
            tiles = {(m // 64, n // 64) for m in range(0, rows, 16) for n in range(0, N, 16)}  # the workgroup of every 16 x 16 tile of the output
            assert g[k]["grid"] == (max(x for x, _ in tiles) + 1, max(y for _, y in tiles) + 1)
            assert g[k]["ctiles"] == [sum(1 for n in range(0, N, 16) if n // 64 == y) for y in range(g[k]["grid"][1])]
            assert g[k]["last_rows"] == sum(1 for m in range(rows) if m // 64 == g[k]["grid"][0] - 1) and g[k]["last_live_waves"] == -(-g[k]["last_rows"] // 16)
        assert g["attend_blocks"] == agents * shape["heads"] * len(range(0, T, 16)) and g["context_waves"] * 16 * shape["heads"] == D
        assert g["norm_blocks"] == len(range(0, agents * T, 32)) and g["final_blocks"] == len(range(0, agents, 16)) and g["embed_blocks"] == len(range(0, agents, 32))
        assert g["final_last_agents"] == len(range(range(0, agents, 16)[-1], agents))  # the agents from the last workgroup's first on
    assert (name in mirror.PATHS) == (name in mirror.NEW_SHAPES)
    if name in mirror.PATHS:
        assert mirror.reaches(name), name
        assert mirror.lds_bytes(shape) == {"wide_head": 133888, "most_tokens": 67072}.get(name, 10240)
    if name == "grid_2d":
        g = mirror.geometry(shape, 9)
        assert 9 * (T - 1) == 144 and g["patch"]["grid"][0] == 3 and 9 * T == 153 and g["qkv"]["grid"][0] == 3 and g["qkv"]["last_rows"] == 25
        assert (g["proj"]["ctiles"], g["qkv"]["ctiles"], g["fc1"]["ctiles"]) == ([4, 1], [4, 4, 4, 3], [4, 4, 4, 1])
    if name == "wide_head":
        g = mirror.geometry(shape, 17)
        assert g["final_blocks"] == 2 and g["final_last_agents"] == 17 - (g["final_blocks"] - 1) * mirror.AGENTS == 1
    if name == "reference_width":  # several column workgroups on 34 rows: one row workgroup, which is why grid_2d exists
        assert mirror.geometry(shape, 2)["qkv"]["grid"] == (1, 18)


def test_host_forward_stays_inside_its_work_space(tmp_path):
    """The host forward as a stand-alone program under AddressSanitizer and UBSan (tests/cpp/vit_host_check.cpp), on parameters, a frame
    and a work space of exactly the counted sizes: the small shapes of the table and corners of the limits -- a feed-forward narrower
    than the width, one token besides the class token, the widest head."""
    assert mirror.reaches("dh48") and mirror.reaches("patch16")  # (a feed-forward narrower than the width; K 768 of the patch embedding)
    exe = str(tmp_path / "vit_host_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "vit_host_check.cpp")], check=True)
    keys = ("image_size", "patch", "dim", "heads", "depth", "dim_feedforward", "head_hidden1", "head_hidden2")
    shapes = [tuple(mirror.SHAPES[name][k] for k in keys) for name in ("tiny", "ten_tokens", "second_tile", "patch4_dh64", "dh48", "patch16")]
    shapes += [(16, 16, 64, 4, 2, 16, 16, 2048), (4, 4, 16, 1, 1, 64, 2048, 16), (48, 16, 128, 2, 1, 48, 32, 32)]
    assert any(ff < D for S, P, D, heads, depth, ff, h1, h2 in shapes)
    r = subprocess.run([exe] + [str(v) for shape in shapes for v in shape], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(len(shapes))], r.stdout[-1000:] + r.stderr[-4000:]
