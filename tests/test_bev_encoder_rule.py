"""The image encoder's rule (include/okenv_bev.h) without a GPU: the float64 mirror against the PyTorch encoder through the exporter,
the host entry okenv_bev_encode_host against the mirror, the rule's edges by hand-computed expectation, the limits of the shape, the
LDS plan, the launch geometry restated and the path each shape was chosen for, and the C ABI's refusals."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import _bev_encoder_numpy as mirror

f32 = np.float32
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SHAPES = tuple(mirror.SHAPES)  # every shape a device case is held to the host entry at

# The bound on |host entry - float64 mirror| of the embedding, from the same frames and fp32 parameters: the largest deviation measured
# here per shape over its four seeds (mirror.HOST_SEEDS: 0 .. 3 wherever those draws pass half of every layer's outputs through its
# ReLU; two frames a seed: random bytes and a rendered-looking one; parameters of mirror.draw_params), times 4, the project's margin
# for an fp32 chain against float64.  The largest |embedding| of a run is 0.15 .. 0.37; per seed the deviations were
#   tiny          5.34e-8, 5.18e-8, 5.60e-8, 3.01e-8        odd           4.56e-8, 5.94e-8, 5.66e-8, 5.61e-8
#   reference     1.16e-7, 1.13e-7, 9.95e-8, 1.28e-7        mixed         6.26e-8, 6.61e-8, 7.55e-8, 8.71e-8
#   front4_back8  6.01e-8, 4.65e-8, 7.75e-8, 5.38e-8  (seeds 0, 2, 4, 5)
#   front4_ragged 5.55e-8, 5.19e-8, 5.63e-8, 7.09e-8  (seeds 0, 2, 4, 5)
#   back4_tiles   6.48e-8, 6.38e-8, 3.75e-8, 4.54e-8        back8_ragged  6.45e-8, 5.87e-8, 6.15e-8, 7.72e-8
#   both4_tiles   7.34e-8, 5.47e-8, 6.22e-8, 5.18e-8  (seeds 0, 3, 4, 5)
MEASURED_DEVIATION = {"tiny": 5.60e-8, "odd": 5.94e-8, "reference": 1.28e-7, "mixed": 8.72e-8, "front4_back8": 7.75e-8, "front4_ragged": 7.10e-8,
                      "back4_tiles": 6.49e-8, "back8_ragged": 7.73e-8, "both4_tiles": 7.34e-8}
TOL = {name: 4 * v for name, v in MEASURED_DEVIATION.items()}


@pytest.fixture(scope="module")
def capi(ok):
    return ok.capi


def config(capi, name_or_members):
    members = mirror.SHAPES[name_or_members] if isinstance(name_or_members, str) else name_or_members
    return capi.bev_config(**members)


def test_mirror_equals_torch_encoder(capi):
    """The mirror against flow.BEVEncoder in float64 through the exporter: the parameter order, the padding, the stride, the /255
    and the pool."""
    from openkitchen_amd import flow
    cfg = mirror.SHAPES["reference"]
    torch.manual_seed(0)
    enc = flow.BEVEncoder().double().eval()
    with torch.no_grad():  # move the biases, so that a swapped pair shows
        for name, p in enc.named_parameters():
            if name.endswith("bias"):
                p.add_(0.2 * torch.randn_like(p))
    sd = enc.state_dict()
    got_cfg = flow.bev_config_from_state_dict(sd)
    assert (got_cfg.image_size, tuple(got_cfg.kernel), tuple(got_cfg.channels), got_cfg.embed_dim) == (128, (5, 3, 3), (32, 64, 128), 128)
    params = flow.bev_params_from_state_dict(sd, dtype=torch.float64).numpy()
    assert params.size == mirror.num_params(cfg) == capi.bev_num_params(got_cfg)
    assert [(n, a, tuple(s)) for n, a, s in capi.bev_layout(got_cfg)] == [(n, a, tuple(s)) for n, a, s in mirror.layout(cfg)]
    frames = np.random.default_rng(0).integers(0, 256, (2, 128, 128, 4), dtype=np.uint8)
    # (frames_to_input divides in float32, the mirror in float64: the module's input is made here in float64, the same way)
    x32 = flow.frames_to_input(torch.from_numpy(frames))
    assert tuple(x32.shape) == (2, 3, 128, 128) and np.array_equal(x32.numpy(), (frames[..., :3].transpose(0, 3, 1, 2) / f32(255.0)).astype(f32))
    with torch.no_grad():
        want = enc(torch.from_numpy(frames[..., :3].astype(np.float64).transpose(0, 3, 1, 2) / 255.0)).numpy()
    got = mirror.forward(cfg, params, frames)
    print("mirror vs torch float64: %.3e" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-9
    # the whole policy's state dict gives the same vector
    policy = flow.ConditionalFlowMatchingPolicy().double()
    policy.bev_encoder.load_state_dict(sd)
    assert np.array_equal(flow.bev_params_from_state_dict(policy.state_dict(), dtype=torch.float64).numpy(), params)


@pytest.fixture(scope="module")
def host_runs(capi):
    """Per shape and seed: (deviation of the host entry from the mirror, the fraction of positive outputs of every layer)."""
    runs = {}
    for name in HOST_SHAPES:
        cfg = mirror.SHAPES[name]
        for seed in mirror.HOST_SEEDS[name]:
            params, frames = mirror.draw_params(cfg, seed), mirror.draw_frames(cfg["image_size"], seed)
            want, acts = mirror.forward(cfg, params, frames, layers=True)
            got = capi.bev_encode_host(config(capi, name), params, frames)
            assert got.dtype == f32 and got.shape == want.shape and np.isfinite(got).all()
            runs[name, seed] = (float(np.abs(got.astype(np.float64) - want).max()), [float((a > 0).mean()) for a in acts], float(np.abs(want).max()))
    return runs


@pytest.mark.parametrize("name", HOST_SHAPES)
def test_host_entry_against_mirror(host_runs, name):
    seeds = mirror.HOST_SEEDS[name]
    # four seeds, the first from 0 upward at which the mirror alone meets the condition asserted below: every seed skipped misses it
    assert len(seeds) == 4 and list(seeds) == sorted(set(seeds)) and seeds[0] >= 0
    for skipped in sorted(set(range(seeds[-1])) - set(seeds)):
        assert not mirror.passes_half(mirror.SHAPES[name], skipped), (name, skipped)
    worst = max(host_runs[name, seed][0] for seed in seeds)
    for seed in seeds:
        dev, positive, scale = host_runs[name, seed]
        print("%s seed %d: deviation %.3e, positive %s, largest |embedding| %.3f" % (name, seed, dev, ["%.2f" % f for f in positive], scale))
        assert all(f >= 0.5 for f in positive), "a layer's ReLU clamps more than half of its outputs: the draw does not test the chain"
    assert worst <= TOL[name], (worst, TOL[name])


# ---- the edges, by hand-computed expectation ------------------------------------------------------------------------------------------

def exact_conv(plane, k, weight, bias):
    """One channel to one channel in exact arithmetic: plane a list of rows of Fractions, stride 2, padding k // 2, one weight per tap
    (weight(ty, tx)), ReLU."""
    side_in, side, p = len(plane), len(plane) // 2, k // 2
    out = [[bias] * side for _ in range(side)]
    for oy in range(side):
        for ox in range(side):
            acc = bias
            for ty in range(k):
                for tx in range(k):
                    y, x = 2 * oy + ty - p, 2 * ox + tx - p
                    if 0 <= y < side_in and 0 <= x < side_in:
                        acc += plane[y][x] * weight(ty, tx)
            out[oy][ox] = max(acc, Fraction(0))
    return out


def one_channel_params(cfg, w0, w1, w2, proj):
    """A parameter vector in which only channel 0 of every layer lives: layer 0 reads the red plane with w0(ty, tx), layers 1 and 2
    read channel 0 with w1, w2; proj[e] weighs the pooled channel 0.  Biases 0."""
    params = np.zeros(mirror.num_params(cfg), f32)
    p = mirror.split(cfg, params)  # views
    for l, w in enumerate((w0, w1, w2)):
        k = cfg["kernel"][l]
        for ty in range(k):
            for tx in range(k):
                p["conv.%d.weight" % (2 * l)][0, 0, ty, tx] = float(w(ty, tx))
    p["proj.weight"][:, 0] = proj
    return params


def test_all_zero_frame_gives_the_chain_of_biases(capi):
    """With a zero frame every term of layer 0's chains is a zero: its outputs are relu(bias), whatever the weights.  Layers 1 and 2
    here have zero weights, so theirs are relu(bias) too, the pool of P equal dyadic values is that value, and the embedding is
    proj.weight relu(conv.4.bias) + proj.bias -- all in multiples of 1/8, exact in fp32 in any order."""
    for name in ("tiny", "odd"):
        cfg = mirror.SHAPES[name]
        rng = np.random.default_rng(7)
        params = np.zeros(mirror.num_params(cfg), f32)
        p = mirror.split(cfg, params)
        p["conv.0.weight"][...] = rng.uniform(-1, 1, p["conv.0.weight"].shape)  # (never meets a non-zero input)
        for key in ("conv.0.bias", "conv.2.bias", "conv.4.bias", "proj.bias", "proj.weight"):
            p[key][...] = rng.integers(-16, 17, p[key].shape) / 8.0
        frames = np.zeros((2, cfg["image_size"], cfg["image_size"], 4), np.uint8)
        frames[..., 3] = 255  # alpha is not an input
        want = p["proj.weight"].astype(np.float64) @ np.maximum(p["conv.4.bias"].astype(np.float64), 0.0) + p["proj.bias"]
        got = capi.bev_encode_host(config(capi, name), params, frames)
        assert np.array_equal(got.astype(np.float64), np.stack([want, want]))


@pytest.mark.parametrize("corner", ["top_left", "bottom_right"])
def test_one_corner_pixel_changes_exactly_the_windows_that_contain_it(capi, corner):
    """Layer 0 weighs the red plane with a different power of two per tap, so an output names the tap under which it saw the pixel;
    layers 1 and 2 sum their windows, the pool sums everything.  The expectation is exact arithmetic on the one channel that lives."""
    for name in ("tiny", "odd"):
        cfg = mirror.SHAPES[name]
        S, k = cfg["image_size"], cfg["kernel"]
        w0 = lambda ty, tx: Fraction(2) ** (ty * k[0] + tx - 12)
        ones = lambda ty, tx: Fraction(1)
        params = one_channel_params(cfg, w0, ones, ones, proj=1.0)
        frames = np.zeros((1, S, S, 4), np.uint8)
        at = (0, 0) if corner == "top_left" else (S - 1, S - 1)
        frames[0, at[0], at[1], 0] = 255
        frames[0, at[0], at[1], 1:] = (17, 99, 3)  # green, blue and alpha meet zero weights
        plane = [[Fraction(int(frames[0, y, x, 0]), 255) for x in range(S)] for y in range(S)]
        a = exact_conv(exact_conv(exact_conv(plane, k[0], w0, Fraction(0)), k[1], ones, Fraction(0)), k[2], ones, Fraction(0))
        total = sum(sum(row) for row in a)
        assert total > 0
        want = float(total / (len(a) * len(a)))
        got = capi.bev_encode_host(config(capi, name), params, frames)
        assert np.array_equal(got, np.full((1, cfg["embed_dim"]), want, f32)), (got[0, :4], want)


def test_white_frame_with_an_exact_channel(capi):
    """Every pixel 255 / 255 = 1.0f; channel 0 of layer 0 weighs all three colours by 1/8 (the other test weighs one), layers 1 and 2
    by 1/4: every partial sum is a small multiple of 2^-7, exact in fp32, so the embedding is the exact count of taps inside the
    image, layer over layer."""
    for name in ("tiny", "odd"):
        cfg = mirror.SHAPES[name]
        S, k = cfg["image_size"], cfg["kernel"]
        eighth, quarter = (lambda ty, tx: Fraction(1, 8)), (lambda ty, tx: Fraction(1, 4))
        params = one_channel_params(cfg, eighth, quarter, quarter, proj=0.5)
        p = mirror.split(cfg, params)
        p["conv.0.weight"][0, 1:, :, :] = 0.125
        p["proj.bias"][...] = 2.0
        frames = np.full((1, S, S, 4), 255, np.uint8)
        plane = [[Fraction(3)] * S for _ in range(S)]  # the three colours' sum
        a = exact_conv(exact_conv(exact_conv(plane, k[0], eighth, Fraction(0)), k[1], quarter, Fraction(0)), k[2], quarter, Fraction(0))
        want = float(sum(sum(row) for row in a) / (len(a) * len(a)) / 2 + 2)
        assert want == f32(want)
        got = capi.bev_encode_host(config(capi, name), params, frames)
        assert np.array_equal(got, np.full((1, cfg["embed_dim"]), want, f32)), (got[0, :4], want)


# ---- the limits ---------------------------------------------------------------------------------------------------------------------------

def legal(members):
    S, k, c, E = members["image_size"], members["kernel"], members["channels"], members["embed_dim"]
    return (16 <= S <= 128 and S % 8 == 0 and all(x in (3, 5) for x in k) and all(16 <= x <= 128 and x % 16 == 0 for x in c)
            and 16 <= E <= 512 and E % 16 == 0)


def test_shape_limits(capi):
    """ok_bev_shape_bad at every limit, seen through okenv_bev_lds_bytes (0 outside) and the host entry's refusal."""
    base = mirror.SHAPES["tiny"]
    frames, out = np.zeros((1, 128, 128, 4), np.uint8), np.zeros((1, 512), f32)
    cases = [dict(image_size=v) for v in (8, 15, 16, 20, 24, 120, 128, 136, 0, -16)]
    cases += [dict(embed_dim=v) for v in (0, 8, 16, 24, 32, 512, 520, 528)]
    for l in range(3):
        for v in (1, 2, 3, 4, 5, 7):
            cases.append(dict(kernel=tuple(v if i == l else 3 for i in range(3))))
        for v in (0, 8, 16, 24, 32, 128, 136, 144):
            cases.append(dict(channels=tuple(v if i == l else 16 for i in range(3))))
    seen = set()
    for change in cases:
        members = dict(base, **change)
        cfg = config(capi, members)
        ok_shape = legal(members)
        seen.add(ok_shape)
        assert (capi.bev_lds_bytes(cfg) > 0) == ok_shape, members
        rc = capi.load().okenv_bev_encode_host(C.byref(cfg), capi.ptr(np.zeros(mirror.num_params(members) if ok_shape else 1, f32)), 1,
                                               capi.ptr(frames), capi.ptr(out))
        assert (rc == 0) == ok_shape, members
        if not ok_shape:
            assert rc == INVALID and b"okenv_bev_encode_host: shape outside the limits" in capi.load().okenv_last_error(None)
    assert seen == {True, False}
    assert capi.load().okenv_bev_lds_bytes(None) == 0


def test_lds_plan_over_every_legal_shape(capi):
    """okenv_bev_lds_bytes and okenv_bev_tiles against the mirror's restatement of the plan, all at or below 160 KB.  (The embedding
    width is not part of the plan: its two ends are run.)"""
    widths = range(16, 129, 16)
    largest = 0
    for S in range(16, 129, 8):
        for k in itertools.product((3, 5), repeat=3):
            for c0, c1 in itertools.product(widths, repeat=2):
                members = dict(image_size=S, kernel=k, channels=(c0, c1, 16), embed_dim=16)
                want, got = mirror.lds_bytes(members), capi.bev_lds_bytes(config(capi, members))
                assert got == want and 0 < got <= mirror.LDS_BUDGET, (members, got, want)
                largest = max(largest, got)
    for S, k, c2, E in itertools.product((16, 48, 128), ((3, 3, 3), (5, 5, 5)), widths, (16, 512)):  # (c2 and E are not part of it either)
        members = dict(image_size=S, kernel=k, channels=(32, 64, c2), embed_dim=E)
        assert capi.bev_lds_bytes(config(capi, members)) == mirror.lds_bytes(members)
    print("largest plan: %d bytes" % largest)
    for name, members in mirror.SHAPES.items():
        assert capi.bev_tiles(config(capi, members)) == mirror.tiles(members) == mirror.PATHS[name], name
    assert set(mirror.PATHS.values()) == {(4, 4), (4, 8), (8, 4), (8, 8)}  # every path the two kernels have


# (LDS bytes, parameters) of the shapes that exist for a path of the kernels, as they were computed when the shapes were chosen
NEW_FIGURES = {"front4_ragged": (69356, 57392), "back4_tiles": (63008, 70496), "back8_ragged": (34828, 5360), "both4_tiles": (70508, 523472)}


def tiles_by_hand(side, T, reads):
    """The tiles of an output `side` wide, pixel by pixel: per tile along one axis its width, and whether every input pixel its
    outputs' windows read -- reads(o): (the input image's side, the input pixels output o reads), per layer under the tile, all T
    outputs of the tile whether they are stored or not -- lies inside the image."""
    out = []
    for o0 in range(0, side, T):
        pixels = [reads(o) for o in range(o0, o0 + T)]
        out.append((len(range(o0, min(o0 + T, side))), all(0 <= p < of for per_layer in pixels for of, ps in per_layer for p in ps)))
    return out


@pytest.mark.parametrize("name", list(mirror.SHAPES))
def test_launch_geometry_restated(capi, name):
    """mirror.geometry at every shape of the table against a count of the tiles pixel by pixel, and the predicate the shape was chosen
    for (mirror.REACHES)."""
    shape = mirror.SHAPES[name]
    assert set(mirror.REACHES) == set(mirror.SHAPES) == set(mirror.PATHS) == set(mirror.HOST_SEEDS) and set(NEW_FIGURES) == set(mirror.NEW_SHAPES)
    S, (k0, k1, k2) = shape["image_size"], shape["kernel"]
    window = lambda o, k: range(2 * o - k // 2, 2 * o - k // 2 + k)  # noqa: E731  (stride 2, padding k // 2)
    for frames in (1, 2, 3, 5):
        g = mirror.geometry(shape, frames)
        assert (g["front"]["T"], g["back"]["T"]) == mirror.PATHS[name] == capi.bev_tiles(config(capi, name))

        def front_reads(o):
            of_layer0 = list(window(o, k1))
            return [(S // 2, of_layer0), (S, [p for q in of_layer0 for p in window(q, k0)])]

        for key, side, reads in (("front", S // 4, front_reads), ("back", S // 8, lambda o: [(S // 4, list(window(o, k2)))])):
            by_hand = tiles_by_hand(side, g[key]["T"], reads)
            assert g[key]["tiles"] == len(by_hand) and g[key]["last_width"] == by_hand[-1][0] and all(w == g[key]["T"] for w, _ in by_hand[:-1])
            assert g[key]["interior_tiles"] == [t for t, (w, inside) in enumerate(by_hand) if inside] and g[key]["interior"] == any(i for _, i in by_hand)
            assert g[key]["row_tiles"] * 16 == g[key]["T"] ** 2
        assert (g["front_blocks"], g["back_blocks"], g["head_blocks"]) == (frames * g["front"]["tiles"] ** 2, frames * g["back"]["tiles"] ** 2, frames)
        # layer 0 under a front tile: the T outputs of layer 1 along an axis read p1 pixels of layer 0, all of them computed
        p1 = len({q for o in range(g["front"]["T"]) for q in window(o, k1)})
        assert g["layer0_rows"] == p1 * p1 and g["layer0_row_blocks"] == len(range(0, p1 * p1, 64))
        assert g["layer0_last_rows"] == len(range(range(0, p1 * p1, 64)[-1], p1 * p1))
    assert mirror.reaches(name), (name, mirror.geometry(shape, mirror.REACHES[name][0]))
    if name in NEW_FIGURES:
        assert (mirror.lds_bytes(shape), mirror.num_params(shape)) == NEW_FIGURES[name] and capi.bev_num_params(config(capi, name)) == NEW_FIGURES[name][1]
    # over the whole table: either tile side in either kernel with one tile, with exact tiles and with a partial tile behind full ones
    geo = {n: mirror.geometry(s) for n, s in mirror.SHAPES.items()}
    # (a lone partial tile of 4 in front would need a layer 1 below 4 pixels, a frame below 16)
    for key, lone4 in (("front", (4, True, False)), ("back", (4, False, True))):
        seen = {(g[key]["T"], g[key]["tiles"] > 1, g[key]["last_width"] < g[key]["T"]) for g in geo.values()}
        assert seen >= {(4, True, True), lone4, (8, True, True), (8, True, False), (8, False, True)}, (key, seen)
    assert any(g["front"]["T"] == 8 and g["front"]["tiles"] == 3 and g["front"]["interior"] and g["front"]["last_width"] < 8 for g in geo.values())


def squeezed(*path):
    return " ".join(open(os.path.join(ROOT, *path)).read().split())


def test_geometry_rests_on_the_source():
    """The constants, the okConv instantiations, the two choices of okBevPlaces and the tile decode that mirror.geometry restates,
    pinned to the source text: a change to any of them fails here and not only in a device case."""
    bev, launch = squeezed("openkitchen_amd", "csrc", "ok_bev.h"), squeezed("openkitchen_amd", "csrc", "okenv_capi.hip")
    assert int(re.search(r"constexpr int kBevThreads\s*=\s*(\d+);", bev).group(1)) == mirror.THREADS == 256
    assert "constexpr int kBevWaves = kBevThreads / 64;" in bev and mirror.WAVES == mirror.THREADS // 64
    assert "constexpr size_t kBevLdsBudget = 160U * 1024U;" in bev and mirror.LDS_BUDGET == 160 * 1024
    assert len(re.findall(r"okConv<", bev)) == 3
    assert bev.count("okConv<OkBevPlanarTaps, 4, kBevWaves, true>(j, to);") == 1 and mirror.LAYER0_ROW_TILES == 4
    assert bev.count("okConv<OkConvWalk, T * T / 16, kBevWaves, true>(j, to);") == 2
    for text in ("at.ta = (ok_bev_side(s, 1) > 4 && static_cast<size_t>(okBevFrontFloats(s, 8)) <= budget) ? 8 : 4;",
                 "at.tb = (ok_bev_side(s, 2) > 4 && static_cast<size_t>(okBevBackFloats(s, 8)) <= budget) ? 8 : 4;",
                 "const size_t budget = kBevLdsBudget / sizeof(float);", "at.p1 = 2 * (at.ta - 1) + s.k[1];", "at.p0 = 2 * (at.p1 - 1) + s.k[0];",
                 "at.p2 = 2 * (at.tb - 1) + s.k[2];",
                 # the front kernel's tile decode and the origins of its two patches
                 "S = sh.S, side0 = S >> 1, side1 = S >> 2, tiles = (side1 + T - 1) / T;",
                 "b = static_cast<int>(blockIdx.x), n = b / (tiles * tiles), t = b - n * tiles * tiles, ty = t / tiles, tx = t - ty * tiles;",
                 "const int y1 = T * ty, x1 = T * tx, y0 = 2 * y1 - sh.k[1] / 2, x0 = 2 * x1 - sh.k[1] / 2, yf = 2 * y0 - sh.k[0] / 2, xf = 2 * x0 - sh.k[0] / 2;",
                 "j.W = pl.p1, j.M = pl.p1 * pl.p1, j.Cout = sh.c[0];",
                 # the back kernel's
                 "side1 = sh.S >> 2, side2 = sh.S >> 3, tiles = (side2 + T - 1) / T, c1 = sh.c[1], c14 = c1 >> 2;",
                 "const int y2 = T * ty, x2 = T * tx, y1 = 2 * y2 - sh.k[2] / 2, x1 = 2 * x2 - sh.k[2] / 2;",
                 "j.W = T, j.M = T * T, j.Cout = sh.c[2];", "j.W = T, j.M = T * T, j.Cout = sh.c[1];"):
        assert text in bev, text
    assert bev.count("b = static_cast<int>(blockIdx.x), n = b / (tiles * tiles), t = b - n * tiles * tiles, ty = t / tiles, tx = t - ty * tiles;") == 2
    for text in ("const auto tiles = [](const int side, const int t) { return static_cast<unsigned>((side + t - 1) / t); };",
                 "ta = tiles(ok_bev_side(s, 1), pl.ta), tb = tiles(ok_bev_side(s, 2), pl.tb);",
                 "hipLaunchKernelGGL(pl.ta == 8 ? okBevFrontKernel<8> : okBevFrontKernel<4>, dim3(N * ta * ta), dim3(kBevThreads), front, h->stream, p);",
                 "hipLaunchKernelGGL(pl.tb == 8 ? okBevBackKernel<8> : okBevBackKernel<4>, dim3(N * tb * tb), dim3(kBevThreads), back, h->stream, p);",
                 "hipLaunchKernelGGL(okBevHeadKernel, dim3(N), dim3(kBevThreads), 0, h->stream, p);"):
        assert text in launch, text


def test_host_entry_refuses_bad_arguments(capi, ok):
    L = capi.load()
    cfg = config(capi, "tiny")
    params, frames, out = np.zeros(mirror.num_params(mirror.SHAPES["tiny"]), f32), np.zeros((1, 16, 16, 4), np.uint8), np.zeros((1, 16), f32)
    args = [C.byref(cfg), capi.ptr(params), 1, capi.ptr(frames), capi.ptr(out)]
    assert L.okenv_bev_encode_host(*args) == 0
    for i in (0, 1, 3, 4):
        bad = list(args)
        bad[i] = None
        assert L.okenv_bev_encode_host(*bad) == INVALID, i
        assert b"okenv_bev_encode_host" in L.okenv_last_error(None)
    assert L.okenv_bev_encode_host(args[0], args[1], -1, args[3], args[4]) == INVALID
    assert L.okenv_bev_encode_host(args[0], args[1], 0, args[3], args[4]) == 0
    tiles = (C.c_int32 * 2)()
    assert L.okenv_bev_tiles(None, tiles) == INVALID and L.okenv_bev_tiles(C.byref(cfg), None) == INVALID
    # a wrong frame size is the device entry's refusal (frame_bytes); on the host side the binding's own check catches the shape
    with pytest.raises(AssertionError):
        capi.bev_encode_host(cfg, params, np.zeros((1, 16, 8, 4), np.uint8))
