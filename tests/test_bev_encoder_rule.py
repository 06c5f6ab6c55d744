"""The image encoder's rule (include/okenv_bev.h) without a GPU: the float64 mirror against the PyTorch encoder through the exporter,
the host entry okenv_bev_encode_host against the mirror, the rule's edges by hand-computed expectation, the limits of the shape, the
LDS plan and the C ABI's refusals."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import _bev_encoder_numpy as mirror

f32 = np.float32
INVALID = -1
SEEDS = (0, 1, 2, 3)
HOST_SHAPES = ("tiny", "odd", "reference")

# The bound on |host entry - float64 mirror| of the embedding, from the same frames and fp32 parameters: the largest deviation measured
# here per shape over seeds 0 .. 3 (two frames a seed: random bytes and a rendered-looking one; parameters of mirror.draw_params),
# times 4, the project's margin for an fp32 chain against float64.  The largest |embedding| of a run is 0.15 .. 0.35; per seed the
# deviations were tiny 5.34e-8, 5.18e-8, 5.60e-8, 3.01e-8; odd 4.56e-8, 5.94e-8, 5.66e-8, 5.61e-8; reference 1.16e-7, 1.13e-7,
# 9.95e-8, 1.28e-7.
MEASURED_DEVIATION = {"tiny": 5.60e-8, "odd": 5.94e-8, "reference": 1.28e-7}
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
        for seed in SEEDS:
            params, frames = mirror.draw_params(cfg, seed), mirror.draw_frames(cfg["image_size"], seed)
            want, acts = mirror.forward(cfg, params, frames, layers=True)
            got = capi.bev_encode_host(config(capi, name), params, frames)
            assert got.dtype == f32 and got.shape == want.shape and np.isfinite(got).all()
            runs[name, seed] = (float(np.abs(got.astype(np.float64) - want).max()), [float((a > 0).mean()) for a in acts], float(np.abs(want).max()))
    return runs


@pytest.mark.parametrize("name", HOST_SHAPES)
def test_host_entry_against_mirror(host_runs, name):
    worst = max(host_runs[name, seed][0] for seed in SEEDS)
    for seed in SEEDS:
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
