"""Pins the CPU oracle against the reference's own compilable translation units (oracle/_ref/libokref.so =
reference Environment/Agent.cpp + Environment/RaceTrack.cpp) and the product's host-side track
builder against both.  The reference's answers to this file's inputs are recorded in tests/golden/ref_answers.npz
(generator make_golden.py): where the shim is built, the reference computes them here and must reproduce the record bit
for bit; everywhere else the record stands in for it."""
import os

import numpy as np
import pytest

import _oracle as O

TRACKS = ["Austin", "Silverstone", "Monza", "Spa"]
NEAREST_TRACKS = ["Austin", "Spa"]
ANSWERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the inputs, and the reference's answers to them computed by its compiled objects (oracle/_ref) ----

def nearest_probes(t):
    rng = np.random.default_rng(1)
    qx = rng.uniform(0, 1600, 3000).astype(np.float32)
    qy = rng.uniform(0, 1400, 3000).astype(np.float32)
    qx[:t.P], qy[:t.P] = t.x, t.y
    return qx, qy


def query_probes(t):
    rng = np.random.default_rng(2)
    qx = rng.uniform(0, 1600, 3000).astype(np.float32)
    qy = rng.uniform(0, 1400, 3000).astype(np.float32)
    qx[:t.P], qy[:t.P] = t.x, t.y
    qx[t.P:2 * t.P], qy[t.P:2 * t.P] = t.li[0::2], t.li[1::2]
    return qx, qy


def kinematics_actions(mode):
    rng = np.random.default_rng(2 + mode)
    n = 3000
    thr = (rng.uniform(0, 100, n) if mode == 0 else rng.uniform(-0.4, 0.6, n)).astype(np.float32)
    steer = rng.uniform(-5, 6, n).astype(np.float32)
    return thr, steer


def ref_track(name):
    t = O.Track(name, "ref")
    return {"%s_%s" % (name, k): getattr(t, k) for k in O.Track.KEYS}


def ref_layout():
    f = np.zeros(4, dtype=np.uint32)
    O.ref().ref_layout_facts(f)
    rays = np.zeros(64, dtype=np.float32)
    n = O.ref().ref_agent_default_rays(rays, 64)
    return {"layout_facts": f, "default_rays": rays[:n].copy()}


def ref_nearest(name):
    qx, qy = nearest_probes(O.Track(name, "oracle"))
    want = np.zeros(qx.size, dtype=np.int32)
    h = O.ref().ref_track_load(O.track_path(name).encode())
    O.ref().ref_nearest_track_idx(h, qx, qy, qx.size, want)
    O.ref().ref_track_free(h)
    return {name + "_nearest": want}


def ref_queries(name):
    qx, qy = query_probes(O.Track(name, "oracle"))
    wb, wl = np.zeros(qx.size, dtype=np.float32), np.zeros(qx.size, dtype=np.float32)
    h = O.ref().ref_track_load(O.track_path(name).encode())
    O.ref().ref_track_queries(h, qx, qy, qx.size, wb, wl)
    O.ref().ref_track_free(h)
    return {name + "_boundary": wb, name + "_lane": wl}


def ref_kinematics(mode):
    thr, steer = kinematics_actions(mode)
    out = [np.zeros(thr.size, dtype=np.float32) for _ in range(5)]
    O.ref().ref_agent_rollout(mode, 700.0, 500.0, 33.0, thr, steer, thr.size, *out)
    return {"kin%d_%s" % (mode, k): a for k, a in zip(("x", "y", "rot", "speed", "acc"), out)}


def ref_reset_probe():
    out = np.zeros(9, dtype=np.float32)
    O.ref().ref_agent_reset_probe(11.0, 22.0, 33.0, out)
    return {"reset_probe": out}


def ref_answers():
    """Everything the tests below ask the reference, from the compiled shim (make_golden.py records it)."""
    out = {}
    for name in TRACKS:
        out.update(ref_track(name))
        out.update(ref_queries(name))
    for name in NEAREST_TRACKS:
        out.update(ref_nearest(name))
    for mode in (0, 1):
        out.update(ref_kinematics(mode))
    out.update(ref_layout())
    out.update(ref_reset_probe())
    return out


def reference(compute, *args):
    """The reference's answers (a mapping of the keys `compute` returns): the recorded ones, which the compiled reference must
    reproduce bit for bit where its shim is built."""
    g = np.load(ANSWERS)
    if O.have_ref():
        for k, v in compute(*args).items():
            assert v.dtype == g[k].dtype and np.array_equal(v.view(np.uint8), g[k].view(np.uint8)), \
                "the reference's answer %s differs from tests/golden/ref_answers.npz" % k
    return g


@pytest.mark.parametrize("name", TRACKS)
def test_track_geometry_bit_equal_to_reference(oracle, name):
    a, b = O.Track(name, "oracle"), reference(ref_track, name)
    for k in O.Track.KEYS:
        assert np.array_equal(bits(getattr(a, k)), bits(b["%s_%s" % (name, k)])), k


@pytest.mark.parametrize("name", TRACKS)
def test_product_track_builder_bit_equal_to_reference(oracle, ok, name):
    a, b = ok.Track(name), reference(ref_track, name)
    assert a.P == b[name + "_x"].size and a.S == 4 * a.P
    for k in O.Track.KEYS:
        assert np.array_equal(bits(getattr(a, k)), bits(b["%s_%s" % (name, k)])), k


def test_layout_facts(oracle):
    r = reference(ref_layout)
    f = r["layout_facts"]
    assert f[0] == 24 and f[1] == 16  # sizeof(Ray_), sizeof(Segment2d)
    assert f[2] == 0x3C8EFA35  # kDeg2Rad
    assert f[3] == 3  # RaceTrack::kStartingIdx
    assert np.array_equal(r["default_rays"], np.arange(-70, 71, 10, dtype=np.float32))


@pytest.mark.parametrize("name", NEAREST_TRACKS)
def test_nearest_index_equal_to_reference(oracle, name):
    t = O.Track(name, "oracle")
    qx, qy = nearest_probes(t)
    want = reference(ref_nearest, name)[name + "_nearest"]
    got = np.zeros(qx.size, dtype=np.int32)
    O.lib().oracle_nearest_track_idx(t.x, t.y, t.P, qx, qy, qx.size, got)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", TRACKS)
def test_track_queries_equal_to_reference(oracle, name):
    """RaceTrack::getNearestDistanceToTrackBoundary / getDistanceToLaneCenter: oracle restatement and the product's own
    RaceTrack (through the C ABI) against the reference's compiled RaceTrack.cpp, bit for bit, 3000 probes."""
    import openkitchen_amd as ok
    t = O.Track(name, "oracle")
    qx, qy = query_probes(t)
    r = reference(ref_queries, name)
    wb, wl = r[name + "_boundary"], r[name + "_lane"]
    gb, gl = np.zeros(qx.size, dtype=np.float32), np.zeros(qx.size, dtype=np.float32)
    O.lib().oracle_boundary_distance(t.li, t.ri, t.P, qx, qy, qx.size, gb)
    O.lib().oracle_lane_center_distance(t.x, t.y, t.wl, t.wr, t.P, qx, qy, qx.size, gl)
    assert np.array_equal(gb.view(np.uint32), wb.view(np.uint32))
    assert np.array_equal(gl.view(np.uint32), wl.view(np.uint32))
    pb, pl = ok.Track(name).queries(qx, qy)
    assert np.array_equal(pb.view(np.uint32), wb.view(np.uint32))
    assert np.array_equal(pl.view(np.uint32), wl.view(np.uint32))


@pytest.mark.parametrize("mode", [0, 1])
def test_kinematics_bit_equal_to_reference_agent(oracle, mode):
    """Oracle kinematics in glibc-trig mode == the reference's Agent::move, bit for bit, over 3000 steps with
    random actions (rot drifts to large unwrapped angles)."""
    thr, steer = kinematics_actions(mode)
    r = reference(ref_kinematics, mode)
    out = [r["kin%d_%s" % (mode, k)] for k in ("x", "y", "rot", "speed", "acc")]
    seg = np.array([[0, 0, 1, 0]], dtype=np.float32)
    env = O.OracleEnv(seg, 1, 1, np.zeros(1, dtype=np.float32))
    env.reset_agents([0], [700.0], [500.0], [33.0])
    env.set(O.F_MODE, np.array([mode], dtype=np.uint8))
    O.lib().oracle_set_trig_mode(1)
    try:
        for s in range(thr.size):
            env.set(O.F_THR, thr[s:s + 1])
            env.set(O.F_STEER, steer[s:s + 1])
            env.set(O.F_DISP_CTR, np.array([1], dtype=np.uint32))  # keep the standstill FSM from firing
            env.move_only()
            got = [env.get(f)[0] for f in (O.F_POS_X, O.F_POS_Y, O.F_ROT, O.F_SPEED, O.F_ACC)]
            for g, w in zip(got, out):
                assert np.float32(g).view(np.uint32) == w[s].view(np.uint32), (s, g, w[s])
    finally:
        O.lib().oracle_set_trig_mode(0)


def test_agent_reset_semantics(oracle):
    out = reference(ref_reset_probe)["reset_probe"]
    assert list(out) == [11.0, 22.0, 33.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    seg = np.array([[0, 0, 1, 0]], dtype=np.float32)
    env = O.OracleEnv(seg, 1, 1, np.zeros(1, dtype=np.float32))
    for f, v in ((O.F_SPEED, 5), (O.F_ACC, 6), (O.F_THR, 7), (O.F_STEER, 8)):
        env.set(f, np.array([v], dtype=np.float32))
    env.set(O.F_CRASHED, np.array([1], dtype=np.uint8))
    env.set(O.F_TIMED_OUT, np.array([1], dtype=np.uint8))
    env.set(O.F_DISP_CTR, np.array([77], dtype=np.uint32))
    env.reset_agents([0], [11.0], [22.0], [33.0])
    s = env.snapshot()
    got = [s[k][0] for k in ("pos_x", "pos_y", "rot", "speed", "acc", "crashed", "timed_out", "thr", "steer")]
    assert got == [11.0, 22.0, 33.0, 0.0, 0.0, 0, 0, 0.0, 0.0]
    assert s["disp_ctr"][0] == 77  # DisplacementStats survive resets
