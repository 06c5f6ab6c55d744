"""The bird's-eye views' draw list on the host (no GPU): okenv_track_band_triangles lists the reference's six band draws
(Visualizer::render -> shadeAreaBetweenCurves) exactly as the independent numpy restatement in _bev_numpy builds them from the
Track's boundary polylines -- same triangles, same vertex order, same ordinals, 6P of them."""
import ctypes as C

import numpy as np
import pytest

import _bev_numpy as bev

TRACKS = ["Austin", "Silverstone", "Monza", "Spa"]
NEW_SYMBOLS = ["okenv_render_create", "okenv_render_views", "okenv_render_get_info", "okenv_track_band_triangles"]


@pytest.mark.parametrize("name", TRACKS)
def test_band_triangles_match_the_numpy_draw_list(ok, name):
    t = ok.Track(name)
    xy, ordinal = t.band_triangles()
    ref_xy, ref_ord = bev.draw_list(t)
    assert xy.shape == (6 * t.P, 3, 2) and ordinal.shape == (6 * t.P,)
    assert np.array_equal(ordinal, ref_ord)
    assert xy.tobytes() == ref_xy.tobytes()
    # ordinals in draw order: three polyline draws of 2(P-1) triangles, then the three seam quads of two each
    expect = np.repeat(np.arange(6, dtype=np.uint8), [2 * (t.P - 1)] * 3 + [2] * 3)
    assert np.array_equal(ordinal, expect)
    # the seam quad between start_line_ = {ro.front, ro.back} and finish_line_ = {lo.front, lo.back} (RaceTrack.cpp:12-13)
    ro, lo = t.ro.reshape(-1, 2), t.lo.reshape(-1, 2)
    seam = {tuple(v) for v in xy[ordinal == 3].reshape(-1, 2)}
    assert seam == {tuple(ro[0]), tuple(ro[-1]), tuple(lo[0]), tuple(lo[-1])}


def test_band_triangles_cap_and_count(ok):
    L = ok.capi.load()
    t = ok.Track("Austin")
    h = C.c_void_p()
    ok.capi.check(L.okenv_track_load(C.byref(h), t.path.encode()))
    try:
        assert L.okenv_track_band_triangles(h, None, None, 0) == 6 * t.P
        xy = np.full((5, 6), -7.0, dtype=np.float32)
        o = np.full(5, 99, dtype=np.uint8)
        assert L.okenv_track_band_triangles(h, ok.capi.ptr(xy[:4]), ok.capi.ptr(o[:4]), 4) == 6 * t.P
        assert (xy[4] == -7.0).all() and o[4] == 99  # nothing written past the cap
        full, _ = t.band_triangles()
        assert np.array_equal(xy[:4], full[:4].reshape(4, 6))
        assert L.okenv_track_band_triangles(h, None, None, -1) == -1
    finally:
        L.okenv_track_free(h)
    assert L.okenv_track_band_triangles(None, None, None, 0) == -1


def test_render_symbols_are_exported(ok):
    lib = C.CDLL(ok.capi.lib_path())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in ok.capi.SYMBOLS


def test_render_entry_points_reject_a_null_handle(ok):
    L = ok.capi.load()
    d = ok.capi.OkenvViewDesc()
    p = np.zeros(8, dtype=np.float32)
    assert L.okenv_render_create(None, *(ok.capi.ptr(p) for _ in range(4)), 4, C.byref(d)) == -1
    assert L.okenv_render_views(None, None, 0) == -1
    assert L.okenv_render_get_info(None, None) == -1


@pytest.mark.parametrize("name", ["Austin", "Silverstone"])
def test_numpy_prefilter_is_the_full_test(ok, name):
    """The restatement's per-view prefilter drops only triangles that contain none of the view's samples."""
    scene = bev.Scene(ok.Track(name))
    rng = np.random.default_rng(7)
    li = ok.Track(name).li.reshape(-1, 2)
    for k in rng.choice(len(li), 3, replace=False):
        for heading_up in (False, True):
            sc = (np.float32(np.sin(0.3 * k)), np.float32(np.cos(0.3 * k)))
            a = bev.render_view(scene, li[k, 0], li[k, 1], sc, False, 24, 21, heading_up=heading_up)
            b = bev.render_view(scene, li[k, 0], li[k, 1], sc, False, 24, 21, heading_up=heading_up, prefilter=False)
            assert np.array_equal(a, b)
