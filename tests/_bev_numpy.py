"""Independent numpy-float32 restatement of the bird's-eye view rule (include/okenv.h).

The draw list is built here from the Track's four boundary polylines, following the reference's Visualizer::render /
shadeAreaBetweenCurves, not taken from the library.  Every sample of a view is tested against every triangle whose bounding
box comes within a margin of the view's samples (the others are far from all of them), and its band is the largest draw
ordinal among the triangles that contain it.  All arithmetic is float32 without fused multiply-adds, as in the kernel.
"""
import numpy as np

f32 = np.float32
OK_DEG2RAD = f32(0.01745329238474369049072265625)
BAND_RGB = {-1: (0, 0, 0), 0: (0, 0, 255), 4: (0, 0, 255), 1: (255, 0, 0), 5: (255, 0, 0), 2: (0, 255, 0), 3: (0, 255, 0)}
BAND_CLASS = {-1: 0, 0: 1, 4: 1, 1: 2, 5: 2, 2: 3, 3: 3}
FOLLOW_W, FOLLOW_H = f32(1600) / f32(15), f32(1400) / f32(15)
PREFILTER_MARGIN = f32(4.0)  # world px around a view's samples


def shade(c1, c2, ordinal):
    """shadeAreaBetweenCurves: two triangles per point pair, reordered by the sign of the cross product of two sides."""
    out = []
    for i in range(len(c1) - 1):
        v1, v2, v3, v4 = c1[i], c2[i], c1[i + 1], c2[i + 1]
        s1, s2 = v2 - v1, v3 - v1
        out.append((v1, v3, v2) if s1[0] * s2[1] - s1[1] * s2[0] >= f32(0) else (v1, v2, v3))
        s1, s2 = v3 - v2, v4 - v2
        out.append((v2, v4, v3) if s1[0] * s2[1] - s1[1] * s2[0] >= f32(0) else (v2, v3, v4))
    return [(np.array(t, dtype=np.float32), ordinal) for t in out]


def draw_list(track):
    """(xy [6P, 3, 2] float32, ordinal [6P] uint8) of the six draws of Visualizer::render with kContinuousLoop."""
    li, lo, ri, ro = (np.asarray(getattr(track, k), dtype=np.float32).reshape(-1, 2) for k in ("li", "lo", "ri", "ro"))
    ends = lambda c: np.stack([c[0], c[-1]])
    tris = (shade(ri, ro, 0) + shade(li, lo, 1) + shade(li, ri, 2) + shade(ends(ro), ends(lo), 3) +
            shade(ends(ri), ends(ro), 4) + shade(ends(li), ends(lo), 5))
    return np.stack([t for t, _ in tris]), np.array([o for _, o in tris], dtype=np.uint8)


class Scene:
    """The draw list of a track, its zero-area triangles dropped, with per-triangle bounding boxes."""

    def __init__(self, track):
        xy, ordinal = draw_list(track)
        a, b, c = xy[:, 0], xy[:, 1], xy[:, 2]
        area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
        keep = area != f32(0)
        self.xy, self.ordinal = xy[keep], ordinal[keep].astype(np.int32)
        self.lo, self.hi = self.xy.min(axis=1), self.xy.max(axis=1)


def band_of(scene, px, py, prefilter=True):
    """Largest ordinal of a triangle containing each sample (px, py float32 arrays), -1 for none."""
    sel = np.arange(len(scene.xy))
    if prefilter and px.size:
        fin = np.isfinite(px) & np.isfinite(py)
        if not fin.any():
            return np.full(px.shape, -1, dtype=np.int32)
        x0, x1 = px[fin].min() - PREFILTER_MARGIN, px[fin].max() + PREFILTER_MARGIN
        y0, y1 = py[fin].min() - PREFILTER_MARGIN, py[fin].max() + PREFILTER_MARGIN
        sel = np.nonzero((scene.hi[:, 0] >= x0) & (scene.lo[:, 0] <= x1) & (scene.hi[:, 1] >= y0) & (scene.lo[:, 1] <= y1))[0]
    band = np.full(px.shape, -1, dtype=np.int32)
    if sel.size == 0:
        return band
    t = scene.xy[sel]
    ax, ay, bx, by, cx, cy = (t[:, k // 2, k % 2][None, :] for k in range(6))
    ords = scene.ordinal[sel][None, :]
    flat_x, flat_y, flat_b = px.reshape(-1), py.reshape(-1), band.reshape(-1)
    chunk = max(1, (1 << 22) // sel.size)
    for s in range(0, flat_x.size, chunk):
        qx, qy = flat_x[s:s + chunk, None], flat_y[s:s + chunk, None]
        e0 = (bx - ax) * (qy - ay) - (by - ay) * (qx - ax)
        e1 = (cx - bx) * (qy - by) - (cy - by) * (qx - bx)
        e2 = (ax - cx) * (qy - cy) - (ay - cy) * (qx - cx)
        z = f32(0)
        inside = ((e0 >= z) & (e1 >= z) & (e2 >= z)) | ((e0 <= z) & (e1 <= z) & (e2 <= z))
        flat_b[s:s + chunk] = np.where(inside, ords, -1).max(axis=1)
    return band


def render_view(scene, pos_x, pos_y, rot_sc, crashed, width, height, samples=1, fmt="rgba", view=(FOLLOW_W, FOLLOW_H),
                heading_up=False, draw_agent=True, draw_heading=True, radius=9.0, agent_rgb=(80, 80, 80), prefilter=True):
    """One agent's view: [H, W, 4] (fmt "rgba") or [H, W] ("class") uint8.  rot_sc = (sin, cos) of OK_DEG2RAD * rot as the
    device's ok_sincosf gives them (okenv_debug_sincos)."""
    s = int(samples)
    vw, vh = f32(view[0]), f32(view[1])
    step_x, step_y = vw / f32(width * s), vh / f32(height * s)
    half_x, half_y = vw * f32(0.5), vh * f32(0.5)
    ox = (np.arange(width * s, dtype=np.float32) + f32(0.5)) * step_x - half_x
    oy = (np.arange(height * s, dtype=np.float32) + f32(0.5)) * step_y - half_y
    OX, OY = np.meshgrid(ox, oy)  # [H*s, W*s], row = sample row
    px, py = f32(pos_x), f32(pos_y)
    sn, cs = f32(rot_sc[0]), f32(rot_sc[1])
    if heading_up:
        wx = px + (OX * (-sn) - OY * cs)
        wy = py + (OX * cs - OY * sn)
    else:
        wx, wy = px + OX, py + OY
    band = band_of(scene, wx, wy, prefilter)
    dx, dy = wx - px, wy - py
    r = f32(radius)
    disc = (dx * dx + dy * dy <= r * r) if draw_agent else np.zeros(band.shape, dtype=bool)
    half = disc & (dx * cs + dy * sn >= f32(0)) if draw_heading else np.zeros(band.shape, dtype=bool)
    if fmt == "class":
        assert s == 1
        cls = np.vectorize(BAND_CLASS.get)(band).astype(np.uint8) if band.size else band.astype(np.uint8)
        cls[disc] = 6 if crashed else 4
        cls[half] = 5
        return cls
    rgb = np.zeros(band.shape + (3,), dtype=np.int64)
    for o, col in BAND_RGB.items():
        rgb[band == o] = col
    if crashed:
        under = rgb[disc]
        rgb[disc] = (np.array([253, 249, 0]) * 150 + under * 105 + 127) // 255
    else:
        rgb[disc] = agent_rgb
    rgb[half] = (255, 255, 255)
    n = s * s
    box = rgb.reshape(height, s, width, s, 3).sum(axis=(1, 3))
    out = np.full((height, width, 4), 255, dtype=np.uint8)
    out[..., :3] = (box + n // 2) // n
    return out
