// ok_render.h -- bird's-eye camera views of every agent (okenv_render_create / okenv_render_views, include/okenv.h).
//
// Host side: the reference's draw list of track bands (Visualizer::render -> shadeAreaBetweenCurves, six draws, 6P triangles
// in DrawTriangle's vertex order) and a uniform grid over it in CSR form, each cell holding copies of the triangles whose
// bounding box (plus kRenderMargin) touches it, sorted by draw ordinal from the last draw to the first.  Device side:
// okRenderViewsKernel, one lane per 4 RGBA pixels or 16 class pixels of one view, 16-byte stores.
//
// Exactness: a sample's band is the largest ordinal among the triangles whose fp32 edge test contains it.
// The kernel tests exactly the triangles of the sample's cell, in descending ordinal, and stops at the first hit -- which is
// that maximum as long as the cell lists every triangle that can contain the sample; it does, because a triangle is registered
// in every cell its bounding box grown by kRenderMargin (1 px, thousands of times the fp32 rounding of the edge functions at
// coordinates <= 2048) touches.  Samples outside the grid's box are background for the same reason.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_math.h"

struct OkRenderTri
{
    float   ax, ay, bx, by; // vertices in DrawTriangle's order: edges (a, b), (b, c), (c, a)
    float   cx, cy;
    int32_t ord;            // draw ordinal 0..5 (later draws paint over earlier ones)
    int32_t pad;
};

constexpr float kRenderMargin = 1.0F;   // px added around every triangle's bounding box when it is registered
constexpr float kRenderCell   = 3.0F;   // default cell edge [px] (OKENV_RENDER_CELL overrides it; 2-8 px measured in docs/HISTORY.md)
constexpr int   kRenderMaxCells = 4096; // per axis; the cell grows for larger boxes

// The six calls of Visualizer::render (reference Environment/Visualizer.cpp:176-194, kContinuousLoop) through
// shadeAreaBetweenCurves (:99-138): per consecutive point pair two triangles, each reordered by the sign of the cross product
// of its first two sides exactly as the reference does before DrawTriangle.  xy pairs, P points each; appends 6P triangles.
inline void okRenderShade(const float *c1, const float *c2, const int n, const int ord, std::vector<OkRenderTri> &out)
{
    auto tri = [&](const float *a, const float *b, const float *c) {
        out.push_back({a[0], a[1], b[0], b[1], c[0], c[1], ord, 0});
    };
    for (int i = 0; i + 1 < n; ++i)
    {
        const float *v1 = c1 + 2 * i, *v2 = c2 + 2 * i, *v3 = c1 + 2 * (i + 1), *v4 = c2 + 2 * (i + 1);
        float        s1x = v2[0] - v1[0], s1y = v2[1] - v1[1], s2x = v3[0] - v1[0], s2y = v3[1] - v1[1];
        float        cross = s1x * s2y - s1y * s2x;
        if (cross >= 0.F)
            tri(v1, v3, v2);
        else
            tri(v1, v2, v3);
        s1x = v3[0] - v2[0], s1y = v3[1] - v2[1], s2x = v4[0] - v2[0], s2y = v4[1] - v2[1];
        cross = s1x * s2y - s1y * s2x;
        if (cross >= 0.F)
            tri(v2, v4, v3);
        else
            tri(v2, v3, v4);
    }
}

// The whole draw list: ordinals 0 right shoulder, 1 left shoulder, 2 driving surface, 3 the lap seam's surface quad
// (start_line_ / finish_line_, RaceTrack.cpp:12-13), 4 / 5 the seam's right / left shoulder quads.
inline std::vector<OkRenderTri> okRenderDrawList(const float *li, const float *lo, const float *ri, const float *ro, const int P)
{
    std::vector<OkRenderTri> t;
    t.reserve(6U * static_cast<size_t>(P));
    okRenderShade(ri, ro, P, 0, t);
    okRenderShade(li, lo, P, 1, t);
    okRenderShade(li, ri, P, 2, t);
    const size_t last = 2U * static_cast<size_t>(P - 1);
    auto ends = [&](const float *c, float *out4) {
        out4[0] = c[0];
        out4[1] = c[1];
        out4[2] = c[last];
        out4[3] = c[last + 1];
    };
    float a[4], b[4];
    ends(ro, a), ends(lo, b), okRenderShade(a, b, 2, 3, t);
    ends(ri, a), ends(ro, b), okRenderShade(a, b, 2, 4, t);
    ends(li, a), ends(lo, b), okRenderShade(a, b, 2, 5, t);
    return t;
}

struct OkRenderGeom
{
    std::vector<OkRenderTri> cell_tris;  // CSR payload: copies of the triangles, per cell by descending ordinal
    std::vector<uint32_t>    cell_start; // nx * ny + 1
    float                    x0{0.F}, y0{0.F}, cell{kRenderCell}, inv_cell{1.F / kRenderCell};
    int                      nx{1}, ny{1};
    int                      triangles{0}; // of the draw list, zero-area ones left out
};

// Grid over the draw list.  Triangles whose area (the edge function of c against (a, b)) is exactly 0 cover nothing and are
// dropped.  Returns false for a draw list with a non-finite coordinate.
inline bool okRenderBuildGrid(const std::vector<OkRenderTri> &list, float cell, OkRenderGeom &g)
{
    std::vector<OkRenderTri> tris;
    float                    lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    for (const OkRenderTri &t : list)
    {
        for (const float v : {t.ax, t.ay, t.bx, t.by, t.cx, t.cy})
            if (!std::isfinite(v))
                return false;
        const float area = (t.bx - t.ax) * (t.cy - t.ay) - (t.by - t.ay) * (t.cx - t.ax);
        if (area == 0.F)
            continue;
        tris.push_back(t);
        lo_x = std::min({lo_x, t.ax, t.bx, t.cx}), hi_x = std::max({hi_x, t.ax, t.bx, t.cx});
        lo_y = std::min({lo_y, t.ay, t.by, t.cy}), hi_y = std::max({hi_y, t.ay, t.by, t.cy});
    }
    g = OkRenderGeom{};
    g.triangles = static_cast<int>(tris.size());
    if (tris.empty())
    {
        g.cell_start.assign(2, 0U);
        return true;
    }
    const float pad = 2.F * kRenderMargin;
    g.x0            = lo_x - pad;
    g.y0            = lo_y - pad;
    const float w = hi_x + pad - g.x0, h = hi_y + pad - g.y0;
    cell          = std::max({cell > 0.F ? cell : kRenderCell, w / kRenderMaxCells, h / kRenderMaxCells});
    g.cell        = cell;
    g.inv_cell    = 1.F / cell;
    g.nx          = std::max(1, static_cast<int>(std::ceil(w * g.inv_cell)));
    g.ny          = std::max(1, static_cast<int>(std::ceil(h * g.inv_cell)));
    g.nx          = std::min(g.nx, kRenderMaxCells + 1);
    g.ny          = std::min(g.ny, kRenderMaxCells + 1);
    // later draws first inside a cell (stable: by draw-list position otherwise)
    std::stable_sort(tris.begin(), tris.end(), [](const OkRenderTri &a, const OkRenderTri &b) { return a.ord > b.ord; });
    const size_t          cells = static_cast<size_t>(g.nx) * g.ny;
    std::vector<uint32_t> count(cells, 0U);
    auto                  range = [&](const OkRenderTri &t, int &i0, int &i1, int &j0, int &j1) {
        const float mnx = std::min({t.ax, t.bx, t.cx}) - kRenderMargin, mxx = std::max({t.ax, t.bx, t.cx}) + kRenderMargin;
        const float mny = std::min({t.ay, t.by, t.cy}) - kRenderMargin, mxy = std::max({t.ay, t.by, t.cy}) + kRenderMargin;
        i0 = std::clamp(static_cast<int>(std::floor((mnx - g.x0) * g.inv_cell)), 0, g.nx - 1);
        i1 = std::clamp(static_cast<int>(std::floor((mxx - g.x0) * g.inv_cell)), 0, g.nx - 1);
        j0 = std::clamp(static_cast<int>(std::floor((mny - g.y0) * g.inv_cell)), 0, g.ny - 1);
        j1 = std::clamp(static_cast<int>(std::floor((mxy - g.y0) * g.inv_cell)), 0, g.ny - 1);
    };
    for (const OkRenderTri &t : tris)
    {
        int i0, i1, j0, j1;
        range(t, i0, i1, j0, j1);
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i)
                ++count[static_cast<size_t>(j) * g.nx + i];
    }
    g.cell_start.assign(cells + 1U, 0U);
    for (size_t c = 0; c < cells; ++c)
        g.cell_start[c + 1] = g.cell_start[c] + count[c];
    g.cell_tris.resize(g.cell_start[cells]);
    std::vector<uint32_t> fill(g.cell_start.begin(), g.cell_start.end() - 1);
    for (const OkRenderTri &t : tris)
    {
        int i0, i1, j0, j1;
        range(t, i0, i1, j0, j1);
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i)
                g.cell_tris[fill[static_cast<size_t>(j) * g.nx + i]++] = t;
    }
    return true;
}

// ---- device ------------------------------------------------------------------------------------------------------------

enum OkRenderFormat : int
{
    kRenderRgba  = 0, // OKENV_VIEW_RGBA8
    kRenderClass = 1, // OKENV_VIEW_CLASS8
};

struct OkRenderParams
{
    const float       *pos_x, *pos_y, *rot;
    const uint8_t     *crashed;
    const OkRenderTri *tris;
    const uint32_t    *cell_start;
    uint8_t           *dst;
    float              x0, y0, inv_cell, fnx, fny;
    int                nx;
    uint32_t           W, hw; // width, width * height
    uint32_t           chunks; // workgroups per view
    float              step_x, step_y, half_x, half_y;
    float              r2;     // radius * radius
    uint32_t           flags;  // OKENV_VIEW_DRAW_AGENT / _DRAW_HEADING
    uint32_t           agent_rgb; // r | g << 8 | b << 16
};

constexpr int kRenderThreads = 256;

// Largest draw ordinal whose triangle contains (px, py), -1 for none: the first hit of the cell's descending list.
__device__ inline int okRenderBand(const OkRenderParams &p, const float px, const float py)
{
    const float fx = (px - p.x0) * p.inv_cell, fy = (py - p.y0) * p.inv_cell;
    if (!(fx >= 0.F && fx < p.fnx && fy >= 0.F && fy < p.fny))
        return -1; // outside the grid's box (NaN included): no triangle is near
    const uint32_t c = static_cast<uint32_t>(fy) * static_cast<uint32_t>(p.nx) + static_cast<uint32_t>(fx);
    const uint32_t e = p.cell_start[c + 1];
    for (uint32_t k = p.cell_start[c]; k < e; ++k)
    {
        const float4 v0 = *reinterpret_cast<const float4 *>(&p.tris[k].ax);
        const float4 v1 = *reinterpret_cast<const float4 *>(&p.tris[k].cx);
        const float  ax = v0.x, ay = v0.y, bx = v0.z, by = v0.w, cx = v1.x, cy = v1.y;
        const float  e0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
        const float  e1 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
        const float  e2 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);
        if ((e0 >= 0.F && e1 >= 0.F && e2 >= 0.F) || (e0 <= 0.F && e1 <= 0.F && e2 <= 0.F))
            return __float_as_int(v1.z);
    }
    return -1;
}

__device__ inline uint32_t okRenderBandRgb(const int band)
{
    // 0 / 4 blue, 1 / 5 red, 2 / 3 green, none black
    return band < 0 ? 0U : ((band == 0 || band == 4) ? 0xFF0000U : ((band == 1 || band == 5) ? 0x0000FFU : 0x00FF00U));
}

__device__ inline uint32_t okRenderBandClass(const int band)
{
    return band < 0 ? 0U : ((band == 0 || band == 4) ? 1U : ((band == 1 || band == 5) ? 2U : 3U));
}

// One view per okenv handle agent; the view's pixels are dealt to lanes kPix at a time (kPix * C = 16 bytes).
template <int kFormat, int kS, bool kHeadingUp>
__global__ void __launch_bounds__(kRenderThreads) okRenderViewsKernel(OkRenderParams p)
{
    constexpr int      kPix = kFormat == kRenderRgba ? 4 : 16;
    const uint32_t     view = blockIdx.x / p.chunks, chunk = blockIdx.x - view * p.chunks;
    const uint32_t     pix0 = (chunk * kRenderThreads + threadIdx.x) * kPix;
    if (pix0 >= p.hw)
        return;
    const float px = p.pos_x[view], py = p.pos_y[view];
    float       sn, cs;
    ok_sincosf(OK_DEG2RAD * p.rot[view], &sn, &cs);
    const bool     crashed = p.crashed[view] != 0;
    const bool     agent   = (p.flags & OKENV_VIEW_DRAW_AGENT) != 0U;
    const bool     heading = agent && (p.flags & OKENV_VIEW_DRAW_HEADING) != 0U;
    uint32_t       row = pix0 / p.W, col = pix0 - row * p.W;
    uint32_t       out[4] = {0U, 0U, 0U, 0U};
    const uint32_t n      = min(static_cast<uint32_t>(kPix), p.hw - pix0);
    for (uint32_t q = 0; q < n; ++q)
    {
        uint32_t acc_r = 0U, acc_g = 0U, acc_b = 0U, cls = 0U;
#pragma unroll
        for (int i = 0; i < kS; ++i)
        {
            const float oy = (static_cast<float>(row * kS + i) + 0.5F) * p.step_y - p.half_y;
#pragma unroll
            for (int j = 0; j < kS; ++j)
            {
                const float ox = (static_cast<float>(col * kS + j) + 0.5F) * p.step_x - p.half_x;
                float       wx, wy;
                if (kHeadingUp)
                {
                    wx = px + (ox * (-sn) - oy * cs);
                    wy = py + (ox * cs - oy * sn);
                }
                else
                {
                    wx = px + ox;
                    wy = py + oy;
                }
                const int   band = okRenderBand(p, wx, wy);
                const float dx = wx - px, dy = wy - py;
                const bool  disc = agent && dx * dx + dy * dy <= p.r2;
                const bool  half = disc && heading && dx * cs + dy * sn >= 0.F;
                if (kFormat == kRenderClass)
                    cls = half ? 5U : (disc ? (crashed ? 6U : 4U) : okRenderBandClass(band));
                else
                {
                    uint32_t rgb = okRenderBandRgb(band);
                    if (half)
                        rgb = 0xFFFFFFU;
                    else if (disc && !crashed)
                        rgb = p.agent_rgb;
                    else if (disc)
                    { // (253, 249, 0) at alpha 150 over the band
                        const uint32_t r = (253U * 150U + (rgb & 0xFFU) * 105U + 127U) / 255U;
                        const uint32_t g = (249U * 150U + ((rgb >> 8) & 0xFFU) * 105U + 127U) / 255U;
                        const uint32_t b = (0U * 150U + ((rgb >> 16) & 0xFFU) * 105U + 127U) / 255U;
                        rgb              = r | g << 8 | b << 16;
                    }
                    acc_r += rgb & 0xFFU;
                    acc_g += (rgb >> 8) & 0xFFU;
                    acc_b += rgb >> 16;
                }
            }
        }
        if (kFormat == kRenderClass)
            out[q >> 2] |= cls << (8U * (q & 3U));
        else
        {
            constexpr uint32_t kN = kS * kS, kHalf = kN / 2;
            out[q] = (acc_r + kHalf) / kN | ((acc_g + kHalf) / kN) << 8 | ((acc_b + kHalf) / kN) << 16 | 0xFF000000U;
        }
        if (++col == p.W)
            col = 0, ++row;
    }
    constexpr uint32_t kC   = kFormat == kRenderRgba ? 4U : 1U;
    uint8_t           *dst  = p.dst + (static_cast<size_t>(view) * p.hw + pix0) * kC;
    if (n == static_cast<uint32_t>(kPix) && (reinterpret_cast<uintptr_t>(dst) & 15U) == 0U)
        *reinterpret_cast<uint4 *>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
    else
        for (uint32_t b = 0; b < n * kC; ++b)
            dst[b] = static_cast<uint8_t>(out[b >> 2] >> (8U * (b & 3U)));
}
