// origin_clearance_check.cpp -- host-side driver of the square the origin test clears (openkitchen_amd/csrc/ok_raycast.h:
// okOriginClearScalar, okOriginMoved) and of the walk's start at the origin (ok_cast_poly_interval<.., .., true> with from_origin set)
// for tests/test_origin_clearance.py and tests/tools/cert_rerun_rate.py.  Built as a shared library; the brute-force side of every
// comparison is numpy's, in float64.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../openkitchen_amd/csrc/ok_grid.h"

namespace
{
struct Split
{
    OkGridHost        gh;
    OkFrontBack       fb;
    OkFrontBackImages imgs;
    OkPolyView        front{};
    bool              ok{false};
};

Split buildSplit(const OkSeg *segs, const int S, const float cell)
{
    Split       sp;
    bool        fits = false;
    OkPolyImage combined;
    sp.gh = okBuildGridAuto(segs, static_cast<size_t>(S), cell, 160U * 1024U, &fits, &combined);
    if (!fits)
        return sp;
    sp.fb   = okClassifyFrontBack(segs, static_cast<size_t>(S), sp.gh, combined.max_seg_len);
    sp.imgs = okBuildFrontBackImages(segs, static_cast<size_t>(S), sp.gh, sp.fb);
    if (!sp.imgs.ok)
        return sp;
    sp.front.g            = sp.gh.g;
    sp.front.slots        = reinterpret_cast<const OkPoint *>(sp.imgs.front.bytes.data());
    sp.front.hdr          = reinterpret_cast<const OkCellHdr *>(sp.imgs.front.bytes.data() + sp.imgs.front.off_hdr);
    sp.front.side_tol     = sp.imgs.front.side_tol;
    sp.front.e_s          = sp.fb.e_s;
    sp.front.e_t          = sp.fb.e_t;
    sp.front.e_s_over_e_t = sp.fb.e_s / sp.fb.e_t;
    sp.ok                 = true;
    return sp;
}

// The half-width in the arithmetic it had before the pieces became host-callable functions: the cell's border and the registered F
// segments' bounding boxes, written out in one place.
float halfWidthWrittenOut(const OkPolyView &front, const float ox, const float oy)
{
    const OkGridGeom &g  = front.g;
    int               ix = (int)__builtin_floorf((ox - g.x0) * g.inv_cell);
    int               iy = (int)__builtin_floorf((oy - g.y0) * g.inv_cell);
    ix                   = ix < 0 ? 0 : (ix >= g.nx ? g.nx - 1 : ix);
    iy                   = iy < 0 ? 0 : (iy >= g.ny ? g.ny - 1 : iy);
    const OkCellHdr hc   = front.hdr[iy * g.nx + ix];
    const uint32_t  k0   = hc.w0 & OKPOLY_IDX_MASK;
    const uint32_t  n8   = (((hc.w0 >> OKPOLY_IDX_BITS) & OKPOLY_N_MASK) + 7U) & ~7U;
    const uint32_t  nf   = hc.w0 >> OKFB_HDR_NF_SHIFT;
    const float     cx0 = g.x0 + static_cast<float>(ix) * g.cell, cy0 = g.y0 + static_cast<float>(iy) * g.cell;
    float           near = __builtin_fminf(__builtin_fminf(ox - cx0, (cx0 + g.cell) - ox), __builtin_fminf(oy - cy0, (cy0 + g.cell) - oy));
    for (uint32_t j = 0; j + 1U < nf; ++j)
    {
        if ((hc.brk >> (n8 - 2U - j)) & 1U)
            continue;
        const OkPoint pa = front.slots[k0 + j], pb = front.slots[k0 + j + 1U];
        const float   bx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(pa.x, pb.x) - ox, ox - __builtin_fmaxf(pa.x, pb.x)), 0.F);
        const float   by = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(pa.y, pb.y) - oy, oy - __builtin_fmaxf(pa.y, pb.y)), 0.F);
        near             = __builtin_fminf(near, __builtin_fmaxf(bx, by));
    }
    return 0.99F * near - 1.0e-3F;
}
} // namespace

extern "C"
{
    // geom: x0, y0, x1, y1, cell; dims: nx, ny; seg_is_f (one byte per segment): member of F, the segments chi flips across
    __attribute__((visibility("default"))) int clearcheck_split(const float *segs_xyxy, int S, float cell, float *geom, int32_t *dims, uint8_t *seg_is_f)
    {
        const Split sp = buildSplit(reinterpret_cast<const OkSeg *>(segs_xyxy), S, cell);
        if (!sp.ok)
            return 1;
        geom[0] = sp.gh.g.x0, geom[1] = sp.gh.g.y0, geom[2] = sp.gh.g.x1, geom[3] = sp.gh.g.y1, geom[4] = sp.gh.g.cell;
        dims[0] = sp.gh.g.nx, dims[1] = sp.gh.g.ny;
        std::memcpy(seg_is_f, sp.fb.chi_def.data(), static_cast<size_t>(S));
        return 0;
    }

    // Per origin: usable (inside the grid box, in a certifiable cell), the half-width of okOriginClearScalar, the same written out
    // (halfWidthWrittenOut, usable origins only), and okOriginChiScalar's answer.
    __attribute__((visibility("default"))) int clearcheck_radii(const float *segs_xyxy, int S, float cell, const float *ox, const float *oy, int n,
                                                                uint8_t *usable, float *half_width, float *written_out, uint8_t *cert)
    {
        const Split sp = buildSplit(reinterpret_cast<const OkSeg *>(segs_xyxy), S, cell);
        if (!sp.ok)
            return 1;
        for (int i = 0; i < n; ++i)
        {
            const OkOriginCell oc = okOriginCellOf(sp.front.g, ox[i], oy[i]);
            const uint32_t     fl = (sp.front.hdr[oc.cell].w0 >> OKFB_HDR_SHIFT_RC) & 15U;
            usable[i]             = (oc.inside && (fl & OKFB_RC_CERT)) ? 1 : 0;
            half_width[i]         = okOriginClearScalar(sp.front, ox[i], oy[i]);
            written_out[i]        = usable[i] ? halfWidthWrittenOut(sp.front, ox[i], oy[i]) : 0.F;
            cert[i]               = static_cast<uint8_t>(okOriginChiScalar(sp.front, ox[i], oy[i], sp.fb.t12, sp.fb.t34));
        }
        return 0;
    }

    // The step loop's rule over a trajectory: n agents, `steps` origins each (ox[s * n + a]); a NaN origin stands for "does not
    // cast this step".  Counts how often the origin test runs when the movement since the last test is measured by okOriginMoved
    // (reruns[0]) and by |dx| + |dy|, the diamond inside the square (reruns[1]); reruns[2]: origin-steps counted.
    __attribute__((visibility("default"))) int clearcheck_reruns(const float *segs_xyxy, int S, float cell, const float *ox, const float *oy, int n, int steps,
                                                                 int64_t *reruns)
    {
        const Split sp = buildSplit(reinterpret_cast<const OkSeg *>(segs_xyxy), S, cell);
        if (!sp.ok)
            return 1;
        reruns[0] = reruns[1] = reruns[2] = 0;
        for (int a = 0; a < n; ++a)
        {
            float fx[2] = {0.F, 0.F}, fy[2] = {0.F, 0.F}, clear[2] = {0.F, 0.F};
            for (int s = 0; s < steps; ++s)
            {
                const float x = ox[static_cast<size_t>(s) * n + a], y = oy[static_cast<size_t>(s) * n + a];
                if (x != x || y != y)
                    continue;
                ++reruns[2];
                const float moved[2] = {okOriginMoved(x, y, fx[0], fy[0]), __builtin_fabsf(x - fx[1]) + __builtin_fabsf(y - fy[1])};
                for (int k = 0; k < 2; ++k)
                    if (!(moved[k] < clear[k]))
                    {
                        clear[k] = okOriginClearScalar(sp.front, x, y);
                        fx[k] = x, fy[k] = y;
                        ++reruns[k];
                    }
            }
        }
        return 0;
    }

    // The walk from the origin, generic set-up against the start in the origin's cell, over the front image with the ambiguity
    // report on (the kernel's phase 1).  Outputs hold the generic walk's result at [i] and the other at [n + i].  Returns 2 if an
    // origin lies outside the grid box (the start at the origin is not defined there).
    __attribute__((visibility("default"))) int clearcheck_walk(const float *segs_xyxy, int S, float cell, const float *ox, const float *oy, const float *dx,
                                                               const float *dy, int n, float t_b, float *min_t, float *t_reached, uint8_t *conclusive,
                                                               uint8_t *amb)
    {
        const Split sp = buildSplit(reinterpret_cast<const OkSeg *>(segs_xyxy), S, cell);
        if (!sp.ok)
            return 1;
        for (int i = 0; i < n; ++i)
        {
            const OkOriginCell oc = okOriginCellOf(sp.front.g, ox[i], oy[i]);
            if (!oc.inside)
                return 2;
            const OkIntervalResult a  = ok_cast_poly_interval<false, true>(sp.front, ox[i], oy[i], dx[i], dy[i], 0.F, t_b, nullptr, nullptr, nullptr);
            const OkIntervalResult b  = ok_cast_poly_interval<false, true, true>(sp.front, ox[i], oy[i], dx[i], dy[i], 0.F, t_b, nullptr, nullptr, nullptr, nullptr,
                                                                                 false, OK_SENSOR_RANGE, true);
            min_t[i] = a.min_t, t_reached[i] = a.t_reached, conclusive[i] = a.conclusive, amb[i] = a.amb;
            min_t[n + i] = b.min_t, t_reached[n + i] = b.t_reached, conclusive[n + i] = b.conclusive, amb[n + i] = b.amb;
        }
        return 0;
    }
}
