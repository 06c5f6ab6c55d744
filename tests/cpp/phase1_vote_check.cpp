// phase1_vote_check.cpp -- host-side driver of the wave's vote in the walk that starts a ray (openkitchen_amd/csrc/ok_raycast.h:
// ok_cast_poly_interval<.., .., .., kVote>) for tests/test_phase1_vote.py.  On the host the wave's count is the caller's
// (vote_host_cells), so the starting walk of every ray is cut after k = 1, 2, ... cells, every k up to the walk's own length, and
// continued from its t_reached the way okStepCoopKernel's coop_pass continues it: m equal parameter intervals of [t_reached, range],
// the last one open-ended, skip_unowned_start set for every interval but a first one that starts at 0.  Built as a shared library.
#include <cstdint>
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

constexpr int kVoteOn = 12; // (any threshold > 0: on the host the caller's count decides, not the threshold)

template <bool kOnly>
int runCuts(const float *segs_xyxy, int S, float cell, const float *ox, const float *oy, const float *dx, const float *dy, int n, float t_b, const int32_t *splits,
            int n_splits, int64_t *counts, int32_t *first_bad)
{
    const Split sp = buildSplit(reinterpret_cast<const OkSeg *>(segs_xyxy), S, cell);
    if (!sp.ok)
        return 1;
    const OkPolyView &v = sp.front;
    for (int c = 0; c < 12; ++c)
        counts[c] = 0;
    *first_bad = -1;
    auto bad   = [&](const int i) {
        if (*first_bad < 0)
            *first_bad = i;
    };
    for (int i = 0; i < n; ++i)
    {
        if (!okOriginCellOf(v.g, ox[i], oy[i]).inside)
            return 2;
        ++counts[0];
        const float            whole   = ok_cast_ray_poly<false>(v, ox[i], oy[i], dx[i], dy[i], nullptr, nullptr, nullptr);
        const OkIntervalResult whole_a = ok_cast_poly_interval<false, true>(v, ox[i], oy[i], dx[i], dy[i], 0.F, OKRC_INF, nullptr, nullptr, nullptr);
        if (okBits(whole_a.min_t) != okBits(whole))
            return 3;
        const bool from_origin = (i & 1) != 0; // (both set-ups: the kernel picks by a ballot of the wave's origins)
        uint32_t   tests = 0, len = 0, points = 0;
        (void)ok_cast_poly_interval<true, true, true, kVoteOn, kOnly>(v, ox[i], oy[i], dx[i], dy[i], 0.F, t_b, &tests, &len, &points, nullptr, false, OK_SENSOR_RANGE,
                                                               from_origin, 0);
        counts[11] = static_cast<int64_t>(len) > counts[11] ? len : counts[11];
        for (uint32_t k = 1; k <= len; ++k)
        {
            uint32_t               cells = 0;
            const OkIntervalResult r1    = ok_cast_poly_interval<true, true, true, kVoteOn, kOnly>(v, ox[i], oy[i], dx[i], dy[i], 0.F, t_b, &tests, &cells, &points, nullptr,
                                                                                         false, OK_SENSOR_RANGE, from_origin, static_cast<int>(k));
            ++counts[2];
            if (cells != k)
            {
                ++counts[7];
                bad(i);
            }
            if (k < len)
                ++counts[3];
            if (r1.conclusive)
            { // a hit inside the covered part, the range, the grid's end: final as it stands
                if (okBits(r1.min_t) != okBits(whole))
                {
                    ++counts[10];
                    bad(i);
                }
                continue;
            }
            const float t0 = r1.t_reached;
            counts[8] += (t0 > 0.F && t0 < 0.5F) ? 1 : 0;
            counts[9] += (t0 == 0.F) ? 1 : 0;
            for (int s = 0; s < n_splits; ++s)
            {
                const int   m     = splits[s];
                const float tl    = OK_SENSOR_RANGE;
                const float inv_m = okRcpApprox(static_cast<float>(m));
                const float dt    = (tl - t0) * inv_m;
                float       best  = r1.min_t;
                bool        amb   = r1.amb;
                for (int j = 0; j < m; ++j)
                {
                    const float            ta = t0 + static_cast<float>(j) * dt;
                    const float            tb = (j + 1 == m) ? OKRC_INF : t0 + static_cast<float>(j + 1) * dt;
                    const OkIntervalResult r2 =
                        ok_cast_poly_interval<false, true>(v, ox[i], oy[i], dx[i], dy[i], ta, tb, nullptr, nullptr, nullptr, nullptr, j > 0 || t0 > 0.F, tl);
                    best = r2.min_t < best ? r2.min_t : best;
                    amb  = amb || r2.amb;
                }
                ++counts[4];
                if (okBits(best) != okBits(whole))
                {
                    ++counts[5];
                    bad(i);
                }
                if (whole_a.amb && !amb)
                {
                    ++counts[6];
                    bad(i);
                }
            }
        }
    }
    return 0;
}
} // namespace

extern "C"
{
    // geom: x0, y0, x1, y1, cell of the grid built for this cell edge
    __attribute__((visibility("default"))) int votecheck_geom(const float *segs_xyxy, int S, float cell, float *geom)
    {
        const Split sp = buildSplit(reinterpret_cast<const OkSeg *>(segs_xyxy), S, cell);
        if (!sp.ok)
            return 1;
        geom[0] = sp.gh.g.x0, geom[1] = sp.gh.g.y0, geom[2] = sp.gh.g.x1, geom[3] = sp.gh.g.y1, geom[4] = sp.gh.g.cell;
        return 0;
    }

    // Every ray, every cut k = 1 .. (cells of its uncut starting walk over [0, t_b]), every m in `splits`.
    // counts: [0] rays walked, [1] rays skipped (always 0: nothing is), [2] starting walks run, [3] of them ended by the vote (not by
    // their own exit), [4] continuations run (a cut that is not conclusive, times the splits), [5] continuations whose minimum
    // differs from the whole walk's in some bit, [6] whole walk ambiguous but no piece is, [7] cut walks whose cell count is not k,
    // [8] cuts with 0 < t_reached < 0.5 px, [9] cuts with t_reached == 0, [10] a conclusive cut whose minimum differs,
    // [11] longest starting walk [cells].  first_bad: index of the first ray with a difference, or -1.
    // Returns 2 if an origin lies outside the grid box (from_origin is not defined there).  vote_only: the walk's kVoteOnly form, which
    // does not look at t_b (the kernels pass +inf).
    __attribute__((visibility("default"))) int votecheck_run(const float *segs_xyxy, int S, float cell, const float *ox, const float *oy, const float *dx,
                                                             const float *dy, int n, float t_b, const int32_t *splits, int n_splits, int64_t *counts,
                                                             int32_t *first_bad, int vote_only)
    {
        return vote_only ? runCuts<true>(segs_xyxy, S, cell, ox, oy, dx, dy, n, t_b, splits, n_splits, counts, first_bad)
                         : runCuts<false>(segs_xyxy, S, cell, ox, oy, dx, dy, n, t_b, splits, n_splits, counts, first_bad);
    }
}
