// wave_model_vote.cpp -- development aid: the lock-step model of wave_model.cpp with the wave's vote that ends phase 1
// (ok_raycast.h, kVote) and with several agents per wave (fans of 32 and 16 rays: two and four agents share a wave's 64 lanes).
//
// After the lanes' phase-1 traces are known, for cell iteration i = 1, 2, ...: A = lanes whose walk has more than i cells, P = lanes
// that ended by then without a conclusive result; at the first i with A > 0 and A + P <= threshold every lane still walking is cut
// after i cells (t_reached = that cell's exit).  Phase 2 is modelled as shipped: the wave's pending rays, m = min(split, 64 / n)
// equal parameter intervals each with the start-cell ownership rule.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I include -I openkitchen_amd/csrc -o tools/_build/libwavemodel_vote.so tests/tools/wave_model_vote.cpp
#include "wave_model.cpp"

// out: [0..2] phase 1 cell iterations / 8-slot point rounds / exact passes per wave-step, [3..5] the same of phase 2, [6] pending
// rays per wave-step, [7] share of wave-steps whose phase 1 the vote ended, [8] waves
extern "C" __attribute__((visibility("default"))) int wavemodel_vote(const float *segs_xyxy, int S, float cell, const float *pos_x, const float *pos_y,
                                                                      const float *rot_deg, int n_agents, const float *ray_deg, int R, float phase1_range,
                                                                      int max_split, int threshold, double *out)
{
    const OkSeg *segs = reinterpret_cast<const OkSeg *>(segs_xyxy);
    OkGridHost   gh   = okBuildGrid(segs, static_cast<size_t>(S), cell);
    OkPolyImage  img  = okBuildPolyImage(segs, static_cast<size_t>(S), gh);
    if (!img.ok)
        return -1;
    OkFrontBack             fbc = okClassifyFrontBack(segs, static_cast<size_t>(S), gh, img.max_seg_len);
    const OkFrontBackImages fbi = okBuildFrontBackImages(segs, static_cast<size_t>(S), gh, fbc);
    if (!fbi.ok)
        return -2;
    OkPolyView pv{};
    pv.g        = fbi.grid_front.g;
    pv.slots    = reinterpret_cast<const OkPoint *>(fbi.front.bytes.data());
    pv.hdr      = reinterpret_cast<const OkCellHdr *>(fbi.front.bytes.data() + fbi.front.off_hdr);
    pv.side_tol = fbi.front.side_tol;
    int G = 1;
    while (G < R)
        G <<= 1;
    if (G > 64)
        return -3;
    const int per_wave = 64 / G;
    WaveCount p1, p2;
    double    n_pending = 0, voted = 0, waves = 0;
    for (int a0 = 0; a0 + per_wave <= n_agents; a0 += per_wave)
    {
        waves += 1;
        std::vector<LaneTrace> l1;
        std::vector<float>     lox, loy, ldx, ldy;
        for (int a = a0; a < a0 + per_wave; ++a)
            for (int r = 0; r < R; ++r)
            {
                float dx, dy;
                ok_sincosf(OK_DEG2RAD * (rot_deg[a] + ray_deg[r]), &dy, &dx);
                lox.push_back(pos_x[a]), loy.push_back(pos_y[a]), ldx.push_back(dx), ldy.push_back(dy);
                l1.push_back(traceInterval(pv, pos_x[a], pos_y[a], dx, dy, 0.F, phase1_range, 1));
            }
        if (threshold > 0)
        {
            size_t longest = 0;
            for (auto &l : l1)
                longest = std::max(longest, l.cells.size());
            for (size_t i = 1; i < longest; ++i)
            {
                int A = 0, P = 0;
                for (auto &l : l1)
                {
                    A += l.cells.size() > i ? 1 : 0;
                    P += (l.cells.size() <= i && !l.cells.empty() && !l.conclusive) ? 1 : 0;
                }
                if (A > 0 && A + P <= threshold)
                {
                    for (size_t k = 0; k < l1.size(); ++k)
                        if (l1[k].cells.size() > i)
                            l1[k] = traceInterval(pv, lox[k], loy[k], ldx[k], ldy[k], 0.F, phase1_range, 1, 0, static_cast<int>(i));
                    voted += 1;
                    break;
                }
            }
        }
        p1.add(l1);
        std::vector<size_t> pend;
        for (size_t k = 0; k < l1.size(); ++k)
            if (!l1[k].conclusive)
                pend.push_back(k);
        if (pend.empty())
            continue;
        n_pending += static_cast<double>(pend.size());
        const int n = static_cast<int>(pend.size());
        int       m = 64 / n;
        m           = m > max_split ? max_split : m;
        std::vector<LaneTrace> l2;
        for (int lane = 0; lane < 64; ++lane)
        {
            const int q = lane / m, j = lane - q * m;
            if (q >= n)
                continue;
            const size_t k  = pend[q];
            const float  t0 = l1[k].t_reached;
            const float  dt = (OK_SENSOR_RANGE - t0) / static_cast<float>(m);
            const float  ta = t0 + static_cast<float>(j) * dt;
            const float  tb = (j + 1 == m) ? OKRC_INF : t0 + static_cast<float>(j + 1) * dt;
            l2.push_back(traceInterval(pv, lox[k], loy[k], ldx[k], ldy[k], ta, tb, 1, 0, 1 << 30, true));
        }
        p2.add(l2);
    }
    const double W = waves > 0 ? waves : 1;
    out[0] = p1.cell_it / W, out[1] = p1.pair_it / W, out[2] = p1.exact_it / W;
    out[3] = p2.cell_it / W, out[4] = p2.pair_it / W, out[5] = p2.exact_it / W;
    out[6] = n_pending / W, out[7] = voted / W, out[8] = waves;
    return 0;
}
