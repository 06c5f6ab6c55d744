// ok_expert.h -- the reference's two expert drivers (FieldNavigators/PotentialFieldAgent.hpp, VFHAgent.hpp) for every agent of a
// handle: one action kernel beside the step.  The rule itself lives in include/okenv_math.h
// (ok_potfield_action, ok_vfh_action, ok_expert_goal_index) and is shared with okExpertActHost below, so the device and the host
// entry agree bit for bit.
//
// This is NOT a step kernel and adds no step-kernel launch site: it reads what the last step left (pos, rot, dist) and writes the
// action the next step consumes.
#ifndef OK_EXPERT_H
#define OK_EXPERT_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "okenv_kernels.h"

// What the kernel needs, by value.  cl_start / geom / P carry the names okNearestBucketed looks up.
struct OkExpertParams
{
    OkDeviceState       st;
    int                 N, R, P;
    const float        *cx, *cy;
    const uint16_t     *cl_start, *cl_idx; // centre line bucketed by the cells of `geom`; nullptr: scan the whole line
    OkGridGeom          geom;
    const double       *ray_cos, *ray_sin; // [R]: cos / sin (angle * M_PI / 180.f) in fp64, made on the host (PotField)
    float               first, last;       // sensor_ray_angles_.front() / .back() (VFH)
    okenv_expert_params ep;
    okenv_expert_record rec;
};

// Lanes per agent.  The nearest-index search looks at 3 x 3 grid cells (or, far from the track, at the whole centre line) and is
// shared by the group; the record slots are copied by the group, consecutive lanes writing consecutive addresses (a wave holds 8
// consecutive agents, whose rows are adjacent); the rule itself -- a few dozen operations -- runs on the group's first lane.
constexpr int kExpertLanes = 8;

// The centre line and its buckets are read through L2 (10 KB for a 1200-point track, shared by every workgroup of the launch): a
// workgroup of 32 agents touches a few hundred bytes of them, far less than staging the whole line in LDS would move.
__global__ __launch_bounds__(256) void okExpertKernel(const OkExpertParams p)
{
    const long t     = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int  lane  = static_cast<int>(threadIdx.x) & (kExpertLanes - 1);
    const long a_raw = t / kExpertLanes;
    const bool valid = a_raw < p.N;
    const long a     = valid ? a_raw : static_cast<long>(p.N) - 1; // (spare lanes of the last wave take part in the shuffles)
    const float px = p.st.pos_x[a], py = p.st.pos_y[a];
    const int nearest = okNearestBucketed(p, p.cx, p.cy, p.cl_start, p.cl_idx, px, py, lane, kExpertLanes);
    if (!valid)
        return;
    const float *dist = p.st.dist + a * p.R;
    // this step's record slots: the observation the action is computed from
    if (p.rec.dist != nullptr)
        for (int i = lane; i < p.R; i += kExpertLanes)
            p.rec.dist[a * p.R + i] = dist[i];
    if (p.rec.rel_xy != nullptr)
    {
        float2 *dst = reinterpret_cast<float2 *>(p.rec.rel_xy) + a * p.R;
        for (int i = lane; i < p.R; i += kExpertLanes)
            dst[i] = make_float2(p.st.rel_x[a * p.R + i], p.st.rel_y[a * p.R + i]);
    }
    if (lane != 0)
        return;
    const int   gi = ok_expert_goal_index(nearest, p.ep.lookahead, p.P, p.ep.goal_wrap);
    const float gx = p.cx[gi], gy = p.cy[gi], rot = p.st.rot[a];
    float       thr, steer;
    if (p.ep.kind == OKENV_EXPERT_POTFIELD)
        ok_potfield_action(px, py, rot, gx, gy, dist, p.ray_cos, p.ray_sin, p.R, p.ep.k_att, p.ep.k_rep, p.ep.effect_range, p.ep.clamp_deg, &thr,
                           &steer);
    else
        ok_vfh_action(px, py, rot, gx, gy, dist, p.R, p.first, p.last, p.ep.vfh_threshold, p.ep.vfh_throttle, &thr, &steer);
    p.st.thr[a]   = thr;
    p.st.steer[a] = steer;
    if (p.rec.action != nullptr)
        reinterpret_cast<float2 *>(p.rec.action)[a] = make_float2(thr, steer);
    if (p.rec.alive != nullptr)
        p.rec.alive[a] = p.st.crashed[a] ? 0 : 1;
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okExpertCheckParams(const okenv_expert_params *ep, const int R)
{
    if (ep == nullptr)
        return "params is NULL";
    if (ep->kind != OKENV_EXPERT_POTFIELD && ep->kind != OKENV_EXPERT_VFH)
        return "unknown kind (OKENV_EXPERT_POTFIELD / OKENV_EXPERT_VFH)";
    if (ep->lookahead < 0)
        return "lookahead < 0";
    if (ep->kind == OKENV_EXPERT_VFH && (R < 2 || R > OK_VFH_MAX_RAYS))
        return "a VFH fan needs 2 .. 64 rays";
    return nullptr;
}

// cos / sin (angle * M_PI / 180.f) as PotentialFieldAgent.hpp:69-70 evaluates them: float * double, / (double)180.f, libm's fp64
inline void okExpertRayTables(const float *ray_deg, const int R, std::vector<double> &c, std::vector<double> &s)
{
    c.resize(static_cast<size_t>(R));
    s.resize(static_cast<size_t>(R));
    for (int i = 0; i < R; ++i)
    {
        const double arg = ray_deg[i] * M_PI / 180.F;
        c[static_cast<size_t>(i)] = std::cos(arg);
        s[static_cast<size_t>(i)] = std::sin(arg);
    }
}

// RaceTrack::findNearestTrackIndexBruteForce (RaceTrack.cpp:16-31): first minimum, index 0 when nothing is closer than FLT_MAX
inline int okExpertNearestHost(const float *cx, const float *cy, const int P, const float px, const float py)
{
    float best = 3.402823466e+38F;
    int   bi   = 0;
    for (int i = 0; i < P; ++i)
    {
        const float dx = px - cx[i], dy = py - cy[i];
        const float d2 = dx * dx + dy * dy;
        if (d2 < best)
        {
            best = d2;
            bi   = i;
        }
    }
    return bi;
}

// updateAction for n agents on host arrays.  Goals come from the centre line, or, when goal_x / goal_y are given, from there.
inline void okExpertActHost(const okenv_expert_params &ep, const float *ray_deg, const int R, const float *cx, const float *cy, const int P, const int n,
                            const float *pos_x, const float *pos_y, const float *rot, const float *dist, const float *goal_x, const float *goal_y,
                            float *throttle, float *steer)
{
    std::vector<double> c, s;
    okExpertRayTables(ray_deg, R, c, s);
    for (int a = 0; a < n; ++a)
    {
        float gx, gy;
        if (goal_x != nullptr)
        {
            gx = goal_x[a];
            gy = goal_y[a];
        }
        else
        {
            const int gi = ok_expert_goal_index(okExpertNearestHost(cx, cy, P, pos_x[a], pos_y[a]), ep.lookahead, P, ep.goal_wrap);
            gx           = cx[gi];
            gy           = cy[gi];
        }
        const float *d = dist + static_cast<size_t>(a) * R;
        if (ep.kind == OKENV_EXPERT_POTFIELD)
            ok_potfield_action(pos_x[a], pos_y[a], rot[a], gx, gy, d, c.data(), s.data(), R, ep.k_att, ep.k_rep, ep.effect_range, ep.clamp_deg,
                               throttle + a, steer + a);
        else
            ok_vfh_action(pos_x[a], pos_y[a], rot[a], gx, gy, d, R, ray_deg[0], ray_deg[R - 1], ep.vfh_threshold, ep.vfh_throttle, throttle + a,
                          steer + a);
    }
}

#endif // OK_EXPERT_H
