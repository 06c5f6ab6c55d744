// ok_actor.h -- the reference's shared-network agents (RLRacers/PPO/PPOAgent.hpp, Reinforce/Policy.hpp, Deep_Q_Learning/DQAgent.hpp):
// updateAction for every agent of a handle as one action kernel beside the step.  The rule itself lives in
// include/okenv_math.h (ok_actor_partial, ok_actor_join, ok_expf, ok_actor_pick, ok_actor_eps_greedy) and is shared with
// okActorActHost below, so the device and the host entry agree bit for bit.
//
// This is NOT a step kernel and adds no step-kernel launch site: it reads what the last step left (dist, crashed) and writes the
// action the next step consumes, plus the learner's record of the step.
#ifndef OK_ACTOR_H
#define OK_ACTOR_H

#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_reinforce.h"
#include "okenv_kernels.h"

// What the act kernels share (okActorKernel here, okDdpgActKernel, okGaussActKernel, okGclActKernel), in two pieces, so that every kernel's
// parameter struct keeps the place its widths and vectors had between them (the kernel-argument layout decides how the loads group,
// docs/HISTORY.md section 29): the step's state with the population, and the words of the draw index
struct OkActFrame
{
    OkDeviceState st;
    int           N, R;
};

struct OkActDrawWords
{
    const uint32_t *step_word;   // the handle's device-side step count (auto-reset on), or nullptr: host_steps
    uint32_t        host_steps;
    const uint32_t *draw_offset; // okenv_actor_ / okenv_ddpg_ / okenv_gauss_set_draw_offset, or nullptr
};

// What the kernel needs, by value
struct OkActorParams
{
    OkActFrame         f;
    const float       *policy, *value; // parameter vectors on the device, each padded to a multiple of four floats
    OkActDrawWords     draw;
    okenv_actor_params ap;
    okenv_actor_record rec;
    ok_reinforce_mask  drop; // okenv_actor_set_dropout: p, its scale and the seed (agent and draw are the kernel's to fill in)
};

// Lanes per agent = the rule's interleave (OK_ACTOR_LANES): lane l of a group owns the hidden units l, l + 8, ... of both networks
// and carries one partial sum per output, so no hidden value ever leaves its lane; the partial sums meet in a butterfly of three
// shuffles per output.  A wave holds 8 consecutive agents, a workgroup 32.
constexpr int kActorLanes   = OK_ACTOR_LANES;
constexpr int kActorThreads = 256;
constexpr int kActorAgents  = kActorThreads / kActorLanes;

// Row stride of the first layer's weights in LDS: odd, so that the 8 lanes of a group, which read 8 consecutive rows at the same
// column, hit 8 different banks for every fan (the 4 groups of a 32-lane half read the same addresses: a broadcast).
__host__ __device__ inline int okActorRowStride(const int R)
{
    return R | 1;
}

// LDS floats of one network's copy / of the whole launch
__host__ __device__ inline int okActorNetFloats(const int R, const int hidden, const int out)
{
    return hidden > 0 ? hidden * okActorRowStride(R) + hidden + out * hidden + out : 0;
}

inline size_t okActorLdsBytes(const int R, const okenv_actor_params &ap)
{
    return sizeof(float) * static_cast<size_t>(okActorNetFloats(R, ap.hidden, ap.num_actions) + okActorNetFloats(R, ap.value_hidden, 1) + kActorAgents * okActorRowStride(R));
}

__device__ __forceinline__ int okActorLdsIndex(const int i, const int R, const int rp, const int n1, const int shift)
{
    return i < n1 ? (i / R) * rp + i % R : i + shift;
}

// One network from global memory into LDS: 16-byte loads (the vector is padded to a multiple of four floats), the first layer's
// rows spread to the odd stride, the rest moved up behind them.
__device__ __forceinline__ void okActorStage(float *dst, const float *src, const int R, const int hidden, const int n_params)
{
    const int rp = okActorRowStride(R), n1 = hidden * R, shift = hidden * (rp - R);
    const float4 *src4 = reinterpret_cast<const float4 *>(src);
    for (int c = static_cast<int>(threadIdx.x); 4 * c < n_params; c += kActorThreads)
    {
        const float4 v = src4[c];
        const int    i = 4 * c;
        if (i < n_params)
            dst[okActorLdsIndex(i, R, rp, n1, shift)] = v.x;
        if (i + 1 < n_params)
            dst[okActorLdsIndex(i + 1, R, rp, n1, shift)] = v.y;
        if (i + 2 < n_params)
            dst[okActorLdsIndex(i + 2, R, rp, n1, shift)] = v.z;
        if (i + 3 < n_params)
            dst[okActorLdsIndex(i + 3, R, rp, n1, shift)] = v.w;
    }
}

// ok_actor_join's tree over the 8 lanes of a group, lane distances 4, 2, 1: every lane gets the sum of the lanes' partial sums
__device__ __forceinline__ float okActorJoinLanes(float v)
{
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 2);
    v = v + __shfl_xor(v, 1);
    return v;
}

// The outputs z[0 .. out) of the network staged at `net` (okActorStage, R inputs) for the group's row x, in every lane of the group:
// the lanes' partial sums, their join, the output's bias.  z[k] = 0 for k >= out.
__device__ __forceinline__ void okActorForward(const float *net, const int R, const int hidden, const int out, const float *x, const int lane, float *z)
{
    const int rp = okActorRowStride(R);
    float     part[OK_ACTOR_MAX_ACTIONS];
    ok_actor_partial(net, rp, net + hidden * rp, net + hidden * rp + hidden, R, hidden, out, x, lane, part);
    const float *b2 = net + hidden * rp + hidden + out * hidden;
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
    {
        z[k] = 0.F;
        if (k < out)
            z[k] = b2[k] + okActorJoinLanes(part[k]);
    }
}

// okActorForward with REINFORCE's dropout mask `m` on the hidden layer (okenv_reinforce.h): every lane evaluates the Philox blocks of
// its own units
__device__ __forceinline__ void okActorForwardDropout(const float *net, const int R, const int hidden, const int out, const float *x, const int lane,
                                                      const ok_reinforce_mask m, float *z)
{
    const int rp = okActorRowStride(R);
    float     part[OK_ACTOR_MAX_ACTIONS];
    ok_reinforce_partial(net, rp, net + hidden * rp, net + hidden * rp + hidden, R, hidden, out, x, lane, m, part);
    const float *b2 = net + hidden * rp + hidden + out * hidden;
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
    {
        z[k] = 0.F;
        if (k < out)
            z[k] = b2[k] + okActorJoinLanes(part[k]);
    }
}

extern __shared__ float ok_actor_lds[];

// ---- shared pieces of the act kernels: the counterpart of ok_learn.h's okLearnBegin -------------------------------------------------

// The index of this act's draws: the steps taken so far plus the caller's offset
__device__ __forceinline__ uint32_t okActDraw(const OkActDrawWords &w)
{
    return (w.step_word != nullptr ? w.step_word[0] : w.host_steps) + (w.draw_offset != nullptr ? w.draw_offset[0] : 0U);
}

// What every act kernel begins with: the group, its lane, its agent and its input row
struct OkActGroup
{
    int    g, lane;
    long   a;     // the group's agent; a spare group of the last workgroup takes the last agent and part in shuffles and barriers
    bool   valid; // false for such a spare group: it stores nothing
    float *x;     // the group's row of xs
};

// The group copies its row x[i] = state(a * R + i) into xs (rows `row_stride` apart) and into the record's state (or nullptr),
// consecutive lanes on consecutive addresses.  The kernel's __syncthreads() follows.
template <class State>
__device__ __forceinline__ OkActGroup okActBegin(const int N, const int R, float *xs, const int row_stride, float *rec_state, const State &state)
{
    OkActGroup s;
    s.g              = static_cast<int>(threadIdx.x) / kActorLanes;
    s.lane           = static_cast<int>(threadIdx.x) & (kActorLanes - 1);
    const long a_raw = static_cast<long>(blockIdx.x) * kActorAgents + s.g;
    s.valid          = a_raw < N;
    s.a              = s.valid ? a_raw : static_cast<long>(N) - 1;
    s.x              = xs + s.g * row_stride;
    for (int i = s.lane; i < R; i += kActorLanes)
    {
        const float v = state(s.a * R + i);
        s.x[i]        = v;
        if (s.valid && rec_state != nullptr)
            rec_state[s.a * R + i] = v;
    }
    return s;
}

// ... with the state of the shared-network actors: x = dist / 200
__device__ __forceinline__ OkActGroup okActBegin(const float *dist, const int N, const int R, float *xs, const int row_stride, float *rec_state)
{
    return okActBegin(N, R, xs, row_stride, rec_state, [dist](const long i) { return dist[i] / OK_SENSOR_RANGE; });
}

// The record's last field, by the group's first lane
__device__ __forceinline__ void okActAlive(const uint8_t *crashed, uint8_t *rec_alive, const long a)
{
    if (rec_alive != nullptr)
        rec_alive[a] = crashed[a] ? 0 : 1;
}

// Dropout: the policy network's hidden layer is masked (okenv_actor_set_dropout with p > 0); false is section 14's kernel as it was
template <bool Dropout>
__global__ __launch_bounds__(kActorThreads) void okActorKernel(const OkActorParams p)
{
    const int R = p.f.R, H = p.ap.hidden, A = p.ap.num_actions, Hv = p.ap.value_hidden, rp = okActorRowStride(R);
    float    *pol = ok_actor_lds, *val = pol + okActorNetFloats(R, H, A), *xs = val + okActorNetFloats(R, Hv, 1);
    okActorStage(pol, p.policy, R, H, ok_actor_num_params(R, H, A));
    if (Hv > 0)
        okActorStage(val, p.value, R, Hv, ok_actor_num_params(R, Hv, 1));
    // (okActBegin and okActDraw written out: with them this kernel's schedule differs from the one it had, docs/HISTORY.md section 29)
    const int  g     = static_cast<int>(threadIdx.x) / kActorLanes;
    const int  lane  = static_cast<int>(threadIdx.x) & (kActorLanes - 1);
    const long a_raw = static_cast<long>(blockIdx.x) * kActorAgents + g;
    const bool valid = a_raw < p.f.N;
    const long a     = valid ? a_raw : static_cast<long>(p.f.N) - 1; // (spare lanes of the last wave take part in the shuffles)
    float     *x     = xs + g * rp; // (the odd stride again: the 4 groups of a half read 4 different banks)
    for (int i = lane; i < R; i += kActorLanes)
    {
        const float v = p.f.st.dist[a * R + i] / OK_SENSOR_RANGE;
        x[i]          = v;
        if (valid && p.rec.state != nullptr)
            p.rec.state[a * R + i] = v;
    }
    __syncthreads();
    float z[OK_ACTOR_MAX_ACTIONS], zv[OK_ACTOR_MAX_ACTIONS];
    if constexpr (Dropout)
    { // the mask belongs to the agent and the draw index the action draw below uses
        ok_reinforce_mask m = p.drop;
        m.agent             = p.ap.agent_base + static_cast<uint32_t>(a);
        m.draw              = (p.draw.step_word != nullptr ? p.draw.step_word[0] : p.draw.host_steps) + (p.draw.draw_offset != nullptr ? p.draw.draw_offset[0] : 0U);
        okActorForwardDropout(pol, R, H, A, x, lane, m, z);
    }
    else
        okActorForward(pol, R, H, A, x, lane, z);
    float value = 0.F;
    if (Hv > 0)
    {
        okActorForward(val, R, Hv, 1, x, lane, zv);
        value = zv[0];
    }
    const int      best  = ok_actor_argmax(z, A);
    const uint32_t draw  = (p.draw.step_word != nullptr ? p.draw.step_word[0] : p.draw.host_steps) + (p.draw.draw_offset != nullptr ? p.draw.draw_offset[0] : 0U);
    const uint32_t agent = p.ap.agent_base + static_cast<uint32_t>(a);
    float          mine  = z[0]; // lane k holds z_k
#pragma unroll
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == lane)
            mine = z[k];
    float prob;
    int   action;
    if (p.ap.mode == OKENV_ACTOR_EPS_GREEDY)
    { // every lane of the group draws the same action; z of that action comes from the lane that holds it
        action = ok_actor_eps_greedy(p.ap.epsilon, p.ap.seed, agent, draw, A, best);
        prob   = __shfl(mine, action, kActorLanes);
    }
    else
    { // the exponentials: lane k takes e_k (an fp64 evaluation each), every lane collects them
        float m = z[0];
#pragma unroll
        for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
            if (k < A && z[k] > m)
                m = z[k];
        const float el = lane < A ? ok_expf(mine - m) : 0.F;
        float       e[OK_ACTOR_MAX_ACTIONS];
#pragma unroll
        for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
            e[k] = __shfl(el, k, kActorLanes);
        const float u = p.ap.mode == OKENV_ACTOR_SAMPLE ? ok_u01(ok_actor_draw(p.ap.seed, agent, draw).v[0]) : 0.F;
        action        = ok_actor_pick(e, A, u, p.ap.mode == OKENV_ACTOR_GREEDY ? best : -1, &prob);
    }
    if (lane != 0 || !valid)
        return;
    float thr = p.ap.action_table[0][0], steer = p.ap.action_table[0][1];
#pragma unroll
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == action)
        {
            thr   = p.ap.action_table[k][0];
            steer = p.ap.action_table[k][1];
        }
    p.f.st.thr[a]   = thr;
    p.f.st.steer[a] = steer;
    if (p.rec.action != nullptr)
        p.rec.action[a] = action;
    if (p.rec.prob != nullptr)
        p.rec.prob[a] = prob;
    if (p.rec.value != nullptr && Hv > 0)
        p.rec.value[a] = value;
    okActAlive(p.f.st.crashed, p.rec.alive, a);
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okActorCheckParams(const okenv_actor_params *ap, const int R)
{
    if (ap == nullptr)
        return "params is NULL";
    if (R < 1 || R > OK_ACTOR_MAX_RAYS)
        return "the fan needs 1 .. 64 rays";
    if (ap->hidden < 1 || ap->hidden > OK_ACTOR_MAX_HIDDEN)
        return "hidden width outside 1 .. 256";
    if (ap->num_actions < 2 || ap->num_actions > OK_ACTOR_MAX_ACTIONS)
        return "number of actions outside 2 .. 8";
    if (ap->value_hidden < 0 || ap->value_hidden > OK_ACTOR_MAX_HIDDEN)
        return "value network's hidden width outside 0 .. 256";
    if (ap->mode != OKENV_ACTOR_SAMPLE && ap->mode != OKENV_ACTOR_GREEDY && ap->mode != OKENV_ACTOR_EPS_GREEDY)
        return "unknown mode (OKENV_ACTOR_SAMPLE / _GREEDY / _EPS_GREEDY)";
    if (!(ap->epsilon >= 0.F && ap->epsilon <= 1.F))
        return "epsilon outside [0, 1]";
    return nullptr;
}

// updateAction for n agents on host arrays; every output may be nullptr
inline void okActorActHost(const okenv_actor_params &ap, const float *policy, const float *value, const int R, const int n, const float *dist,
                           const uint8_t *crashed, const uint32_t draw_index, float *throttle, float *steer, int64_t *action, float *prob,
                           float *value_out, float *state, uint8_t *alive)
{
    std::vector<float> x(static_cast<size_t>(R));
    for (int a = 0; a < n; ++a)
    {
        float     pr = 0.F, v = 0.F;
        const int act = ok_actor_agent(policy, value, R, ap.hidden, ap.num_actions, ap.value_hidden, ap.mode, ap.epsilon, ap.seed,
                                       ap.agent_base + static_cast<uint32_t>(a), draw_index, dist + static_cast<size_t>(a) * R, x.data(), &pr, &v);
        if (throttle != nullptr)
            throttle[a] = ap.action_table[act][0];
        if (steer != nullptr)
            steer[a] = ap.action_table[act][1];
        if (action != nullptr)
            action[a] = act;
        if (prob != nullptr)
            prob[a] = pr;
        if (value_out != nullptr && ap.value_hidden > 0)
            value_out[a] = v;
        if (state != nullptr)
            for (int i = 0; i < R; ++i)
                state[static_cast<size_t>(a) * R + i] = x[static_cast<size_t>(i)];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

// The same with REINFORCE's dropout on the policy network's hidden layer (okenv_reinforce.h); p == 0 is okActorActHost
inline void okActorActDropoutHost(const okenv_actor_params &ap, const float p, const uint32_t dropout_seed, const float *policy, const float *value,
                                  const int R, const int n, const float *dist, const uint8_t *crashed, const uint32_t draw_index, float *throttle,
                                  float *steer, int64_t *action, float *prob, float *value_out, float *state, uint8_t *alive)
{
    if (!(p > 0.F))
        return okActorActHost(ap, policy, value, R, n, dist, crashed, draw_index, throttle, steer, action, prob, value_out, state, alive);
    const int          H = ap.hidden, A = ap.num_actions, Hv = ap.value_hidden;
    std::vector<float> x(static_cast<size_t>(R));
    ok_reinforce_mask  m{p, ok_reinforce_scale(p), dropout_seed, 0U, draw_index};
    const float       *b1 = policy + H * R, *w2 = b1 + H, *b2 = w2 + A * H;
    for (int a = 0; a < n; ++a)
    {
        m.agent = ap.agent_base + static_cast<uint32_t>(a);
        for (int i = 0; i < R; ++i)
            x[static_cast<size_t>(i)] = dist[static_cast<size_t>(a) * R + i] / OK_SENSOR_RANGE;
        float part[OK_ACTOR_LANES][OK_ACTOR_MAX_ACTIONS], col[OK_ACTOR_LANES], z[OK_ACTOR_MAX_ACTIONS];
        for (int l = 0; l < OK_ACTOR_LANES; ++l)
            ok_reinforce_partial(policy, R, b1, w2, R, H, A, x.data(), l, m, part[l]);
        for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        {
            for (int l = 0; l < OK_ACTOR_LANES; ++l)
                col[l] = k < A ? part[l][k] : 0.F;
            z[k] = k < A ? ok_actor_join(col, b2[k]) : 0.F;
        }
        float v = 0.F;
        if (Hv > 0)
        {
            const float *vb1 = value + Hv * R, *vw2 = vb1 + Hv, *vb2 = vw2 + Hv;
            for (int l = 0; l < OK_ACTOR_LANES; ++l)
            {
                ok_actor_partial(value, R, vb1, vw2, R, Hv, 1, x.data(), l, part[l]);
                col[l] = part[l][0];
            }
            v = ok_actor_join(col, vb2[0]);
        }
        float     pr  = 0.F;
        const int act = ok_actor_choose(ap.mode, ap.epsilon, ap.seed, m.agent, draw_index, z, A, &pr);
        if (throttle != nullptr)
            throttle[a] = ap.action_table[act][0];
        if (steer != nullptr)
            steer[a] = ap.action_table[act][1];
        if (action != nullptr)
            action[a] = act;
        if (prob != nullptr)
            prob[a] = pr;
        if (value_out != nullptr && Hv > 0)
            value_out[a] = v;
        if (state != nullptr)
            for (int i = 0; i < R; ++i)
                state[static_cast<size_t>(a) * R + i] = x[static_cast<size_t>(i)];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

#endif // OK_ACTOR_H
