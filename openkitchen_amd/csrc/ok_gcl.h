// ok_gcl.h -- guided cost learning on the device: updateAction, the cost update and updatePolicy of
// RLRacers/GuidedCostLearning (GCLAgent.hpp:52-180, main.cpp:150-187) through the three networks of Networks.hpp.  The rule lives in
// include/okenv_gcl.h (ok_gcl_state, ok_gcl_sample, ok_gcl_ratio_seed, ok_gcl_policy_seed, ok_gcl_cost_seed, ok_gcl_adv, ok_gcl_hidden,
// ok_gcl_back) on top of the Gaussian learner's, and is shared with the host functions below, so the device and the host entries agree
// bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.
//   okGclActKernel            32 agents x 8 lanes per workgroup: x = |hit|^2 / 200^2, the policy network, the draw, the squash, the record
//   okGclForwardKernel<Tanh>  one workgroup per 32 rows, forward only: the cost of [state | action] rows (Tanh) or the value sweep of the
//                             advantages (raw = G - v and the chunk's fp64 partials of its statistics)
//   okGclAdvStatsKernel       one workgroup: ok_batch_tree over the chunk partials, ok_batch_finish
//   okGclAdvNormKernel        adv = (raw - mean) / (std + 1e-8f)
//   okGclGradKernel<Head>     okGaussGradKernel's plan and pieces (ok_gauss.h: okMlp2Stage, okMlp2Forward, okMlp2Backward, okGaussOuterSums,
//                             okGaussVecSums) for the three heads (policy, value, cost); the heads differ in input assembly, activation,
//                             the output squash, the seed and the clip count only
//   okGclClipCountKernel      the policy slices' clip counts into the step's slot
//   okReinforceStepKernel     section 19's join kernels on the policy's and the value's parameter vector (OkJoinParams)
//   okGclCostStepKernel       the cost update's join: two sets, each divided by its own count, then added, Adam in place
// No atomics anywhere: the sums' order is the rule's.
#ifndef OK_GCL_H
#define OK_GCL_H

#include <algorithm>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_gcl.h"
#include "ok_gauss.h"

// ---- LDS ---------------------------------------------------------------------------------------------------------------------------

// The gradient kernels' LDS: okGaussPlaces' [net | xs | h1s | d1s | h2s | d2s | dzs | dlss | terms] and one more row of 32 clip flags
inline size_t okGclGradLdsBytes(const int in, const int H1, const int H2, const int A)
{
    return okGaussShapeInRange(in, H1, H2, A) ? sizeof(float) * static_cast<size_t>(okGaussPlaces(in, H1, H2, A).end + OK_LEARN_CHUNK) : 0U;
}

// The forward-only kernel's LDS: [net | xs | h1s | h2s | raws]
inline size_t okGclForwardLdsBytes(const int in, const int H1, const int H2)
{
    return sizeof(float) * static_cast<size_t>(okGaussNet(in, H1, H2, 1).floats +
                                               OK_LEARN_CHUNK * (okActorRowStride(in) + okGaussHiddenStride(H1) + okGaussHiddenStride(H2) + 1));
}

inline bool okGclShapeInRange(const int R, const int H1, const int H2, const int C1, const int C2)
{
    return okGaussShapeInRange(R, H1, H2, 2) && okGaussShapeInRange(R + 2, C1, C2, 1);
}

// The largest of the three gradient kernels; 0 outside the rule's limits
inline size_t okGclLdsBytes(const int R, const int H1, const int H2, const int C1, const int C2)
{
    if (!okGclShapeInRange(R, H1, H2, C1, C2))
        return 0U;
    return std::max(std::max(okGclGradLdsBytes(R, H1, H2, 2), okGclGradLdsBytes(R, H1, H2, 1)), okGclGradLdsBytes(R + 2, C1, C2, 1));
}

// ---- acting ------------------------------------------------------------------------------------------------------------------------

struct OkGclActParams
{
    OkActFrame       f; // (ok_actor.h)
    int              H1, H2;
    const float     *params;
    OkActDrawWords   draw;
    float            scale[2], bias[2];
    int              greedy;
    uint32_t         seed, agent_base;
    okenv_gcl_record rec;
};

__global__ __launch_bounds__(kActorThreads) void okGclActKernel(const OkGclActParams p)
{
    const int        R = p.f.R, H1 = p.H1, H2 = p.H2;
    const OkGaussNet ln  = okGaussNet(R, H1, H2, 2);
    float           *net = ok_actor_lds, *xs = net + ln.floats, *h1s = xs + kActorAgents * ln.rp, *h2s = h1s + kActorAgents * okGaussHiddenStride(H1);
    okMlp2Stage(net, p.params, ln, ok_gauss_offsets(R, H1, H2, 2), R, H1);
    // this learner's state: the squared norm of the hit over the squared range
    const float     *rel_x = p.f.st.rel_x, *rel_y = p.f.st.rel_y;
    const OkActGroup s = okActBegin(p.f.N, R, xs, ln.rp, p.rec.state, [rel_x, rel_y](const long i) { return ok_gcl_state(rel_x[i], rel_y[i]); });
    const int        g = s.g, lane = s.lane;
    __syncthreads();
    const float z3 = okMlp2Forward<false>(net, ln, R, H1, H2, 2, s.x, h1s + g * okGaussHiddenStride(H1), h2s + g * okGaussHiddenStride(H2), lane);
    // lanes 0 and 1 take one component each
    const int   k   = lane & 1;
    const float ls  = net[ln.ls + k], mu = ok_tanhf(z3);
    float       eps = 0.F;
    if (p.greedy == 0 && lane < 2)
        eps = ok_gcl_eps(p.seed, p.agent_base + static_cast<uint32_t>(s.a), okActDraw(p.draw), k);
    const ok_gcl_comp c    = ok_gcl_sample(mu, ls, eps, p.greedy);
    const float       act  = ok_gauss_action(c.squashed, k == 1 ? p.scale[1] : p.scale[0], k == 1 ? p.bias[1] : p.bias[0]);
    const float       logp = __shfl(c.n, 0, kActorLanes) + __shfl(c.n, 1, kActorLanes);
    okMlp2ActStore(p.f, s, p.rec, p.greedy, act, eps, c.pre, logp, p.rec.squashed, c.squashed);
}

// ---- forward only: the cost of rows, the value sweep -------------------------------------------------------------------------------

struct OkGclForwardParams
{
    int          R, in, H1, H2, M;
    const float *state;    // [M][R]
    const float *squashed; // [M][2]: the input's tail (the cost network), or nullptr
    const float *ret;      // [M]: out = ret - value and the statistics' partials (the value sweep), or nullptr: out = the output
    const float *params;
    float       *out;      // [M]
    double      *stat;     // with ret: [2][C], the chunks' S then the chunks' Q
    int          C;
};

template <bool Tanh>
__global__ __launch_bounds__(kLearnThreads) void okGclForwardKernel(const OkGclForwardParams p)
{
    const int        in = p.in, H1 = p.H1, H2 = p.H2, R = p.R;
    const OkGaussNet ln = okGaussNet(in, H1, H2, 1);
    const int        s1 = okGaussHiddenStride(H1), s2 = okGaussHiddenStride(H2);
    float           *net = ok_learn_lds, *xs = net + ln.floats, *h1s = xs + OK_LEARN_CHUNK * ln.rp, *h2s = h1s + OK_LEARN_CHUNK * s1;
    float           *raws = h2s + OK_LEARN_CHUNK * s2;
    const int        g = static_cast<int>(threadIdx.x) / kLearnLanes, lane = static_cast<int>(threadIdx.x) & (kLearnLanes - 1);
    const int        chunk = static_cast<int>(blockIdx.x);
    const int        left = p.M - chunk * OK_LEARN_CHUNK, n = left < OK_LEARN_CHUNK ? left : OK_LEARN_CHUNK;
    const size_t     idx = static_cast<size_t>(chunk) * OK_LEARN_CHUNK + static_cast<size_t>(g < n ? g : n - 1); // (spare groups: the last row)
    float *__restrict__ x = xs + g * ln.rp;
    for (int i = lane; i < in; i += kLearnLanes)
        x[i] = i < R ? p.state[idx * static_cast<size_t>(R) + i] : p.squashed[idx * 2U + (i - R)];
    okMlp2Stage(net, p.params, ln, ok_gcl_offsets(in, H1, H2, 1, 0), in, H1);
    __syncthreads();
    const float z = okMlp2Forward<Tanh>(net, ln, in, H1, H2, 1, x, h1s + g * s1, h2s + g * s2, lane);
    if (lane == 0 && g < n)
    {
        const float v = p.ret != nullptr ? p.ret[idx] - z : z;
        p.out[idx]    = v;
        raws[g]       = v;
    }
    if (p.ret == nullptr)
        return;
    __syncthreads();
    if (threadIdx.x == 0)
    { // the chunk's fp64 partials, ascending
        double s = 0.0, q = 0.0;
        for (int i = 0; i < n; ++i)
        {
            const double r = static_cast<double>(raws[i]);
            s              = s + r;
            q              = q + r * r;
        }
        p.stat[chunk]       = s;
        p.stat[p.C + chunk] = q;
    }
}

// ok_batch_tree over the C chunk partials of S and of Q in place, level by level, then mean and std into ms[0], ms[1]
constexpr int kGclStatsThreads = 256;
__global__ __launch_bounds__(kGclStatsThreads) void okGclAdvStatsKernel(double *stat, const int C, const int M, float *ms)
{
    double        *s = stat, *q = stat + C;
    const uint32_t n = static_cast<uint32_t>(C);
    for (uint32_t h = ok_batch_tree_width(n) >> 1; h >= 1U; h >>= 1)
    {
        for (uint32_t i = threadIdx.x; i < h; i += kGclStatsThreads)
            if (i + h < n)
            {
                s[i] = s[i] + s[i + h];
                q[i] = q[i] + q[i + h];
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        ok_batch_finish(static_cast<uint32_t>(M), s[0], q[0], &ms[0], &ms[1]);
}

__global__ __launch_bounds__(256) void okGclAdvNormKernel(float *adv, const float *ms, const int M, float *out)
{
    const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= M)
        return;
    const float a = ok_gcl_adv(adv[i], ms[0], ms[1]);
    adv[i]        = a;
    if (out != nullptr)
        out[i] = a;
}

// ---- the gradient kernels ------------------------------------------------------------------------------------------------------------

// What a gradient kernel needs for one launch, by value
struct OkGclGradParams
{
    int            R, in, H1, H2;
    int            M, Bk;    // policy / value: samples, positions of this slice; cost: Bk = the policy rows Mp
    int            P, cols;  // parameters; columns of the partials: [params | loss]
    long           base;     // first position of the slice: k * B
    const int32_t *order;    // or nullptr
    const float   *state, *pre, *logp, *ret, *adv, *squashed;
    const float   *bank_state, *bank_action; // cost: the expert bank
    int            E, Me, Ce;                // cost: bank rows, expert positions, expert chunks (the first Ce workgroups)
    uint32_t       seed, draw;               // cost: the expert draws' key and update number
    float          lo, hi;                   // policy: the ratio's range
    const float   *params;
    float         *part;      // [C][cols]
    uint32_t      *part_clip; // policy: [C], or nullptr
};

template <int Head>
__global__ __launch_bounds__(kLearnThreads) void okGclGradKernel(const OkGclGradParams p)
{
    constexpr bool kTanh = Head == OK_GCL_COST;
    constexpr int  A = Head == OK_GCL_POLICY ? 2 : 1, kNls = Head == OK_GCL_POLICY ? 2 : 0;
    const int           R = p.R, in = p.in, H1 = p.H1, H2 = p.H2;
    const OkGaussNet    ln = okGaussNet(in, H1, H2, A);
    const OkGaussPlaces at = okGaussPlaces(in, H1, H2, A);
    const int           s1 = okGaussHiddenStride(H1), s2 = okGaussHiddenStride(H2);
    float              *net = ok_learn_lds, *xs = net + at.xs, *h1s = net + at.h1s, *d1s = net + at.d1s, *h2s = net + at.h2s, *d2s = net + at.d2s;
    float              *dzs = net + at.dzs, *dlss = net + at.dlss, *terms = net + at.terms;
    int                *clips = reinterpret_cast<int *>(net + at.end);
    const int           g = static_cast<int>(threadIdx.x) / kLearnLanes, lane = static_cast<int>(threadIdx.x) & (kLearnLanes - 1);
    const int           chunk = static_cast<int>(blockIdx.x);
    // the cost update's two sets: the expert chunks come first
    const bool expert = Head == OK_GCL_COST && chunk < p.Ce;
    const int  set_chunk = (Head == OK_GCL_COST && !expert) ? chunk - p.Ce : chunk, count = expert ? p.Me : p.Bk;
    const int  left = count - set_chunk * OK_LEARN_CHUNK, n = left < OK_LEARN_CHUNK ? left : OK_LEARN_CHUNK;
    // (the spare groups of a set's last chunk work on its last sample; the sums never read their rows)
    const long q = static_cast<long>(set_chunk) * OK_LEARN_CHUNK + (g < n ? g : n - 1);
    float *__restrict__ x = xs + g * ln.rp, *__restrict__ h1 = h1s + g * s1, *__restrict__ d1 = d1s + g * s1, *__restrict__ h2 = h2s + g * s2;
    float *__restrict__ d2 = d2s + g * s2, *__restrict__ dz = dzs + g * OK_ACTOR_MAX_ACTIONS;
    size_t idx = 0;
    if constexpr (Head == OK_GCL_COST)
    {
        const float *srow, *arow;
        if (expert)
        {
            const size_t row = ok_gcl_expert_row(p.seed, static_cast<uint32_t>(q), p.draw, static_cast<uint32_t>(p.E));
            srow             = p.bank_state + row * static_cast<size_t>(R);
            arow             = p.bank_action + row * 2U;
        }
        else
        {
            srow = p.state + static_cast<size_t>(q) * static_cast<size_t>(R);
            arow = p.squashed + static_cast<size_t>(q) * 2U;
        }
        for (int i = lane; i < in; i += kLearnLanes)
            x[i] = i < R ? srow[i] : arow[i - R];
    }
    else
    {
        const long pos = p.base + q;
        idx = static_cast<size_t>(ok_learn_clamp_index(p.order != nullptr ? static_cast<long long>(p.order[pos]) : static_cast<long long>(pos), p.M));
        for (int i = lane; i < R; i += kLearnLanes)
            x[i] = p.state[idx * static_cast<size_t>(R) + i];
    }
    const ok_gauss_layout pv = ok_gcl_offsets(in, H1, H2, A, kNls);
    okMlp2Stage(net, p.params, ln, pv, in, H1);
    __syncthreads();
    const float z3 = okMlp2Forward<kTanh>(net, ln, in, H1, H2, A, x, h1, h2, lane);
    float       seed = 0.F, dls = 0.F, term = 0.F;
    int         clipped = 0;
    if constexpr (Head == OK_GCL_POLICY)
    { // lane k takes component k: exp, tanh and the two seeds; every lane of the group forms the ratio
        const int   k  = lane < A ? lane : 0;
        const float mu = ok_tanhf(z3), ls = net[ln.ls + k];
        float       sd;
        const float z    = ok_gcl_z(p.pre[idx * 2U + k], mu, ls, &sd);
        const float nk   = ok_gcl_normal_term(z, ls);
        const float logp = __shfl(nk, 0, kLearnLanes) + __shfl(nk, 1, kLearnLanes);
        float       surr, dmu;
        const float gr = ok_gcl_ratio_seed(logp, p.logp[idx], p.adv[idx], p.lo, p.hi, &surr, &clipped);
        ok_gcl_policy_seed(gr, z, sd, &dmu, &dls);
        seed = ok_gcl_tanh_back(dmu, mu);
        term = -surr;
    }
    else if constexpr (Head == OK_GCL_VALUE)
        ok_learn_value_seed(z3, p.ret[idx], &seed, &term);
    else
        ok_gcl_cost_seed(z3, expert ? 0 : 1, &term, &seed);
    dz[lane]                              = lane < A ? seed : 0.F;
    dlss[g * OK_ACTOR_MAX_ACTIONS + lane] = lane < kNls ? dls : 0.F;
    if (lane == 0)
    {
        terms[g] = term;
        clips[g] = clipped;
    }
    okMlp2Backward<kTanh>(net, ln, H1, H2, A, dz, h1, h2, d1, d2, lane);
    // the per-parameter walks into the chunk's row [params | loss]
    float *col = p.part + static_cast<size_t>(chunk) * static_cast<size_t>(p.cols);
    okGaussOuterSums(col + pv.w2, d2s, s2, H2, h1s, s1, H1, n);
    okGaussOuterSums(col + pv.w1, d1s, s1, H1, xs, ln.rp, in, n);
    okGaussOuterSums(col + pv.w3, dzs, OK_ACTOR_MAX_ACTIONS, A, h2s, s2, H2, n);
    if constexpr (kNls > 0)
        okGaussVecSums(col + pv.log_std, dlss, OK_ACTOR_MAX_ACTIONS, kNls, n);
    okGaussVecSums(col + pv.b1, d1s, s1, H1, n);
    okGaussVecSums(col + pv.b2, d2s, s2, H2, n);
    okGaussVecSums(col + pv.b3, dzs, OK_ACTOR_MAX_ACTIONS, A, n);
    okLearnSumTerms(terms, n, col + p.P);
    if constexpr (Head == OK_GCL_POLICY)
        if (threadIdx.x == 0 && p.part_clip != nullptr)
        {
            uint32_t cnt = 0U;
            for (int i = 0; i < n; ++i)
                cnt += static_cast<uint32_t>(clips[i]);
            p.part_clip[chunk] = cnt;
        }
}

// The C chunk counts of a policy slice added into the step's slot (an integer sum: any order)
__global__ __launch_bounds__(256) void okGclClipCountKernel(const uint32_t *part_clip, const int C, int32_t *slot)
{
    __shared__ uint32_t sums[256];
    uint32_t            mine = 0U;
    for (int i = static_cast<int>(threadIdx.x); i < C; i += 256)
        mine += part_clip[i];
    sums[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    uint32_t total = 0U;
    for (int i = 0; i < 256; ++i)
        total += sums[i];
    *slot += static_cast<int32_t>(total);
}

// The cost update's join: the tree over the expert chunks and over the policy chunks of every column, each sum divided by its own
// count, the two added (expert first), then the gradient's output and Adam in place, or the loss
struct OkGclCostJoinParams
{
    int                  P, cols, Ce, Cp;
    float               *part; // [Ce + Cp][cols]: the expert chunks, then the policy chunks
    float                me, mp;
    float               *params, *m, *v;
    ok_learn_adam_consts adam;
    float               *loss, *grad;
};

__host__ __device__ inline void okGclCostJoinStep(const OkGclCostJoinParams &p, const int column, const float sum_e, const float sum_p)
{
    const float ge = sum_e / p.me, gp = sum_p / p.mp;
    const float g  = ge + gp;
    if (column < p.P)
        okLearnStepParam(p.params, p.m, p.v, p.grad, column, g, p.adam);
    else if (p.loss != nullptr)
        *p.loss = g;
}

__global__ __launch_bounds__(kLearnStepCols *kLearnStepRows) void okGclCostStepKernel(const OkGclCostJoinParams p)
{
    __shared__ float last[kLearnStepRows][kLearnStepCols];
    int              column = 0;
    float            sum_e = 0.F, sum_p = 0.F;
    (void)okLearnColumnSum(p.part, p.cols, p.Ce, last, &column, &sum_e);
    __syncthreads(); // `last` is free again
    if (!okLearnColumnSum(p.part + static_cast<size_t>(p.Ce) * static_cast<size_t>(p.cols), p.cols, p.Cp, last, &column, &sum_p))
        return;
    okGclCostJoinStep(p, column, sum_e, sum_p);
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okGclCheckShape(const int R, const int H1, const int H2, const int C1, const int C2)
{
    if (R < 1 || R + 2 > OK_ACTOR_MAX_RAYS)
        return "the fan needs 1 .. 62 rays (the cost network reads R + 2 inputs)";
    if (H1 < 1 || H1 > OK_GAUSS_MAX_HIDDEN || H2 < 1 || H2 > OK_GAUSS_MAX_HIDDEN || C1 < 1 || C1 > OK_GAUSS_MAX_HIDDEN || C2 < 1 || C2 > OK_GAUSS_MAX_HIDDEN)
        return "a hidden width outside 1 .. 128";
    if (okGclLdsBytes(R, H1, H2, C1, C2) > kGaussLdsBudget)
        return "a gradient kernel's LDS for this shape exceeds 160 KB (okenv_gcl_lds_bytes)";
    return nullptr;
}

inline const char *okGclCheckConfig(const okenv_gcl_config *c, const int R)
{
    if (c == nullptr)
        return "config is NULL";
    if (const char *why = okGclCheckShape(R, c->hidden1, c->hidden2, c->cost_hidden1, c->cost_hidden2))
        return why;
    return okMlp2CheckAct(c->greedy, c->scale, c->bias);
}

inline const char *okGclCheckCostCall(const okenv_gcl_cost_batch *batch, const int32_t Mp, const int32_t Me)
{
    if (batch == nullptr)
        return "batch is NULL";
    if (batch->state == nullptr || batch->squashed == nullptr)
        return "state and squashed are required";
    if (Mp < 1 || Me < 1)
        return "Mp and Me must be at least 1";
    return nullptr;
}

inline const char *okGclCheckCall(const okenv_gcl_update_config *cfg, const okenv_gcl_batch *batch, const int32_t M, const int32_t B)
{
    if (cfg == nullptr)
        return "config is NULL";
    if (batch == nullptr)
        return "batch is NULL";
    if (batch->state == nullptr || batch->pre == nullptr || batch->logp == nullptr || batch->ret == nullptr)
        return "state, pre, logp and ret are required";
    if (M < 1 || B < 1)
        return "M and B must be at least 1";
    if (cfg->reduce != OKENV_REINFORCE_SUM && cfg->reduce != OKENV_REINFORCE_MEAN)
        return "unknown reduce (OKENV_REINFORCE_SUM / _MEAN)";
    return nullptr;
}

inline bool okGclStateComplete(const okenv_gcl_state *s)
{
    return s != nullptr && s->params != nullptr && s->m != nullptr && s->v != nullptr && s->t >= 0;
}

// Network `which` of a fan of R rays on the host
inline OkMlp2HostNet okGclHostNet(const int which, const int R, const int H1, const int H2, const float *par)
{
    return okMlp2HostNet(ok_gcl_in(which, R), H1, H2, ok_gcl_out(which), ok_gcl_nls(which), which == OK_GCL_COST ? 1 : 0, par);
}

// The action of n agents on host arrays; every output may be nullptr
inline void okGclActHost(const okenv_gcl_config &c, const float *par, const int R, const int n, const float *rel_x, const float *rel_y, const uint8_t *crashed,
                         const uint32_t draw_index, float *throttle, float *steer, float *eps_out, float *pre_out, float *squashed, float *action,
                         float *logp, float *state, uint8_t *alive)
{
    const OkMlp2HostNet net = okGclHostNet(OK_GCL_POLICY, R, c.hidden1, c.hidden2, par);
    std::vector<float> x(static_cast<size_t>(R)), h1(static_cast<size_t>(net.H1)), h2(static_cast<size_t>(net.H2));
    for (int a = 0; a < n; ++a)
    {
        const size_t sa = static_cast<size_t>(a);
        for (int i = 0; i < R; ++i)
            x[static_cast<size_t>(i)] = ok_gcl_state(rel_x[sa * R + i], rel_y[sa * R + i]);
        float z3[OK_ACTOR_MAX_ACTIONS] = {0.F}, eps[2], nn[2];
        okMlp2HostForward(net, x.data(), h1.data(), h2.data(), z3);
        for (int k = 0; k < 2; ++k)
        {
            eps[k]              = c.greedy != 0 ? 0.F : ok_gcl_eps(c.seed, c.agent_base + static_cast<uint32_t>(a), draw_index, k);
            const ok_gcl_comp co = ok_gcl_sample(ok_tanhf(z3[k]), par[k], eps[k], c.greedy);
            const float       act = ok_gauss_action(co.squashed, c.scale[k], c.bias[k]);
            nn[k]               = co.n;
            if (k == 0 && throttle != nullptr)
                throttle[a] = act;
            if (k == 1 && steer != nullptr)
                steer[a] = act;
            if (eps_out != nullptr && c.greedy == 0)
                eps_out[2 * sa + k] = eps[k];
            if (pre_out != nullptr)
                pre_out[2 * sa + k] = co.pre;
            if (squashed != nullptr)
                squashed[2 * sa + k] = co.squashed;
            if (action != nullptr)
                action[2 * sa + k] = act;
        }
        if (logp != nullptr)
            logp[a] = nn[0] + nn[1];
        if (state != nullptr)
            for (int i = 0; i < R; ++i)
                state[sa * R + i] = x[static_cast<size_t>(i)];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

// out[s] = the output of network `which` (value or cost) for M rows; squashed: the cost network's input tail
inline void okGclForwardHost(const OkMlp2HostNet &net, const int R, const float *state, const float *squashed, const int M, float *out)
{
    std::vector<float> x(static_cast<size_t>(net.in)), h1(static_cast<size_t>(net.H1)), h2(static_cast<size_t>(net.H2));
    for (int s = 0; s < M; ++s)
    {
        for (int i = 0; i < net.in; ++i)
            x[static_cast<size_t>(i)] = i < R ? state[static_cast<size_t>(s) * R + i] : squashed[static_cast<size_t>(s) * 2U + (i - R)];
        float z3[OK_ACTOR_MAX_ACTIONS] = {0.F};
        okMlp2HostForward(net, x.data(), h1.data(), h2.data(), z3);
        out[s] = z3[0];
    }
}

// The cost update on host arrays; every output may be nullptr
inline void okGclCostUpdateHost(const okenv_learner_params &lp, const uint32_t seed, const int R, const int C1, const int C2, okenv_gcl_state &st,
                                const float *bank_state, const float *bank_action, const int E, const okenv_gcl_cost_batch &in, const int Mp, const int Me,
                                const okenv_gcl_cost_output &out)
{
    const OkMlp2HostNet net = okGclHostNet(OK_GCL_COST, R, C1, C2, st.params);
    OkMlp2HostRows      rows(net);
    const int          P = net.pv.total, cols = P + 1, Ce = (Me + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK, Cp = (Mp + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
    std::vector<float> part(static_cast<size_t>(Ce + Cp) * cols);
    const uint32_t     draw = static_cast<uint32_t>(st.t);
    for (int chunk = 0; chunk < Ce + Cp; ++chunk)
    {
        const bool expert = chunk < Ce;
        const long first  = static_cast<long>(expert ? chunk : chunk - Ce) * OK_LEARN_CHUNK;
        const int  n      = static_cast<int>(std::min<long>(OK_LEARN_CHUNK, (expert ? Me : Mp) - first));
        (void)okMlp2HostChunk(
            net, rows, n, part.data() + static_cast<size_t>(chunk) * cols,
            [&](const int q, float *x)
            {
                const size_t row  = expert ? ok_gcl_expert_row(seed, static_cast<uint32_t>(first + q), draw, static_cast<uint32_t>(E)) : static_cast<size_t>(first + q);
                const float *srow = (expert ? bank_state : in.state) + row * static_cast<size_t>(R), *arow = (expert ? bank_action : in.squashed) + row * 2U;
                for (int i = 0; i < net.in; ++i)
                    x[i] = i < R ? srow[i] : arow[i - R];
            },
            [&](const int, const float *z3, float *dz, float *, float *term, int *) { ok_gcl_cost_seed(z3[0], expert ? 0 : 1, term, &dz[0]); });
    }
    st.t += 1;
    OkGclCostJoinParams j{};
    j.P      = P;
    j.me     = static_cast<float>(Me);
    j.mp     = static_cast<float>(Mp);
    j.params = st.params;
    j.m      = st.m;
    j.v      = st.v;
    j.adam   = okLearnAdamConsts(lp, st.t);
    j.loss   = out.loss;
    j.grad   = out.grad;
    for (int column = 0; column < cols; ++column)
    {
        const float sum_e = ok_learn_tree(part.data() + column, cols, static_cast<uint32_t>(Ce));
        const float sum_p = ok_learn_tree(part.data() + static_cast<size_t>(Ce) * cols + column, cols, static_cast<uint32_t>(Cp));
        okGclCostJoinStep(j, column, sum_e, sum_p);
    }
}

// The advantages of a call on host arrays: adv [M]
inline void okGclAdvHost(const OkMlp2HostNet &value, const int R, const float *state, const float *ret, const int M, float *adv)
{
    okGclForwardHost(value, R, state, nullptr, M, adv);
    const int           C = (M + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
    std::vector<double> s(static_cast<size_t>(C)), q(static_cast<size_t>(C));
    for (int chunk = 0; chunk < C; ++chunk)
    {
        double cs = 0.0, cq = 0.0;
        for (int i = chunk * OK_LEARN_CHUNK; i < std::min(M, (chunk + 1) * OK_LEARN_CHUNK); ++i)
        {
            adv[i]         = ret[i] - adv[i];
            const double r = static_cast<double>(adv[i]);
            cs             = cs + r;
            cq             = cq + r * r;
        }
        s[static_cast<size_t>(chunk)] = cs;
        q[static_cast<size_t>(chunk)] = cq;
    }
    float mean, sd;
    ok_batch_finish(static_cast<uint32_t>(M), ok_batch_tree(s.data(), static_cast<uint32_t>(C)), ok_batch_tree(q.data(), static_cast<uint32_t>(C)), &mean, &sd);
    for (int i = 0; i < M; ++i)
        adv[i] = ok_gcl_adv(adv[i], mean, sd);
}

// The policy / value update on host arrays; every output may be nullptr
inline void okGclPolicyUpdateHost(const okenv_learner_params &lp, const okenv_gcl_update_config &cfg, const int R, const int H1, const int H2,
                                  okenv_gcl_state &pol, okenv_gcl_state &val, const okenv_gcl_batch &in, const int M, const int B, const int32_t *order,
                                  const okenv_gcl_output &out)
{
    const OkMlp2HostNet pn = okGclHostNet(OK_GCL_POLICY, R, H1, H2, pol.params), vn = okGclHostNet(OK_GCL_VALUE, R, H1, H2, val.params);
    std::vector<float> adv(static_cast<size_t>(M));
    okGclAdvHost(vn, R, in.state, in.ret, M, adv.data());
    if (out.adv != nullptr)
        std::copy(adv.begin(), adv.end(), out.adv);
    const float lo = okLearnClipLo(lp.clip), hi = okLearnClipHi(lp.clip);
    const bool  accumulate = cfg.accumulate != 0;
    const auto  sample     = [&](const long pos) { return static_cast<size_t>(ok_learn_clamp_index(order != nullptr ? static_cast<long long>(order[pos]) : static_cast<long long>(pos), M)); };
    const auto  fill_from  = [&](const long first)
    {
        return [&, first](const int q, float *x)
        {
            const size_t idx = sample(first + q);
            for (int i = 0; i < R; ++i)
                x[i] = in.state[idx * static_cast<size_t>(R) + i];
        };
    };
    // the policy's slices; the clip counts of the chunks of a step's slices add up in its slot
    int64_t tp = pol.t, tv = pol.t;
    if (out.clipped != nullptr)
        std::fill(out.clipped, out.clipped + (accumulate ? 1 : okLearnMinibatches(M, B)), 0);
    {
        OkMlp2HostRows rows(pn);
        okSliceUpdateHost(lp, accumulate, okJoinOn(pn.pv.total, pol.params, pol.m, pol.v, cfg.reduce, out.grad_policy), tp, M, B, out.policy_loss,
                          [&](const long first, const int n, float *col)
                          {
                              const uint32_t cnt = okMlp2HostChunk(pn, rows, n, col, fill_from(first),
                                                                  [&](const int q, const float *z3, float *dz, float *dls, float *term, int *clipped)
                                                                  {
                                                                      const size_t idx = sample(first + q);
                                                                      float        mu[2], z[2], sd[2], nn[2];
                                                                      for (int k = 0; k < 2; ++k)
                                                                      {
                                                                          mu[k] = ok_tanhf(z3[k]);
                                                                          z[k]  = ok_gcl_z(in.pre[idx * 2U + k], mu[k], pol.params[k], &sd[k]);
                                                                          nn[k] = ok_gcl_normal_term(z[k], pol.params[k]);
                                                                      }
                                                                      float       surr;
                                                                      const float gr = ok_gcl_ratio_seed(nn[0] + nn[1], in.logp[idx], adv[idx], lo, hi, &surr, clipped);
                                                                      for (int k = 0; k < 2; ++k)
                                                                      {
                                                                          float dmu;
                                                                          ok_gcl_policy_seed(gr, z[k], sd[k], &dmu, &dls[k]);
                                                                          dz[k] = ok_gcl_tanh_back(dmu, mu[k]);
                                                                      }
                                                                      *term = -surr;
                                                                  });
                              if (out.clipped != nullptr)
                                  out.clipped[accumulate ? 0 : first / B] += static_cast<int32_t>(cnt);
                          });
    }
    {
        OkMlp2HostRows rows(vn);
        okSliceUpdateHost(lp, accumulate, okJoinOn(vn.pv.total, val.params, val.m, val.v, cfg.reduce, out.grad_value), tv, M, B, out.value_loss,
                          [&](const long first, const int n, float *col)
                          {
                              (void)okMlp2HostChunk(vn, rows, n, col, fill_from(first),
                                                   [&](const int q, const float *z3, float *dz, float *, float *term, int *)
                                                   { ok_learn_value_seed(z3[0], in.ret[sample(first + q)], &dz[0], term); });
                          });
    }
    pol.t = tp;
    val.t = tv;
}

#endif // OK_GCL_H
