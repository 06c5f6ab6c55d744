// ok_learn.h -- PPO's update on the device: the minibatch loop of PPOAgent::updatePolicy
// (RLRacers/PPO/PPOAgent.hpp:109-151) on the batch okenv_batch_prepare leaves.  The rule lives in include/okenv_learn.h
// (ok_learn_policy_seed, ok_learn_value_seed, ok_learn_pre, ok_learn_back_hidden, ok_learn_term, ok_learn_tree, ok_learn_adam) on top
// of the actor's forward (ok_actor_partial, ok_expf, ok_actor_pick) and is shared with okLearnUpdateHost below, so the device and the
// host entry agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  Two launches per minibatch on the handle's stream:
//   okLearnGradKernel   one workgroup per chunk of 32 positions: forward and backward of both networks, the chunk's partial of every
//                       parameter's gradient, of the two losses and of the clip count
//   okLearnStepKernel   the fixed tree over the chunk partials of every column, the division by B_k, Adam on both networks in place
// No atomics anywhere: the sums' order is the rule's.
#ifndef OK_LEARN_H
#define OK_LEARN_H

#include <algorithm>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_learn.h"
#include "ok_actor.h"

// What the kernels need for one minibatch, by value
struct OkLearnParams
{
    int                  R, H, A, Hv;
    int                  M, Bk, C;     // samples, positions of this minibatch, its chunks
    int                  Pp, Pv, cols; // parameters of the two networks; columns of the partials: [policy | value | surr | sq]
    long                 base;         // first position of the minibatch: k * B
    const int32_t       *order;        // this epoch's row of the order, or nullptr
    okenv_ppo_batch      in;
    float               *policy, *value, *pol_m, *pol_v, *val_m, *val_v;
    float               *part;         // [C][cols]
    uint32_t            *part_clip;    // [C]
    float                lo, hi;
    ok_learn_adam_consts adam;
    float               *actor_loss, *critic_loss; // this minibatch's slots, or nullptr
    int32_t             *clipped;
    float               *grad_policy, *grad_value;
};

// The gradient kernel's shape is the actor's: 8 lanes per sample (the rule's interleave), 32 samples = one chunk per workgroup.
constexpr int kLearnThreads = kActorThreads;
constexpr int kLearnLanes   = kActorLanes;
static_assert(kLearnThreads / kLearnLanes == OK_LEARN_CHUNK, "one workgroup is one chunk");
// The step kernel: 16 columns per workgroup, 16 threads per column; thread r of a column owns the partials r, r + 16, ...
constexpr int kLearnStepCols = 16;
constexpr int kLearnStepRows = 16;

// Row stride of the per-sample hidden rows in LDS: the 8 groups of a wave write 8 consecutive units each, 8 banks apart
__host__ __device__ inline int okLearnHiddenStride(const int H, const int Hv)
{
    return (H > Hv ? H : Hv) + 8;
}

// One network at a time in LDS (the value network first, then the policy network in the same place): the larger of the two
__host__ __device__ inline int okLearnNetFloats(const int R, const int H, const int A, const int Hv)
{
    const int a = okActorNetFloats(R, H, A), b = okActorNetFloats(R, Hv, 1);
    return a > b ? a : b;
}

// ---- shared pieces of the learners' kernels (PPO here, Deep-Q in ok_dqn.h, DDPG in ok_ddpg.h) ---------------

// The LDS of a gradient kernel, in floats from its start: [net | xs | hs | dss | dzs | terms], that is the staged network, then for
// the chunk's 32 samples the input rows (`in` wide), the hidden values and hidden seeds (stride hp), the output seeds and `terms`
// rows of per-sample terms (a loss term; PPO has three: surrogate, squared error, clip flag).  `end` is the launch's size.
struct OkLearnPlaces
{
    int xs, hs, dss, dzs, terms, end;
};

__host__ __device__ inline OkLearnPlaces okLearnPlaces(const int net_floats, const int in, const int hp, const int terms)
{
    OkLearnPlaces at;
    at.xs    = net_floats;
    at.hs    = at.xs + OK_LEARN_CHUNK * okActorRowStride(in);
    at.dss   = at.hs + OK_LEARN_CHUNK * hp;
    at.dzs   = at.dss + OK_LEARN_CHUNK * hp;
    at.terms = at.dzs + OK_LEARN_CHUNK * OK_ACTOR_MAX_ACTIONS;
    at.end   = at.terms + OK_LEARN_CHUNK * terms;
    return at;
}

inline size_t okLearnLdsBytes(const int R, const int H, const int A, const int Hv)
{
    return sizeof(float) * static_cast<size_t>(okLearnPlaces(okLearnNetFloats(R, H, A, Hv), R, okLearnHiddenStride(H, Hv), 3).end);
}

extern __shared__ float ok_learn_lds[];

// What every gradient kernel begins with: the LDS places, the group's lane, the chunk and the group's sample
struct OkLearnChunk
{
    float *net, *xs, *hs, *dss, *dzs, *terms, *x; // x: the group's input row
    int    g, lane, chunk, n, q, rp, hp;          // n: samples of this chunk; q: the group's position in the batch of B
};

__device__ __forceinline__ OkLearnChunk okLearnBegin(const int net_floats, const int in, const int hp, const int terms, const int B)
{
    const OkLearnPlaces at = okLearnPlaces(net_floats, in, hp, terms);
    OkLearnChunk        s;
    s.rp    = okActorRowStride(in);
    s.hp    = hp;
    s.net   = ok_learn_lds;
    s.xs    = s.net + at.xs;
    s.hs    = s.net + at.hs;
    s.dss   = s.net + at.dss;
    s.dzs   = s.net + at.dzs;
    s.terms = s.net + at.terms;
    s.g     = static_cast<int>(threadIdx.x) / kLearnLanes;
    s.lane  = static_cast<int>(threadIdx.x) & (kLearnLanes - 1);
    s.chunk = static_cast<int>(blockIdx.x);
    const int left = B - s.chunk * OK_LEARN_CHUNK;
    s.n            = left < OK_LEARN_CHUNK ? left : OK_LEARN_CHUNK;
    // (the spare groups of the last chunk take part in the shuffles with its last sample; the sums never read their rows)
    s.q = s.chunk * OK_LEARN_CHUNK + (s.g < s.n ? s.g : s.n - 1);
    s.x = s.xs + s.g * s.rp;
    return s;
}

// Thread 0 sums the chunk's n terms in ascending order into the column behind the parameters
__device__ __forceinline__ void okLearnSumTerms(const float *terms, const int n, float *dst)
{
    if (threadIdx.x != 0)
        return;
    float acc = 0.F;
    for (int q = 0; q < n; ++q)
        acc = acc + terms[q];
    *dst = acc;
}

// The same sum in a host entry
inline float okLearnHostSumTerms(const float *terms, const int n)
{
    float acc = 0.F;
    for (int q = 0; q < n; ++q)
        acc = acc + terms[q];
    return acc;
}

// A column that is parameter k of a network, in a step kernel and in a host entry's loop: the gradient's output, Adam in place
__host__ __device__ inline void okLearnStepParam(float *par, float *m, float *v, float *grad_out, const int k, const float g, const ok_learn_adam_consts &adam)
{
    if (grad_out != nullptr)
        grad_out[k] = g;
    ok_learn_adam(par + k, m + k, v + k, g, adam);
}

// Phase B: threads own parameters and walk the chunk's samples in ascending position.  ok_learn_term's four kinds, the choice hoisted
// out of the walk.
__device__ __forceinline__ void okLearnChunkSums(const int P, const int in, const int hidden, const int out, const float *xs, const float *hs,
                                                 const float *dss, const float *dzs, const int rp, const int hp, const int n, float *dst)
{
    for (int pi = static_cast<int>(threadIdx.x); pi < P; pi += kLearnThreads)
    {
        const ok_learn_slot s  = ok_learn_decode(pi, in, hidden, out);
        const float        *a  = (s.kind < 2 ? dss : dzs) + s.a;
        const int           sa = s.kind < 2 ? hp : OK_ACTOR_MAX_ACTIONS;
        const float        *b  = s.kind == 0 ? xs + s.b : hs + s.b;
        const int           sb = s.kind == 0 ? rp : hp;
        float               acc = 0.F;
        if ((s.kind & 1) != 0)
            for (int q = 0; q < n; ++q)
                acc = acc + a[q * sa];
        else
            for (int q = 0; q < n; ++q)
                acc = acc + a[q * sa] * b[q * sb];
        dst[pi] = acc;
    }
}

// Phase A's second half for the lane's hidden units: hidden value and hidden seed of every unit into the sample's LDS rows
__device__ __forceinline__ void okLearnHidden(const float *net, const int rp, const int R, const int hidden, const int out, const float *x, const float *dz,
                                              const int lane, float *h_row, float *ds_row)
{
    const float *b1 = net + hidden * rp, *w2 = b1 + hidden;
    for (int j = lane; j < hidden; j += kLearnLanes)
    {
        const float s = ok_learn_pre(net, rp, b1, R, x, j);
        h_row[j]      = s > 0.F ? s : 0.F;
        ds_row[j]     = ok_learn_back_hidden(w2, hidden, out, dz, j, s);
    }
}

__global__ __launch_bounds__(kLearnThreads) void okLearnGradKernel(const OkLearnParams p)
{
    const int          R = p.R, H = p.H, A = p.A, Hv = p.Hv;
    const OkLearnChunk s = okLearnBegin(okLearnNetFloats(R, H, A, Hv), R, okLearnHiddenStride(H, Hv), 3, p.Bk);
    const int          g = s.g, lane = s.lane, rp = s.rp, hp = s.hp, n = s.n;
    float             *net = s.net, *x = s.x, *surrs = s.terms, *sqs = surrs + OK_LEARN_CHUNK;
    int               *clips = reinterpret_cast<int *>(sqs + OK_LEARN_CHUNK);
    const long         pos = p.base + s.q;
    const int  idx = ok_learn_clamp_index(p.order != nullptr ? static_cast<long long>(p.order[pos]) : static_cast<long long>(pos), p.M);
    for (int i = lane; i < R; i += kLearnLanes)
        x[i] = p.in.state[static_cast<size_t>(idx) * static_cast<size_t>(R) + i];
    const float ret = p.in.ret[idx];
    float       adv = p.in.adv != nullptr ? p.in.adv[idx] : 0.F;
    float      *col = p.part + static_cast<size_t>(s.chunk) * static_cast<size_t>(p.cols);
    float       z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS];
    if (Hv > 0)
    { // the critic: its value is also the advantage's, from before either step
        okActorStage(net, p.value, R, Hv, p.Pv);
        __syncthreads();
        okActorForward(net, R, Hv, 1, x, lane, z);
        const float value = z[0];
        float       sq;
#pragma unroll
        for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
            dz[k] = 0.F;
        ok_learn_value_seed(value, ret, &dz[0], &sq);
        if (p.in.adv == nullptr)
            adv = ret - value;
        okLearnHidden(net, rp, R, Hv, 1, x, dz, lane, s.hs + g * hp, s.dss + g * hp);
        if (lane == 0)
        {
            s.dzs[g * OK_ACTOR_MAX_ACTIONS] = dz[0];
            sqs[g]                          = sq;
        }
        __syncthreads();
        okLearnChunkSums(p.Pv, R, Hv, 1, s.xs, s.hs, s.dss, s.dzs, rp, hp, n, col + p.Pp);
        okLearnSumTerms(sqs, n, col + p.Pp + p.Pv + 1);
        __syncthreads(); // the network's place and the rows are free again
    }
    else if (threadIdx.x == 0)
        col[p.Pp + p.Pv + 1] = 0.F;
    okActorStage(net, p.policy, R, H, p.Pp);
    __syncthreads();
    okActorForward(net, R, H, A, x, lane, z);
    const int action = ok_learn_clamp_index(static_cast<long long>(p.in.action[idx]), A);
    float     surr;
    int       clipped;
    ok_learn_policy_seed(z, A, action, p.in.prob[idx], adv, p.lo, p.hi, dz, &surr, &clipped);
    okLearnHidden(net, rp, R, H, A, x, dz, lane, s.hs + g * hp, s.dss + g * hp);
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == lane)
            s.dzs[g * OK_ACTOR_MAX_ACTIONS + k] = dz[k];
    if (lane == 0)
    {
        surrs[g] = surr;
        clips[g] = clipped;
    }
    __syncthreads();
    okLearnChunkSums(p.Pp, R, H, A, s.xs, s.hs, s.dss, s.dzs, rp, hp, n, col);
    okLearnSumTerms(surrs, n, col + p.Pp + p.Pv);
    if (threadIdx.x == 0)
    {
        uint32_t cnt = 0U;
        for (int q = 0; q < n; ++q)
            cnt += static_cast<uint32_t>(clips[q]);
        p.part_clip[s.chunk] = cnt;
    }
}

// ok_learn_tree over the C chunk partials of every column, split so that no two threads ever touch the same partial: at the levels
// h >= 16 the partials i and i + h have the same residue mod 16, so thread r of a column does all of them for its residue in place;
// the 16 that remain meet in LDS, where thread 0 of the column takes the last four levels, the division by B_k and the Adam step.
// The whole workgroup calls it (there is a barrier inside); true for the one thread per live column that holds the column's sum.
__device__ __forceinline__ bool okLearnColumnSum(float *part, const int cols, const int chunks, float (*last)[kLearnStepCols], int *column_out, float *sum_out)
{
    const int      c = static_cast<int>(threadIdx.x) % kLearnStepCols, r = static_cast<int>(threadIdx.x) / kLearnStepCols;
    const int      column = static_cast<int>(blockIdx.x) * kLearnStepCols + c;
    const bool     live   = column < cols;
    const uint32_t n      = static_cast<uint32_t>(chunks);
    const size_t   stride = static_cast<size_t>(cols);
    uint32_t       w      = 1U;
    while (w < n)
        w <<= 1;
    float *x = part + (live ? column : 0);
    if (live)
    {
        for (uint32_t h = w >> 1; h >= static_cast<uint32_t>(kLearnStepRows); h >>= 1)
            for (uint32_t i = static_cast<uint32_t>(r); i < h; i += kLearnStepRows)
                if (i + h < n)
                    x[i * stride] = x[i * stride] + x[(i + h) * stride];
        last[r][c] = static_cast<uint32_t>(r) < n ? x[static_cast<size_t>(r) * stride] : 0.F;
    }
    __syncthreads();
    if (!live || r != 0)
        return false;
    for (uint32_t h = (w >> 1) < kLearnStepRows / 2U ? (w >> 1) : kLearnStepRows / 2U; h >= 1U; h >>= 1)
        for (uint32_t i = 0; i < h; ++i)
            if (i + h < n)
                last[i][c] = last[i][c] + last[i + h][c];
    *column_out = column;
    *sum_out    = last[0][c];
    return true;
}

__global__ __launch_bounds__(kLearnStepCols *kLearnStepRows) void okLearnStepKernel(const OkLearnParams p)
{
    __shared__ float last[kLearnStepRows][kLearnStepCols];
    int              column = 0;
    float            sum    = 0.F;
    if (!okLearnColumnSum(p.part, p.cols, p.C, last, &column, &sum))
        return;
    const uint32_t n  = static_cast<uint32_t>(p.C);
    const float    bk = static_cast<float>(p.Bk);
    if (column < p.Pp)
        okLearnStepParam(p.policy, p.pol_m, p.pol_v, p.grad_policy, column, sum / bk, p.adam);
    else if (column < p.Pp + p.Pv)
        okLearnStepParam(p.value, p.val_m, p.val_v, p.grad_value, column - p.Pp, sum / bk, p.adam);
    else if (column == p.Pp + p.Pv)
    {
        if (p.actor_loss != nullptr)
            *p.actor_loss = -(sum / bk);
    }
    else
    {
        if (p.critic_loss != nullptr)
            *p.critic_loss = sum / bk;
        if (p.clipped != nullptr)
        {
            uint32_t cnt = 0U;
            for (uint32_t i = 0; i < n; ++i)
                cnt += p.part_clip[i];
            *p.clipped = static_cast<int32_t>(cnt);
        }
    }
}

// ok_learn_adam alone, one parameter per thread (okenv_debug_adam_device): the Adam of every join kernel above without the join
__global__ void __launch_bounds__(256) okDebugAdamKernel(float *p, float *m, float *v, const float *g, const ok_learn_adam_consts adam, const unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        ok_learn_adam(p + i, m + i, v + i, g[i], adam);
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okLearnCheckParams(const okenv_learner_params *lp)
{
    if (lp == nullptr)
        return "params is NULL";
    if (!(lp->lr > 0.F) || !(lp->lr < 3.0e38F))
        return "lr must be positive and finite";
    if (!(lp->clip >= 0.F && lp->clip < 1.F))
        return "clip outside [0, 1)";
    if (!(lp->beta1 >= 0.F && lp->beta1 < 1.F) || !(lp->beta2 >= 0.F && lp->beta2 < 1.F))
        return "a beta outside [0, 1)";
    if (!(lp->eps > 0.F) || !(lp->eps < 3.0e38F))
        return "eps must be positive and finite";
    return nullptr;
}

inline const char *okLearnCheckCall(const okenv_ppo_batch *batch, const int32_t M, const int32_t B, const int32_t epochs, const int value_hidden)
{
    if (batch == nullptr)
        return "batch is NULL";
    if (batch->state == nullptr || batch->action == nullptr || batch->prob == nullptr || batch->ret == nullptr)
        return "state, action, prob and ret are required";
    if (M < 1 || B < 1 || epochs < 1)
        return "M, B and epochs must be at least 1";
    if (static_cast<int64_t>(epochs) * M >= (INT64_C(1) << 31))
        return "epochs * M must stay below 2^31";
    if (batch->adv == nullptr && value_hidden == 0)
        return "without adv the advantage needs a value network";
    return nullptr;
}

// Minibatches per epoch, ceil(M / B), without leaving int32 for any B >= 1 (M >= 1)
inline int okLearnMinibatches(const int32_t M, const int32_t B)
{
    return static_cast<int>((static_cast<int64_t>(M) + B - 1) / B);
}

// The constants of the step with number t
inline ok_learn_adam_consts okLearnAdamConsts(const okenv_learner_params &lp, const int64_t t)
{
    ok_learn_adam_consts c;
    c.beta1 = lp.beta1;
    c.omb1  = static_cast<float>(1.0 - static_cast<double>(lp.beta1));
    c.beta2 = lp.beta2;
    c.omb2  = static_cast<float>(1.0 - static_cast<double>(lp.beta2));
    c.eps   = lp.eps;
    ok_learn_factors(lp.lr, lp.beta1, lp.beta2, t, &c.step, &c.bc2);
    return c;
}

inline float okLearnClipLo(const float clip)
{
    return static_cast<float>(1.0 - static_cast<double>(clip));
}

inline float okLearnClipHi(const float clip)
{
    return static_cast<float>(1.0 + static_cast<double>(clip));
}

// One network's rows of one chunk on the host: what the kernel keeps in LDS
struct OkLearnHostRows
{
    std::vector<float> h, ds, dz; // [32][hidden], [32][hidden], [32][8]
};

// Forward of one network for one sample: the outputs z (8 entries)
inline void okLearnHostForward(const float *net, const int R, const int hidden, const int out, const float *x, float *z)
{
    float        part[OK_ACTOR_LANES][OK_ACTOR_MAX_ACTIONS], colv[OK_ACTOR_LANES];
    const float *b1 = net + hidden * R, *w2 = b1 + hidden, *b2 = w2 + out * hidden;
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        ok_actor_partial(net, R, b1, w2, R, hidden, out, x, l, part[l]);
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
    {
        for (int l = 0; l < OK_ACTOR_LANES; ++l)
            colv[l] = k < out ? part[l][k] : 0.F;
        z[k] = k < out ? ok_actor_join(colv, b2[k]) : 0.F;
    }
}

inline void okLearnHostHidden(const float *net, const int R, const int hidden, const int out, const float *x, const float *dz, float *h_row, float *ds_row)
{
    const float *b1 = net + hidden * R, *w2 = b1 + hidden;
    for (int j = 0; j < hidden; ++j)
    {
        const float s = ok_learn_pre(net, R, b1, R, x, j);
        h_row[j]      = s > 0.F ? s : 0.F;
        ds_row[j]     = ok_learn_back_hidden(w2, hidden, out, dz, j, s);
    }
}

inline void okLearnHostChunkSums(const int P, const int R, const int hidden, const int out, const float *xs, const OkLearnHostRows &rows, const int n, float *dst)
{
    for (int pi = 0; pi < P; ++pi)
    {
        const ok_learn_slot s   = ok_learn_decode(pi, R, hidden, out);
        float               acc = 0.F;
        for (int q = 0; q < n; ++q)
            acc = acc + ok_learn_term(s, xs + static_cast<size_t>(q) * R, rows.h.data() + static_cast<size_t>(q) * hidden,
                                      rows.ds.data() + static_cast<size_t>(q) * hidden, rows.dz.data() + static_cast<size_t>(q) * OK_ACTOR_MAX_ACTIONS);
        dst[pi] = acc;
    }
}

// The rule on host arrays; every output may be nullptr
inline void okLearnUpdateHost(const okenv_learner_params &lp, const int R, const int H, const int A, const int Hv, okenv_learner_state &st,
                              const okenv_ppo_batch &in, const int M, const int B, const int epochs, const int32_t *order, const okenv_ppo_output &out)
{
    const int    Pp = ok_actor_num_params(R, H, A), Pv = Hv > 0 ? ok_actor_num_params(R, Hv, 1) : 0, cols = Pp + Pv + 2;
    const int    per_epoch = okLearnMinibatches(M, B), c_max = (std::min(B, M) + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
    const float  lo = okLearnClipLo(lp.clip), hi = okLearnClipHi(lp.clip);
    const size_t hm = static_cast<size_t>(std::max(H, Hv));
    std::vector<float>    part(static_cast<size_t>(c_max) * cols), xs(static_cast<size_t>(OK_LEARN_CHUNK) * R), surrs(OK_LEARN_CHUNK), sqs(OK_LEARN_CHUNK);
    std::vector<uint32_t> part_clip(static_cast<size_t>(c_max));
    OkLearnHostRows       rows;
    rows.h.resize(OK_LEARN_CHUNK * hm);
    rows.ds.resize(OK_LEARN_CHUNK * hm);
    rows.dz.resize(static_cast<size_t>(OK_LEARN_CHUNK) * OK_ACTOR_MAX_ACTIONS);
    std::vector<float> advs(OK_LEARN_CHUNK), rets(OK_LEARN_CHUNK), olds(OK_LEARN_CHUNK);
    std::vector<int>   acts(OK_LEARN_CHUNK), clips(OK_LEARN_CHUNK);
    for (int e = 0; e < epochs; ++e)
        for (int k = 0; k < per_epoch; ++k)
        {
            const long base = static_cast<long>(k) * B;
            const int  Bk = static_cast<int>(std::min<long>(B, M - base)), C = (Bk + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
            for (int chunk = 0; chunk < C; ++chunk)
            {
                const int n   = std::min(OK_LEARN_CHUNK, Bk - chunk * OK_LEARN_CHUNK);
                float    *col = part.data() + static_cast<size_t>(chunk) * cols;
                for (int q = 0; q < n; ++q)
                {
                    const long pos = base + chunk * OK_LEARN_CHUNK + q;
                    const int  idx = ok_learn_clamp_index(order != nullptr ? static_cast<long long>(order[static_cast<size_t>(e) * M + pos]) : static_cast<long long>(pos), M);
                    for (int i = 0; i < R; ++i)
                        xs[static_cast<size_t>(q) * R + i] = in.state[static_cast<size_t>(idx) * R + i];
                    rets[q] = in.ret[idx];
                    advs[q] = in.adv != nullptr ? in.adv[idx] : 0.F;
                    olds[q] = in.prob[idx];
                    acts[q] = ok_learn_clamp_index(static_cast<long long>(in.action[idx]), A);
                }
                if (Hv > 0)
                {
                    for (int q = 0; q < n; ++q)
                    {
                        float z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS] = {0.F};
                        okLearnHostForward(st.value, R, Hv, 1, xs.data() + static_cast<size_t>(q) * R, z);
                        ok_learn_value_seed(z[0], rets[q], &dz[0], &sqs[q]);
                        if (in.adv == nullptr)
                            advs[q] = rets[q] - z[0];
                        okLearnHostHidden(st.value, R, Hv, 1, xs.data() + static_cast<size_t>(q) * R, dz, rows.h.data() + static_cast<size_t>(q) * Hv,
                                          rows.ds.data() + static_cast<size_t>(q) * Hv);
                        for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
                            rows.dz[static_cast<size_t>(q) * OK_ACTOR_MAX_ACTIONS + a] = dz[a];
                    }
                    okLearnHostChunkSums(Pv, R, Hv, 1, xs.data(), rows, n, col + Pp);
                    col[Pp + Pv + 1] = okLearnHostSumTerms(sqs.data(), n);
                }
                else
                    col[Pp + Pv + 1] = 0.F;
                for (int q = 0; q < n; ++q)
                {
                    float z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS];
                    okLearnHostForward(st.policy, R, H, A, xs.data() + static_cast<size_t>(q) * R, z);
                    ok_learn_policy_seed(z, A, acts[q], olds[q], advs[q], lo, hi, dz, &surrs[q], &clips[q]);
                    okLearnHostHidden(st.policy, R, H, A, xs.data() + static_cast<size_t>(q) * R, dz, rows.h.data() + static_cast<size_t>(q) * H,
                                      rows.ds.data() + static_cast<size_t>(q) * H);
                    for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
                        rows.dz[static_cast<size_t>(q) * OK_ACTOR_MAX_ACTIONS + a] = dz[a];
                }
                okLearnHostChunkSums(Pp, R, H, A, xs.data(), rows, n, col);
                uint32_t cnt = 0U;
                for (int q = 0; q < n; ++q)
                    cnt += static_cast<uint32_t>(clips[q]);
                col[Pp + Pv]     = okLearnHostSumTerms(surrs.data(), n);
                part_clip[chunk] = cnt;
            }
            st.t += 1;
            const ok_learn_adam_consts adam = okLearnAdamConsts(lp, st.t);
            const float                bk   = static_cast<float>(Bk);
            const size_t               slot = static_cast<size_t>(e) * per_epoch + k;
            for (int column = 0; column < cols; ++column)
            {
                const float sum = ok_learn_tree(part.data() + column, cols, static_cast<uint32_t>(C));
                if (column < Pp)
                    okLearnStepParam(st.policy, st.policy_m, st.policy_v, out.grad_policy, column, sum / bk, adam);
                else if (column < Pp + Pv)
                    okLearnStepParam(st.value, st.value_m, st.value_v, out.grad_value, column - Pp, sum / bk, adam);
                else if (column == Pp + Pv)
                {
                    if (out.actor_loss != nullptr)
                        out.actor_loss[slot] = -(sum / bk);
                }
                else if (out.critic_loss != nullptr)
                    out.critic_loss[slot] = sum / bk;
            }
            if (out.clipped != nullptr)
            {
                uint32_t cnt = 0U;
                for (int chunk = 0; chunk < C; ++chunk)
                    cnt += part_clip[static_cast<size_t>(chunk)];
                out.clipped[slot] = static_cast<int32_t>(cnt);
            }
        }
}

#endif // OK_LEARN_H
