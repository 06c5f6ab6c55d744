// ok_reinforce.h -- REINFORCE's update on the device: updatePolicy of RLRacers/Reinforce/ReinforceAgent.hpp:91-123
// on the batch okenv_batch_prepare leaves, through the network of Policy.hpp:22-29 with its dropout.  The rule lives in
// include/okenv_reinforce.h (ok_reinforce_kept_lane, ok_reinforce_hidden, ok_reinforce_back_hidden, ok_reinforce_seed,
// ok_reinforce_reduce) on top of the actor's and the learner's, and is shared with okReinforceUpdateHost below, so the device and the
// host entry agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  Two launches per slice on the handle's stream, built from the
// learners' shared pieces (ok_learn.h):
//   okReinforceGradKernel         one workgroup per chunk of 32 positions: the sample's mask regenerated from its flat index, forward,
//                                 seed and backward, the chunk's partial of every parameter's gradient and of the loss
//   okReinforceStepKernel<false>  the fixed tree over the chunk partials of every column, added into the accumulator
//   okReinforceStepKernel<true>   the same tree, the accumulator joined in (when there is one), reduce, Adam in place
// No atomics anywhere: the sums' order is the rule's.
#ifndef OK_REINFORCE_H
#define OK_REINFORCE_H

#include <algorithm>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_reinforce.h"
#include "ok_learn.h"

// What the join kernel okReinforceStepKernel<Step> reads, by value: the whole-episode updates (this one, ok_gauss.h's) share it
struct OkJoinParams
{
    int                  Pp, cols, C; // parameters; columns of the partials: [parameters | loss]; chunks of this slice
    float               *policy, *pol_m, *pol_v;
    float               *part;        // [C][cols] (the tree works in place)
    float               *acc;         // [cols], or nullptr when every slice steps
    int                  reduce;
    float                count;
    ok_learn_adam_consts adam;
    float               *loss;        // this step's slot, or nullptr
    float               *grad_policy;
};

// The join of a parameter vector of P floats with its moments; C, part, acc, count, adam and loss are the slice loop's to fill in
inline OkJoinParams okJoinOn(const int P, float *par, float *par_m, float *par_v, const int reduce, float *grad)
{
    OkJoinParams j{};
    j.Pp          = P;
    j.cols        = P + 1;
    j.policy      = par;
    j.pol_m       = par_m;
    j.pol_v       = par_v;
    j.reduce      = reduce;
    j.grad_policy = grad;
    return j;
}

// A column's total behind the last join of a step, in the join kernel and in the host frame: `reduce`, then the parameter's gradient
// output and Adam in place, or the step's loss slot
__host__ __device__ inline void okJoinStep(const OkJoinParams &p, const int column, const float total)
{
    const float g = ok_reinforce_reduce(total, p.reduce, p.count);
    if (column < p.Pp)
        okLearnStepParam(p.policy, p.pol_m, p.pol_v, p.grad_policy, column, g, p.adam);
    else if (p.loss != nullptr)
        *p.loss = g;
}

// What the gradient kernel needs for one slice, by value
struct OkReinforceParams
{
    int                   R, H, A;
    int                   M, Bk;    // samples, positions of this slice
    int                   Pp, cols; // parameters of the network; columns of the partials: [policy | loss]
    long                  base;     // first position of the slice: k * B
    const int32_t        *order;    // or nullptr
    okenv_reinforce_batch in;
    ok_reinforce_mask     drop;     // p, s and the seed; agent and draw come from the sample's index
    uint32_t              agent_base, draw_first;
    int                   N;        // agents per recorded row: index = row * N + agent
    const float          *policy;
    float                *part;     // [chunks][cols]
};

inline size_t okReinforceLdsBytes(const int R, const int H, const int A)
{
    return sizeof(float) * static_cast<size_t>(okLearnPlaces(okActorNetFloats(R, H, A), R, okLearnHiddenStride(H, 0), 1).end);
}

// okLearnHidden with the mask: hidden value and hidden seed of the lane's units into the sample's LDS rows
__device__ __forceinline__ void okReinforceHidden(const float *net, const int rp, const int R, const int hidden, const int out, const float *x, const float *dz,
                                                  const int lane, const ok_reinforce_mask m, float *h_row, float *ds_row)
{
    const float *b1 = net + hidden * rp, *w2 = b1 + hidden;
    ok_u32x4     r{};
    for (int j = lane, i = 0; j < hidden; j += kLearnLanes, ++i)
    {
        const int   kept = ok_reinforce_kept_lane(m, &r, lane, i);
        const float pre  = ok_learn_pre(net, rp, b1, R, x, j);
        h_row[j]         = ok_reinforce_hidden(pre, kept, m.s);
        ds_row[j]        = ok_reinforce_back_hidden(w2, hidden, out, dz, j, pre, kept, m.s);
    }
}

__global__ __launch_bounds__(kLearnThreads) void okReinforceGradKernel(const OkReinforceParams p)
{
    const int          R = p.R, H = p.H, A = p.A;
    const OkLearnChunk s = okLearnBegin(okActorNetFloats(R, H, A), R, okLearnHiddenStride(H, 0), 1, p.Bk);
    const int          g = s.g, lane = s.lane, rp = s.rp, hp = s.hp, n = s.n;
    float             *net = s.net, *x = s.x;
    const long         pos = p.base + s.q;
    const int  idx = ok_learn_clamp_index(p.order != nullptr ? static_cast<long long>(p.order[pos]) : static_cast<long long>(pos), p.M);
    for (int i = lane; i < R; i += kLearnLanes)
        x[i] = p.in.state[static_cast<size_t>(idx) * static_cast<size_t>(R) + i];
    ok_reinforce_mask m = p.drop;
    if (m.p > 0.F)
    { // whose mask: the sample's flat index is row * N + agent (an index below 0 counts as 0: device data is not validated)
        const int32_t  raw  = p.in.index[idx];
        const uint32_t flat = raw < 0 ? 0U : static_cast<uint32_t>(raw);
        m.agent             = p.agent_base + flat % static_cast<uint32_t>(p.N);
        m.draw              = p.draw_first + flat / static_cast<uint32_t>(p.N);
    }
    okActorStage(net, p.policy, R, H, p.Pp);
    __syncthreads();
    float z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS];
    okActorForwardDropout(net, R, H, A, x, lane, m, z);
    const int action = ok_learn_clamp_index(static_cast<long long>(p.in.action[idx]), A);
    float     term;
    ok_reinforce_seed(z, A, action, p.in.ret[idx], dz, &term);
    okReinforceHidden(net, rp, R, H, A, x, dz, lane, m, s.hs + g * hp, s.dss + g * hp);
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == lane)
            s.dzs[g * OK_ACTOR_MAX_ACTIONS + k] = dz[k];
    if (lane == 0)
        s.terms[g] = term;
    __syncthreads();
    float *col = p.part + static_cast<size_t>(s.chunk) * static_cast<size_t>(p.cols);
    okLearnChunkSums(p.Pp, R, H, A, s.xs, s.hs, s.dss, s.dzs, rp, hp, n, col);
    okLearnSumTerms(s.terms, n, col + p.Pp);
}

// Step: false adds the slice's column sums into the accumulator; true joins the accumulator in (when there is one), applies `reduce`
// and takes the Adam step in place
template <bool Step>
__global__ __launch_bounds__(kLearnStepCols *kLearnStepRows) void okReinforceStepKernel(const OkJoinParams p)
{
    __shared__ float last[kLearnStepRows][kLearnStepCols];
    int              column = 0;
    float            sum    = 0.F;
    if (!okLearnColumnSum(p.part, p.cols, p.C, last, &column, &sum))
        return;
    if constexpr (!Step)
        p.acc[column] = p.acc[column] + sum;
    else
        okJoinStep(p, column, p.acc != nullptr ? p.acc[column] + sum : sum);
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okReinforceCheckCall(const okenv_reinforce_config *cfg, const okenv_reinforce_batch *batch, const int32_t M, const int32_t B,
                                        const bool dropout)
{
    if (cfg == nullptr)
        return "config is NULL";
    if (batch == nullptr)
        return "batch is NULL";
    if (batch->state == nullptr || batch->action == nullptr || batch->ret == nullptr)
        return "state, action and ret are required";
    if (M < 1 || B < 1)
        return "M and B must be at least 1";
    if (cfg->reduce != OKENV_REINFORCE_SUM && cfg->reduce != OKENV_REINFORCE_MEAN)
        return "unknown reduce (OKENV_REINFORCE_SUM / _MEAN)";
    if (dropout && batch->index == nullptr)
        return "with dropout on the samples' flat indices (index) are required";
    if (dropout && cfg->num_agents < 1)
        return "with dropout on num_agents must be at least 1";
    return nullptr;
}

// The frame of a whole-episode update on host arrays: slices of B positions, chunks of OK_LEARN_CHUNK, and behind every slice the join
// (the fixed tree over the chunk partials of every column, then the accumulator or okJoinStep).  j: okJoinOn's; loss: one value per
// step, or nullptr.  chunk_sums(first, n, col) writes the columns [parameters | loss] of the chunk of n positions from `first` on.
template <class ChunkSums>
inline void okSliceUpdateHost(const okenv_learner_params &lp, const bool accumulate, OkJoinParams j, int64_t &t, const int M, const int B, float *loss,
                              const ChunkSums &chunk_sums)
{
    const int          cols = j.cols, slices = okLearnMinibatches(M, B), c_max = (std::min(B, M) + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
    std::vector<float> part(static_cast<size_t>(c_max) * cols), acc(static_cast<size_t>(cols), 0.F);
    int                slot = 0;
    for (int k = 0; k < slices; ++k)
    {
        const long base = static_cast<long>(k) * B;
        const int  Bk = static_cast<int>(std::min<long>(B, M - base)), C = (Bk + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
        for (int chunk = 0; chunk < C; ++chunk)
            chunk_sums(base + chunk * OK_LEARN_CHUNK, std::min(OK_LEARN_CHUNK, Bk - chunk * OK_LEARN_CHUNK), part.data() + static_cast<size_t>(chunk) * cols);
        const bool step = !accumulate || k + 1 == slices;
        if (step)
        {
            t += 1;
            j.count = static_cast<float>(accumulate ? M : Bk);
            j.adam  = okLearnAdamConsts(lp, t);
            j.loss  = loss != nullptr ? loss + slot : nullptr;
            ++slot;
        }
        for (int column = 0; column < cols; ++column)
        {
            const float sum = ok_learn_tree(part.data() + column, cols, static_cast<uint32_t>(C));
            if (step)
                okJoinStep(j, column, accumulate ? acc[static_cast<size_t>(column)] + sum : sum);
            else
                acc[static_cast<size_t>(column)] = acc[static_cast<size_t>(column)] + sum;
        }
    }
}

// The rule on host arrays; every output may be nullptr
inline void okReinforceUpdateHost(const okenv_learner_params &lp, const okenv_reinforce_config &cfg, const float p_drop, const uint32_t dropout_seed,
                                  const uint32_t agent_base, const int R, const int H, const int A, okenv_learner_state &st,
                                  const okenv_reinforce_batch &in, const int M, const int B, const int32_t *order, const okenv_reinforce_output &out)
{
    const int          Pp = ok_actor_num_params(R, H, A);
    std::vector<float> xs(static_cast<size_t>(OK_LEARN_CHUNK) * R), terms(OK_LEARN_CHUNK);
    OkLearnHostRows    rows;
    rows.h.resize(static_cast<size_t>(OK_LEARN_CHUNK) * H);
    rows.ds.resize(static_cast<size_t>(OK_LEARN_CHUNK) * H);
    rows.dz.resize(static_cast<size_t>(OK_LEARN_CHUNK) * OK_ACTOR_MAX_ACTIONS);
    ok_reinforce_mask m{p_drop > 0.F ? p_drop : 0.F, ok_reinforce_scale(p_drop > 0.F ? p_drop : 0.F), dropout_seed, 0U, 0U};
    const float      *b1 = st.policy + H * R, *w2 = b1 + H, *b2 = w2 + A * H;
    // the per-sample mathematics of one chunk
    const auto chunk_sums = [&](const long first, const int n, float *col)
    {
        for (int q = 0; q < n; ++q)
        {
            const long pos = first + q;
            const int  idx = ok_learn_clamp_index(order != nullptr ? static_cast<long long>(order[pos]) : static_cast<long long>(pos), M);
            float     *x   = xs.data() + static_cast<size_t>(q) * R;
            for (int i = 0; i < R; ++i)
                x[i] = in.state[static_cast<size_t>(idx) * R + i];
            if (m.p > 0.F)
            {
                const int32_t  raw  = in.index[idx];
                const uint32_t flat = raw < 0 ? 0U : static_cast<uint32_t>(raw);
                m.agent             = agent_base + flat % static_cast<uint32_t>(cfg.num_agents);
                m.draw              = cfg.draw_first + flat / static_cast<uint32_t>(cfg.num_agents);
            }
            float part_l[OK_ACTOR_LANES][OK_ACTOR_MAX_ACTIONS], colv[OK_ACTOR_LANES], z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS];
            for (int l = 0; l < OK_ACTOR_LANES; ++l)
                ok_reinforce_partial(st.policy, R, b1, w2, R, H, A, x, l, m, part_l[l]);
            for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
            {
                for (int l = 0; l < OK_ACTOR_LANES; ++l)
                    colv[l] = a < A ? part_l[l][a] : 0.F;
                z[a] = a < A ? ok_actor_join(colv, b2[a]) : 0.F;
            }
            const int action = ok_learn_clamp_index(static_cast<long long>(in.action[idx]), A);
            ok_reinforce_seed(z, A, action, in.ret[idx], dz, &terms[static_cast<size_t>(q)]);
            float *h_row = rows.h.data() + static_cast<size_t>(q) * H, *ds_row = rows.ds.data() + static_cast<size_t>(q) * H;
            for (int j = 0; j < H; ++j)
            {
                const int   kept = ok_reinforce_kept(m, j);
                const float pre  = ok_learn_pre(st.policy, R, b1, R, x, j);
                h_row[j]         = ok_reinforce_hidden(pre, kept, m.s);
                ds_row[j]        = ok_reinforce_back_hidden(w2, H, A, dz, j, pre, kept, m.s);
            }
            for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
                rows.dz[static_cast<size_t>(q) * OK_ACTOR_MAX_ACTIONS + a] = dz[a];
        }
        okLearnHostChunkSums(Pp, R, H, A, xs.data(), rows, n, col);
        col[Pp] = okLearnHostSumTerms(terms.data(), n);
    };
    okSliceUpdateHost(lp, cfg.accumulate != 0, okJoinOn(Pp, st.policy, st.policy_m, st.policy_v, cfg.reduce, out.grad_policy), st.t, M, B, out.loss, chunk_sums);
}

#endif // OK_REINFORCE_H
