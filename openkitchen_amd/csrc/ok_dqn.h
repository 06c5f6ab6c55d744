// ok_dqn.h -- Deep-Q learning on the device: the replay ring's push, and updateDQN's iterations
// (RLRacers/Deep_Q_Learning/DQAgent.hpp:106-150) on uniform samples of it.  The rule lives in include/okenv_dqn.h (ok_dqn_*) on top of
// the actor's forward and the learner's backward, sums and Adam, and is shared with okReplayPushHost / okDqnUpdateHost below, so the
// device and the host entries agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  On the handle's stream:
//   okReplayCountKernel    per workgroup of 256 agents: the number of selected agents (popcount of ballots); saves `pushed`
//   okReplayScatterKernel  each workgroup re-sums the counts in front of it, ranks its agents by ballot prefixes and writes the
//                          survivors' slots; the last workgroup advances `pushed`
//   okDqnGradKernel        one workgroup per chunk of 32 positions: draws and gathers its samples from the ring, forward of s' to y,
//                          forward and backward of s, the chunk's partial of every parameter's gradient and of the loss
//   okDqnStepKernel        the fixed tree over the chunk partials, the scale 2 / (B A), Adam in place
// No workgroup waits on another and there are no atomics: an order between workgroups is only ever the order of two launches.
#ifndef OK_DQN_H
#define OK_DQN_H

#include <algorithm>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_dqn.h"
#include "ok_learn.h"

static_assert(OKENV_REPLAY_PUSH_ALL == OK_REPLAY_PUSH_ALL && OKENV_DQN_MASK_DONE == OK_DQN_MASK_DONE, "the ABI's flags are the rule's");

// ---- the push -------------------------------------------------------------------------------------------------------------------

struct OkReplayParams
{
    int                N, R;
    uint32_t           flags;
    uint64_t           capacity;
    okenv_replay_ring  ring;
    uint64_t          *pushed;   // the ring's counter
    uint64_t          *snapshot; // its value before this push (the count kernel saves it, the scatter kernel reads only this)
    uint32_t          *counts;   // [workgroups]
    okenv_actor_record rec;
    const float       *dist;     // OKENV_F_DIST and crashed_ after the step
    const uint8_t     *crashed;
    const float       *reward;   // or nullptr: the clearance rule
};

constexpr int kReplayThreads = 256;
constexpr int kReplayWave    = 64;
constexpr int kReplayWaves   = kReplayThreads / kReplayWave;
constexpr int kReplayLanes   = kActorLanes; // the group-copy pattern: 8 lanes per row

// (The kernels of the push are templates over the parameter struct: ok_ddpg.h shares them with a ring whose action is two floats.
// A struct brings its fields under the names used here and an okReplayStoreAction / okReplayReward of its own.)
template <class P>
__device__ __forceinline__ bool okReplaySelected(const P &p, const long a)
{
    return a < p.N && ((p.flags & OK_REPLAY_PUSH_ALL) != 0U || p.rec.alive[a] != 0);
}

__device__ __forceinline__ void okReplayStoreAction(const OkReplayParams &p, const long long slot, const long a)
{
    p.ring.action[slot] = p.rec.action[a];
}

__device__ __forceinline__ float okReplayReward(const OkReplayParams &p, const int crash, const long a)
{
    return p.reward != nullptr ? p.reward[a] : ok_dqn_reward(crash, p.dist + a * p.R, p.R);
}

template <class P>
__global__ __launch_bounds__(kReplayThreads) void okReplayCountKernel(const P p)
{
    __shared__ uint32_t wave_count[kReplayWaves];
    const int           wv = static_cast<int>(threadIdx.x) / kReplayWave, lane = static_cast<int>(threadIdx.x) % kReplayWave;
    const unsigned long long b = __ballot(okReplaySelected(p, static_cast<long>(blockIdx.x) * kReplayThreads + threadIdx.x));
    if (lane == 0)
        wave_count[wv] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t s = 0;
        for (int w = 0; w < kReplayWaves; ++w)
            s += wave_count[w];
        p.counts[blockIdx.x] = s;
        if (blockIdx.x == 0)
            p.snapshot[0] = p.pushed[0];
    }
}

template <class P>
__global__ __launch_bounds__(kReplayThreads) void okReplayScatterKernel(const P p)
{
    __shared__ uint32_t      wave_count[kReplayWaves];
    __shared__ uint32_t      before_part[kReplayThreads], total_part[kReplayThreads];
    __shared__ long long     slot_of[kReplayThreads]; // slot of the workgroup's agent, or -1
    const int  wv = static_cast<int>(threadIdx.x) / kReplayWave, lane = static_cast<int>(threadIdx.x) % kReplayWave;
    const long a  = static_cast<long>(blockIdx.x) * kReplayThreads + threadIdx.x;
    // the selected agents of the workgroups in front of this one, and of all of them (integer sums: any order)
    uint32_t before = 0, total = 0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += kReplayThreads)
    {
        const uint32_t c = p.counts[b];
        total += c;
        if (b < blockIdx.x)
            before += c;
    }
    before_part[threadIdx.x] = before;
    total_part[threadIdx.x]  = total;
    const bool               sel = okReplaySelected(p, a);
    const unsigned long long b   = __ballot(sel);
    const uint32_t           pre = static_cast<uint32_t>(__popcll(b & ((1ULL << lane) - 1ULL)));
    if (lane == 0)
        wave_count[wv] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    for (int h = kReplayThreads / 2; h >= 1; h >>= 1)
    {
        if (static_cast<int>(threadIdx.x) < h)
        {
            before_part[threadIdx.x] += before_part[threadIdx.x + h];
            total_part[threadIdx.x] += total_part[threadIdx.x + h];
        }
        __syncthreads();
    }
    const uint64_t n = total_part[0], start = p.snapshot[0];
    uint64_t       k = before_part[0] + pre;
    for (int w = 0; w < wv; ++w)
        k += wave_count[w];
    long long slot = -1;
    if (sel && ok_dqn_survives(k, n, p.capacity))
    {
        slot            = static_cast<long long>(ok_dqn_slot(start + k, p.capacity));
        const int crash = p.crashed[a] != 0;
        okReplayStoreAction(p, slot, a);
        p.ring.done[slot]   = crash ? 1.F : 0.F;
        p.ring.reward[slot] = okReplayReward(p, crash, a);
    }
    slot_of[threadIdx.x] = slot;
    __syncthreads();
    // the rows: a group of 8 lanes per agent, consecutive lanes on consecutive addresses
    const int g = static_cast<int>(threadIdx.x) / kReplayLanes, l = static_cast<int>(threadIdx.x) % kReplayLanes;
    for (int q = g; q < kReplayThreads; q += kReplayThreads / kReplayLanes)
    {
        const long long s = slot_of[q];
        if (s < 0)
            continue;
        const long   src = (static_cast<long>(blockIdx.x) * kReplayThreads + q) * p.R;
        const size_t dst = static_cast<size_t>(s) * static_cast<size_t>(p.R);
        for (int i = l; i < p.R; i += kReplayLanes)
        {
            p.ring.state[dst + i]      = p.rec.state[src + i];
            p.ring.next_state[dst + i] = p.dist[src + i] / OK_SENSOR_RANGE;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        p.pushed[0] = start + n;
}

// ---- the update -----------------------------------------------------------------------------------------------------------------

struct OkDqnParams
{
    int                  R, H, A;
    int                  B, C;   // positions of a batch, its chunks
    int                  Pp, cols; // parameters; columns of the partials: [policy | e^2]
    uint64_t             capacity;
    const uint64_t      *pushed;
    okenv_replay_ring    ring;
    float               *policy, *pol_m, *pol_v;
    const float         *target; // the network of q': the online parameters or the frozen copy
    float               *part;   // [C][cols]
    float                gamma;
    uint32_t             flags, seed, draw;
    ok_learn_adam_consts adam;
    float               *loss;   // this iteration's slot, or nullptr
    float               *grad_policy;
    int32_t             *index;
};

inline size_t okDqnLdsBytes(const int R, const int H, const int A)
{
    return sizeof(float) * static_cast<size_t>(okLearnPlaces(okActorNetFloats(R, H, A), R, okLearnHiddenStride(H, 0), 1).end);
}

// The ring draw of the sampling learners (P: OkDqnParams, ok_ddpg.h's OkDdpgParams) for position q of the batch: the slot, and
// whether the ring holds anything (an empty ring gives zeros everywhere and a zero gradient)
template <class P>
__device__ __forceinline__ size_t okReplayDraw(const P &p, const int q, int *live)
{
    const uint32_t size = static_cast<uint32_t>(ok_dqn_size(p.pushed[0], p.capacity));
    *live               = size != 0U;
    return *live ? ok_dqn_sample(p.seed, static_cast<uint32_t>(q), p.draw, size) : 0U;
}

// Row idx of the ring's `state` or `next_state` into the group's LDS row, consecutive lanes on consecutive addresses
__device__ __forceinline__ void okReplayGatherRow(float *x, const float *rows, const size_t idx, const int R, const int lane, const int live)
{
    for (int i = lane; i < R; i += kLearnLanes)
        x[i] = live ? rows[idx * static_cast<size_t>(R) + i] : 0.F;
}

__global__ __launch_bounds__(kLearnThreads) void okDqnGradKernel(const OkDqnParams p)
{
    const int          R = p.R, H = p.H, A = p.A;
    const OkLearnChunk s = okLearnBegin(okActorNetFloats(R, H, A), R, okLearnHiddenStride(H, 0), 1, p.B);
    const int          g = s.g, lane = s.lane;
    int                live;
    const size_t       idx = okReplayDraw(p, s.q, &live);
    float             *net = s.net, *x = s.x;
    // s' through the target's network, to y
    okActorStage(net, p.target, R, H, p.Pp);
    okReplayGatherRow(x, p.ring.next_state, idx, R, lane, live);
    __syncthreads();
    float z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS];
    okActorForward(net, R, H, A, x, lane, z);
    const float y = ok_dqn_target(live ? p.ring.reward[idx] : 0.F, live ? p.ring.done[idx] : 0.F, p.gamma, ok_dqn_max(z, A), p.flags);
    __syncthreads(); // every group has read its s' row and the target's network: both places are free
    // s through the online network, in the same rows
    if (p.target != p.policy)
        okActorStage(net, p.policy, R, H, p.Pp);
    okReplayGatherRow(x, p.ring.state, idx, R, lane, live);
    __syncthreads();
    okActorForward(net, R, H, A, x, lane, z);
    const int action = live ? ok_learn_clamp_index(static_cast<long long>(p.ring.action[idx]), A) : 0;
    float     mine = z[0], sq; // lane k holds q_k
#pragma unroll
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == lane)
            mine = z[k];
    ok_dqn_seed(__shfl(mine, action, kLearnLanes), action, y, live, dz, &sq);
    okLearnHidden(net, s.rp, R, H, A, x, dz, lane, s.hs + g * s.hp, s.dss + g * s.hp);
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == lane)
            s.dzs[g * OK_ACTOR_MAX_ACTIONS + k] = dz[k];
    if (lane == 0)
    {
        s.terms[g] = sq;
        if (g < s.n && p.index != nullptr)
            p.index[s.q] = static_cast<int32_t>(idx);
    }
    __syncthreads();
    float *col = p.part + static_cast<size_t>(s.chunk) * static_cast<size_t>(p.cols);
    okLearnChunkSums(p.Pp, R, H, A, s.xs, s.hs, s.dss, s.dzs, s.rp, s.hp, s.n, col);
    okLearnSumTerms(s.terms, s.n, col + p.Pp);
}

__global__ __launch_bounds__(kLearnStepCols *kLearnStepRows) void okDqnStepKernel(const OkDqnParams p)
{
    __shared__ float last[kLearnStepRows][kLearnStepCols];
    int              column = 0;
    float            sum    = 0.F;
    if (!okLearnColumnSum(p.part, p.cols, p.C, last, &column, &sum))
        return;
    const float count = ok_dqn_count(p.B, p.A);
    if (column < p.Pp)
        okLearnStepParam(p.policy, p.pol_m, p.pol_v, p.grad_policy, column, ok_dqn_scale_grad(sum, count), p.adam);
    else if (p.loss != nullptr)
        *p.loss = ok_dqn_scale_loss(sum, count);
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okDqnCheckConfig(const okenv_dqn_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (!(c->gamma >= 0.F && c->gamma <= 1.F))
        return "gamma outside [0, 1]";
    if ((c->flags & ~static_cast<uint32_t>(OKENV_DQN_MASK_DONE)) != 0U)
        return "unknown flags (OKENV_DQN_MASK_DONE)";
    if (c->target_network != 0 && c->target_network != 1)
        return "target_network must be 0 or 1";
    return nullptr;
}

inline const char *okDqnCheckCall(const int32_t B, const int32_t iterations, const int num_actions)
{
    if (B < 1 || iterations < 1)
        return "B and iterations must be at least 1";
    if (static_cast<int64_t>(B) * num_actions >= (INT64_C(1) << 31))
        return "B * A must stay below 2^31";
    return nullptr;
}

inline const char *okReplayCheckCreate(const int32_t capacity, const uint32_t flags)
{
    if (capacity < 1)
        return "capacity must be at least 1";
    if ((flags & ~static_cast<uint32_t>(OKENV_REPLAY_PUSH_ALL)) != 0U)
        return "unknown flags (OKENV_REPLAY_PUSH_ALL)";
    return nullptr;
}

// (okenv_replay_ring or okenv_ddpg_ring)
template <class Ring>
inline bool okReplayRingComplete(const Ring *r)
{
    return r != nullptr && r->state != nullptr && r->next_state != nullptr && r->action != nullptr && r->reward != nullptr && r->done != nullptr;
}

// What the two rings differ in on the host, as okReplayStoreAction / okReplayReward above on the device: the action's row and the
// reward of a push without one (ok_ddpg.h has the pair for a ring whose action is two floats)
inline void okReplayStoreActionHost(const okenv_replay_ring &ring, const size_t slot, const int64_t *action, const size_t a)
{
    ring.action[slot] = action[a];
}

inline float okReplayRewardHost(const okenv_replay_ring &, const int crash, const float *dist_row, const int R)
{
    return ok_dqn_reward(crash, dist_row, R);
}

// One push, agent by agent
template <class Ring, class Action>
inline void okReplayPushHost(const Ring &ring, const uint64_t capacity, const int R, uint64_t *pushed, const uint32_t flags, const int n_agents,
                             const float *state, const Action *action, const uint8_t *alive, const float *dist, const uint8_t *crashed, const float *reward)
{
    const bool all = (flags & OK_REPLAY_PUSH_ALL) != 0U;
    uint64_t   n   = 0;
    for (int a = 0; a < n_agents; ++a)
        n += (all || alive[a] != 0) ? 1U : 0U;
    uint64_t k = 0;
    for (int a = 0; a < n_agents; ++a)
    {
        if (!(all || alive[a] != 0))
            continue;
        if (ok_dqn_survives(k, n, capacity))
        {
            const size_t slot = static_cast<size_t>(ok_dqn_slot(*pushed + k, capacity)), src = static_cast<size_t>(a) * R;
            const int    crash = crashed[a] != 0;
            for (int i = 0; i < R; ++i)
            {
                ring.state[slot * R + i]      = state[src + i];
                ring.next_state[slot * R + i] = dist[src + i] / OK_SENSOR_RANGE;
            }
            okReplayStoreActionHost(ring, slot, action, static_cast<size_t>(a));
            ring.done[slot]   = crash ? 1.F : 0.F;
            ring.reward[slot] = reward != nullptr ? reward[a] : okReplayRewardHost(ring, crash, dist + src, R);
        }
        ++k;
    }
    *pushed += n;
}

// The update on host arrays; every output may be nullptr
inline void okDqnUpdateHost(const okenv_learner_params &lp, const okenv_dqn_config &cfg, const int R, const int H, const int A, okenv_learner_state &st,
                            const float *target, const okenv_replay_ring &ring, const uint32_t size, const int B, const int iterations, const bool resample,
                            const uint32_t draw_base, const okenv_dqn_output &out)
{
    const int          Pp = ok_actor_num_params(R, H, A), cols = Pp + 1, C = (B + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
    const int          live = size != 0U;
    const float        count = ok_dqn_count(B, A);
    std::vector<float> part(static_cast<size_t>(C) * cols), xs(static_cast<size_t>(OK_LEARN_CHUNK) * R), xn(static_cast<size_t>(R)), sqs(OK_LEARN_CHUNK);
    OkLearnHostRows    rows;
    rows.h.resize(static_cast<size_t>(OK_LEARN_CHUNK) * H);
    rows.ds.resize(static_cast<size_t>(OK_LEARN_CHUNK) * H);
    rows.dz.resize(static_cast<size_t>(OK_LEARN_CHUNK) * OK_ACTOR_MAX_ACTIONS);
    for (int it = 0; it < iterations; ++it)
    {
        const uint32_t draw = draw_base + (resample ? static_cast<uint32_t>(it) : 0U);
        const float   *tgt  = cfg.target_network != 0 ? target : st.policy;
        for (int chunk = 0; chunk < C; ++chunk)
        {
            const int n   = std::min(OK_LEARN_CHUNK, B - chunk * OK_LEARN_CHUNK);
            float    *col = part.data() + static_cast<size_t>(chunk) * cols;
            for (int s = 0; s < n; ++s)
            {
                const int    q   = chunk * OK_LEARN_CHUNK + s;
                const size_t idx = live ? ok_dqn_sample(cfg.seed, static_cast<uint32_t>(q), draw, size) : 0U;
                float       *x   = xs.data() + static_cast<size_t>(s) * R;
                float        z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS];
                for (int i = 0; i < R; ++i)
                {
                    xn[static_cast<size_t>(i)] = live ? ring.next_state[idx * R + i] : 0.F;
                    x[i]                       = live ? ring.state[idx * R + i] : 0.F;
                }
                okLearnHostForward(tgt, R, H, A, xn.data(), z);
                const float y = ok_dqn_target(live ? ring.reward[idx] : 0.F, live ? ring.done[idx] : 0.F, cfg.gamma, ok_dqn_max(z, A), cfg.flags);
                okLearnHostForward(st.policy, R, H, A, x, z);
                const int action = live ? ok_learn_clamp_index(static_cast<long long>(ring.action[idx]), A) : 0;
                ok_dqn_seed(z[action], action, y, live, dz, &sqs[static_cast<size_t>(s)]);
                okLearnHostHidden(st.policy, R, H, A, x, dz, rows.h.data() + static_cast<size_t>(s) * H, rows.ds.data() + static_cast<size_t>(s) * H);
                for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
                    rows.dz[static_cast<size_t>(s) * OK_ACTOR_MAX_ACTIONS + a] = dz[a];
                if (out.index != nullptr)
                    out.index[q] = static_cast<int32_t>(idx);
            }
            okLearnHostChunkSums(Pp, R, H, A, xs.data(), rows, n, col);
            col[Pp] = okLearnHostSumTerms(sqs.data(), n);
        }
        st.t += 1;
        const ok_learn_adam_consts adam = okLearnAdamConsts(lp, st.t);
        for (int column = 0; column < cols; ++column)
        {
            const float sum = ok_learn_tree(part.data() + column, cols, static_cast<uint32_t>(C));
            if (column < Pp)
                okLearnStepParam(st.policy, st.policy_m, st.policy_v, out.grad_policy, column, ok_dqn_scale_grad(sum, count), adam);
            else if (out.loss != nullptr)
                out.loss[it] = ok_dqn_scale_loss(sum, count);
        }
    }
}

#endif // OK_DQN_H
