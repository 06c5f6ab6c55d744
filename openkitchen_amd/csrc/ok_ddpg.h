// ok_ddpg.h -- DDPG on the device: the continuous actor's action kernel, the push of a ring whose action is
// two floats, and DDPGAgent::update's iterations (RLRacers/DDPG/DDPGAgent.hpp:127-170) on uniform samples of it.  The rule lives in
// include/okenv_ddpg.h (ok_ddpg_*) on top of the actor's forward, the learner's backward, sums and Adam, and the ring's rules, and is
// shared with okDdpgActHost / okReplayPushHost (ok_dqn.h) / okDdpgUpdateHost below, so the device and the host entries agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  On the handle's stream:
//   okDdpgActKernel         32 agents x 8 lanes per workgroup: x = dist / 200, the actor, tanh * scale + bias, noise, the record
//   okReplayCountKernel /   section 17's push (ok_dqn.h), instantiated for a two-float action row
//   okReplayScatterKernel
//   okDdpgCriticGradKernel  one workgroup per chunk of 32 positions: draws and gathers its rows, a' and q' with the target networks
//                           (staged one at a time in the same LDS), the online critic's forward and backward, the chunk's partials
//   okDdpgActorGradKernel   the same shape: the online actor, the stepped critic, da by shuffles over the group, the actor's backward
//   okDdpgStepKernel        the fixed tree over the chunk partials, the scale, Adam in place, the soft update of that network's target
// An iteration is four launches.  No atomics, no MFMA (a chain of them does not compute the rule's order), and no workgroup waits on
// another: an order between workgroups is only ever the order of two launches.
#ifndef OK_DDPG_H
#define OK_DDPG_H

#include <algorithm>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_ddpg.h"
#include "ok_dqn.h"

// ---- acting ---------------------------------------------------------------------------------------------------------------------

struct OkDdpgActParams
{
    OkActFrame        f; // (ok_actor.h)
    int               H;
    const float      *actor; // padded to a multiple of four floats
    OkActDrawWords    draw;
    float             scale[2], bias[2], noise[2];
    uint32_t          seed, agent_base;
    okenv_ddpg_record rec;
};

inline size_t okDdpgActLdsBytes(const int R, const int H)
{
    return sizeof(float) * static_cast<size_t>(okActorNetFloats(R, H, 2) + kActorAgents * okActorRowStride(R));
}

// tanh * scale + bias of both outputs: lanes 0 and 1 of the group take one ok_tanhf each (an fp64 evaluation), every lane gets both
__device__ __forceinline__ void okDdpgGroupAction(const float z0, const float z1, const float *scale, const float *bias, const int lane, float *a, float *t)
{
    float       tm = 0.F;
    const float am = ok_ddpg_action(lane == 1 ? z1 : z0, lane == 1 ? scale[1] : scale[0], lane == 1 ? bias[1] : bias[0], &tm);
    a[0]           = __shfl(am, 0, kActorLanes);
    a[1]           = __shfl(am, 1, kActorLanes);
    t[0]           = __shfl(tm, 0, kActorLanes);
    t[1]           = __shfl(tm, 1, kActorLanes);
}

__global__ __launch_bounds__(kActorThreads) void okDdpgActKernel(const OkDdpgActParams p)
{
    const int R = p.f.R, H = p.H;
    float    *net = ok_actor_lds, *xs = net + okActorNetFloats(R, H, 2);
    okActorStage(net, p.actor, R, H, ok_actor_num_params(R, H, 2));
    const OkActGroup s    = okActBegin(p.f.st.dist, p.f.N, R, xs, okActorRowStride(R), p.rec.state);
    const int        lane = s.lane;
    const long       a    = s.a;
    __syncthreads();
    float z[OK_ACTOR_MAX_ACTIONS], act[2], t[2];
    okActorForward(net, R, H, 2, s.x, lane, z);
    okDdpgGroupAction(z[0], z[1], p.scale, p.bias, lane, act, t);
    if (lane != 0 || !s.valid)
        return;
    if (p.noise[0] > 0.F || p.noise[1] > 0.F)
    {
        const ok_u32x4 r = ok_ddpg_draw(p.seed, p.agent_base + static_cast<uint32_t>(a), okActDraw(p.draw));
        act[0]           = ok_ddpg_explore(act[0], p.noise[0], r.v[0], p.scale[0], p.bias[0]);
        act[1]           = ok_ddpg_explore(act[1], p.noise[1], r.v[1], p.scale[1], p.bias[1]);
    }
    p.f.st.thr[a]   = act[0];
    p.f.st.steer[a] = act[1];
    if (p.rec.action != nullptr)
    {
        p.rec.action[2 * a]     = act[0];
        p.rec.action[2 * a + 1] = act[1];
    }
    okActAlive(p.f.st.crashed, p.rec.alive, a);
}

// ---- the push: section 17's kernels with a two-float action row -----------------------------------------------------------------------

struct OkDdpgReplayParams
{
    int               N, R;
    uint32_t          flags;
    uint64_t          capacity;
    okenv_ddpg_ring   ring;
    uint64_t         *pushed, *snapshot;
    uint32_t         *counts;
    okenv_ddpg_record rec;
    const float      *dist;
    const uint8_t    *crashed;
    const float      *reward; // or nullptr: 1.0f
};

__device__ __forceinline__ void okReplayStoreAction(const OkDdpgReplayParams &p, const long long slot, const long a)
{
    p.ring.action[2 * slot]     = p.rec.action[2 * a];
    p.ring.action[2 * slot + 1] = p.rec.action[2 * a + 1];
}

__device__ __forceinline__ float okReplayReward(const OkDdpgReplayParams &p, const int, const long a)
{
    return p.reward != nullptr ? p.reward[a] : 1.F;
}

// ---- the update -----------------------------------------------------------------------------------------------------------------

struct OkDdpgParams
{
    int                  R, H, Hc;
    int                  B, C;   // positions of a batch, its chunks
    int                  Pa, Pc; // parameters of the two networks
    uint64_t             capacity;
    const uint64_t      *pushed;
    okenv_ddpg_ring      ring;
    float               *actor, *critic, *actor_t, *critic_t;
    float               *act_m, *act_v, *cri_m, *cri_v;
    float               *part;   // [C][max(Pa, Pc) + 1]: one network's columns at a time, [parameters | loss term]
    float                scale[2], bias[2];
    float                gamma, tau, omt;
    uint32_t             seed, draw;
    ok_learn_adam_consts adam_actor, adam_critic;
    float               *critic_loss, *actor_loss; // this iteration's slots, or nullptr
    float               *grad_critic, *grad_actor;
    int32_t             *index;
};

// LDS floats: one network at a time, the chunk's input rows [state, a_0, a_1], hidden values and hidden seeds, output seeds, loss terms
__host__ __device__ inline int okDdpgNetFloats(const int R, const int H, const int Hc)
{
    const int a = okActorNetFloats(R, H, 2), b = okActorNetFloats(R + 2, Hc, 1);
    return a > b ? a : b;
}

inline size_t okDdpgLdsBytes(const int R, const int H, const int Hc)
{
    return sizeof(float) * static_cast<size_t>(okLearnPlaces(okDdpgNetFloats(R, H, Hc), R + 2, okLearnHiddenStride(H, Hc), 1).end);
}

// What both gradient kernels begin with: the chunk (its rows hold the critic's input [state, a_0, a_1]) and the group's ring draw
__device__ __forceinline__ OkLearnChunk okDdpgBegin(const OkDdpgParams &p, size_t *idx, int *live)
{
    const OkLearnChunk s = okLearnBegin(okDdpgNetFloats(p.R, p.H, p.Hc), p.R + 2, okLearnHiddenStride(p.H, p.Hc), 1, p.B);
    *idx                 = okReplayDraw(p, s.q, live);
    return s;
}

__global__ __launch_bounds__(kLearnThreads) void okDdpgCriticGradKernel(const OkDdpgParams p)
{
    const int          R = p.R, H = p.H, Hc = p.Hc, in = R + 2;
    size_t             idx;
    int                live;
    const OkLearnChunk s = okDdpgBegin(p, &idx, &live);
    const int          lane = s.lane;
    float             *x = s.x;
    // a' = the target actor's action on s'
    okActorStage(s.net, p.actor_t, R, H, p.Pa);
    okReplayGatherRow(x, p.ring.next_state, idx, R, lane, live);
    __syncthreads();
    float z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS], act[2], t[2];
    okActorForward(s.net, R, H, 2, x, lane, z);
    okDdpgGroupAction(z[0], z[1], p.scale, p.bias, lane, act, t);
    if (lane < 2)
        x[R + lane] = lane == 1 ? act[1] : act[0];
    __syncthreads(); // every group is done with the target actor: its place is free
    // q' = the target critic on [s', a'], to y
    okActorStage(s.net, p.critic_t, in, Hc, p.Pc);
    __syncthreads();
    okActorForward(s.net, in, Hc, 1, x, lane, z);
    const float y = ok_dqn_target(live ? p.ring.reward[idx] : 0.F, live ? p.ring.done[idx] : 0.F, p.gamma, z[0], OK_DQN_MASK_DONE);
    __syncthreads(); // every group has read its row and the target critic: both places are free
    // the online critic on [s, a], in the same rows
    okActorStage(s.net, p.critic, in, Hc, p.Pc);
    okReplayGatherRow(x, p.ring.state, idx, R, lane, live);
    if (lane < 2)
        x[R + lane] = live ? p.ring.action[2U * idx + static_cast<size_t>(lane)] : 0.F;
    __syncthreads();
    okActorForward(s.net, in, Hc, 1, x, lane, z);
    const float e = live ? z[0] - y : 0.F;
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        dz[k] = k == 0 ? e : 0.F;
    okLearnHidden(s.net, s.rp, in, Hc, 1, x, dz, lane, s.hs + s.g * s.hp, s.dss + s.g * s.hp);
    if (lane == 0)
    {
        s.dzs[s.g * OK_ACTOR_MAX_ACTIONS] = e;
        s.terms[s.g]                      = e * e;
        if (s.g < s.n && p.index != nullptr)
            p.index[s.q] = static_cast<int32_t>(idx);
    }
    __syncthreads();
    float *col = p.part + static_cast<size_t>(s.chunk) * static_cast<size_t>(p.Pc + 1);
    okLearnChunkSums(p.Pc, in, Hc, 1, s.xs, s.hs, s.dss, s.dzs, s.rp, s.hp, s.n, col);
    okLearnSumTerms(s.terms, s.n, col + p.Pc);
}

__global__ __launch_bounds__(kLearnThreads) void okDdpgActorGradKernel(const OkDdpgParams p)
{
    const int          R = p.R, H = p.H, Hc = p.Hc, in = R + 2;
    size_t             idx;
    int                live;
    const OkLearnChunk s = okDdpgBegin(p, &idx, &live);
    const int          lane = s.lane, rpa = okActorRowStride(R), rpc = s.rp;
    float             *x = s.x;
    // a = the online actor's action on s
    okActorStage(s.net, p.actor, R, H, p.Pa);
    okReplayGatherRow(x, p.ring.state, idx, R, lane, live);
    __syncthreads();
    float z[OK_ACTOR_MAX_ACTIONS], act[2], t[2];
    okActorForward(s.net, R, H, 2, x, lane, z);
    okDdpgGroupAction(z[0], z[1], p.scale, p.bias, lane, act, t);
    if (lane < 2)
        x[R + lane] = lane == 1 ? act[1] : act[0];
    __syncthreads(); // every group is done with the actor: its place is free
    // q and da through the stepped critic: lane l owns the hidden units l, l + 8, ..., which is the rule's partial j mod 8
    okActorStage(s.net, p.critic, in, Hc, p.Pc);
    __syncthreads();
    float pq, pda[2];
    ok_ddpg_critic_lane(s.net, rpc, s.net + Hc * rpc, s.net + Hc * rpc + Hc, in, Hc, x, lane, live ? 1.F : 0.F, &pq, pda);
    const float qv  = s.net[Hc * rpc + Hc + Hc] + okActorJoinLanes(pq);
    const float da0 = okActorJoinLanes(pda[0]), da1 = okActorJoinLanes(pda[1]);
    float       dz[OK_ACTOR_MAX_ACTIONS];
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        dz[k] = 0.F;
    dz[0] = ok_ddpg_seed(da0, p.scale[0], t[0]);
    dz[1] = ok_ddpg_seed(da1, p.scale[1], t[1]);
    __syncthreads(); // every group is done with the critic
    // the actor's backward
    okActorStage(s.net, p.actor, R, H, p.Pa);
    __syncthreads();
    okLearnHidden(s.net, rpa, R, H, 2, x, dz, lane, s.hs + s.g * s.hp, s.dss + s.g * s.hp);
    if (lane < 2)
        s.dzs[s.g * OK_ACTOR_MAX_ACTIONS + lane] = lane == 1 ? dz[1] : dz[0];
    if (lane == 0)
        s.terms[s.g] = live ? qv : 0.F;
    __syncthreads();
    float *col = p.part + static_cast<size_t>(s.chunk) * static_cast<size_t>(p.Pa + 1);
    okLearnChunkSums(p.Pa, R, H, 2, s.xs, s.hs, s.dss, s.dzs, s.rp, s.hp, s.n, col);
    okLearnSumTerms(s.terms, s.n, col + p.Pa);
}

// The step of one network (kActor: the actor's, else the critic's) and the soft update of its target in the thread that owns the
// parameter
template <bool kActor>
__global__ __launch_bounds__(kLearnStepCols *kLearnStepRows) void okDdpgStepKernel(const OkDdpgParams p)
{
    __shared__ float last[kLearnStepRows][kLearnStepCols];
    const int        P = kActor ? p.Pa : p.Pc;
    int              column = 0;
    float            sum    = 0.F;
    if (!okLearnColumnSum(p.part, P + 1, p.C, last, &column, &sum))
        return;
    const float count = static_cast<float>(p.B);
    if (column < P)
    {
        float *par = kActor ? p.actor : p.critic, *tgt = (kActor ? p.actor_t : p.critic_t) + column;
        okLearnStepParam(par, kActor ? p.act_m : p.cri_m, kActor ? p.act_v : p.cri_v, kActor ? p.grad_actor : p.grad_critic, column,
                         ok_ddpg_scale_grad(sum, count, kActor ? 1 : 0), kActor ? p.adam_actor : p.adam_critic);
        *tgt = ok_ddpg_soft(par[column], *tgt, p.tau, p.omt);
    }
    else
    {
        float *loss = kActor ? p.actor_loss : p.critic_loss;
        if (loss != nullptr)
            *loss = ok_ddpg_scale_loss(sum, count, kActor ? 1 : 0);
    }
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okDdpgCheckConfig(const okenv_ddpg_config *c, const int R)
{
    if (c == nullptr)
        return "config is NULL";
    if (R < 1 || R > OK_DDPG_MAX_RAYS)
        return "the fan needs 1 .. 62 rays";
    if (c->hidden < 1 || c->hidden > OK_ACTOR_MAX_HIDDEN || c->critic_hidden < 1 || c->critic_hidden > OK_ACTOR_MAX_HIDDEN)
        return "a hidden width outside 1 .. 256";
    if (!(c->gamma >= 0.F && c->gamma <= 1.F))
        return "gamma outside [0, 1]";
    if (!(c->tau >= 0.F && c->tau <= 1.F))
        return "tau outside [0, 1]";
    if (!(c->noise[0] >= 0.F) || !(c->noise[1] >= 0.F))
        return "negative noise";
    if (!(c->lr_actor > 0.F) || !(c->lr_actor < 3.0e38F) || !(c->lr_critic > 0.F) || !(c->lr_critic < 3.0e38F))
        return "a learning rate must be positive and finite";
    if (!(c->beta1 >= 0.F && c->beta1 < 1.F) || !(c->beta2 >= 0.F && c->beta2 < 1.F))
        return "a beta outside [0, 1)";
    if (!(c->eps > 0.F) || !(c->eps < 3.0e38F))
        return "eps must be positive and finite";
    return nullptr;
}

inline ok_learn_adam_consts okDdpgAdamConsts(const okenv_ddpg_config &c, const float lr, const int64_t t)
{
    const okenv_learner_params lp{lr, 0.F, c.beta1, c.beta2, c.eps};
    return okLearnAdamConsts(lp, t);
}

// The action of n agents on host arrays; every output may be nullptr
inline void okDdpgActHost(const okenv_ddpg_config &c, const float *actor, const int R, const int n, const float *dist, const uint8_t *crashed,
                          const uint32_t draw_index, float *throttle, float *steer, float *action, float *state, uint8_t *alive)
{
    std::vector<float> x(static_cast<size_t>(R));
    for (int a = 0; a < n; ++a)
    {
        for (int i = 0; i < R; ++i)
            x[static_cast<size_t>(i)] = dist[static_cast<size_t>(a) * R + i] / OK_SENSOR_RANGE;
        float z[OK_ACTOR_MAX_ACTIONS], act[2], t;
        okLearnHostForward(actor, R, c.hidden, 2, x.data(), z);
        act[0] = ok_ddpg_action(z[0], c.scale[0], c.bias[0], &t);
        act[1] = ok_ddpg_action(z[1], c.scale[1], c.bias[1], &t);
        if (c.noise[0] > 0.F || c.noise[1] > 0.F)
        {
            const ok_u32x4 r = ok_ddpg_draw(c.seed, c.agent_base + static_cast<uint32_t>(a), draw_index);
            act[0]           = ok_ddpg_explore(act[0], c.noise[0], r.v[0], c.scale[0], c.bias[0]);
            act[1]           = ok_ddpg_explore(act[1], c.noise[1], r.v[1], c.scale[1], c.bias[1]);
        }
        if (throttle != nullptr)
            throttle[a] = act[0];
        if (steer != nullptr)
            steer[a] = act[1];
        if (action != nullptr)
        {
            action[2 * static_cast<size_t>(a)]     = act[0];
            action[2 * static_cast<size_t>(a) + 1] = act[1];
        }
        if (state != nullptr)
            for (int i = 0; i < R; ++i)
                state[static_cast<size_t>(a) * R + i] = x[static_cast<size_t>(i)];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

// okReplayPushHost's two pieces (ok_dqn.h) for a ring whose action is two floats
inline void okReplayStoreActionHost(const okenv_ddpg_ring &ring, const size_t slot, const float *action, const size_t a)
{
    ring.action[2 * slot]     = action[2 * a];
    ring.action[2 * slot + 1] = action[2 * a + 1];
}

inline float okReplayRewardHost(const okenv_ddpg_ring &, const int, const float *, const int)
{
    return 1.F;
}

// The join, the scale, Adam and the soft update of one network on the host: okDdpgStepKernel
inline void okDdpgStepHost(std::vector<float> &part, const int P, const int C, const float count, const bool is_actor, float *par, float *m, float *v, float *tgt,
                           const ok_learn_adam_consts &adam, const float tau, const float omt, float *grad, float *loss)
{
    const int cols = P + 1;
    for (int column = 0; column < cols; ++column)
    {
        const float sum = ok_learn_tree(part.data() + column, cols, static_cast<uint32_t>(C));
        if (column < P)
        {
            okLearnStepParam(par, m, v, grad, column, ok_ddpg_scale_grad(sum, count, is_actor ? 1 : 0), adam);
            tgt[column] = ok_ddpg_soft(par[column], tgt[column], tau, omt);
        }
        else if (loss != nullptr)
            *loss = ok_ddpg_scale_loss(sum, count, is_actor ? 1 : 0);
    }
}

// The update on host arrays; every output may be nullptr
inline void okDdpgUpdateHost(const okenv_ddpg_config &cfg, const int R, okenv_ddpg_state &st, const okenv_ddpg_ring &ring, const uint32_t size, const int B,
                             const int iterations, const bool resample, const uint32_t draw_base, const okenv_ddpg_output &out)
{
    const int   H = cfg.hidden, Hc = cfg.critic_hidden, in = R + 2;
    const int   Pa = ok_actor_num_params(R, H, 2), Pc = ok_ddpg_critic_params(R, Hc), C = (B + OK_LEARN_CHUNK - 1) / OK_LEARN_CHUNK;
    const int   live = size != 0U;
    const float count = static_cast<float>(B), omt = 1.F - cfg.tau;
    const size_t hm = static_cast<size_t>(std::max(H, Hc));
    std::vector<float> part(static_cast<size_t>(C) * (static_cast<size_t>(std::max(Pa, Pc)) + 1U)), xs(static_cast<size_t>(OK_LEARN_CHUNK) * in), xn(static_cast<size_t>(in)),
        terms(OK_LEARN_CHUNK);
    OkLearnHostRows rows;
    rows.h.resize(OK_LEARN_CHUNK * hm);
    rows.ds.resize(OK_LEARN_CHUNK * hm);
    rows.dz.resize(static_cast<size_t>(OK_LEARN_CHUNK) * OK_ACTOR_MAX_ACTIONS);
    for (int it = 0; it < iterations; ++it)
    {
        const uint32_t draw = draw_base + (resample ? static_cast<uint32_t>(it) : 0U);
        st.t += 1;
        // 1, 2: the target and the critic
        for (int chunk = 0; chunk < C; ++chunk)
        {
            const int n   = std::min(OK_LEARN_CHUNK, B - chunk * OK_LEARN_CHUNK);
            float    *col = part.data() + static_cast<size_t>(chunk) * (Pc + 1);
            for (int s = 0; s < n; ++s)
            {
                const int    q   = chunk * OK_LEARN_CHUNK + s;
                const size_t idx = live ? ok_dqn_sample(cfg.sample_seed, static_cast<uint32_t>(q), draw, size) : 0U;
                float       *x   = xs.data() + static_cast<size_t>(s) * in;
                float        z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS] = {0.F}, t;
                for (int i = 0; i < R; ++i)
                {
                    xn[static_cast<size_t>(i)] = live ? ring.next_state[idx * R + i] : 0.F;
                    x[i]                       = live ? ring.state[idx * R + i] : 0.F;
                }
                okLearnHostForward(st.actor_target, R, H, 2, xn.data(), z);
                xn[static_cast<size_t>(R)]     = ok_ddpg_action(z[0], cfg.scale[0], cfg.bias[0], &t);
                xn[static_cast<size_t>(R) + 1] = ok_ddpg_action(z[1], cfg.scale[1], cfg.bias[1], &t);
                okLearnHostForward(st.critic_target, in, Hc, 1, xn.data(), z);
                const float y = ok_dqn_target(live ? ring.reward[idx] : 0.F, live ? ring.done[idx] : 0.F, cfg.gamma, z[0], OK_DQN_MASK_DONE);
                x[R]     = live ? ring.action[2 * idx] : 0.F;
                x[R + 1] = live ? ring.action[2 * idx + 1] : 0.F;
                okLearnHostForward(st.critic, in, Hc, 1, x, z);
                const float e = live ? z[0] - y : 0.F;
                dz[0]         = e;
                terms[static_cast<size_t>(s)] = e * e;
                okLearnHostHidden(st.critic, in, Hc, 1, x, dz, rows.h.data() + static_cast<size_t>(s) * Hc, rows.ds.data() + static_cast<size_t>(s) * Hc);
                for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
                    rows.dz[static_cast<size_t>(s) * OK_ACTOR_MAX_ACTIONS + a] = dz[a];
                if (out.index != nullptr)
                    out.index[q] = static_cast<int32_t>(idx);
            }
            okLearnHostChunkSums(Pc, in, Hc, 1, xs.data(), rows, n, col);
            col[Pc] = okLearnHostSumTerms(terms.data(), n);
        }
        okDdpgStepHost(part, Pc, C, count, false, st.critic, st.critic_m, st.critic_v, st.critic_target, okDdpgAdamConsts(cfg, cfg.lr_critic, st.t), cfg.tau, omt,
                       out.grad_critic, out.critic_loss != nullptr ? out.critic_loss + it : nullptr);
        // 3: the actor through the stepped critic.  (The state rows are kept R wide for the sums; the critic's row is built beside.)
        std::vector<float> xa(static_cast<size_t>(OK_LEARN_CHUNK) * R);
        for (int chunk = 0; chunk < C; ++chunk)
        {
            const int n   = std::min(OK_LEARN_CHUNK, B - chunk * OK_LEARN_CHUNK);
            float    *col = part.data() + static_cast<size_t>(chunk) * (Pa + 1);
            for (int s = 0; s < n; ++s)
            {
                const int    q   = chunk * OK_LEARN_CHUNK + s;
                const size_t idx = live ? ok_dqn_sample(cfg.sample_seed, static_cast<uint32_t>(q), draw, size) : 0U;
                float       *x   = xa.data() + static_cast<size_t>(s) * R;
                float        z[OK_ACTOR_MAX_ACTIONS], dz[OK_ACTOR_MAX_ACTIONS] = {0.F}, t[2], pq[OK_ACTOR_LANES], p0[OK_ACTOR_LANES], p1[OK_ACTOR_LANES];
                for (int i = 0; i < R; ++i)
                    xn[static_cast<size_t>(i)] = x[i] = live ? ring.state[idx * R + i] : 0.F;
                okLearnHostForward(st.actor, R, H, 2, x, z);
                xn[static_cast<size_t>(R)]     = ok_ddpg_action(z[0], cfg.scale[0], cfg.bias[0], &t[0]);
                xn[static_cast<size_t>(R) + 1] = ok_ddpg_action(z[1], cfg.scale[1], cfg.bias[1], &t[1]);
                const float *b1 = st.critic + Hc * in, *w2 = b1 + Hc;
                for (int l = 0; l < OK_ACTOR_LANES; ++l)
                {
                    float pda[2];
                    ok_ddpg_critic_lane(st.critic, in, b1, w2, in, Hc, xn.data(), l, live ? 1.F : 0.F, &pq[l], pda);
                    p0[l] = pda[0];
                    p1[l] = pda[1];
                }
                const float qv = ok_actor_join(pq, w2[Hc]);
                dz[0]          = ok_ddpg_seed(ok_ddpg_join(p0), cfg.scale[0], t[0]);
                dz[1]          = ok_ddpg_seed(ok_ddpg_join(p1), cfg.scale[1], t[1]);
                terms[static_cast<size_t>(s)] = live ? qv : 0.F;
                okLearnHostHidden(st.actor, R, H, 2, x, dz, rows.h.data() + static_cast<size_t>(s) * H, rows.ds.data() + static_cast<size_t>(s) * H);
                for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
                    rows.dz[static_cast<size_t>(s) * OK_ACTOR_MAX_ACTIONS + a] = dz[a];
            }
            okLearnHostChunkSums(Pa, R, H, 2, xa.data(), rows, n, col);
            col[Pa] = okLearnHostSumTerms(terms.data(), n);
        }
        okDdpgStepHost(part, Pa, C, count, true, st.actor, st.actor_m, st.actor_v, st.actor_target, okDdpgAdamConsts(cfg, cfg.lr_actor, st.t), cfg.tau, omt,
                       out.grad_actor, out.actor_loss != nullptr ? out.actor_loss + it : nullptr);
    }
}

#endif // OK_DDPG_H
