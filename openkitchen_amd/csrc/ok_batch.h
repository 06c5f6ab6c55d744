// ok_batch.h -- from a recorded episode to the learner's batch: the data side of the reference's updatePolicy
// (RLRacers/PPO/ExperienceBuffer.hpp:15-68, ReinforceAgent.hpp:94-106, GCLAgent.hpp:75-84,137-148) for T rows of N agents.  The rule
// lives in include/okenv_batch.h (ok_batch_walk_row, ok_batch_tree, ok_batch_finish, ok_batch_normalize) and is shared with
// okBatchPrepareHost below, so the device and the host entry agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site: they read a record the caller owns and write the caller's batch.
// Five launches on the handle's stream:
//   okBatchWalkKernel    one lane per agent column, t = T-1 .. 0: G and A planes, the fp64 column partials
//   okBatchTreeKernel    one workgroup: the fixed tree over the agent index, then mean and std
//   okBatchCountKernel   alive samples per group of 16 wave-wide chunks of a row (popcount of ballots)
//   okBatchScanKernel    one workgroup: exclusive scan over the groups in step-major order, and M
//   okBatchGatherKernel  every alive sample to its dense slot (ballot prefix inside a chunk), normalised on the way
// No atomics anywhere: the sample order is a pure function of `alive`, the sums' order is the rule's.
#ifndef OK_BATCH_H
#define OK_BATCH_H

#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_batch.h"

// What the kernels need, by value
struct OkBatchParams
{
    int                T, N, R, W;   // W: 64-agent chunks per row
    long               rs, fs;       // record / field row strides in agent slots
    long               L, groups;    // T * W chunks, ceil(L / 16) groups
    float              gamma, gl;
    uint32_t           normalize;
    okenv_batch_input  in;
    okenv_batch_output out;
    float             *g_plane, *a_plane; // dense [T][N]: the caller's planes, or the handle's scratch
    double            *part;              // [4][N]: column partials s_g, q_g, s_a, q_a
    uint32_t          *part_m;            // [N]
    uint32_t          *group;             // [groups]: counts, then exclusive offsets
    okenv_batch_stats *stats;             // the handle's copy (the gather reads it)
    int32_t           *count;             // the handle's copy of M
};

constexpr int kBatchWave        = 64;
constexpr int kBatchUnroll      = 8;    // rows per batch of the walk; two batches are in flight
constexpr int kBatchWalkThreads = 64;   // default workgroup of the walk: 4096 agents are 64 waves, one per CU
constexpr int kBatchGroupChunks = 16;   // chunks per workgroup of the count and gather kernels
constexpr int kBatchWideThreads = kBatchGroupChunks * kBatchWave;

template <bool HAS_VALUE>
struct OkBatchRows
{
    float   r[kBatchUnroll], v[kBatchUnroll];
    uint8_t a[kBatchUnroll];
};

// rows t, t-1, .. t-U+1 of column i: all loads issued before any is consumed
template <bool HAS_VALUE>
__device__ __forceinline__ void okBatchLoadRows(OkBatchRows<HAS_VALUE> &b, const float *__restrict__ rew, const uint8_t *__restrict__ alv,
                                                const float *__restrict__ val, const long t, const long rs)
{
#pragma unroll
    for (int k = 0; k < kBatchUnroll; ++k)
    {
        const long o = (t - k) * rs;
        b.r[k]       = rew[o];
        b.a[k]       = alv[o];
        b.v[k]       = HAS_VALUE ? val[o] : 0.F;
    }
}

// The column walk.  The chain per row is two dependent fp32 operations (four with the advantage) that must not be reassociated, so
// the kernel is parallel over agents only and bound by latency, not bandwidth; its loads do not depend on the chain, so while one
// batch of rows is consumed the next one is already on its way.  Consecutive lanes hold consecutive agents: every access is coalesced.
template <bool HAS_VALUE>
__global__ __launch_bounds__(1024) void okBatchWalkKernel(const OkBatchParams p)
{
    const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= p.N)
        return;
    const float *__restrict__ rew   = p.in.reward + i;
    const uint8_t *__restrict__ alv = p.in.alive + i;
    const float *__restrict__ val   = HAS_VALUE ? p.in.value + i : nullptr;
    float *__restrict__ gp          = p.g_plane + i;
    float *__restrict__ ap          = HAS_VALUE ? p.a_plane + i : nullptr;
    const long  rs = p.rs, N = p.N;
    const float gamma = p.gamma, gl = p.gl;
    ok_batch_walk w;
    ok_batch_walk_init(&w, (HAS_VALUE && p.in.last_value != nullptr) ? p.in.last_value[i] : 0.F);
    long t = static_cast<long>(p.T) - 1;
    for (int k = p.T % kBatchUnroll; k > 0; --k, --t)
    { // the newest T mod U rows one by one: what is left is whole batches
        float g, a;
        ok_batch_walk_row(&w, alv[t * rs] != 0, rew[t * rs], HAS_VALUE ? val[t * rs] : 0.F, HAS_VALUE, gamma, gl, &g, &a);
        gp[t * N] = g;
        if (HAS_VALUE)
            ap[t * N] = a;
    }
    OkBatchRows<HAS_VALUE> cur, nxt;
    if (t >= 0)
        okBatchLoadRows<HAS_VALUE>(cur, rew, alv, val, t, rs);
    while (t >= 0)
    {
        const long tn = t - kBatchUnroll;
        if (tn >= 0)
            okBatchLoadRows<HAS_VALUE>(nxt, rew, alv, val, tn, rs);
#pragma unroll
        for (int k = 0; k < kBatchUnroll; ++k)
        {
            float g, a;
            ok_batch_walk_row(&w, cur.a[k] != 0, cur.r[k], cur.v[k], HAS_VALUE, gamma, gl, &g, &a);
            gp[(t - k) * N] = g;
            if (HAS_VALUE)
                ap[(t - k) * N] = a;
        }
        if (tn >= 0)
            cur = nxt;
        t = tn;
    }
    p.part[i]         = w.s_g;
    p.part[N + i]     = w.q_g;
    p.part[2 * N + i] = w.s_a;
    p.part[3 * N + i] = w.q_a;
    p.part_m[i]       = w.m;
}

// ok_batch_tree over the column partials, level by level in one workgroup, then ok_batch_finish
__global__ __launch_bounds__(1024) void okBatchTreeKernel(const OkBatchParams p)
{
    const uint32_t n = static_cast<uint32_t>(p.N);
    for (uint32_t h = ok_batch_tree_width(n) >> 1; h >= 1U; h >>= 1)
    {
        for (uint32_t i = threadIdx.x; i < h; i += blockDim.x)
            if (i + h < n)
            {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    p.part[static_cast<size_t>(q) * n + i] = p.part[static_cast<size_t>(q) * n + i] + p.part[static_cast<size_t>(q) * n + i + h];
                p.part_m[i] += p.part_m[i + h];
            }
        __syncthreads();
    }
    if (threadIdx.x != 0)
        return;
    okenv_batch_stats s;
    s.sum_ret   = p.part[0];
    s.sumsq_ret = p.part[n];
    s.sum_adv   = p.part[2 * static_cast<size_t>(n)];
    s.sumsq_adv = p.part[3 * static_cast<size_t>(n)];
    s.count     = static_cast<int32_t>(p.part_m[0]);
    s.reserved  = 0;
    ok_batch_finish(p.part_m[0], s.sum_ret, s.sumsq_ret, &s.mean_ret, &s.std_ret);
    ok_batch_finish(p.in.value != nullptr ? p.part_m[0] : 0U, s.sum_adv, s.sumsq_adv, &s.mean_adv, &s.std_adv);
    *p.stats = s;
    if (p.out.stats != nullptr)
        *p.out.stats = s;
}

// One wave per chunk of 64 consecutive agents of one row; chunks are numbered step-major.
__device__ __forceinline__ bool okBatchChunkAlive(const OkBatchParams &p, const long chunk, const int lane, long *t_out, int *i_out)
{
    if (chunk >= p.L)
        return false;
    const long t = chunk / p.W;
    const int  i = static_cast<int>(chunk - t * p.W) * kBatchWave + lane;
    *t_out       = t;
    *i_out       = i;
    return i < p.N && p.in.alive[t * p.rs + i] != 0;
}

__global__ __launch_bounds__(kBatchWideThreads) void okBatchCountKernel(const OkBatchParams p)
{
    __shared__ uint32_t wave_count[kBatchGroupChunks];
    const int           wv = static_cast<int>(threadIdx.x) / kBatchWave, lane = static_cast<int>(threadIdx.x) % kBatchWave;
    long                t = 0;
    int                 i = 0;
    const bool          alive = okBatchChunkAlive(p, static_cast<long>(blockIdx.x) * kBatchGroupChunks + wv, lane, &t, &i);
    const unsigned long long b = __ballot(alive);
    if (lane == 0)
        wave_count[wv] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < kBatchGroupChunks; ++k)
            s += wave_count[k];
        p.group[blockIdx.x] = s;
    }
}

// Exclusive scan of the group counts in place (integers: the grouping cannot change the result), and M
__global__ __launch_bounds__(1024) void okBatchScanKernel(const OkBatchParams p)
{
    __shared__ uint32_t s[1024];
    const int  tid = static_cast<int>(threadIdx.x);
    const long per = (p.groups + 1023) / 1024, lo = tid * per, hi = lo + per < p.groups ? lo + per : p.groups;
    uint32_t   sum = 0;
    for (long j = lo; j < hi; ++j)
        sum += p.group[j];
    s[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1)
    {
        const uint32_t v = tid >= d ? s[tid - d] : 0U;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    uint32_t run = s[tid] - sum;
    for (long j = lo; j < hi; ++j)
    {
        const uint32_t c = p.group[j];
        p.group[j]       = run;
        run += c;
    }
    if (tid == 1023)
    {
        *p.count = static_cast<int32_t>(s[1023]);
        if (p.out.count != nullptr)
            *p.out.count = static_cast<int32_t>(s[1023]);
    }
}

// Every alive sample to slot k = group offset + alive samples of the group's earlier chunks + ballot prefix inside the chunk.  The
// state rows move with the group-copy pattern of ok_actor.h: the chunk's alive rows land in one contiguous piece of the output, and
// consecutive lanes write consecutive floats of it.
__global__ __launch_bounds__(kBatchWideThreads) void okBatchGatherKernel(const OkBatchParams p)
{
    __shared__ uint32_t wave_count[kBatchGroupChunks];
    __shared__ int      agent_of[kBatchGroupChunks][kBatchWave];
    const int           wv = static_cast<int>(threadIdx.x) / kBatchWave, lane = static_cast<int>(threadIdx.x) % kBatchWave;
    long                t = 0;
    int                 i = 0;
    const bool          alive = okBatchChunkAlive(p, static_cast<long>(blockIdx.x) * kBatchGroupChunks + wv, lane, &t, &i);
    const unsigned long long b = __ballot(alive);
    const int cnt = __popcll(b), pre = __popcll(b & ((1ULL << lane) - 1ULL));
    if (lane == 0)
        wave_count[wv] = static_cast<uint32_t>(cnt);
    if (alive)
        agent_of[wv][pre] = i;
    __syncthreads();
    size_t base = p.group[blockIdx.x];
    for (int k = 0; k < wv; ++k)
        base += wave_count[k];
    if (alive)
    {
        const size_t k = base + static_cast<size_t>(pre);
        const long   src = t * p.fs + i, flat = t * p.N + i;
        if (p.out.index != nullptr)
            p.out.index[k] = static_cast<int32_t>(flat);
        if (p.out.action != nullptr)
            p.out.action[k] = p.in.action[src];
        if (p.out.prob != nullptr)
            p.out.prob[k] = p.in.prob[src];
        if (p.out.ret != nullptr)
        {
            const float g = p.g_plane[flat];
            p.out.ret[k]  = (p.normalize & OKENV_BATCH_NORMALIZE_RETURN) != 0U ? ok_batch_normalize(g, p.stats->mean_ret, p.stats->std_ret) : g;
        }
        if (p.out.adv != nullptr)
        {
            const float a = p.a_plane[flat];
            p.out.adv[k]  = (p.normalize & OKENV_BATCH_NORMALIZE_ADVANTAGE) != 0U ? ok_batch_normalize(a, p.stats->mean_adv, p.stats->std_adv) : a;
        }
    }
    if (p.out.state != nullptr)
    {
        const int    R   = p.R;
        float       *dst = p.out.state + base * static_cast<size_t>(R);
        const float *row = p.in.state + static_cast<size_t>(t * p.fs) * static_cast<size_t>(R);
        for (int e = lane; e < cnt * R; e += kBatchWave)
        {
            const int s = e / R, r = e - s * R;
            dst[e]      = row[static_cast<size_t>(agent_of[wv][s]) * static_cast<size_t>(R) + r];
        }
    }
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

// nullptr, or what is wrong with the arguments
inline const char *okBatchCheck(const okenv_batch_params *bp, const okenv_batch_input *in, const okenv_batch_output *out)
{
    if (bp == nullptr || in == nullptr || out == nullptr)
        return "params, input or output is NULL";
    if (bp->num_steps < 1 || bp->num_agents < 1)
        return "T and N must be at least 1";
    if (static_cast<int64_t>(bp->num_steps) * bp->num_agents >= (INT64_C(1) << 31))
        return "T * N must stay below 2^31";
    if (in->reward == nullptr || in->alive == nullptr)
        return "reward and alive are required";
    if (!(bp->gamma >= 0.F && bp->gamma <= 1.F))
        return "gamma outside [0, 1]";
    if (!(bp->lambda >= 0.F && bp->lambda <= 1.F))
        return "lambda outside [0, 1]";
    if ((bp->record_stride != 0 && bp->record_stride < bp->num_agents) || (bp->field_stride != 0 && bp->field_stride < bp->num_agents))
        return "a row stride is smaller than a row";
    if ((bp->normalize & ~(OKENV_BATCH_NORMALIZE_RETURN | OKENV_BATCH_NORMALIZE_ADVANTAGE)) != 0U)
        return "unknown normalize bits";
    const int bt = bp->block_threads;
    if (bt != 0 && bt != 64 && bt != 128 && bt != 256 && bt != 512 && bt != 1024)
        return "block_threads must be 0, 64, 128, 256, 512 or 1024";
    if (in->value == nullptr && (out->adv != nullptr || out->adv_plane != nullptr))
        return "advantages need the value plane";
    if (in->value == nullptr && in->last_value != nullptr)
        return "last_value without the value plane";
    if ((out->state != nullptr && in->state == nullptr) || (out->action != nullptr && in->action == nullptr) || (out->prob != nullptr && in->prob == nullptr))
        return "an output field is requested whose input is NULL";
    if (out->state != nullptr && bp->state_width < 1)
        return "state_width must be at least 1 when state is gathered";
    return nullptr;
}

// The rule on host arrays; every output may be nullptr.  Returns M.
inline int32_t okBatchPrepareHost(const okenv_batch_params &bp, const okenv_batch_input &in, const okenv_batch_output &out)
{
    const size_t T = static_cast<size_t>(bp.num_steps), N = static_cast<size_t>(bp.num_agents), R = static_cast<size_t>(bp.state_width > 0 ? bp.state_width : 0);
    const size_t rs = bp.record_stride != 0 ? static_cast<size_t>(bp.record_stride) : N, fs = bp.field_stride != 0 ? static_cast<size_t>(bp.field_stride) : N;
    const bool   has_value = in.value != nullptr;
    const float  gl = static_cast<float>(static_cast<double>(bp.gamma) * static_cast<double>(bp.lambda));
    std::vector<float>  g_own(out.ret_plane == nullptr ? T * N : 0U), a_own((has_value && out.adv_plane == nullptr) ? T * N : 0U);
    float              *gp = out.ret_plane != nullptr ? out.ret_plane : g_own.data();
    float              *ap = !has_value ? nullptr : (out.adv_plane != nullptr ? out.adv_plane : a_own.data());
    std::vector<double> part(4U * N);
    uint32_t            m = 0;
    for (size_t i = 0; i < N; ++i)
    {
        ok_batch_walk w;
        ok_batch_walk_init(&w, (has_value && in.last_value != nullptr) ? in.last_value[i] : 0.F);
        for (size_t t = T; t-- > 0;)
        {
            float g, a;
            ok_batch_walk_row(&w, in.alive[t * rs + i] != 0, in.reward[t * rs + i], has_value ? in.value[t * rs + i] : 0.F, has_value ? 1 : 0, bp.gamma,
                              gl, &g, &a);
            gp[t * N + i] = g;
            if (has_value)
                ap[t * N + i] = a;
        }
        part[i]         = w.s_g;
        part[N + i]     = w.q_g;
        part[2 * N + i] = w.s_a;
        part[3 * N + i] = w.q_a;
        m += w.m;
    }
    okenv_batch_stats s;
    s.sum_ret   = ok_batch_tree(part.data(), static_cast<uint32_t>(N));
    s.sumsq_ret = ok_batch_tree(part.data() + N, static_cast<uint32_t>(N));
    s.sum_adv   = ok_batch_tree(part.data() + 2 * N, static_cast<uint32_t>(N));
    s.sumsq_adv = ok_batch_tree(part.data() + 3 * N, static_cast<uint32_t>(N));
    s.count     = static_cast<int32_t>(m);
    s.reserved  = 0;
    ok_batch_finish(m, s.sum_ret, s.sumsq_ret, &s.mean_ret, &s.std_ret);
    ok_batch_finish(has_value ? m : 0U, s.sum_adv, s.sumsq_adv, &s.mean_adv, &s.std_adv);
    if (out.stats != nullptr)
        *out.stats = s;
    if (out.count != nullptr)
        *out.count = s.count;
    size_t k = 0;
    for (size_t t = 0; t < T; ++t)
        for (size_t i = 0; i < N; ++i)
        {
            if (in.alive[t * rs + i] == 0)
                continue;
            const size_t src = t * fs + i, flat = t * N + i;
            if (out.index != nullptr)
                out.index[k] = static_cast<int32_t>(flat);
            if (out.action != nullptr)
                out.action[k] = in.action[src];
            if (out.prob != nullptr)
                out.prob[k] = in.prob[src];
            if (out.ret != nullptr)
                out.ret[k] = (bp.normalize & OKENV_BATCH_NORMALIZE_RETURN) != 0U ? ok_batch_normalize(gp[flat], s.mean_ret, s.std_ret) : gp[flat];
            if (out.adv != nullptr)
                out.adv[k] = (bp.normalize & OKENV_BATCH_NORMALIZE_ADVANTAGE) != 0U ? ok_batch_normalize(ap[flat], s.mean_adv, s.std_adv) : ap[flat];
            if (out.state != nullptr)
                for (size_t r = 0; r < R; ++r)
                    out.state[k * R + r] = in.state[src * R + r];
            ++k;
        }
    return s.count;
}

#endif // OK_BATCH_H
