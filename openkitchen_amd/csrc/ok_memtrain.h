// ok_memtrain.h -- the training of the world-model racers' memory on the device: train_rnn.py's recipe for the
// GRUDynamics network, backpropagation through time included.  The rule lives in include/okenv_memtrain.h and is shared with
// okMemTrainUpdateHost below, so the device and the host entries agree bit for bit.
//
// Every contraction of the rule is one primitive, the blocked chain, and one kernel runs it on v_mfma_f32_16x16x4_f32:
//   okMemTrainGemmKernel     C[m][n] = bias[n] continued, per block of 64 k's, by the block's product A[m][k] B[k][n] accumulated from a
//                            zero C and added on.  A, B and C are given with strides, so the same kernel takes x Wih^T and h Whh^T of
//                            the forward, head.w^T dzn, Wih^T dgi and Whh^T dgh of the backward (torch's [3H][in] layout is the B
//                            operand of the transposed product as it lies) and the parameter sums over positions (k = the positions,
//                            A = the delta rows read down their columns, B = the saved inputs with a 1.0f column behind them for the
//                            bias).  A wave owns a 16 x 16 tile and reads its operands straight from global memory, as
//                            okVitHeadGradKernel does: no LDS, no barrier.  A launch takes a list of jobs (blockIdx.y): ONE launch
//                            covers the [W | b] tiles of all 2 L + 1 matrices and the loss column.
// Around it, a thread per element, the arithmetic of the rule in registers:
//   okMemTrainGatherKernel   the windows' rows -> the normalised inputs x0 [P][Z + 2] and targets y [P][Z], positions step-major
//   okMemTrainGateKernel     one step of one layer behind its two products: r, u, n, gh_n and h' to the workspace
//   okMemTrainSeedKernel     e, t and dzn of every position
//   okMemTrainCellKernel     one step of one layer backwards: dh' = (down + keep) + back, the delta rows dgi and dgh, the new keep
//   okMemTrainLossKernel, okMemTrainSquareKernel, okMemTrainSumKernel (a launch per level), okMemTrainTickKernel (the step number and
//   Adam's factors, on the device so that a captured update replays with its own step numbers), okMemTrainStepKernel (clip and AdamW in
//   place in the handle's network vector).
// The forward goes layer by layer: a layer's input products x Wih^T do not depend on the recurrence and are ONE launch over all S
// steps; behind it S times (h Whh^T, gates).  The backward goes top layer first, and in a layer from step S - 1 down to 0: (cell,
// Whh^T dgh) per step, then Wih^T dgi for all steps at once as the layer below's `down`.  Nothing waits on another workgroup inside a
// launch; what crosses workgroups crosses a launch boundary.  No atomics.  An update enqueues only: no synchronisation, no allocation.
#ifndef OK_MEMTRAIN_H
#define OK_MEMTRAIN_H

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_memtrain.h"
#include "ok_learn.h"
#include "ok_memory.h"

constexpr int kMemTrainWaves   = 4; // tiles of a workgroup of the product kernel, a wave each
constexpr int kMemTrainThreads = 64 * kMemTrainWaves;
constexpr int kMemTrainJobs    = 2 * OK_MEMORY_MAX_LAYERS + 2; // the matrices' parameter sums and the loss column

// The learner's workspace in floats, for windows of S steps and minibatches of up to B windows (P = B S positions).  A layer's hidden
// states lie behind B rows of zeros that nothing writes: the rows of a minibatch of Bk windows begin at row B - Bk, so that row p from
// there is h_prev of position p and row Bk + p its h'.
struct OkMemTrainPlaces
{
    size_t m, v, grad, sum_a, sum_b, x0, y, zn, tt, gi, gh, down, keep, back, lossj, scalars;
    size_t r[OK_MEMORY_MAX_LAYERS], u[OK_MEMORY_MAX_LAYERS], n[OK_MEMORY_MAX_LAYERS], ghn[OK_MEMORY_MAX_LAYERS], h[OK_MEMORY_MAX_LAYERS];
    size_t dgi[OK_MEMORY_MAX_LAYERS], dgh[OK_MEMORY_MAX_LAYERS];
    size_t words;
};

// scalars: [0] the sum of squares is wherever the last level leaves it; these are the fixed ones, in 4-byte words from `scalars`
constexpr int kMemTrainStepAt   = 0; // int64: the step number t (two words, 8-byte aligned)
constexpr int kMemTrainConstsAt = 2; // ok_learn_adam_consts of the step in flight (7 floats)
constexpr int kMemTrainLossAt   = 10;
constexpr int kMemTrainScalars  = 16;

__host__ __device__ inline OkMemTrainPlaces okMemTrainPlaces(const ok_memory_shape s, const int S, const int B)
{
    OkMemTrainPlaces at;
    const size_t     T = static_cast<size_t>(ok_memtrain_trainable(s)), P = static_cast<size_t>(B) * S, H = static_cast<size_t>(s.H), Z = static_cast<size_t>(s.Z);
    size_t           w = 0;
    const auto take = [&w](const size_t n) {
        const size_t here = w;
        w += (n + 3U) & ~static_cast<size_t>(3U);
        return here;
    };
    at.scalars = take(kMemTrainScalars);
    at.m       = take(T);
    at.v       = take(T);
    at.grad    = take(T);
    at.sum_a   = take((T + OK_MEMTRAIN_BLOCK - 1) / OK_MEMTRAIN_BLOCK);
    at.sum_b   = take((T + OK_MEMTRAIN_BLOCK * OK_MEMTRAIN_BLOCK - 1) / (OK_MEMTRAIN_BLOCK * OK_MEMTRAIN_BLOCK));
    at.x0      = take(P * (Z + OK_MEMORY_ACTIONS));
    at.y       = take(P * Z);
    at.zn      = take(P * Z);
    at.tt      = take(P * Z);
    at.gi      = take(P * 3U * H);
    at.gh      = take(static_cast<size_t>(B) * 3U * H);
    at.down    = take(P * H);
    at.keep    = take(static_cast<size_t>(B) * H);
    at.back    = take(static_cast<size_t>(B) * H);
    at.lossj   = take(Z);
    for (int l = 0; l < OK_MEMORY_MAX_LAYERS; ++l)
    {
        const size_t live = l < s.L ? 1U : 0U;
        at.r[l]   = take(live * P * H);
        at.u[l]   = take(live * P * H);
        at.n[l]   = take(live * P * H);
        at.ghn[l] = take(live * P * H);
        at.h[l]   = take(live * (static_cast<size_t>(B) + P) * H);
        at.dgi[l] = take(live * P * 3U * H);
        at.dgh[l] = take(live * P * 3U * H);
    }
    at.words = w;
    return at;
}

// The kernels keep everything in registers and global memory.  (A product kernel that staged 64 x 32 tiles of a K block in LDS, the
// layer kernel's way, gave the same bits and was measured 1.7 x SLOWER per minibatch at the reference shape, 4.85 against 2.87 ms: the
// recurrence's products have 256 rows, and its 64 .. 96 workgroups left most of the device idle.  docs/HISTORY.md section 51.)
inline size_t okMemTrainLdsBytes(const ok_memory_shape s)
{
    (void)s;
    return 0U;
}

// ---- the product kernel -----------------------------------------------------------------------------------------------------------------

struct OkMemTrainGemm
{
    const float *a; // A[m][k] at a + m * a_rs + k * a_cs
    long         a_rs, a_cs;
    const float *b; // B[k][n] at b + k * b_rs + n * b_cs
    long         b_rs, b_cs;
    const float *bias;   // [N], or nullptr: +0.0f
    float       *c;      // C[m][n] at c + m * c_rs + n
    long         c_rs;
    float       *c_ones; // [M]: the results of a column of 1.0f behind B's N columns, or nullptr: there is none
    int          M, N, K;
    float        div; // every result is divided by it; 0: no division
};

struct OkMemTrainGemmJobs
{
    int            count;
    OkMemTrainGemm job[kMemTrainJobs];
};

__host__ __device__ inline int okMemTrainTiles(const OkMemTrainGemm &j)
{
    const int cols = j.N + (j.c_ones != nullptr ? 1 : 0);
    return ((j.M + 15) / 16) * ((cols + 15) / 16);
}

// Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; accumulator register r is C[row 4 (l >> 4) + r][col l & 15]
// (ok_lidar.h).  A K block runs ceil(kc / 4) steps; the k's of the last step beyond K are the rule's zero terms.  Every address is
// formed only where its row, column and k are inside the job's M, N and K.  Grid (tiles of the largest job / 4, jobs).
__global__ __launch_bounds__(kMemTrainThreads) void okMemTrainGemmKernel(const OkMemTrainGemmJobs js)
{
    const OkMemTrainGemm &j = js.job[blockIdx.y];
    const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int cols = j.N + (j.c_ones != nullptr ? 1 : 0), cts = (cols + 15) / 16, tile = static_cast<int>(blockIdx.x) * kMemTrainWaves + wave;
    if (tile >= ((j.M + 15) / 16) * cts)
        return; // (the whole wave)
    const int    rt = tile / cts, ct = tile - rt * cts, row_a = 16 * rt + i, col_b = 16 * ct + i;
    const bool   a_live = row_a < j.M, b_live = col_b < j.N;
    const float  b_fill = (col_b == j.N && j.c_ones != nullptr) ? 1.F : 0.F;
    const float *ap = j.a + (a_live ? static_cast<long>(row_a) * j.a_rs : 0L), *bp = j.b + (b_live ? static_cast<long>(col_b) * j.b_cs : 0L);
    const float  start = (j.bias != nullptr && b_live) ? j.bias[col_b] : 0.F;
    okLidarAcc   acc = {start, start, start, start};
    for (int k0 = 0; k0 < j.K; k0 += OK_MEMTRAIN_BLOCK)
    {
        const int steps = okLidarMin(OK_MEMTRAIN_BLOCK / 4, (j.K - k0 + 3) / 4);
        float     a[OK_MEMTRAIN_BLOCK / 4], b[OK_MEMTRAIN_BLOCK / 4];
#pragma unroll
        for (int s = 0; s < OK_MEMTRAIN_BLOCK / 4; ++s)
        {
            const int  k = k0 + 4 * s + g;
            const bool k_live = k < j.K;
            a[s] = (a_live && k_live) ? ap[static_cast<long>(k) * j.a_cs] : 0.F;
            b[s] = k_live ? (b_live ? bp[static_cast<long>(k) * j.b_rs] : b_fill) : 0.F;
        }
        okLidarAcc part = {0.F, 0.F, 0.F, 0.F};
#pragma unroll
        for (int s = 0; s < OK_MEMTRAIN_BLOCK / 4; ++s)
        {
            if (s < steps) // (wave-uniform)
                part = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], part, 0, 0, 0);
        }
        acc = acc + part; // the rule's acc = acc + part: one rounded addition per element
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
    {
        const int row = 16 * rt + 4 * g + r;
        if (row >= j.M)
            continue;
        const float v = j.div != 0.F ? acc[r] / j.div : acc[r];
        if (b_live)
            j.c[static_cast<long>(row) * j.c_rs + col_b] = v;
        else if (b_fill != 0.F)
            j.c_ones[row] = v;
    }
}

// ---- the element kernels ----------------------------------------------------------------------------------------------------------------

struct OkMemTrainGatherJob
{
    const float *latent, *action, *net;
    const int   *start, *order; // order: the epoch's row, or nullptr
    float       *x0, *y;
    long         base;
    int          rows, M, stride, Bk, S, Z;
    ok_memory_layout at;
};

// A thread per (position, column of [x0 | y])
__global__ __launch_bounds__(256) void okMemTrainGatherKernel(const OkMemTrainGatherJob j)
{
    const int  Z = j.Z, wide = 2 * Z + OK_MEMORY_ACTIONS;
    const long t = static_cast<long>(blockIdx.x) * 256 + static_cast<long>(threadIdx.x);
    const long p = t / wide;
    const int  c = static_cast<int>(t - p * wide);
    if (p >= static_cast<long>(j.Bk) * j.S)
        return;
    const int s = static_cast<int>(p / j.Bk), q = static_cast<int>(p - static_cast<long>(s) * j.Bk);
    const int first = j.start[ok_memtrain_window(j.order, j.base, q, j.M)];
    if (c < Z)
        j.x0[p * (Z + OK_MEMORY_ACTIONS) + c] =
            ok_memory_normalise(j.latent[static_cast<long>(ok_memtrain_row(first, s, j.stride, j.rows)) * Z + c], j.net[j.at.z_mean + c], j.net[j.at.z_std + c]);
    else if (c < Z + OK_MEMORY_ACTIONS)
    {
        const int k = c - Z;
        j.x0[p * (Z + OK_MEMORY_ACTIONS) + c] = ok_memory_normalise(j.action[static_cast<long>(ok_memtrain_row(first, s, j.stride, j.rows)) * OK_MEMORY_ACTIONS + k],
                                                                    j.net[j.at.a_mean + k], j.net[j.at.a_std + k]);
    }
    else
    {
        const int k = c - Z - OK_MEMORY_ACTIONS;
        j.y[p * Z + k] = ok_memory_normalise(j.latent[static_cast<long>(ok_memtrain_row(first, s + 1, j.stride, j.rows)) * Z + k], j.net[j.at.z_mean + k],
                                             j.net[j.at.z_std + k]);
    }
}

struct OkMemTrainGateJob
{
    const float *gi, *gh;    // the step's rows: [Bk][3H] each
    const float *xa, *tail;  // layer 0: the step's x0 rows and Wih [3H][Z + 2] as set, for the two action columns; otherwise nullptr
    const float *h_prev;     // [Bk][H]
    float       *h, *r, *u, *n, *ghn; // the step's rows [Bk][H]
    int          Bk, H, Z;
};

__global__ __launch_bounds__(256) void okMemTrainGateKernel(const OkMemTrainGateJob j)
{
    const long t = static_cast<long>(blockIdx.x) * 256 + static_cast<long>(threadIdx.x);
    const int  H = j.H;
    const long q = t / H;
    const int  unit = static_cast<int>(t - q * H);
    if (q >= j.Bk)
        return;
    float s[3], hh[3];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
    {
        s[gate]  = j.gi[q * 3 * H + gate * H + unit];
        hh[gate] = j.gh[q * 3 * H + gate * H + unit];
        if (j.tail != nullptr)
            s[gate] = s[gate] + ok_memory_action_part(j.xa + q * (j.Z + OK_MEMORY_ACTIONS) + j.Z,
                                                      j.tail + static_cast<long>(gate * H + unit) * (j.Z + OK_MEMORY_ACTIONS) + j.Z);
    }
    float r, u, n;
    j.h[q * H + unit]   = ok_memtrain_cell(s[0], s[1], s[2], hh[0], hh[1], hh[2], j.h_prev[q * H + unit], &r, &u, &n);
    j.r[q * H + unit]   = r;
    j.u[q * H + unit]   = u;
    j.n[q * H + unit]   = n;
    j.ghn[q * H + unit] = hh[2];
}

// zn [count] in place -> dzn; tt [count]: the terms
__global__ __launch_bounds__(256) void okMemTrainSeedKernel(float *zn, const float *y, float *tt, const long count)
{
    const long e = static_cast<long>(blockIdx.x) * 256 + static_cast<long>(threadIdx.x);
    if (e >= count)
        return;
    float t, d;
    ok_memtrain_seed(zn[e], y[e], &t, &d);
    tt[e] = t;
    zn[e] = d;
}

struct OkMemTrainCellJob
{
    const float *down;                     // the step's rows [Bk][H]
    const float *back;                     // [Bk][H]: Whh^T dgh of step s + 1
    float       *keep;                     // [Bk][H]: read (step s + 1's) and written (this step's)
    const float *r, *u, *n, *ghn, *h_prev; // the step's rows [Bk][H]
    float       *dgi, *dgh;                // the step's rows [Bk][3H]
    int          Bk, H, last;              // last: step S - 1, whose keep and back are +0.0f
};

__global__ __launch_bounds__(256) void okMemTrainCellKernel(const OkMemTrainCellJob j)
{
    const long t = static_cast<long>(blockIdx.x) * 256 + static_cast<long>(threadIdx.x);
    const int  H = j.H;
    const long q = t / H;
    const int  unit = static_cast<int>(t - q * H);
    if (q >= j.Bk)
        return;
    const long  e = q * H + unit;
    const float dh = ok_memtrain_dh(j.down[e], j.last != 0 ? 0.F : j.keep[e], j.last != 0 ? 0.F : j.back[e]);
    float       keep, d[4];
    const float r = j.r[e];
    ok_memtrain_cell_back(dh, r, j.u[e], j.n[e], j.ghn[e], j.h_prev[e], &keep, d);
    j.keep[e] = keep;
    float *gi = j.dgi + q * 3 * H + unit, *gh = j.dgh + q * 3 * H + unit;
    gi[0]     = d[0];
    gi[H]     = d[1];
    gi[2 * H] = d[2];
    gh[0]     = d[0];
    gh[H]     = d[1];
    gh[2 * H] = d[3];
}

// One thread: the loss from its Z columns
__global__ void okMemTrainLossKernel(const float *lossj, const int Z, const float count, float *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        *out = ok_memtrain_chain(lossj, 1, nullptr, 0, Z, 0.F) / count;
}

// Level 0 of the sum of squares: a thread per block of 64 gradients
__global__ __launch_bounds__(256) void okMemTrainSquareKernel(const float *grad, const int n, float *out)
{
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b * OK_MEMTRAIN_BLOCK >= n)
        return;
    out[b] = ok_memtrain_sq_block(grad + static_cast<long>(b) * OK_MEMTRAIN_BLOCK, okLidarMin(OK_MEMTRAIN_BLOCK, n - b * OK_MEMTRAIN_BLOCK));
}

// A further level: a thread per group of 64 values of the level before; in and out are different buffers
__global__ __launch_bounds__(256) void okMemTrainSumKernel(const float *in, const int n, float *out)
{
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b * OK_MEMTRAIN_BLOCK >= n)
        return;
    out[b] = ok_memtrain_sum_group(in + static_cast<long>(b) * OK_MEMTRAIN_BLOCK, okLidarMin(OK_MEMTRAIN_BLOCK, n - b * OK_MEMTRAIN_BLOCK));
}

// One thread: the step number advances, and Adam's constants of that step go to the workspace
__global__ void okMemTrainTickKernel(long long *t, ok_learn_adam_consts *out, ok_learn_adam_consts c, const float lr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const long long now = *t + 1;
    *t = now;
    ok_memtrain_factors(lr, c.beta1, c.beta2, now, &c.step, &c.bc2);
    *out = c;
}

struct OkMemTrainStepJob
{
    float                      *params, *m, *v, *grad; // grad: the divided gradient in, the clipped one out
    const float                *total;                 // the sum of squares
    const ok_learn_adam_consts *adam;
    float                      *norm_out, *grad_out; // each may be nullptr
    float                       clip_grad, decay;
    int                         T;
};

__global__ __launch_bounds__(256) void okMemTrainStepKernel(const OkMemTrainStepJob j)
{
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= j.T)
        return;
    float       norm;
    const float coef = ok_memtrain_clip(*j.total, j.clip_grad, &norm);
    const float gc   = ok_memtrain_step(j.params + i, j.m + i, j.v + i, j.grad[i], coef, j.decay, *j.adam);
    j.grad[i]        = gc;
    if (j.grad_out != nullptr)
        j.grad_out[i] = gc;
    if (i == 0 && j.norm_out != nullptr)
        *j.norm_out = norm;
}

// ---- host side (no GPU) -----------------------------------------------------------------------------------------------------------------

inline okenv_learner_params okMemTrainAdam(const okenv_memory_learner_config &c)
{
    okenv_learner_params lp{};
    lp.lr    = c.lr;
    lp.clip  = 0.F;
    lp.beta1 = c.beta1;
    lp.beta2 = c.beta2;
    lp.eps   = c.eps;
    return lp;
}

// Adam's constants without the two factors of the step number
inline ok_learn_adam_consts okMemTrainConsts(const okenv_memory_learner_config &c)
{
    ok_learn_adam_consts k{};
    k.beta1 = c.beta1;
    k.omb1  = static_cast<float>(1.0 - static_cast<double>(c.beta1));
    k.beta2 = c.beta2;
    k.omb2  = static_cast<float>(1.0 - static_cast<double>(c.beta2));
    k.eps   = c.eps;
    return k;
}

inline const char *okMemTrainCheckConfig(const okenv_memory_learner_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    const okenv_learner_params lp = okMemTrainAdam(*c);
    if (const char *why = okLearnCheckParams(&lp))
        return why;
    if (!std::isfinite(c->weight_decay) || !(c->weight_decay >= 0.F))
        return "weight_decay must be finite and not negative";
    if (!std::isfinite(c->clip_grad) || !(c->clip_grad >= 0.F))
        return "clip_grad must be finite and not negative (0: no clipping)";
    if (c->seq_len < 1 || c->seq_len > OK_MEMTRAIN_MAX_SEQ)
        return "seq_len outside 1 .. 16";
    if (c->max_batch < 1 || static_cast<int64_t>(c->max_batch) * c->seq_len * 3 * OK_MEMORY_MAX_HIDDEN >= (INT64_C(1) << 31))
        return "max_batch must be at least 1, and max_batch * seq_len * 1536 below 2^31";
    return nullptr;
}

inline const char *okMemTrainCheckCall(const float *latent, const float *action, const int32_t rows, const int32_t *start, const int32_t M, const int32_t B,
                                       const int32_t epochs)
{
    if (latent == nullptr || action == nullptr || start == nullptr)
        return "latent, action and start are required (NULL argument)";
    if (rows < 1 || M < 1 || B < 1 || epochs < 1)
        return "rows, M, B and epochs must be at least 1";
    if (static_cast<int64_t>(epochs) * M >= (INT64_C(1) << 31))
        return "epochs * M must stay below 2^31";
    return nullptr;
}

// What a minibatch's forward leaves for its backward, positions step-major
struct OkMemTrainSaved
{
    int                Bk{0}, S{0};
    std::vector<float> x0, y, zn, r, u, n, ghn, h; // [P][Z + 2], [P][Z], [P][Z]; [L][P][H] each
};

// The forward of the windows `first` (their start rows) over S steps
inline void okMemTrainForwardHost(const ok_memory_shape s, const float *net, const float *latent, const float *action, const int rows, const int stride,
                                  const int S, const std::vector<int> &first, OkMemTrainSaved &sv)
{
    const ok_memory_layout at = ok_memory_offsets(s);
    const int              Z = s.Z, H = s.H, in0 = Z + OK_MEMORY_ACTIONS, Bk = static_cast<int>(first.size());
    const size_t           P = static_cast<size_t>(Bk) * S;
    sv.Bk = Bk, sv.S = S;
    sv.x0.assign(P * in0, 0.F), sv.y.assign(P * Z, 0.F), sv.zn.assign(P * Z, 0.F);
    for (std::vector<float> *v : {&sv.r, &sv.u, &sv.n, &sv.ghn, &sv.h})
        v->assign(static_cast<size_t>(s.L) * P * H, 0.F);
    const std::vector<float> zeros(static_cast<size_t>(H), 0.F);
    for (int st = 0; st < S; ++st)
        for (int q = 0; q < Bk; ++q)
        {
            const size_t p = static_cast<size_t>(st) * Bk + q;
            const float *z = latent + static_cast<size_t>(ok_memtrain_row(first[q], st, stride, rows)) * Z;
            const float *a = action + static_cast<size_t>(ok_memtrain_row(first[q], st, stride, rows)) * OK_MEMORY_ACTIONS;
            const float *zt = latent + static_cast<size_t>(ok_memtrain_row(first[q], st + 1, stride, rows)) * Z;
            for (int j = 0; j < Z; ++j)
            {
                sv.x0[p * in0 + j] = ok_memory_normalise(z[j], net[at.z_mean + j], net[at.z_std + j]);
                sv.y[p * Z + j]    = ok_memory_normalise(zt[j], net[at.z_mean + j], net[at.z_std + j]);
            }
            for (int k = 0; k < OK_MEMORY_ACTIONS; ++k)
                sv.x0[p * in0 + Z + k] = ok_memory_normalise(a[k], net[at.a_mean + k], net[at.a_std + k]);
            const float *x = sv.x0.data() + p * in0;
            for (int l = 0; l < s.L; ++l)
            {
                const int    in = ok_memory_in(s, l);
                const float *wih = net + at.wih[l], *whh = net + at.whh[l], *bih = net + at.bih[l], *bhh = net + at.bhh[l];
                const size_t lp = (static_cast<size_t>(l) * P + p) * H;
                const float *hp = st == 0 ? zeros.data() : sv.h.data() + (static_cast<size_t>(l) * P + p - Bk) * H;
                for (int j = 0; j < H; ++j)
                {
                    float gi[3], gh[3];
                    for (int g = 0; g < 3; ++g)
                    {
                        const int row = g * H + j;
                        gi[g] = ok_memtrain_chain(x, 1, wih + static_cast<size_t>(row) * in, 1, l == 0 ? Z : H, bih[row]);
                        if (l == 0)
                            gi[g] = gi[g] + ok_memory_action_part(x + Z, wih + static_cast<size_t>(row) * in + Z);
                        gh[g] = ok_memtrain_chain(hp, 1, whh + static_cast<size_t>(row) * H, 1, H, bhh[row]);
                    }
                    sv.h[lp + j]   = ok_memtrain_cell(gi[0], gi[1], gi[2], gh[0], gh[1], gh[2], hp[j], &sv.r[lp + j], &sv.u[lp + j], &sv.n[lp + j]);
                    sv.ghn[lp + j] = gh[2];
                }
                x = sv.h.data() + lp;
            }
            for (int j = 0; j < Z; ++j)
                sv.zn[p * Z + j] = ok_memtrain_chain(x, 1, net + at.hw + static_cast<size_t>(j) * H, 1, H, net[at.hb + j]);
        }
}

// The start rows of minibatch `base` .. base + Bk - 1 of an epoch
inline std::vector<int> okMemTrainWindows(const int32_t *start, const int32_t *order, const long base, const int Bk, const int M)
{
    std::vector<int> first(static_cast<size_t>(Bk));
    for (int q = 0; q < Bk; ++q)
        first[q] = start[ok_memtrain_window(order, base, q, M)];
    return first;
}

// One minibatch on the host: its loss, and with grad != nullptr the divided gradient [T]
inline void okMemTrainMinibatchHost(const ok_memory_shape s, const float *net, const float *latent, const float *action, const int rows, const int stride, const int S,
                                    const std::vector<int> &first, float *grad, float *loss)
{
    const ok_memory_layout at = ok_memory_offsets(s);
    const int              Z = s.Z, H = s.H, H3 = 3 * s.H, in0 = Z + OK_MEMORY_ACTIONS, Bk = static_cast<int>(first.size()), P = Bk * S;
    OkMemTrainSaved        sv;
    okMemTrainForwardHost(s, net, latent, action, rows, stride, S, first, sv);
    std::vector<float> dzn(static_cast<size_t>(P) * Z), tt(static_cast<size_t>(P) * Z), lossj(static_cast<size_t>(Z));
    for (size_t e = 0; e < dzn.size(); ++e)
        ok_memtrain_seed(sv.zn[e], sv.y[e], &tt[e], &dzn[e]);
    const float count = static_cast<float>(Bk * S * Z);
    for (int j = 0; j < Z; ++j)
        lossj[j] = ok_memtrain_chain(tt.data() + j, Z, nullptr, 0, P, 0.F);
    *loss = ok_memtrain_chain(lossj.data(), 1, nullptr, 0, Z, 0.F) / count;
    if (grad == nullptr)
        return;
    const size_t       PH = static_cast<size_t>(P) * H;
    std::vector<float> down(PH), keep(static_cast<size_t>(Bk) * H), back(static_cast<size_t>(Bk) * H), dgi(static_cast<size_t>(s.L) * P * H3),
        dgh(static_cast<size_t>(s.L) * P * H3), zeros(static_cast<size_t>(H), 0.F);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < H; ++j)
            down[static_cast<size_t>(p) * H + j] = ok_memtrain_chain(dzn.data() + static_cast<size_t>(p) * Z, 1, net + at.hw + j, H, Z, 0.F);
    for (int l = s.L - 1; l >= 0; --l)
    {
        float *gi_l = dgi.data() + static_cast<size_t>(l) * P * H3, *gh_l = dgh.data() + static_cast<size_t>(l) * P * H3;
        for (int st = S - 1; st >= 0; --st)
        {
            for (int q = 0; q < Bk; ++q)
            {
                const size_t p = static_cast<size_t>(st) * Bk + q, lp = (static_cast<size_t>(l) * P + p) * H;
                const float *hp = st == 0 ? zeros.data() : sv.h.data() + lp - static_cast<size_t>(Bk) * H;
                for (int j = 0; j < H; ++j)
                {
                    const size_t e = static_cast<size_t>(q) * H + j;
                    const float  dh = ok_memtrain_dh(down[p * H + j], st == S - 1 ? 0.F : keep[e], st == S - 1 ? 0.F : back[e]);
                    float        d[4];
                    ok_memtrain_cell_back(dh, sv.r[lp + j], sv.u[lp + j], sv.n[lp + j], sv.ghn[lp + j], hp[j], &keep[e], d);
                    float *gi = gi_l + p * H3 + j, *gh = gh_l + p * H3 + j;
                    gi[0] = d[0], gi[H] = d[1], gi[2 * H] = d[2];
                    gh[0] = d[0], gh[H] = d[1], gh[2 * H] = d[3];
                }
            }
            if (st > 0)
                for (int q = 0; q < Bk; ++q)
                    for (int j = 0; j < H; ++j)
                        back[static_cast<size_t>(q) * H + j] =
                            ok_memtrain_chain(gh_l + (static_cast<size_t>(st) * Bk + q) * H3, 1, net + at.whh[l] + j, H, H3, 0.F);
        }
        if (l > 0)
            for (int p = 0; p < P; ++p)
                for (int j = 0; j < H; ++j)
                    down[static_cast<size_t>(p) * H + j] = ok_memtrain_chain(gi_l + static_cast<size_t>(p) * H3, 1, net + at.wih[l] + j, H, H3, 0.F);
    }
    // the parameter sums over the positions
    for (int l = 0; l < s.L; ++l)
    {
        const int    in = ok_memory_in(s, l);
        const float *gi_l = dgi.data() + static_cast<size_t>(l) * P * H3, *gh_l = dgh.data() + static_cast<size_t>(l) * P * H3;
        const float *x = l == 0 ? sv.x0.data() : sv.h.data() + static_cast<size_t>(l - 1) * PH;
        // h_prev of every position: the layer's h' a step earlier, zeros at step 0
        std::vector<float> prev(PH, 0.F);
        std::copy(sv.h.begin() + static_cast<long>(l * PH), sv.h.begin() + static_cast<long>(l * PH + PH - static_cast<size_t>(Bk) * H), prev.begin() + static_cast<long>(Bk) * H);
        for (int i = 0; i < H3; ++i)
        {
            for (int k = 0; k < in; ++k)
                grad[at.wih[l] + i * in + k] = ok_memtrain_chain(gi_l + i, H3, x + k, l == 0 ? in0 : H, P, 0.F) / count;
            for (int k = 0; k < H; ++k)
                grad[at.whh[l] + i * H + k] = ok_memtrain_chain(gh_l + i, H3, prev.data() + k, H, P, 0.F) / count;
            grad[at.bih[l] + i] = ok_memtrain_chain(gi_l + i, H3, nullptr, 0, P, 0.F) / count;
            grad[at.bhh[l] + i] = ok_memtrain_chain(gh_l + i, H3, nullptr, 0, P, 0.F) / count;
        }
    }
    const float *top = sv.h.data() + static_cast<size_t>(s.L - 1) * PH;
    for (int j = 0; j < Z; ++j)
    {
        for (int k = 0; k < H; ++k)
            grad[at.hw + j * H + k] = ok_memtrain_chain(dzn.data() + j, Z, top + k, H, P, 0.F) / count;
        grad[at.hb + j] = ok_memtrain_chain(dzn.data() + j, Z, nullptr, 0, P, 0.F) / count;
    }
}

inline void okMemTrainUpdateHost(const okenv_memory_learner_config &c, const ok_memory_shape s, okenv_memory_learner_state &st, const float *latent,
                                 const float *action, const int32_t rows, const int32_t *start, const int32_t M, const int32_t stride, const int32_t B,
                                 const int32_t epochs, const int32_t *order, const float *lr_schedule, const okenv_memory_learner_output &out)
{
    const int          T = ok_memtrain_trainable(s), slices = okLearnMinibatches(M, B);
    std::vector<float> grad(static_cast<size_t>(T)), work(static_cast<size_t>((T + OK_MEMTRAIN_BLOCK - 1) / OK_MEMTRAIN_BLOCK));
    for (int e = 0; e < epochs; ++e)
        for (int k = 0; k < slices; ++k)
        {
            const long   base = static_cast<long>(k) * B;
            const int    Bk = static_cast<int>(std::min<long>(B, M - base));
            const size_t at_step = static_cast<size_t>(e) * slices + k;
            float        loss = 0.F, norm = 0.F;
            okMemTrainMinibatchHost(s, st.params, latent, action, rows, stride, c.seq_len,
                                    okMemTrainWindows(start, order != nullptr ? order + static_cast<size_t>(e) * M : nullptr, base, Bk, M), grad.data(), &loss);
            const float          coef = ok_memtrain_clip(ok_memtrain_sumsq(grad.data(), T, work.data()), c.clip_grad, &norm);
            const float          lr = lr_schedule != nullptr ? lr_schedule[at_step] : c.lr;
            ok_learn_adam_consts adam = okMemTrainConsts(c);
            ok_memtrain_factors(lr, c.beta1, c.beta2, st.t + 1, &adam.step, &adam.bc2);
            const float decay = ok_memtrain_decay(lr, c.weight_decay);
            for (int i = 0; i < T; ++i)
                grad[i] = ok_memtrain_step(st.params + i, st.m + i, st.v + i, grad[i], coef, decay, adam);
            st.t += 1;
            if (out.loss != nullptr)
                out.loss[at_step] = loss;
            if (out.norm != nullptr)
                out.norm[at_step] = norm;
        }
    if (out.grad != nullptr)
        std::copy(grad.begin(), grad.end(), out.grad);
}

inline void okMemTrainEvalHost(const ok_memory_shape s, const int S, const float *net, const float *latent, const float *action, const int32_t rows,
                               const int32_t *start, const int32_t M, const int32_t stride, const int32_t B, float *loss)
{
    const int slices = okLearnMinibatches(M, B);
    for (int k = 0; k < slices; ++k)
    {
        const long base = static_cast<long>(k) * B;
        okMemTrainMinibatchHost(s, net, latent, action, rows, stride, S, okMemTrainWindows(start, nullptr, base, static_cast<int>(std::min<long>(B, M - base)), M),
                                nullptr, loss + k);
    }
}

#endif // OK_MEMTRAIN_H
