// ok_gauss.h -- the continuous REINFORCE learner on the device: updateAction and updatePolicy of
// RLRacers/ReinforceContinuous/ReinforceAgent.hpp:65-135 through the network of Policy.hpp:17-53, two hidden layers and a Gaussian head.
// The rule lives in include/okenv_gauss.h (ok_gauss_pre, ok_gauss_back, ok_gauss_eps, ok_gauss_component, ok_gauss_seed, ok_gauss_term) on
// top of the actor's and the learner's, and is shared with okGaussActHost / okGaussUpdateHost below, so the device and the host entries
// agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.
//   okGaussActKernel       32 agents x 8 lanes per workgroup: x = dist / 200, the network, the draw, tanh * scale + bias, the record
//   okGaussGradKernel      one workgroup per chunk of 32 positions: forward, seed and backward into the samples' LDS rows, then the
//                          chunk's partial of every parameter's gradient (register tiles over the weight matrices) and of the loss
//   okReinforceStepKernel  section 19's join kernels on this parameter vector (ok_reinforce.h: OkJoinParams)
// No atomics anywhere: the sums' order is the rule's.
//
// The first section holds what every in -> H1 -> H2 -> out network of the library is built from (okMlp2*, OkGaussNet, OkGaussPlaces,
// okGaussOuterSums, okGaussVecSums, and their host counterparts); guided cost learning's three networks (ok_gcl.h) use the same pieces.
// The gradient kernels' frame (places, group rows, the chunk's n) and their eight walks stay written out in okGaussGradKernel and in
// okGclGradKernel: every shared form of them compiled to other instructions, and the measured ones were slower (docs/HISTORY.md
// section 35).
#ifndef OK_GAUSS_H
#define OK_GAUSS_H

#include <algorithm>
#include <vector>

#include "../../include/okenv.h"
// (ok_gcl_hidden and ok_gcl_back, the hidden layers' activation with ReLU or tanh, are the shared network's and carry the later learner's
// name only because they are part of the public rule header that the C programs and the numpy restatements read as it is)
#include "../../include/okenv_gcl.h"
#include "ok_reinforce.h"

// ==== the two-hidden-layer network: what this learner and guided cost learning share ==================================================

// The network's copy in LDS, in floats from its start: the weight rows of both hidden layers spread to odd strides (the 8 lanes of a
// group read 8 consecutive rows at the same column: 8 different banks), the rest behind them, log_std last
struct OkGaussNet
{
    int rp, hp;                     // row strides of w1 and w2
    int w1, b1, w2, b2, w3, b3, ls; // (b2, w3, b3 are contiguous, as in the parameter vector)
    int floats;
};

__host__ __device__ inline OkGaussNet okGaussNet(const int R, const int H1, const int H2, const int A)
{
    OkGaussNet at;
    at.rp     = okActorRowStride(R);
    at.hp     = H1 | 1;
    at.w1     = 0;
    at.b1     = H1 * at.rp;
    at.w2     = at.b1 + H1;
    at.b2     = at.w2 + H2 * at.hp;
    at.w3     = at.b2 + H2;
    at.b3     = at.w3 + A * H2;
    at.ls     = at.b3 + A;
    at.floats = at.ls + A;
    return at;
}

// Row strides of the per-sample hidden rows (okLearnHiddenStride's choice: the 8 groups of a wave lie 8 banks apart)
__host__ __device__ inline int okGaussHiddenStride(const int H)
{
    return H + 8;
}

// The act kernel's LDS: [net | xs | h1s | h2s]
inline size_t okGaussActLdsBytes(const int R, const int H1, const int H2)
{
    return sizeof(float) * static_cast<size_t>(okGaussNet(R, H1, H2, 2).floats +
                                               kActorAgents * (okActorRowStride(R) + okGaussHiddenStride(H1) + okGaussHiddenStride(H2)));
}

// The gradient kernel's LDS: [net | xs | h1s | d1s | h2s | d2s | dzs | dlss | terms], the rows of the chunk's 32 samples
struct OkGaussPlaces
{
    int xs, h1s, d1s, h2s, d2s, dzs, dlss, terms, end;
};

__host__ __device__ inline OkGaussPlaces okGaussPlaces(const int R, const int H1, const int H2, const int A)
{
    OkGaussPlaces at;
    const int     s1 = okGaussHiddenStride(H1), s2 = okGaussHiddenStride(H2);
    at.xs    = okGaussNet(R, H1, H2, A).floats;
    at.h1s   = at.xs + OK_LEARN_CHUNK * okActorRowStride(R);
    at.d1s   = at.h1s + OK_LEARN_CHUNK * s1;
    at.h2s   = at.d1s + OK_LEARN_CHUNK * s1;
    at.d2s   = at.h2s + OK_LEARN_CHUNK * s2;
    at.dzs   = at.d2s + OK_LEARN_CHUNK * s2;
    at.dlss  = at.dzs + OK_LEARN_CHUNK * OK_ACTOR_MAX_ACTIONS;
    at.terms = at.dlss + OK_LEARN_CHUNK * OK_ACTOR_MAX_ACTIONS;
    at.end   = at.terms + OK_LEARN_CHUNK;
    return at;
}

constexpr size_t kGaussLdsBudget = 160U * 1024U;

inline bool okGaussShapeInRange(const int R, const int H1, const int H2, const int A)
{
    return R >= 1 && R <= OK_ACTOR_MAX_RAYS && H1 >= 1 && H1 <= OK_GAUSS_MAX_HIDDEN && H2 >= 1 && H2 <= OK_GAUSS_MAX_HIDDEN && A >= 1 &&
           A <= OK_ACTOR_MAX_ACTIONS;
}

inline size_t okGaussLdsBytes(const int R, const int H1, const int H2, const int A)
{
    return okGaussShapeInRange(R, H1, H2, A) ? sizeof(float) * static_cast<size_t>(okGaussPlaces(R, H1, H2, A).end) : 0U;
}

// ---- device pieces --------------------------------------------------------------------------------------------------------------

// Where element i of the parameter vector lies in the LDS copy
__device__ __forceinline__ int okGaussLdsIndex(const int i, const ok_gauss_layout &pv, const OkGaussNet &ln, const int R, const int H1)
{
    if (i < pv.w1)
        return ln.ls + i;
    if (i < pv.b1)
    {
        const int q = i - pv.w1, row = q / R;
        return ln.w1 + row * ln.rp + (q - row * R);
    }
    if (i < pv.w2)
        return ln.b1 + (i - pv.b1);
    if (i < pv.b2)
    {
        const int q = i - pv.w2, row = q / H1;
        return ln.w2 + row * ln.hp + (q - row * H1);
    }
    return ln.b2 + (i - pv.b2);
}

// A parameter vector with the layout `pv` from global memory into LDS (a vector that begins with log_std has matrices that are not
// 16-byte aligned: 4-byte loads, consecutive threads on consecutive addresses).  A thread issues kGaussStageBatch loads before it stores
// the first of them, so that their latencies overlap: one workgroup per CU has nobody else to hide them behind.
constexpr int kGaussStageBatch = 8;
__device__ __forceinline__ void okMlp2Stage(float *__restrict__ dst, const float *__restrict__ src, const OkGaussNet ln, const ok_gauss_layout pv, const int in,
                                            const int H1)
{
    for (int base = static_cast<int>(threadIdx.x); base < pv.total; base += kActorThreads * kGaussStageBatch)
    {
        float v[kGaussStageBatch];
#pragma unroll
        for (int u = 0; u < kGaussStageBatch; ++u)
        {
            const int i = base + u * kActorThreads;
            v[u]        = i < pv.total ? src[i] : 0.F;
        }
#pragma unroll
        for (int u = 0; u < kGaussStageBatch; ++u)
        {
            const int i = base + u * kActorThreads;
            if (i < pv.total)
                dst[okGaussLdsIndex(i, pv, ln, in, H1)] = v[u];
        }
    }
}

// Both hidden layers of the group's sample into its LDS rows (tanh or ReLU), then the third layer's output k in lane k (0 in the lanes
// from A on).  Lane l owns the units l, l + 8, ... of both layers; h1 passes through LDS between them.  The whole workgroup calls it
// (two barriers inside).
// (The rows do not overlap the network or each other: __restrict__ lets two units' loads be in flight at once.)
template <bool Tanh>
__device__ __forceinline__ float okMlp2Forward(const float *__restrict__ net, const OkGaussNet ln, const int in, const int H1, const int H2, const int A,
                                               const float *__restrict__ x, float *__restrict__ h1, float *__restrict__ h2, const int lane)
{
    for (int j = lane; j < H1; j += kActorLanes)
        h1[j] = ok_gcl_hidden(ok_learn_pre(net + ln.w1, ln.rp, net + ln.b1, in, x, j), Tanh ? 1 : 0);
    __syncthreads();
    if constexpr (Tanh) // (the tanh layer's loop carries no pragma: the compiler chooses, as it did)
        for (int j = lane; j < H2; j += kActorLanes)
            h2[j] = ok_gcl_hidden(ok_gauss_pre(net + ln.w2, ln.hp, net + ln.b2, H1, h1, j), 1);
    else
#pragma unroll 2
        for (int j = lane; j < H2; j += kActorLanes)
            h2[j] = ok_gcl_hidden(ok_gauss_pre(net + ln.w2, ln.hp, net + ln.b2, H1, h1, j), 0);
    __syncthreads();
    return lane < A ? ok_gauss_pre(net + ln.w3, H2, net + ln.b3, H2, h2, lane) : 0.F;
}

// From the output seeds dz to the hidden seeds d2 and d1 of the group's sample (three barriers inside; the first orders dz, dlss and
// terms before their readers)
template <bool Tanh>
__device__ __forceinline__ void okMlp2Backward(const float *__restrict__ net, const OkGaussNet ln, const int H1, const int H2, const int A,
                                               const float *__restrict__ dz, const float *__restrict__ h1, const float *__restrict__ h2, float *__restrict__ d1,
                                               float *__restrict__ d2, const int lane)
{
    __syncthreads();
    for (int j = lane; j < H2; j += kLearnLanes)
        d2[j] = ok_gcl_back(ok_learn_back_hidden(net + ln.w3, H2, A, dz, j, 1.F), h2[j], Tanh ? 1 : 0);
    __syncthreads();
#pragma unroll 2
    for (int i = lane; i < H1; i += kLearnLanes)
        d1[i] = ok_gcl_back(ok_gauss_back(net + ln.w2, ln.hp, H2, d2, i), h1[i], Tanh ? 1 : 0);
    __syncthreads();
}

// Threads own parameters of a bias-like piece and walk the chunk's samples in ascending position
__device__ __forceinline__ void okGaussVecSums(float *dst, const float *rows, const int stride, const int count, const int n)
{
    for (int pi = static_cast<int>(threadIdx.x); pi < count; pi += kLearnThreads)
    {
        float acc = 0.F;
        for (int q = 0; q < n; ++q)
            acc = acc + rows[q * stride + pi];
        dst[pi] = acc;
    }
}

// The chunk's partial of a weight matrix [na][nb], term a_rows[q][a] * b_rows[q][b]: the workgroup is 8 x 32 threads and a thread holds a
// register tile of 4 x 4 pairs (a = a0 + 8 i, b = b0 + 32 j), so that a sample's four a values and four b values are read from LDS once
// per 16 pairs; each pair's own sum still runs over the samples in ascending position.  Within a wave the a reads are two addresses
// (a broadcast each) and the b reads are 32 consecutive floats: no bank conflict.
constexpr int kGaussTile = 4;
__device__ __forceinline__ void okGaussOuterSums(float *dst, const float *a_rows, const int sa, const int na, const float *b_rows, const int sb, const int nb,
                                                 const int n)
{
    const int tx = static_cast<int>(threadIdx.x) & 31, ty = static_cast<int>(threadIdx.x) >> 5;
    for (int a0 = ty; a0 < na; a0 += 8 * kGaussTile)
        for (int b0 = tx; b0 < nb; b0 += 32 * kGaussTile)
        {
            int   ai[kGaussTile], bi[kGaussTile];
            float acc[kGaussTile][kGaussTile];
#pragma unroll
            for (int i = 0; i < kGaussTile; ++i)
            { // (a pair outside the matrix reads the matrix's last row / column and is not stored)
                ai[i] = a0 + 8 * i < na ? a0 + 8 * i : na - 1;
                bi[i] = b0 + 32 * i < nb ? b0 + 32 * i : nb - 1;
#pragma unroll
                for (int j = 0; j < kGaussTile; ++j)
                    acc[i][j] = 0.F;
            }
            for (int q = 0; q < n; ++q)
            {
                float av[kGaussTile], bv[kGaussTile];
#pragma unroll
                for (int i = 0; i < kGaussTile; ++i)
                {
                    av[i] = a_rows[q * sa + ai[i]];
                    bv[i] = b_rows[q * sb + bi[i]];
                }
#pragma unroll
                for (int i = 0; i < kGaussTile; ++i)
#pragma unroll
                    for (int j = 0; j < kGaussTile; ++j)
                        acc[i][j] = acc[i][j] + av[i] * bv[j];
            }
#pragma unroll
            for (int i = 0; i < kGaussTile; ++i)
#pragma unroll
                for (int j = 0; j < kGaussTile; ++j)
                    if (a0 + 8 * i < na && b0 + 32 * j < nb)
                        dst[(a0 + 8 * i) * nb + b0 + 32 * j] = acc[i][j];
        }
}

// The end of a two-component act kernel: lanes 0 and 1 of the group hold one component's act, eps and pre (and squashed: only where the
// record has that field) and every lane logp; the group's first lane stores the controls and the record `rec`
// (a kernel whose record has no squashed passes none: the constant 0 makes its exchange below dead code, and the compiler drops it)
template <class Rec>
__device__ __forceinline__ void okMlp2ActStore(const OkActFrame &f, const OkActGroup &s, const Rec &rec, const int greedy, const float act, const float eps,
                                               const float pre, const float logp, float *rec_squashed = nullptr, const float squashed = 0.F)
{
    const float act1 = __shfl(act, 1, kActorLanes), eps1 = __shfl(eps, 1, kActorLanes), pre1 = __shfl(pre, 1, kActorLanes);
    const float sq1  = __shfl(squashed, 1, kActorLanes);
    if (s.lane != 0 || !s.valid)
        return;
    const long a  = s.a;
    f.st.thr[a]   = act;
    f.st.steer[a] = act1;
    if (rec.eps != nullptr && greedy == 0)
    {
        rec.eps[2 * a]     = eps;
        rec.eps[2 * a + 1] = eps1;
    }
    if (rec.pre != nullptr)
    {
        rec.pre[2 * a]     = pre;
        rec.pre[2 * a + 1] = pre1;
    }
    if (rec_squashed != nullptr)
    {
        rec_squashed[2 * a]     = squashed;
        rec_squashed[2 * a + 1] = sq1;
    }
    if (rec.action != nullptr)
    {
        rec.action[2 * a]     = act;
        rec.action[2 * a + 1] = act1;
    }
    if (rec.logp != nullptr)
        rec.logp[a] = logp;
    okActAlive(f.st.crashed, rec.alive, a);
}

// ---- the same on the host (no GPU) ----------------------------------------------------------------------------------------------

// What the act configurations of both learners share
inline const char *okMlp2CheckAct(const int greedy, const float *scale, const float *bias)
{
    if (greedy != 0 && greedy != 1)
        return "greedy must be 0 or 1";
    for (int k = 0; k < 2; ++k)
        if (!(scale[k] - scale[k] == 0.F) || !(bias[k] - bias[k] == 0.F))
            return "a scale or bias is not finite";
    return nullptr;
}

// One network on the host: its shape, its hidden layers' activation and where its pieces begin
struct OkMlp2HostNet
{
    int             in, H1, H2, A, nls, tanh;
    ok_gauss_layout pv;
    const float    *par;
};

inline OkMlp2HostNet okMlp2HostNet(const int in, const int H1, const int H2, const int A, const int nls, const int tanh, const float *par)
{
    return OkMlp2HostNet{in, H1, H2, A, nls, tanh, ok_gauss_offsets_nls(in, H1, H2, A, nls), par};
}

// Both hidden layers and the third layer's outputs of one sample
inline void okMlp2HostForward(const OkMlp2HostNet &n, const float *x, float *h1, float *h2, float *z3)
{
    const float *par = n.par;
    for (int j = 0; j < n.H1; ++j)
        h1[j] = ok_gcl_hidden(ok_learn_pre(par + n.pv.w1, n.in, par + n.pv.b1, n.in, x, j), n.tanh);
    for (int j = 0; j < n.H2; ++j)
        h2[j] = ok_gcl_hidden(ok_gauss_pre(par + n.pv.w2, n.H1, par + n.pv.b2, n.H1, h1, j), n.tanh);
    for (int k = 0; k < n.A; ++k)
        z3[k] = ok_gauss_pre(par + n.pv.w3, n.H2, par + n.pv.b3, n.H2, h2, k);
}

// The rows of one chunk on the host: what a gradient kernel keeps in LDS
struct OkMlp2HostRows
{
    std::vector<float> xs, h1s, d1s, h2s, d2s, dzs, dlss, terms;
    std::vector<int>   clips;
    explicit OkMlp2HostRows(const OkMlp2HostNet &n)
        : xs(static_cast<size_t>(OK_LEARN_CHUNK) * n.in), h1s(static_cast<size_t>(OK_LEARN_CHUNK) * n.H1), d1s(h1s.size()),
          h2s(static_cast<size_t>(OK_LEARN_CHUNK) * n.H2), d2s(h2s.size()), dzs(static_cast<size_t>(OK_LEARN_CHUNK) * OK_ACTOR_MAX_ACTIONS), dlss(dzs.size()),
          terms(OK_LEARN_CHUNK), clips(OK_LEARN_CHUNK)
    {
    }
};

// A chunk of n samples: fill(q, x) writes sample q's input row; seed(q, z3, dz, dls, &term, &clipped) its output seeds from the third
// layer's outputs.  Writes the columns [parameters | loss] and returns the chunk's clip count.
template <class Fill, class Seed>
inline uint32_t okMlp2HostChunk(const OkMlp2HostNet &net, OkMlp2HostRows &r, const int n, float *col, const Fill &fill, const Seed &seed)
{
    const size_t W = OK_ACTOR_MAX_ACTIONS;
    const int    P = net.pv.total;
    for (int q = 0; q < n; ++q)
    {
        const size_t sq = static_cast<size_t>(q);
        float       *x = r.xs.data() + sq * net.in, *h1 = r.h1s.data() + sq * net.H1, *d1 = r.d1s.data() + sq * net.H1, *h2 = r.h2s.data() + sq * net.H2;
        float       *d2 = r.d2s.data() + sq * net.H2, *dz = r.dzs.data() + sq * W, *dls = r.dlss.data() + sq * W;
        float        z3[OK_ACTOR_MAX_ACTIONS] = {0.F};
        fill(q, x);
        okMlp2HostForward(net, x, h1, h2, z3);
        for (size_t a = 0; a < W; ++a)
            dz[a] = dls[a] = 0.F;
        r.clips[sq] = 0;
        seed(q, z3, dz, dls, &r.terms[sq], &r.clips[sq]);
        for (int j = 0; j < net.H2; ++j)
            d2[j] = ok_gcl_back(ok_learn_back_hidden(net.par + net.pv.w3, net.H2, net.A, dz, j, 1.F), h2[j], net.tanh);
        for (int i = 0; i < net.H1; ++i)
            d1[i] = ok_gcl_back(ok_gauss_back(net.par + net.pv.w2, net.H1, net.H2, d2, i), h1[i], net.tanh);
    }
    for (int pi = 0; pi < P; ++pi)
    {
        const ok_learn_slot s = ok_gauss_decode_nls(pi, net.in, net.H1, net.H2, net.A, net.nls);
        float               a = 0.F;
        for (int q = 0; q < n; ++q)
        {
            const size_t sq = static_cast<size_t>(q);
            a = a + ok_gauss_term(s, r.xs.data() + sq * net.in, r.h1s.data() + sq * net.H1, r.h2s.data() + sq * net.H2, r.d1s.data() + sq * net.H1,
                                  r.d2s.data() + sq * net.H2, r.dzs.data() + sq * W, r.dlss.data() + sq * W);
        }
        col[pi] = a;
    }
    col[P]       = okLearnHostSumTerms(r.terms.data(), n);
    uint32_t cnt = 0U;
    for (int q = 0; q < n; ++q)
        cnt += static_cast<uint32_t>(r.clips[static_cast<size_t>(q)]);
    return cnt;
}

// ==== the continuous REINFORCE learner =================================================================================================

// logp in every lane of the group from the components' n and l, one per lane
__device__ __forceinline__ float okGaussGroupLogp(const float nk, const float lk, const int A)
{
    float n[OK_ACTOR_MAX_ACTIONS], l[OK_ACTOR_MAX_ACTIONS];
#pragma unroll
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
    {
        n[k] = __shfl(nk, k, kActorLanes);
        l[k] = __shfl(lk, k, kActorLanes);
    }
    return ok_gauss_logp(n, l, A);
}

// ---- acting ---------------------------------------------------------------------------------------------------------------------

struct OkGaussActParams
{
    OkActFrame         f; // (ok_actor.h)
    int                H1, H2;
    const float       *params;
    OkActDrawWords     draw;
    float              scale[2], bias[2];
    int                greedy;
    uint32_t           seed, agent_base;
    okenv_gauss_record rec;
};

__global__ __launch_bounds__(kActorThreads) void okGaussActKernel(const OkGaussActParams p)
{
    const int        R = p.f.R, H1 = p.H1, H2 = p.H2;
    const OkGaussNet ln  = okGaussNet(R, H1, H2, 2);
    float           *net = ok_actor_lds, *xs = net + ln.floats, *h1s = xs + kActorAgents * ln.rp, *h2s = h1s + kActorAgents * okGaussHiddenStride(H1);
    okMlp2Stage(net, p.params, ln, ok_gauss_offsets(R, H1, H2, 2), R, H1);
    const OkActGroup s = okActBegin(p.f.st.dist, p.f.N, R, xs, ln.rp, p.rec.state);
    const int        g = s.g, lane = s.lane;
    __syncthreads();
    const float mu = okMlp2Forward<false>(net, ln, R, H1, H2, 2, s.x, h1s + g * okGaussHiddenStride(H1), h2s + g * okGaussHiddenStride(H2), lane);
    // lanes 0 and 1 take one component each: the draw, exp, tanh and log (fp64 evaluations)
    const int   k  = lane & 1;
    const float ls = net[ln.ls + k];
    float       eps = 0.F;
    if (p.greedy == 0 && lane < 2)
        eps = ok_gauss_eps(p.seed, p.agent_base + static_cast<uint32_t>(s.a), okActDraw(p.draw), k);
    float               z;
    const ok_gauss_comp c   = ok_gauss_component(mu, ls, eps, 0.F, 0, p.greedy, &z);
    const float         act = ok_gauss_action(c.t, k == 1 ? p.scale[1] : p.scale[0], k == 1 ? p.bias[1] : p.bias[0]);
    okMlp2ActStore(p.f, s, p.rec, p.greedy, act, eps, c.pre, okGaussGroupLogp(c.n, c.l, 2));
}

// ok_gauss_normal_pair alone, one word pair per thread (okenv_debug_normal)
__global__ void __launch_bounds__(256) okDebugNormalKernel(const uint32_t *w0, const uint32_t *w1, float *out0, float *out1, const unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        ok_gauss_normal_pair(w0[i], w1[i], out0 + i, out1 + i);
}

// ---- the update -----------------------------------------------------------------------------------------------------------------

// What the gradient kernel needs for one slice, by value (the join kernels take section 19's OkJoinParams)
struct OkGaussParams
{
    int               R, H1, H2, A;
    int               M, Bk;
    int               P, cols; // parameters; columns of the partials: [params | loss]
    long              base;    // first position of the slice: k * B
    const int32_t    *order;   // or nullptr
    okenv_gauss_batch in;
    int               mode;
    const float      *params;
    float            *part; // [C][cols]
};

__global__ __launch_bounds__(kLearnThreads) void okGaussGradKernel(const OkGaussParams p)
{
    const int           R = p.R, H1 = p.H1, H2 = p.H2, A = p.A;
    const OkGaussNet    ln = okGaussNet(R, H1, H2, A);
    const OkGaussPlaces at = okGaussPlaces(R, H1, H2, A);
    const int           s1 = okGaussHiddenStride(H1), s2 = okGaussHiddenStride(H2);
    float              *net = ok_learn_lds, *xs = net + at.xs, *h1s = net + at.h1s, *d1s = net + at.d1s, *h2s = net + at.h2s, *d2s = net + at.d2s;
    float              *dzs = net + at.dzs, *dlss = net + at.dlss, *terms = net + at.terms;
    const int           g = static_cast<int>(threadIdx.x) / kLearnLanes, lane = static_cast<int>(threadIdx.x) & (kLearnLanes - 1);
    const int           chunk = static_cast<int>(blockIdx.x);
    const int           left = p.Bk - chunk * OK_LEARN_CHUNK, n = left < OK_LEARN_CHUNK ? left : OK_LEARN_CHUNK;
    // (the spare groups of the last chunk work on its last sample; the sums never read their rows)
    const long pos = p.base + chunk * OK_LEARN_CHUNK + (g < n ? g : n - 1);
    const int  idx = ok_learn_clamp_index(p.order != nullptr ? static_cast<long long>(p.order[pos]) : static_cast<long long>(pos), p.M);
    // (the group's rows: none overlaps another or the network)
    float *__restrict__ x = xs + g * ln.rp, *__restrict__ h1 = h1s + g * s1, *__restrict__ d1 = d1s + g * s1, *__restrict__ h2 = h2s + g * s2;
    float *__restrict__ d2 = d2s + g * s2, *__restrict__ dz = dzs + g * OK_ACTOR_MAX_ACTIONS;
    for (int i = lane; i < R; i += kLearnLanes)
        x[i] = p.in.state[static_cast<size_t>(idx) * static_cast<size_t>(R) + i];
    const ok_gauss_layout pv = ok_gauss_offsets(R, H1, H2, A);
    okMlp2Stage(net, p.params, ln, pv, R, H1);
    __syncthreads();
    const float mu = okMlp2Forward<false>(net, ln, R, H1, H2, A, x, h1, h2, lane);
    // lane k takes component k: exp, tanh, log and the two seeds
    const float G     = p.in.ret[idx];
    const bool  score = p.mode == OK_GAUSS_GRAD_SCORE, mine = lane < A;
    const int   k     = mine ? lane : 0;
    const float eps   = (!score && mine) ? p.in.eps[static_cast<size_t>(idx) * static_cast<size_t>(A) + k] : 0.F;
    const float pre   = (score && mine) ? p.in.pre[static_cast<size_t>(idx) * static_cast<size_t>(A) + k] : 0.F;
    float       z, dmu, dls;
    const ok_gauss_comp c = ok_gauss_component(mu, net[ln.ls + k], eps, pre, score ? 1 : 0, 0, &z);
    ok_gauss_seed(p.mode, c, z, G, &dmu, &dls);
    const float logp                      = okGaussGroupLogp(c.n, c.l, A);
    dz[lane]                              = mine ? dmu : 0.F;
    dlss[g * OK_ACTOR_MAX_ACTIONS + lane] = mine ? dls : 0.F;
    if (lane == 0)
        terms[g] = -(logp * G);
    okMlp2Backward<false>(net, ln, H1, H2, A, dz, h1, h2, d1, d2, lane);
    // the per-parameter walks into the chunk's row [params | loss]
    float *col = p.part + static_cast<size_t>(chunk) * static_cast<size_t>(p.cols);
    okGaussOuterSums(col + pv.w2, d2s, s2, H2, h1s, s1, H1, n);
    okGaussOuterSums(col + pv.w1, d1s, s1, H1, xs, ln.rp, R, n);
    okGaussOuterSums(col + pv.w3, dzs, OK_ACTOR_MAX_ACTIONS, A, h2s, s2, H2, n);
    okGaussVecSums(col + pv.log_std, dlss, OK_ACTOR_MAX_ACTIONS, A, n);
    okGaussVecSums(col + pv.b1, d1s, s1, H1, n);
    okGaussVecSums(col + pv.b2, d2s, s2, H2, n);
    okGaussVecSums(col + pv.b3, dzs, OK_ACTOR_MAX_ACTIONS, A, n);
    okLearnSumTerms(terms, n, col + p.P);
}

// ---- host side (no GPU) ------------------------------------------------------------------------------------------------------

inline const char *okGaussCheckShape(const int R, const int H1, const int H2, const int A)
{
    if (R < 1 || R > OK_ACTOR_MAX_RAYS)
        return "the fan needs 1 .. 64 rays";
    if (H1 < 1 || H1 > OK_GAUSS_MAX_HIDDEN || H2 < 1 || H2 > OK_GAUSS_MAX_HIDDEN)
        return "a hidden width outside 1 .. 128";
    if (A < 1 || A > OK_ACTOR_MAX_ACTIONS)
        return "number of outputs outside 1 .. 8";
    if (okGaussLdsBytes(R, H1, H2, A) > kGaussLdsBudget)
        return "the gradient kernel's LDS for this shape exceeds 160 KB (okenv_gauss_lds_bytes)";
    return nullptr;
}

inline const char *okGaussCheckConfig(const okenv_gauss_config *c, const int R)
{
    if (c == nullptr)
        return "config is NULL";
    if (const char *why = okGaussCheckShape(R, c->hidden1, c->hidden2, 2))
        return why;
    return okMlp2CheckAct(c->greedy, c->scale, c->bias);
}

inline const char *okGaussCheckCall(const okenv_gauss_update_config *cfg, const okenv_gauss_batch *batch, const int32_t M, const int32_t B)
{
    if (cfg == nullptr)
        return "config is NULL";
    if (batch == nullptr)
        return "batch is NULL";
    if (batch->state == nullptr || batch->ret == nullptr)
        return "state and ret are required";
    if (M < 1 || B < 1)
        return "M and B must be at least 1";
    if (cfg->reduce != OKENV_REINFORCE_SUM && cfg->reduce != OKENV_REINFORCE_MEAN)
        return "unknown reduce (OKENV_REINFORCE_SUM / _MEAN)";
    if (cfg->grad_mode != OKENV_GAUSS_GRAD_REFERENCE && cfg->grad_mode != OKENV_GAUSS_GRAD_SCORE)
        return "unknown grad_mode (OKENV_GAUSS_GRAD_REFERENCE / _SCORE)";
    if (cfg->grad_mode == OKENV_GAUSS_GRAD_REFERENCE && batch->eps == nullptr)
        return "OKENV_GAUSS_GRAD_REFERENCE needs the recorded eps";
    if (cfg->grad_mode == OKENV_GAUSS_GRAD_SCORE && batch->pre == nullptr)
        return "OKENV_GAUSS_GRAD_SCORE needs the recorded pre";
    return nullptr;
}

// The action of n agents on host arrays; every output may be nullptr
inline void okGaussActHost(const okenv_gauss_config &c, const float *par, const int R, const int n, const float *dist, const uint8_t *crashed,
                           const uint32_t draw_index, float *throttle, float *steer, float *eps_out, float *pre_out, float *action, float *logp,
                           float *state, uint8_t *alive)
{
    const OkMlp2HostNet net = okMlp2HostNet(R, c.hidden1, c.hidden2, 2, 2, 0, par);
    std::vector<float>  x(static_cast<size_t>(R)), h1(static_cast<size_t>(net.H1)), h2(static_cast<size_t>(net.H2));
    for (int a = 0; a < n; ++a)
    {
        const size_t sa = static_cast<size_t>(a);
        for (int i = 0; i < R; ++i)
            x[static_cast<size_t>(i)] = dist[sa * R + i] / OK_SENSOR_RANGE;
        float mu[OK_ACTOR_MAX_ACTIONS], nn[OK_ACTOR_MAX_ACTIONS] = {0.F}, ll[OK_ACTOR_MAX_ACTIONS] = {0.F}, act[2], eps[2], pre[2];
        okMlp2HostForward(net, x.data(), h1.data(), h2.data(), mu);
        for (int k = 0; k < 2; ++k)
        {
            eps[k] = c.greedy != 0 ? 0.F : ok_gauss_eps(c.seed, c.agent_base + static_cast<uint32_t>(a), draw_index, k);
            float               z;
            const ok_gauss_comp co = ok_gauss_component(mu[k], par[k], eps[k], 0.F, 0, c.greedy, &z);
            act[k]                 = ok_gauss_action(co.t, c.scale[k], c.bias[k]);
            pre[k]                 = co.pre;
            nn[k]                  = co.n;
            ll[k]                  = co.l;
        }
        if (throttle != nullptr)
            throttle[a] = act[0];
        if (steer != nullptr)
            steer[a] = act[1];
        for (int k = 0; k < 2; ++k)
        {
            if (eps_out != nullptr && c.greedy == 0)
                eps_out[2 * sa + k] = eps[k];
            if (pre_out != nullptr)
                pre_out[2 * sa + k] = pre[k];
            if (action != nullptr)
                action[2 * sa + k] = act[k];
        }
        if (logp != nullptr)
            logp[a] = ok_gauss_logp(nn, ll, 2);
        if (state != nullptr)
            for (int i = 0; i < R; ++i)
                state[sa * R + i] = x[static_cast<size_t>(i)];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

// The rule on host arrays; every output may be nullptr
inline void okGaussUpdateHost(const okenv_learner_params &lp, const okenv_gauss_update_config &cfg, const int R, const int H1, const int H2, const int A,
                              okenv_gauss_state &st, const okenv_gauss_batch &in, const int M, const int B, const int32_t *order,
                              const okenv_gauss_output &out)
{
    const OkMlp2HostNet net = okMlp2HostNet(R, H1, H2, A, A, 0, st.params);
    OkMlp2HostRows      rows(net);
    const bool          score  = cfg.grad_mode == OK_GAUSS_GRAD_SCORE;
    const auto          sample = [&](const long pos)
    { return static_cast<size_t>(ok_learn_clamp_index(order != nullptr ? static_cast<long long>(order[pos]) : static_cast<long long>(pos), M)); };
    const auto fill_from = [&](const long first)
    {
        return [&, first](const int q, float *x)
        {
            const size_t si = sample(first + q);
            for (int i = 0; i < R; ++i)
                x[i] = in.state[si * R + i];
        };
    };
    const auto seed_from = [&](const long first)
    {
        return [&, first](const int q, const float *mu, float *dz, float *dls, float *term, int *)
        {
            const size_t si = sample(first + q);
            const float  G  = in.ret[si];
            float        nn[OK_ACTOR_MAX_ACTIONS] = {0.F}, ll[OK_ACTOR_MAX_ACTIONS] = {0.F};
            for (int a = 0; a < A; ++a)
            {
                float               z;
                const ok_gauss_comp c =
                    ok_gauss_component(mu[a], net.par[a], score ? 0.F : in.eps[si * A + a], score ? in.pre[si * A + a] : 0.F, score ? 1 : 0, 0, &z);
                ok_gauss_seed(cfg.grad_mode, c, z, G, &dz[a], &dls[a]);
                nn[a] = c.n;
                ll[a] = c.l;
            }
            *term = -(ok_gauss_logp(nn, ll, A) * G);
        };
    };
    okSliceUpdateHost(lp, cfg.accumulate != 0, okJoinOn(net.pv.total, st.params, st.m, st.v, cfg.reduce, out.grad), st.t, M, B, out.loss,
                      [&](const long first, const int n, float *col) { (void)okMlp2HostChunk(net, rows, n, col, fill_from(first), seed_from(first)); });
}

#endif // OK_GAUSS_H
