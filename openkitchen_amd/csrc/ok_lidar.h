// ok_lidar.h -- the lidar transformer driver on the device: ImitationLearningTransformer's LidarTransformer
// (laser_transformer.py) driven as infer_torch_traced_main.cpp:19-43 drives it, for every agent of a handle.  The rule lives in
// include/okenv_lidar.h (ok_lidar_dot, ok_lidar_attend, ok_lidar_sum_part, ok_lidar_sq_part, ok_lidar_norm, ok_lidar_input,
// ok_lidar_output) and is shared with okLidarActHost below, so the device and the host entry agree bit for bit.
//
// This is NOT a step kernel and adds no step-kernel launch site.
//   okLidarActKernel  16 agents per workgroup of 4 waves.  A 16-row tile is "token t of the 16 agents", so the activations are R
//                     tiles; they stay in LDS.  Every linear layer runs on v_mfma_f32_16x16x4_f32 with the accumulator started from
//                     the bias: its result is the rule's k-ascending fmaf chain.  Softmax, LayerNorm and the final 2-wide layer run
//                     on the VALU.  Rows of a partial last workgroup repeat the last agent and are never stored.
// The weights are read from global memory (L2 / Infinity Cache) in torch's layout by every workgroup.
#ifndef OK_LIDAR_H
#define OK_LIDAR_H

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_lidar.h"
#include "ok_actor.h"

constexpr int kLidarAgents  = 16;  // agents per workgroup: the rows of one MFMA tile
constexpr int kLidarThreads = 256; // 4 waves
constexpr int kLidarWaves   = kLidarThreads / 64;
constexpr int kLidarRowBlock = 4;  // row tiles a wave carries through one pass over a weight tile, at most 4 (okLidarLinear's switch)
constexpr int kLidarColBlock = 64; // columns of the feed-forward's hidden layer (and of out_proj's output) produced at a time
constexpr int kLidarPad      = 4;  // floats behind every LDS row: the 16 rows of a tile start 4 banks apart, the 4 k's of an MFMA step fill them

typedef float okLidarAcc __attribute__((ext_vector_type(4)));

__host__ __device__ inline int okLidarMax(const int a, const int b)
{
    return a > b ? a : b;
}

__host__ __device__ inline int okLidarMin(const int a, const int b)
{
    return a < b ? a : b;
}

__host__ __device__ inline ok_lidar_shape okLidarShape(const okenv_lidar_config &c)
{
    ok_lidar_shape s;
    s.R      = c.num_points;
    s.d      = c.d_model;
    s.ff     = c.dim_feedforward;
    s.h1     = c.head_hidden1;
    s.h2     = c.head_hidden2;
    s.nhead  = c.nhead;
    s.layers = c.num_layers;
    return s;
}

// Columns of q, k and v built at a time: whole heads and whole MFMA tiles, lcm(dh, 16) (divides d, since dh and 16 do)
__host__ __device__ inline int okLidarHeadGroup(const int dh)
{
    int w = dh;
    while (w % 16 != 0)
        w += dh;
    return w;
}

// The act kernel's LDS, in floats: [x | c | s].  x: the activations, rows x (d + pad).  c: the attention's context, the feed-forward's
// output, the head's first hidden layer.  s: q, k, v of one head group and the softmax rows of the 256 threads; a column block of
// out_proj or of the feed-forward's hidden layer; the head's second hidden layer; the normalised inputs.
struct OkLidarPlaces
{
    int rows, ldx, ldq, ldb, ldp;
    int x, c, s, q, k, v, p, end;
};

__host__ __device__ inline OkLidarPlaces okLidarPlaces(const ok_lidar_shape sh)
{
    OkLidarPlaces at;
    const int     W = okLidarHeadGroup(sh.d / sh.nhead);
    at.rows = sh.R * kLidarAgents;
    at.ldx  = sh.d + kLidarPad;
    at.ldq  = W + kLidarPad;
    at.ldb  = kLidarColBlock + kLidarPad;
    at.ldp  = sh.R | 1;
    const int c_floats = okLidarMax(at.rows * at.ldx, kLidarAgents * (sh.h1 + kLidarPad));
    const int s_floats = okLidarMax(okLidarMax(3 * at.rows * at.ldq + kLidarThreads * at.ldp, at.rows * at.ldb), okLidarMax(kLidarAgents * (sh.h2 + kLidarPad), 2 * at.rows));
    at.x   = 0;
    at.c   = at.x + at.rows * at.ldx;
    at.s   = at.c + c_floats;
    at.q   = at.s;
    at.k   = at.q + at.rows * at.ldq;
    at.v   = at.k + at.rows * at.ldq;
    at.p   = at.v + at.rows * at.ldq;
    at.end = at.s + s_floats;
    return at;
}

constexpr size_t kLidarLdsBudget = 160U * 1024U;

inline size_t okLidarLdsBytes(const ok_lidar_shape s)
{
    return ok_lidar_shape_bad(s) ? 0U : sizeof(float) * static_cast<size_t>(okLidarPlaces(s).end);
}

// ---- the linear piece ------------------------------------------------------------------------------------------------------------

// out[r][n] = (from_out ? out[r][n] : bias[n]) continued by the chain over k = 0 .. K - 1 of x[r][k] * w[n][k], for the Mt row tiles
// of 16 rows and the N (a multiple of 16) columns; relu behind it when asked.  x and out lie in LDS and are given as offsets in floats from its start (the address space stays known to the compiler
// through the switch below), w and bias in global memory.
// x[r][k] is x[r * ldx + (k / kseg) * seg_stride + k % kseg] (the head reads the R tokens of an agent as one row: kseg = d); K and
// kseg are multiples of 16.  The whole workgroup calls it; the caller's __syncthreads() follows.  `rot` turns the assignment of work
// to waves, so that calls which follow each other without a barrier start on different waves.
//
// A wave owns a 16-column tile of w and up to kLidarRowBlock row tiles at a time (okLidarUnit).  Lane l holds A[row l & 15][k = l >> 4]
// and B[k = l >> 4][col l & 15] = w[n0 + (l & 15)][k]; accumulator register r is D[row 4 (l >> 4) + r][col l & 15].  One instruction
// continues the chain of each of its 256 outputs by 4 terms, k ascending.
template <int kTiles> // row tiles of this unit, from row r0 on: kTiles independent accumulators
__device__ __forceinline__ void okLidarUnit(const int xo, const int ldx, const int kseg, const int seg_stride, const int r0, const int K,
                                            const float *__restrict__ w, const int ldw, const float *__restrict__ bias, const int n0, const bool relu,
                                            const bool from_out, const int oo, const int ldo)
{
    const int  lane = static_cast<int>(threadIdx.x) & 63, i = lane & 15, g = lane >> 4;
    const float *x = ok_actor_lds + xo;
    float       *out = ok_actor_lds + oo;
    okLidarAcc   acc[kTiles];
#pragma unroll
    for (int m = 0; m < kTiles; ++m)
    {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[m][r] = from_out ? out[(r0 + 16 * m + 4 * g + r) * ldo + n0 + i] : bias[n0 + i];
    }
    const float *wl = w + static_cast<long>(n0 + i) * ldw + g;
    for (int k0 = 0; k0 < K; k0 += kseg)
    {
        const float *xs = x + (k0 / kseg) * seg_stride + (r0 + i) * ldx + g;
        const float *ws = wl + k0;
        for (int kk = 0; kk < kseg; kk += 16) // four steps at a time: their weight loads go out together
        {
            float b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                b[q] = ws[kk + 4 * q];
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
#pragma unroll
                for (int m = 0; m < kTiles; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[16 * m * ldx + kk + 4 * q], b[q], acc[m], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < kTiles; ++m)
    {
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const float v = acc[m][r];
            out[(r0 + 16 * m + 4 * g + r) * ldo + n0 + i] = relu ? ok_lidar_relu(v) : v;
        }
    }
}

__device__ __forceinline__ void okLidarLinear(const int xo, const int ldx, const int kseg, const int seg_stride, const int Mt, const int K,
                                              const float *__restrict__ w, const int ldw, const float *__restrict__ bias, const int N, const bool relu,
                                              const bool from_out, const int oo, const int ldo, const int rot)
{
    const int wave = static_cast<int>(threadIdx.x) >> 6;
    const int Nt = N >> 4, Mb = (Mt + kLidarRowBlock - 1) / kLidarRowBlock, units = Nt * Mb;
    for (int u = (wave + kLidarWaves - (rot & (kLidarWaves - 1))) & (kLidarWaves - 1); u < units; u += kLidarWaves)
    {
        const int nt = u / Mb, m0 = (u - nt * Mb) * kLidarRowBlock, n0 = nt << 4, r0 = m0 << 4;
        switch (okLidarMin(kLidarRowBlock, Mt - m0)) // (the same for every lane of the wave)
        {
        case 1: okLidarUnit<1>(xo, ldx, kseg, seg_stride, r0, K, w, ldw, bias, n0, relu, from_out, oo, ldo); break;
        case 2: okLidarUnit<2>(xo, ldx, kseg, seg_stride, r0, K, w, ldw, bias, n0, relu, from_out, oo, ldo); break;
        case 3: okLidarUnit<3>(xo, ldx, kseg, seg_stride, r0, K, w, ldw, bias, n0, relu, from_out, oo, ldo); break;
        default: okLidarUnit<4>(xo, ldx, kseg, seg_stride, r0, K, w, ldw, bias, n0, relu, from_out, oo, ldo); break;
        }
    }
}

// x = LayerNorm(x + y) over the rows of x, 8 lanes per row; add == false: LayerNorm(x), y is not read.  A lane touches its own columns only.
__device__ __forceinline__ void okLidarAddNorm(float *x, const int ldx, const bool add, const float *y, const int ldy, const int rows, const int d,
                                               const float *__restrict__ gam, const float *__restrict__ bet)
{
    const int lane = static_cast<int>(threadIdx.x) & (OK_ACTOR_LANES - 1);
    // (every group of a wave takes part in the shuffles: the loop's bound is rounded up to whole passes of the workgroup)
    const int groups = kLidarThreads / OK_ACTOR_LANES, passes = (rows + groups - 1) / groups;
    for (int pass = 0; pass < passes; ++pass)
    {
        const int  r_raw = pass * groups + static_cast<int>(threadIdx.x) / OK_ACTOR_LANES;
        const bool live  = r_raw < rows;
        float     *row   = x + (live ? r_raw : 0) * ldx; // (a group past the last row reads and writes nothing)
        if (live && add)
            for (int c = lane; c < d; c += OK_ACTOR_LANES)
                row[c] = row[c] + y[r_raw * ldy + c];
        float part[OK_ACTOR_LANES];
        const float mine = live ? ok_lidar_sum_part(row, d, lane) : 0.F;
#pragma unroll
        for (int l = 0; l < OK_ACTOR_LANES; ++l)
            part[l] = __shfl(mine, l, OK_ACTOR_LANES);
        const float mean = ok_gauss_tree(part) / static_cast<float>(d);
        const float sq   = live ? ok_lidar_sq_part(row, d, lane, mean) : 0.F;
#pragma unroll
        for (int l = 0; l < OK_ACTOR_LANES; ++l)
            part[l] = __shfl(sq, l, OK_ACTOR_LANES);
        const float den = ok_lidar_den(ok_gauss_tree(part) / static_cast<float>(d));
        if (live)
            for (int c = lane; c < d; c += OK_ACTOR_LANES)
                row[c] = ok_lidar_norm(row[c], mean, den, gam[c], bet[c]);
    }
}

// ---- acting ----------------------------------------------------------------------------------------------------------------------

struct OkLidarActParams
{
    OkDeviceState      st;
    int                N;
    ok_lidar_shape     s;
    const float       *params;
    float              lo[2], hi[2], range, scale; // scale: ok_lidar_scale(dh), made on the host
    okenv_lidar_record rec;
};

__global__ __launch_bounds__(kLidarThreads) void okLidarActKernel(const OkLidarActParams p)
{
    const ok_lidar_shape  sh = p.s;
    const ok_lidar_layout at = ok_lidar_offsets(sh);
    const OkLidarPlaces   pl = okLidarPlaces(sh);
    const int             R = sh.R, d = sh.d, dh = d / sh.nhead, W = okLidarHeadGroup(dh), rows = pl.rows;
    const int             tid = static_cast<int>(threadIdx.x);
    float                *X = ok_actor_lds + pl.x, *Cb = ok_actor_lds + pl.c, *S = ok_actor_lds + pl.s;
    float                *Q = ok_actor_lds + pl.q, *Kb = ok_actor_lds + pl.k, *V = ok_actor_lds + pl.v, *P = ok_actor_lds + pl.p;
    const float          *prm = p.params;
    const long            a0  = static_cast<long>(blockIdx.x) * kLidarAgents;

    // the normalised points: S[row][2], row = t * 16 + i; consecutive threads read consecutive floats of the agents' rays
    for (int e = tid; e < rows * 2; e += kLidarThreads)
    {
        const int  i = e / (2 * R), rest = e - i * 2 * R, t = rest >> 1, comp = rest & 1;
        const long a_raw = a0 + i, a = a_raw < p.N ? a_raw : static_cast<long>(p.N) - 1;
        const float raw = (comp ? p.st.rel_y : p.st.rel_x)[a * R + t];
        const float v   = ok_lidar_input(raw, p.range);
        S[(t * kLidarAgents + i) * 2 + comp] = v;
        if (a_raw < p.N && p.rec.input != nullptr)
            p.rec.input[(a * R + t) * 2 + comp] = v;
    }
    __syncthreads();
    // the embedding and the positional term
    for (int e = tid; e < rows * d; e += kLidarThreads)
    {
        const int r = e / d, c = e - r * d, t = r / kLidarAgents;
        X[r * pl.ldx + c] = ok_lidar_dot(S + 2 * r, prm + at.emb_w + 2 * c, 2, prm[at.emb_b + c]) + prm[at.pos + t * d + c];
    }
    __syncthreads();

    for (int layer = 0; layer < sh.layers; ++layer)
    {
        const float *lp = prm + at.layer0 + static_cast<long>(layer) * at.layer_stride;
        // attention, one group of whole heads (W columns) at a time: q, k, v of the group, then every (agent, head, query)
        for (int c0 = 0; c0 < d; c0 += W)
        {
            okLidarLinear(pl.x, pl.ldx, d, 0, R, d, lp + at.in_w + static_cast<long>(c0) * d, d, lp + at.in_b + c0, W, false, false, pl.q, pl.ldq, 0);
            okLidarLinear(pl.x, pl.ldx, d, 0, R, d, lp + at.in_w + static_cast<long>(d + c0) * d, d, lp + at.in_b + d + c0, W, false, false, pl.k, pl.ldq, 2);
            okLidarLinear(pl.x, pl.ldx, d, 0, R, d, lp + at.in_w + static_cast<long>(2 * d + c0) * d, d, lp + at.in_b + 2 * d + c0, W, false, false, pl.v, pl.ldq, 1);
            __syncthreads();
            const int heads = W / dh;
            for (int e = tid; e < kLidarAgents * heads * R; e += kLidarThreads)
            {
                const int i = e & (kLidarAgents - 1), rest = e / kLidarAgents, tq = rest % R, hd = rest / R;
                const int col = hd * dh;
                ok_lidar_attend(Q + (tq * kLidarAgents + i) * pl.ldq + col, Kb + i * pl.ldq + col, V + i * pl.ldq + col, kLidarAgents * pl.ldq, R, dh,
                                p.scale, P + tid * pl.ldp, Cb + (tq * kLidarAgents + i) * pl.ldx + c0 + col);
            }
            __syncthreads();
        }
        // out_proj in column blocks through S, added to x as they come
        for (int n0 = 0; n0 < d; n0 += kLidarColBlock)
        {
            const int nb = okLidarMin(kLidarColBlock, d - n0);
            okLidarLinear(pl.c, pl.ldx, d, 0, R, d, lp + at.out_w + static_cast<long>(n0) * d, d, lp + at.out_b + n0, nb, false, false, pl.s, pl.ldb, 0);
            __syncthreads();
            for (int e = tid; e < rows * nb; e += kLidarThreads)
            {
                const int r = e / nb, c = e - r * nb;
                X[r * pl.ldx + n0 + c] = X[r * pl.ldx + n0 + c] + S[r * pl.ldb + c];
            }
            __syncthreads();
        }
        okLidarAddNorm(X, pl.ldx, false, Cb, pl.ldx, rows, d, lp + at.n1_g, lp + at.n1_b);
        __syncthreads();
        // the feed-forward: the hidden layer in column blocks; linear2's chains go on in c from block to block, k ascending
        for (int f0 = 0; f0 < sh.ff; f0 += kLidarColBlock)
        {
            const int nb = okLidarMin(kLidarColBlock, sh.ff - f0);
            okLidarLinear(pl.x, pl.ldx, d, 0, R, d, lp + at.l1_w + static_cast<long>(f0) * d, d, lp + at.l1_b + f0, nb, true, false, pl.s, pl.ldb, 0);
            __syncthreads();
            okLidarLinear(pl.s, pl.ldb, nb, 0, R, nb, lp + at.l2_w + f0, sh.ff, lp + at.l2_b, d, false, f0 > 0, pl.c, pl.ldx, 0);
            __syncthreads();
        }
        okLidarAddNorm(X, pl.ldx, true, Cb, pl.ldx, rows, d, lp + at.n2_g, lp + at.n2_b);
        __syncthreads();
    }

    // the control head: an agent's R tokens are one row of R d values
    const int ld1 = sh.h1 + kLidarPad, ld2 = sh.h2 + kLidarPad;
    okLidarLinear(pl.x, pl.ldx, d, kLidarAgents * pl.ldx, 1, R * d, prm + at.hw0, R * d, prm + at.hb0, sh.h1, true, false, pl.c, ld1, 0);
    __syncthreads();
    okLidarLinear(pl.c, ld1, sh.h1, 0, 1, sh.h1, prm + at.hw1, sh.h1, prm + at.hb1, sh.h2, true, false, pl.s, ld2, 0);
    __syncthreads();
    if (tid >= 2 * kLidarAgents)
        return;
    const int  i = tid >> 1, k = tid & 1;
    const long a = a0 + i;
    if (a >= p.N)
        return;
    const float o   = ok_lidar_dot(S + i * ld2, prm + at.hw2 + k * sh.h2, sh.h2, prm[at.hb2 + k]);
    const float act = ok_lidar_output(o, k ? p.lo[1] : p.lo[0], k ? p.hi[1] : p.hi[0]);
    (k ? p.st.steer : p.st.thr)[a] = act;
    if (p.rec.action != nullptr)
        p.rec.action[2 * a + k] = act;
    if (k == 0)
        okActAlive(p.st.crashed, p.rec.alive, a);
}

// okenv_debug_lidar_linear: 16 rows of x per workgroup into LDS (rows past M are zero and never stored), okLidarLinear, the rows back
__global__ __launch_bounds__(kLidarThreads) void okDebugLidarLinearKernel(const int M, const int K, const int N, const float *x, const float *w,
                                                                        const float *bias, const int relu, float *out)
{
    const int ldx = K + kLidarPad, ldo = N + kLidarPad;
    float    *xs = ok_actor_lds, *os = xs + kLidarAgents * ldx;
    const int r0 = static_cast<int>(blockIdx.x) * kLidarAgents;
    for (int e = static_cast<int>(threadIdx.x); e < kLidarAgents * K; e += kLidarThreads)
    {
        const int r = e / K, k = e - r * K;
        xs[r * ldx + k] = r0 + r < M ? x[static_cast<long>(r0 + r) * K + k] : 0.F;
    }
    __syncthreads();
    okLidarLinear(0, ldx, K, 0, 1, K, w, K, bias, N, relu != 0, false, kLidarAgents * ldx, ldo, 0);
    __syncthreads();
    for (int e = static_cast<int>(threadIdx.x); e < kLidarAgents * N; e += kLidarThreads)
    {
        const int r = e / N, n = e - r * N;
        if (r0 + r < M)
            out[static_cast<long>(r0 + r) * N + n] = os[r * ldo + n];
    }
}

inline size_t okDebugLidarLinearLdsBytes(const int K, const int N)
{
    return sizeof(float) * static_cast<size_t>(kLidarAgents) * static_cast<size_t>(K + N + 2 * kLidarPad);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okLidarCheckConfig(const okenv_lidar_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_lidar_shape_bad(okLidarShape(*c)))
        return "shape outside the limits (num_points 1 .. 16; d_model, dim_feedforward, head_hidden1/2 multiples of 16 within their limits; nhead "
               "dividing d_model; num_layers 1 .. 8)";
    if (okLidarLdsBytes(okLidarShape(*c)) > kLidarLdsBudget)
        return "the act kernel's LDS (okenv_lidar_lds_bytes) does not fit 160 KB";
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(c->action_lo[k]) || !std::isfinite(c->action_hi[k]))
            return "action_lo / action_hi must be finite";
    if (!std::isfinite(c->sensor_range) || !(c->sensor_range > 0.F))
        return "sensor_range must be finite and > 0";
    return nullptr;
}

inline void okLidarActHost(const okenv_lidar_config &c, const float *params, const int n, const float *rel_xy, const uint8_t *crashed, float *throttle,
                           float *steer, float *input, uint8_t *alive)
{
    const ok_lidar_shape s = okLidarShape(c);
    std::vector<float>   work(static_cast<size_t>(ok_lidar_work_floats(s))), in(static_cast<size_t>(2 * s.R));
    for (int a = 0; a < n; ++a)
    {
        for (int e = 0; e < 2 * s.R; ++e)
        {
            in[static_cast<size_t>(e)] = ok_lidar_input(rel_xy[static_cast<size_t>(a) * 2U * s.R + e], c.sensor_range);
            if (input != nullptr)
                input[static_cast<size_t>(a) * 2U * s.R + e] = in[static_cast<size_t>(e)];
        }
        float o[2];
        ok_lidar_forward(s, params, in.data(), work.data(), o);
        if (throttle != nullptr)
            throttle[a] = ok_lidar_output(o[0], c.action_lo[0], c.action_hi[0]);
        if (steer != nullptr)
            steer[a] = ok_lidar_output(o[1], c.action_lo[1], c.action_hi[1]);
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

inline void okLidarLinearHost(const int M, const int K, const int N, const float *x, const float *w, const float *bias, const int relu, float *out)
{
    for (int m = 0; m < M; ++m)
        for (int j = 0; j < N; ++j)
        {
            const float v = ok_lidar_dot(x + static_cast<size_t>(m) * K, w + static_cast<size_t>(j) * K, K, bias[j]);
            out[static_cast<size_t>(m) * N + j] = relu ? ok_lidar_relu(v) : v;
        }
}

#endif // OK_LIDAR_H
