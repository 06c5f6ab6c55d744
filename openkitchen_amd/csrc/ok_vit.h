// ok_vit.h -- the image transformer driver on the device: DinoControl's frozen ViT and its policy head, for
// every agent of a handle.  The rule lives in include/okenv_vit.h and is shared with okVitActHost below, so the device and the host
// entry agree bit for bit.
//
// This is NOT a step kernel and adds no step-kernel launch site.  The activations live in a workspace in global memory, [x | n | ctx |
// qkv | hid] for the agents of one pass (ok_vit_agent_floats each); the act loops one fixed launch sequence over the passes:
//   okVitLinearKernel<kVitSrcPatch, kVitEpiPos>   the patch embedding: an implicit GEMM whose A tile is built from the camera's bytes;
//                                                the positional term behind it; the class token's row
//   per block: okVitNormKernel, okVitLinearKernel (qkv), okVitAttendKernel, okVitLinearKernel<.., kVitEpiResidual> (proj),
//              okVitNormKernel, okVitLinearKernel<.., kVitEpiGelu> (fc1), okVitLinearKernel<.., kVitEpiResidual> (fc2)
//   okVitFinalKernel                             the class token's LayerNorm, the head (okLidarLinear), the action fields, the record
// Every matrix product runs on v_mfma_f32_16x16x4_f32 with the accumulator started from the bias (or 0.0f where the rule says so): its
// result is the rule's k-ascending fmaf chain (section 22).  LayerNorm is a kernel of its own.  The weights are read in torch's layout:
// there is no packed copy.
#ifndef OK_VIT_H
#define OK_VIT_H

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_vit.h"
#include "ok_lidar.h"

constexpr int kVitThreads = 256; // 4 waves
constexpr int kVitTile    = 64;  // rows and columns of a workgroup's output tile in the linear kernel: a wave owns 16 rows x 64 columns
constexpr int kVitKBlock  = 16;  // k's staged at a time
constexpr int kVitLd      = kVitKBlock + 4; // floats of a staged row: the 16 rows of a tile start 20 banks apart
constexpr int kVitQueries = 16;  // queries of an attention workgroup: the rows of one MFMA tile
constexpr int kVitAgents  = 16;  // agents of a workgroup of the final kernel
constexpr int kVitNormRows = kVitThreads / OK_ACTOR_LANES; // rows of a workgroup of the LayerNorm kernel

enum { kVitSrcPlain, kVitSrcPatch };
enum { kVitEpiNone, kVitEpiGelu, kVitEpiResidual, kVitEpiPos };

__host__ __device__ inline ok_vit_shape okVitShape(const okenv_vit_config &c)
{
    ok_vit_shape s;
    s.S     = c.image_size;
    s.P     = c.patch;
    s.D     = c.dim;
    s.heads = c.heads;
    s.depth = c.depth;
    s.ff    = c.dim_feedforward;
    s.h1    = c.head_hidden1;
    s.h2    = c.head_hidden2;
    return s;
}

inline ok_vit_consts okVitConsts(const okenv_vit_config &c)
{
    ok_vit_consts k;
    for (int i = 0; i < 3; ++i)
    {
        k.mean[i] = c.mean[i];
        k.std[i]  = c.std[i];
    }
    k.eps         = c.ln_eps;
    k.throttle    = c.throttle;
    k.steer_scale = c.steer_scale;
    return k;
}

// The LDS plan, in floats.  attend: [q 16 x (dh + 4) | the softmax rows 16 x (Tp + 4)], Tp = T rounded up to whole key tiles.
// final: [the normalised class tokens 16 x (D + 4) | hidden 1 16 x (H1 + 4) | hidden 2 16 x (H2 + 4)].  The linear kernel's two staged
// tiles are static.
struct OkVitPlaces
{
    int T, Tp, dh, ldq, lds, attend, ldx, ld1, ld2, h1_at, h2_at, final, linear;
};

__host__ __device__ inline OkVitPlaces okVitPlaces(const ok_vit_shape s)
{
    OkVitPlaces at;
    at.T      = ok_vit_tokens(s);
    at.Tp     = (at.T + 15) / 16 * 16;
    at.dh     = s.D / s.heads;
    at.ldq    = at.dh + kLidarPad;
    at.lds    = at.Tp + kLidarPad;
    at.attend = kVitQueries * (at.ldq + at.lds);
    at.ldx    = s.D + kLidarPad;
    at.ld1    = s.h1 + kLidarPad;
    at.ld2    = s.h2 + kLidarPad;
    at.h1_at  = kVitAgents * at.ldx;
    at.h2_at  = at.h1_at + kVitAgents * at.ld1;
    at.final  = at.h2_at + kVitAgents * at.ld2;
    at.linear = 2 * kVitTile * kVitLd;
    return at;
}

inline size_t okVitLdsBytes(const ok_vit_shape s)
{
    if (ok_vit_shape_bad(s))
        return 0U;
    const OkVitPlaces at = okVitPlaces(s);
    return sizeof(float) * static_cast<size_t>(std::max(std::max(at.attend, at.final), at.linear));
}

// ---- the linear kernel -----------------------------------------------------------------------------------------------------------

// out[m][n] = epilogue(bias[n] continued by the chain over k = 0 .. K - 1 of a[m][k] * w[n][k]) for the M rows of a pass taken flat
// (a 16-row tile may hold rows of two agents; the last tile is partial) and the N columns (a multiple of 16).  K is a multiple of 16.
// kVitSrcPatch: row m is patch m % (T - 1) of agent m / (T - 1), a[m][k] is ok_vit_patch_input of the agent's frame, and the row lands
// at token 1 + patch of the agent in out.
struct OkVitLinearParams
{
    long           M;
    int            K, N;
    const float   *a;
    long           lda;
    const float   *w, *bias;
    float         *out;
    long           ldo;
    const uint8_t *frames; // kVitSrcPatch: the pass's first frame
    int            S, P, side, T;
    float          mean[3], std[3];
    const float   *pos, *cls; // kVitEpiPos
};

typedef float okVitVec4 __attribute__((ext_vector_type(4)));

template <int kSrc, int kEpi>
__global__ __launch_bounds__(kVitThreads) void okVitLinearKernel(const OkVitLinearParams p)
{
    __shared__ __attribute__((aligned(16))) float As[kVitTile * kVitLd];
    __shared__ __attribute__((aligned(16))) float Ws[kVitTile * kVitLd];
    const int  tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const long m0 = static_cast<long>(blockIdx.x) * kVitTile;
    const int  n0 = static_cast<int>(blockIdx.y) * kVitTile;
    const int  ctiles = okLidarMin(kVitTile / 16, (p.N - n0) >> 4); // (the same for the whole workgroup)
    okLidarAcc acc[kVitTile / 16];
#pragma unroll
    for (int ct = 0; ct < kVitTile / 16; ++ct)
    {
        const float b = ct < ctiles ? p.bias[n0 + 16 * ct + i] : 0.F;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[ct][r] = b;
    }
    // staging: thread (sr, sq) brings four consecutive k's of row sr of each tile; rows past the end are zero and never stored
    const int  sr = tid >> 2, sq = (tid & 3) * 4;
    const long am = m0 + sr;
    const int  wn = n0 + sr;
    const bool a_live = am < p.M, w_live = wn < p.N;
    long       a_row = 0;
    int        py = 0, px = 0;
    const uint8_t *frame = nullptr;
    if (kSrc == kVitSrcPatch)
    {
        if (a_live)
        {
            const long agent = am / (p.T - 1);
            const int  patch = static_cast<int>(am - agent * (p.T - 1));
            py    = patch / p.side;
            px    = patch - py * p.side;
            frame = p.frames + agent * p.S * p.S * 4;
        }
    }
    else
        a_row = am * p.lda;
    for (int k0 = 0; k0 < p.K; k0 += kVitKBlock)
    {
        okVitVec4 va = {0.F, 0.F, 0.F, 0.F}, vw = {0.F, 0.F, 0.F, 0.F};
        if (a_live)
        {
            if (kSrc == kVitSrcPatch)
            {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    va[j] = ok_vit_patch_input(frame, p.S, p.P, py, px, k0 + sq + j, p.mean, p.std);
            }
            else
                va = *reinterpret_cast<const okVitVec4 *>(p.a + a_row + k0 + sq);
        }
        if (w_live)
            vw = *reinterpret_cast<const okVitVec4 *>(p.w + static_cast<long>(wn) * p.K + k0 + sq);
        __syncthreads(); // (the previous block's reads are done)
        *reinterpret_cast<okVitVec4 *>(As + sr * kVitLd + sq) = va;
        *reinterpret_cast<okVitVec4 *>(Ws + sr * kVitLd + sq) = vw;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kVitKBlock / 4; ++q)
        {
            const float a = As[(16 * wave + i) * kVitLd + 4 * q + g];
#pragma unroll
            for (int ct = 0; ct < kVitTile / 16; ++ct)
                if (ct < ctiles)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ws[(16 * ct + i) * kVitLd + 4 * q + g], acc[ct], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < kVitTile / 16; ++ct)
    {
        if (ct >= ctiles)
            continue;
        const int col = n0 + 16 * ct + i;
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const long m = m0 + 16 * wave + 4 * g + r;
            if (m >= p.M)
                continue;
            const float v = acc[ct][r];
            if (kEpi == kVitEpiPos)
            {
                const long agent = m / (p.T - 1);
                const int  patch = static_cast<int>(m - agent * (p.T - 1));
                float     *row   = p.out + (agent * p.T + 1 + patch) * p.ldo;
                row[col] = v + p.pos[static_cast<long>(1 + patch) * p.N + col];
                if (patch == 0) // the class token's row of this agent, these columns
                    row[col - p.ldo] = p.cls[col] + p.pos[col];
            }
            else if (kEpi == kVitEpiResidual)
                p.out[m * p.ldo + col] = p.out[m * p.ldo + col] + v;
            else
                p.out[m * p.ldo + col] = kEpi == kVitEpiGelu ? ok_vit_gelu(v) : v;
        }
    }
}

// ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------

// out[m] = LayerNorm(x[m]) for the M rows of a pass, 8 lanes a row (the rule's partial sums), 32 rows a workgroup
__global__ __launch_bounds__(kVitThreads) void okVitNormKernel(const long M, const int D, const float *__restrict__ x, const float *__restrict__ gam,
                                                              const float *__restrict__ bet, const float eps, float *__restrict__ out)
{
    const int    lane = static_cast<int>(threadIdx.x) & (OK_ACTOR_LANES - 1);
    const long   r_raw = static_cast<long>(blockIdx.x) * kVitNormRows + static_cast<int>(threadIdx.x) / OK_ACTOR_LANES;
    const bool   live = r_raw < M; // (a group past the last row takes part in the shuffles and stores nothing)
    const float *row = x + (live ? r_raw : 0) * D;
    float        part[OK_ACTOR_LANES];
    const float  mine = live ? ok_lidar_sum_part(row, D, lane) : 0.F;
#pragma unroll
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        part[l] = __shfl(mine, l, OK_ACTOR_LANES);
    const float mean = ok_gauss_tree(part) / static_cast<float>(D);
    const float sq   = live ? ok_lidar_sq_part(row, D, lane, mean) : 0.F;
#pragma unroll
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        part[l] = __shfl(sq, l, OK_ACTOR_LANES);
    const float den = ok_vit_den(ok_gauss_tree(part) / static_cast<float>(D), eps);
    if (live)
        for (int c = lane; c < D; c += OK_ACTOR_LANES)
            out[r_raw * D + c] = ok_lidar_norm(row[c], mean, den, gam[c], bet[c]);
}

// ---- attention ---------------------------------------------------------------------------------------------------------------------

// One workgroup per (sequence, head, tile of 16 queries): the scores by MFMA into LDS (a wave takes every fourth key tile), the softmax
// rows there (8 lanes a row: the rule's partials), the context by MFMA over the keys (a wave takes a 16-column tile of the head).
// qkv [seqs][T][3 D] -> ctx [seqs][T][D].  Keys past T - 1 in the last key tile: k reads as 0.0f, p is 0.0f, v reads as -0.0f (the
// rule's ZERO TERMS).  Queries past T - 1 are zero rows and never stored.
struct OkVitAttendParams
{
    int          T, D, heads, dh, qtiles;
    float        scale;
    const float *qkv;
    float       *ctx;
};

__global__ __launch_bounds__(kVitThreads) void okVitAttendKernel(const OkVitAttendParams p)
{
    const int  tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int  T = p.T, dh = p.dh, Tp = (T + 15) / 16 * 16, ldq = dh + kLidarPad, lds = Tp + kLidarPad;
    const long unit = static_cast<long>(blockIdx.x);
    const int  qt = static_cast<int>(unit % p.qtiles), hd = static_cast<int>((unit / p.qtiles) % p.heads);
    const long seq = unit / (static_cast<long>(p.qtiles) * p.heads);
    const int  q0 = qt * kVitQueries;
    const long ld3 = 3L * p.D;
    const float *base = p.qkv + seq * T * ld3 + hd * dh;
    float       *Q = ok_actor_lds, *Sc = Q + kVitQueries * ldq;
    for (int e = tid; e < kVitQueries * dh; e += kVitThreads)
    {
        const int r = e / dh, c = e - r * dh;
        Q[r * ldq + c] = q0 + r < T ? base[(q0 + r) * ld3 + c] : 0.F;
    }
    __syncthreads();
    for (int kt = wave; kt < Tp / 16; kt += kVitThreads / 64)
    {
        const int   key = kt * 16 + i;
        const bool  live = key < T;
        const float *kr = base + p.D + (live ? key : 0) * ld3 + g;
        okLidarAcc  acc = {0.F, 0.F, 0.F, 0.F};
        for (int c0 = 0; c0 < dh; c0 += 16)
        {
            float b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                b[q] = live ? kr[c0 + 4 * q] : 0.F;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Q[i * ldq + c0 + 4 * q + g], b[q], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            Sc[(4 * g + r) * lds + kt * 16 + i] = acc[r] * p.scale;
    }
    __syncthreads();
    if (tid < kVitQueries * OK_ACTOR_LANES) // (whole waves: the shuffles below stay inside 8-lane groups)
    {
        float    *row = Sc + (tid / OK_ACTOR_LANES) * lds;
        const int l = tid & (OK_ACTOR_LANES - 1);
        float     m = row[0];
        for (int t = l; t < T; t += OK_ACTOR_LANES)
            m = row[t] > m ? row[t] : m;
#pragma unroll
        for (int d = OK_ACTOR_LANES / 2; d > 0; d >>= 1)
        {
            const float o = __shfl_xor(m, d, OK_ACTOR_LANES);
            m = o > m ? o : m;
        }
        float mine = 0.0F;
        for (int t = l; t < T; t += OK_ACTOR_LANES)
        {
            const float e = ok_expf(row[t] - m);
            row[t] = e;
            mine   = mine + e;
        }
        float part[OK_ACTOR_LANES];
#pragma unroll
        for (int j = 0; j < OK_ACTOR_LANES; ++j)
            part[j] = __shfl(mine, j, OK_ACTOR_LANES);
        const float sum = ok_gauss_tree(part);
        for (int t = l; t < T; t += OK_ACTOR_LANES)
            row[t] = row[t] / sum;
        for (int t = T + l; t < Tp; t += OK_ACTOR_LANES)
            row[t] = 0.F;
    }
    __syncthreads();
    if (wave < dh / 16)
    {
        const int    n0 = wave * 16;
        const float *vb = base + 2 * p.D + n0 + i;
        okLidarAcc   acc = {0.F, 0.F, 0.F, 0.F};
        for (int t0 = 0; t0 < Tp; t0 += 16)
        {
            float b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
                const int key = t0 + 4 * q + g;
                b[q] = key < T ? vb[key * ld3] : -0.F;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Sc[i * lds + t0 + 4 * q + g], b[q], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const int tq = q0 + 4 * g + r;
            if (tq < T)
                p.ctx[(seq * T + tq) * p.D + hd * dh + n0 + i] = acc[r];
        }
    }
}

inline size_t okVitAttendLdsBytes(const int T, const int dh)
{
    return sizeof(float) * static_cast<size_t>(kVitQueries) * static_cast<size_t>(dh + (T + 15) / 16 * 16 + 2 * kLidarPad);
}

// ---- the final kernel --------------------------------------------------------------------------------------------------------------

struct OkVitFinalParams
{
    OkDeviceState    st;
    long             a0;    // the pass's first agent
    int              count; // its agents
    ok_vit_shape     s;
    const float     *params, *x; // x: the pass's activations [count][T][D]
    float            eps, throttle, steer_scale;
    okenv_vit_record rec;
};

// 16 agents a workgroup: the class tokens' LayerNorm into LDS (8 lanes a row), the head's two hidden layers by okLidarLinear, the
// output, the action fields and the record.  Rows of a partial last workgroup repeat the pass's last agent and are never stored.
__global__ __launch_bounds__(kLidarThreads) void okVitFinalKernel(const OkVitFinalParams p)
{
    const ok_vit_shape  sh = p.s;
    const ok_vit_layout at = ok_vit_offsets(sh);
    const OkVitPlaces   pl = okVitPlaces(sh);
    const int           D = sh.D, T = pl.T, tid = static_cast<int>(threadIdx.x);
    const float        *prm = p.params;
    float              *X = ok_actor_lds, *H2 = ok_actor_lds + pl.h2_at;
    const int           b0 = static_cast<int>(blockIdx.x) * kVitAgents;
    if (tid < kVitAgents * OK_ACTOR_LANES)
    {
        const int    r = tid / OK_ACTOR_LANES, lane = tid & (OK_ACTOR_LANES - 1);
        const bool   live = b0 + r < p.count;
        const int    local = live ? b0 + r : p.count - 1;
        const float *row = p.x + static_cast<long>(local) * T * D;
        float        part[OK_ACTOR_LANES];
        const float  mine = ok_lidar_sum_part(row, D, lane);
#pragma unroll
        for (int l = 0; l < OK_ACTOR_LANES; ++l)
            part[l] = __shfl(mine, l, OK_ACTOR_LANES);
        const float mean = ok_gauss_tree(part) / static_cast<float>(D);
        const float sq   = ok_lidar_sq_part(row, D, lane, mean);
#pragma unroll
        for (int l = 0; l < OK_ACTOR_LANES; ++l)
            part[l] = __shfl(sq, l, OK_ACTOR_LANES);
        const float den = ok_vit_den(ok_gauss_tree(part) / static_cast<float>(D), p.eps);
        for (int c = lane; c < D; c += OK_ACTOR_LANES)
        {
            const float v = ok_lidar_norm(row[c], mean, den, prm[at.norm_g + c], prm[at.norm_b + c]);
            X[r * pl.ldx + c] = v;
            if (live && p.rec.embedding != nullptr)
                p.rec.embedding[(p.a0 + local) * D + c] = v;
        }
    }
    __syncthreads();
    okLidarLinear(0, pl.ldx, D, 0, 1, D, prm + at.hw0, D, prm + at.hb0, sh.h1, true, false, pl.h1_at, pl.ld1, 0);
    __syncthreads();
    okLidarLinear(pl.h1_at, pl.ld1, sh.h1, 0, 1, sh.h1, prm + at.hw1, sh.h1, prm + at.hb1, sh.h2, true, false, pl.h2_at, pl.ld2, 0);
    __syncthreads();
    if (tid >= kVitAgents || b0 + tid >= p.count)
        return;
    const long  a = p.a0 + b0 + tid;
    const float o = ok_lidar_dot(H2 + tid * pl.ld2, prm + at.hw2, sh.h2, prm[at.hb2]);
    const float steer = ok_vit_steer(o, p.steer_scale);
    p.st.thr[a]   = p.throttle;
    p.st.steer[a] = steer;
    if (p.rec.action != nullptr)
    {
        p.rec.action[2 * a]     = p.throttle;
        p.rec.action[2 * a + 1] = steer;
    }
    if (p.rec.output != nullptr)
        p.rec.output[a] = o;
    okActAlive(p.st.crashed, p.rec.alive, a);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

constexpr size_t kVitDefaultWorkspace = static_cast<size_t>(1) << 30;

inline const char *okVitCheckConfig(const okenv_vit_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_vit_shape_bad(okVitShape(*c)))
        return "shape outside the limits (patch 4, 8 or 16; image_size a multiple of patch with at most 1024 tokens; dim a multiple of 16 up to 768; "
               "dim / heads a multiple of 16 up to 64; depth 1 .. 12; dim_feedforward a multiple of 16 up to 4 dim; head_hidden1/2 multiples of 16 up "
               "to 2048)";
    if (okVitLdsBytes(okVitShape(*c)) > kLidarLdsBudget)
        return "the kernels' LDS (okenv_vit_lds_bytes) does not fit 160 KB";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(c->mean[k]) || !std::isfinite(c->std[k]) || !(c->std[k] > 0.F))
            return "mean must be finite, std finite and > 0";
    if (!std::isfinite(c->ln_eps) || !(c->ln_eps > 0.F))
        return "ln_eps must be finite and > 0";
    if (!std::isfinite(c->throttle) || !std::isfinite(c->steer_scale) || !(c->steer_scale >= 0.F))
        return "throttle must be finite, steer_scale finite and >= 0";
    if (c->agents_per_pass < 0 || c->workspace_bytes < 0)
        return "agents_per_pass and workspace_bytes must not be negative";
    return nullptr;
}

// The agents of a pass for a population of N: agents_per_pass, or as many as fit workspace_bytes (0: 1 GiB), at least one; never more
// than N.  size_t arithmetic throughout.
inline size_t okVitAgentsPerPass(const okenv_vit_config &c, const size_t N)
{
    const size_t per_agent = sizeof(float) * ok_vit_agent_floats(okVitShape(c));
    size_t       a = static_cast<size_t>(c.agents_per_pass);
    if (a == 0U)
    {
        const size_t room = c.workspace_bytes > 0 ? static_cast<size_t>(c.workspace_bytes) : kVitDefaultWorkspace;
        a = std::max<size_t>(room / per_agent, 1U);
    }
    return std::min(a, std::max<size_t>(N, 1U));
}

// nullptr, or why the workspace of `agents` agents cannot be: its rows or its bytes leave the kernels' index range
inline const char *okVitWorkspaceBad(const okenv_vit_config &c, const size_t agents)
{
    const ok_vit_shape s = okVitShape(c);
    const size_t       qtiles = (static_cast<size_t>(ok_vit_tokens(s)) + kVitQueries - 1U) / kVitQueries;
    if (agents > 0x7FFFFFFFU / (qtiles * static_cast<size_t>(s.heads)) || agents > (static_cast<size_t>(1) << 40) / ok_vit_agent_floats(s))
        return "the workspace of a pass is too large (agents_per_pass x tokens)";
    return nullptr;
}

inline void okVitActHost(const okenv_vit_config &c, const float *params, const int n, const uint8_t *frames, const uint8_t *crashed, float *throttle,
                         float *steer, float *output, float *embedding, uint8_t *alive)
{
    const ok_vit_shape  s = okVitShape(c);
    const ok_vit_consts k = okVitConsts(c);
    std::vector<float>  work(ok_vit_work_floats(s));
    const size_t        frame = static_cast<size_t>(s.S) * static_cast<size_t>(s.S) * 4U;
    for (int a = 0; a < n; ++a)
    {
        float o = 0.F;
        ok_vit_forward(s, k, params, frames + static_cast<size_t>(a) * frame, work.data(), embedding != nullptr ? embedding + static_cast<size_t>(a) * s.D : nullptr, &o);
        if (throttle != nullptr)
            throttle[a] = k.throttle;
        if (steer != nullptr)
            steer[a] = ok_vit_steer(o, k.steer_scale);
        if (output != nullptr)
            output[a] = o;
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

// okenv_debug_vit_attend on the host: qkv [seqs][T][3 D] -> ctx [seqs][T][D]
inline void okVitAttendHost(const int seqs, const int T, const int heads, const int dh, const float *qkv, float *ctx)
{
    const int          D = heads * dh;
    const float        scale = ok_lidar_scale(dh);
    std::vector<float> p(static_cast<size_t>(T));
    for (int s = 0; s < seqs; ++s)
    {
        const float *base = qkv + static_cast<size_t>(s) * T * 3U * D;
        for (int t = 0; t < T; ++t)
            for (int hd = 0; hd < heads; ++hd)
                ok_vit_attend(base + static_cast<size_t>(t) * 3U * D + hd * dh, base + D + hd * dh, base + 2 * D + hd * dh, 3L * D, T, dh, scale, p.data(),
                              ctx + (static_cast<size_t>(s) * T + t) * D + hd * dh);
    }
}

#endif // OK_VIT_H
