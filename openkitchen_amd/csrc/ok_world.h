// ok_world.h -- the world-model racers on the device: WorldModelVaeRnn's conv-VAE encoder (train_vae.py) and the
// per-candidate controller, driven as main.cpp's CmaEsAgent drives them, from the camera's RGBA8 frames to the action fields for every
// agent of a handle, and the fitness main.cpp accumulates.  The rule lives in include/okenv_world.h and is shared with okWorldActHost /
// okWorldScoreHost below, so the device and the host entries agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  All matrix work runs on v_mfma_f32_16x16x4_f32 with the accumulator
// started from the bias (the latent's partial chains: from +0.0f), k in the rule's order, four terms an instruction; B comes from the
// weights as okWorldPackKernel laid them out at set_params (ok_conv.h's layout and group step).
//   okWorldListKernel       the agents an act works for, in ascending order, and their number: all of them, or (skip_crashed) those not
//                           crashed.  Everything behind it works on list slots, so a crashed agent costs nothing.
//   okWorldConvKernel<F>    one convolution as an implicit GEMM whose rows are the output pixels of ALL listed frames, one after the other
//                           (a tile of 64 rows spans frames where a frame has fewer), columns the output channels, 128 to a workgroup of
//                           8 waves; K blocked by (tap, chunk of up to 64 input channels) in the chain's own order: the block's A tile is
//                           gathered into LDS (padding taps as 0.0f), a wave carries 4 row tiles of one column tile through it with B
//                           straight from L2.  No split-K: one chain per output.  F: layer 0, whose whole chain (16 taps of R, G, B and the
//                           alpha slot) is one block gathered from the frames' bytes.  Activations are channels-last in global memory.
//   okWorldLatentKernel     fc_mu's partial chains: a workgroup owns 16 list slots and one position, a wave 16 latents.
//   okWorldHeadKernel       a wave per list slot: the partial chains joined in the rule's order, the state, the controller (okCtrlLayer,
//                           the agent's own parameters) and the action.
//   okWorldScoreKernel      a thread per agent: main.cpp:329-342.
#ifndef OK_WORLD_H
#define OK_WORLD_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_world.h"
#include "ok_conv.h"
#include "ok_lidar.h"
#include "okenv_kernels.h"

constexpr int    kWorldThreads   = 512; // 8 waves
constexpr int    kWorldWaves     = kWorldThreads / 64;
constexpr int    kWorldRowBlock  = 4;                   // row tiles a wave carries through a K block
constexpr int    kWorldRows      = 16 * kWorldRowBlock; // rows of a workgroup's tile
constexpr int    kWorldCols      = 16 * kWorldWaves;    // columns of a workgroup's tile
constexpr int    kWorldChunk     = 64;                  // input channels of a K block
constexpr int    kWorldLda       = kWorldChunk + 2;     // floats between the A tile's rows: 2 mod 32, so that the 16 rows and the two
                                                        // k's of a ds_read_b32's 32 lanes fall on 32 banks; even for 8-byte stores
constexpr int    kWorldAgents    = 16;                  // list slots per workgroup of the latent kernel: the rows of one MFMA tile
constexpr int    kWorldHeadSlots = 4;                   // list slots per workgroup of the head kernel, a wave each
constexpr size_t kWorldLdsBudget = 160U * 1024U;

__host__ __device__ inline ok_world_shape okWorldShape(const okenv_world_config &c)
{
    ok_world_shape s;
    s.S = c.image_size;
    for (int l = 0; l < 4; ++l)
        s.c[l] = c.channels[l];
    s.Z = c.latent;
    s.h = c.hidden;
    return s;
}

// Where the packed matrices begin, in floats (0 .. 3 the convolutions, 4 fc_mu), and the workspace of N agents, in 4-byte words:
// [pack | controllers | act0 .. act3 | part | fitness | list | count]
struct OkWorldPlaces
{
    int    pack[5], pack_total;
    size_t ctrl, act[4], part, fitness, list, count, words;
};

// Groups of 16 k's in a matrix's chain: layer 0 has 4 k's a tap (R, G, B and the alpha slot)
__host__ __device__ inline int okWorldGroups(const ok_world_shape s, const int l)
{
    return l == 0 ? 4 : (l == 4 ? ok_world_features(s) / 16 : s.c[l - 1]);
}

__host__ __device__ inline OkWorldPlaces okWorldPlaces(const ok_world_shape s, const size_t N)
{
    OkWorldPlaces at;
    int           o = 0;
    for (int l = 0; l < 5; ++l)
    {
        at.pack[l] = o;
        o += okWorldGroups(s, l) * (l == 4 ? s.Z : s.c[l]) * 16;
    }
    at.pack_total = o;
    size_t w      = static_cast<size_t>(o);
    at.ctrl       = w;
    w += N * static_cast<size_t>(ok_world_controller_params(s));
    w = (w + 3U) & ~static_cast<size_t>(3U); // (the activations are read 16 bytes at a time)
    for (int l = 0; l < 4; ++l)
    {
        at.act[l] = w;
        w += N * static_cast<size_t>(ok_world_side(s, l) * ok_world_side(s, l)) * static_cast<size_t>(s.c[l]);
    }
    at.part = w;
    w += N * static_cast<size_t>(ok_world_side(s, 3) * ok_world_side(s, 3)) * static_cast<size_t>(s.Z);
    at.fitness = w;
    w += N;
    at.list = w;
    w += N;
    at.count = w;
    at.words = w + 1U;
    return at;
}

// The larger kernel's dynamic LDS: the conv kernels' A tile or the latent kernel's 16 rows of c3 + 2 floats
inline size_t okWorldLdsBytes(const ok_world_shape s)
{
    if (ok_world_shape_bad(s))
        return 0U;
    return sizeof(float) * static_cast<size_t>(okLidarMax(kWorldRows * kWorldLda, kWorldAgents * (s.c[3] + 2)));
}

// What names a layer's path through okWorldConvKernel: the workgroups its columns take (a last one with idle waves where c_l is no
// multiple of 128), the K blocks per tap (0: layer 0, whose whole chain is one block) and the channels of a tap's last block
inline void okWorldPlan(const ok_world_shape s, int32_t *plan)
{
    for (int l = 0; l < 4; ++l)
    {
        const int Cin   = ok_world_cin(s, l);
        plan[3 * l]     = (s.c[l] + kWorldCols - 1) / kWorldCols;
        plan[3 * l + 1] = l == 0 ? 0 : (Cin + kWorldChunk - 1) / kWorldChunk;
        plan[3 * l + 2] = l == 0 ? 64 : Cin - (plan[3 * l + 1] - 1) * kWorldChunk;
    }
}

// ---- the weights as the kernels read them ----------------------------------------------------------------------------------------------

// ok_conv.h's layout, k the place in the rule's chain: the convolutions' k = tap * Cin' + ch (tap = 4 ty + tx; Cin' = Cin, layer 0: 4),
// fc_mu's k = p * c3 + ch.  Layer 0's alpha slot is 0.0f.
struct OkWorldPackParams
{
    ok_world_shape s;
    const float   *params;
    float         *pack;
};

__global__ __launch_bounds__(256) void okWorldPackKernel(const OkWorldPackParams p)
{
    const ok_world_layout at = ok_world_offsets(p.s);
    const OkWorldPlaces   pl = okWorldPlaces(p.s, 0U);
    const int             e  = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= pl.pack_total)
        return;
    // (no array indexed by l: it would live in scratch)
    const int l    = e >= pl.pack[4] ? 4 : (e >= pl.pack[3] ? 3 : (e >= pl.pack[2] ? 2 : (e >= pl.pack[1] ? 1 : 0)));
    const int base = l == 4 ? pl.pack[4] : (l == 3 ? pl.pack[3] : (l == 2 ? pl.pack[2] : (l == 1 ? pl.pack[1] : 0)));
    const int Cout = l == 4 ? p.s.Z : (l == 3 ? p.s.c[3] : (l == 2 ? p.s.c[2] : (l == 1 ? p.s.c[1] : p.s.c[0])));
    const auto [n, kk] = okConvPackAt(e - base, Cout);
    float      v       = 0.F;
    if (l == 0)
    {
        const int tap = kk >> 2, ch = kk & 3;
        if (ch < 3)
            v = p.params[at.w[0] + (n * 3 + ch) * 16 + tap];
    }
    else if (l == 4)
    {
        const int c3 = p.s.c[3], P = ok_world_side(p.s, 3) * ok_world_side(p.s, 3), pos = kk / c3, ch = kk - pos * c3;
        v = p.params[at.mw + n * (c3 * P) + ch * P + pos];
    }
    else
    {
        const int Cin = l == 3 ? p.s.c[2] : (l == 2 ? p.s.c[1] : p.s.c[0]);
        v = p.params[(l == 3 ? at.w[3] : (l == 2 ? at.w[2] : at.w[1])) + okConvWeightAt(n, kk, Cin, 16)];
    }
    p.pack[e] = v;
}

// ---- the list ---------------------------------------------------------------------------------------------------------------------------

// list[0 .. count) = the agents an act works for, ascending.  One workgroup of 256: a ballot and two sums per 256 agents, nothing that
// depends on scheduling.
__global__ __launch_bounds__(256) void okWorldListKernel(const uint8_t *crashed, const int N, const int skip_crashed, int *list, int *count)
{
    __shared__ int sums[4];
    const int      tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    int            base = 0; // (the same in every thread)
    for (int a0 = 0; a0 < N; a0 += 256)
    {
        const int                a    = a0 + tid;
        const bool               keep = a < N && !(skip_crashed != 0 && crashed[a] != 0);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0)
            sums[wave] = __popcll(mask);
        __syncthreads();
        int before = base, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
        {
            before += w < wave ? sums[w] : 0;
            all += sums[w];
        }
        if (keep)
            list[before + __popcll(mask & ((1ULL << lane) - 1ULL))] = a;
        base += all;
        __syncthreads();
    }
    if (tid == 0)
        *count = base;
}

// ---- the convolutions ------------------------------------------------------------------------------------------------------------------

// One layer: the input [slot][S][S][Cin] floats, channels last (kFirst: the frames' bytes, frame list[slot]), the output
// [slot][side][side][Cout], side = S / 2; w the layer's packed weights, bias its bias.
struct OkWorldConvJob
{
    const uint8_t *frames;
    const float   *in;
    float         *out;
    const float   *w, *bias;
    const int     *list, *count;
    int            S, side, Cin, Cout;
};

// Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; accumulator register r is D[row 4 (l >> 4) + r][col l & 15]
// (ok_lidar.h).  Rows past the last listed frame are gathered as 0.0f and not stored.  A wave whose column tile lies past Cout takes
// part in the gathers and barriers only.
template <bool kFirst>
__global__ __launch_bounds__(kWorldThreads) void okWorldConvKernel(const OkWorldConvJob j)
{
    constexpr int  RB = kWorldRowBlock;
    __shared__ int rows[kWorldRows * 3]; // per row: its frame (kFirst) or list slot, -1 past the end; the input pixel of tap (0, 0)
    const int      tid = static_cast<int>(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
    const int      P = j.side * j.side, M = j.count[0] * P, m0 = static_cast<int>(blockIdx.x) * kWorldRows;
    if (m0 >= M)
        return; // (the whole workgroup: the grid is sized for every agent)
    if (tid < kWorldRows)
    {
        const int m = m0 + tid, f = m / P, pos = m - f * P, oy = pos / j.side, ox = pos - oy * j.side;
        rows[3 * tid]     = m < M ? (kFirst ? j.list[f] : f) : -1;
        rows[3 * tid + 1] = 2 * oy - 1;
        rows[3 * tid + 2] = 2 * ox - 1;
    }
    __syncthreads();

    const int  ct = static_cast<int>(blockIdx.y) * kWorldWaves + wave, Nt = j.Cout >> 4, n0 = (ct < Nt ? ct : 0) << 4;
    const bool live = ct < Nt;
    okLidarAcc acc[RB];
#pragma unroll
    for (int m = 0; m < RB; ++m)
    {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[m][r] = j.bias[n0 + i];
    }
    const float4 *wp = reinterpret_cast<const float4 *>(j.w) + (n0 + i) * 4 + g;
    const int     gstride = j.Cout * 4; // float4's between groups
    const int     S = j.S, Cin = j.Cin;
    const int     blocks = kFirst ? 1 : 16 * ((Cin + kWorldChunk - 1) / kWorldChunk);
    int           tap = 0, c0 = 0, gbase = 0;
    for (int b = 0; b < blocks; ++b)
    {
        const int kc = kFirst ? 64 : okLidarMin(kWorldChunk, Cin - c0), ngrp = kc >> 4;
        // the block's weights first: they are on their way while the tile is gathered
        float4 bv[4];
#pragma unroll
        for (int grp = 0; grp < 4; ++grp)
            bv[grp] = wp[static_cast<size_t>(gbase + (grp < ngrp ? grp : 0)) * gstride];
        if constexpr (kFirst)
        {
            const uint32_t *frames = reinterpret_cast<const uint32_t *>(j.frames);
            for (int e = tid; e < kWorldRows * 16; e += kWorldThreads)
            {
                const int  row = e >> 4, t = e & 15, a = rows[3 * row], y = rows[3 * row + 1] + (t >> 2), x = rows[3 * row + 2] + (t & 3);
                const bool inside = a >= 0 && y >= 0 && y < S && x >= 0 && x < S;
                const uint32_t rgba = inside ? frames[(static_cast<size_t>(a) * S + y) * S + x] : 0U;
                float2 *d = reinterpret_cast<float2 *>(ok_actor_lds + row * kWorldLda + 4 * t);
                d[0] = make_float2(ok_bev_pixel(static_cast<uint8_t>(rgba)), ok_bev_pixel(static_cast<uint8_t>(rgba >> 8)));
                d[1] = make_float2(ok_bev_pixel(static_cast<uint8_t>(rgba >> 16)), 0.F);
            }
        }
        else
        {
            const int kc4 = kc >> 2, ty = tap >> 2, tx = tap & 3;
            for (int e = tid; e < kWorldRows * kc4; e += kWorldThreads)
            {
                const int  row = e / kc4, c4 = e - row * kc4, f = rows[3 * row], y = rows[3 * row + 1] + ty, x = rows[3 * row + 2] + tx;
                const bool inside = f >= 0 && y >= 0 && y < S && x >= 0 && x < S;
                float4     v = make_float4(0.F, 0.F, 0.F, 0.F);
                if (inside)
                    v = *reinterpret_cast<const float4 *>(j.in + ((static_cast<size_t>(f) * S + y) * S + x) * Cin + c0 + 4 * c4);
                float2 *d = reinterpret_cast<float2 *>(ok_actor_lds + row * kWorldLda + 4 * c4);
                d[0] = make_float2(v.x, v.y);
                d[1] = make_float2(v.z, v.w);
            }
        }
        __syncthreads();
        if (live)
        {
#pragma unroll
            for (int grp = 0; grp < 4; ++grp)
            {
                if (grp < ngrp)
                {
                    float a[4][RB];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                    {
#pragma unroll
                        for (int m = 0; m < RB; ++m)
                            a[q][m] = ok_actor_lds[(16 * m + i) * kWorldLda + 16 * grp + 4 * q + g];
                    }
                    okConvMfma(a, bv[grp], acc);
                }
            }
        }
        __syncthreads();
        gbase += ngrp;
        c0 += kc;
        if (c0 >= Cin)
            c0 = 0, ++tap;
    }
    if (!live)
        return;
#pragma unroll
    for (int m = 0; m < RB; ++m)
    {
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const int row = m0 + 16 * m + 4 * g + r;
            if (row < M)
                j.out[static_cast<size_t>(row) * j.Cout + n0 + i] = ok_lidar_relu(acc[m][r]);
        }
    }
}

// ---- fc_mu's partial chains ------------------------------------------------------------------------------------------------------------

// act3 [slot][P][C], w fc_mu's packed weights (k = p C + ch), part [slot][P][Z].  Grid (slots / 16, P), Z / 16 waves.  Rows of a
// partial last workgroup repeat the last slot and are not stored.
struct OkWorldLatentJob
{
    const float *act3, *w;
    float       *part;
    const int   *count;
    int          P, C, Z;
};

__global__ __launch_bounds__(kWorldThreads) void okWorldLatentKernel(const OkWorldLatentJob j)
{
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4, n0 = (tid >> 6) << 4;
    const int count = j.count[0], a0 = static_cast<int>(blockIdx.x) * kWorldAgents, p = static_cast<int>(blockIdx.y);
    if (a0 >= count)
        return;
    const int C = j.C, lda = C + 2, c4n = C >> 2;
    for (int e = tid; e < kWorldAgents * c4n; e += static_cast<int>(blockDim.x))
    {
        const int    r = e / c4n, c4 = e - r * c4n, slot = okLidarMin(a0 + r, count - 1);
        const float4 v = *reinterpret_cast<const float4 *>(j.act3 + (static_cast<size_t>(slot) * j.P + p) * C + 4 * c4);
        float2      *d = reinterpret_cast<float2 *>(ok_actor_lds + r * lda + 4 * c4);
        d[0] = make_float2(v.x, v.y);
        d[1] = make_float2(v.z, v.w);
    }
    __syncthreads();
    okLidarAcc    acc = {0.F, 0.F, 0.F, 0.F};
    const float4 *wp = reinterpret_cast<const float4 *>(j.w) + (n0 + i) * 4 + g;
    const int     gstride = j.Z * 4, groups = C >> 4;
    for (int grp = 0; grp < groups; ++grp)
    {
        const float4 bv = wp[static_cast<size_t>(p * groups + grp) * gstride];
        float        a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            a[q] = ok_actor_lds[i * lda + 16 * grp + 4 * q + g];
        okConvMfma(a, bv, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
    {
        const int slot = a0 + 4 * g + r;
        if (slot < count)
            j.part[(static_cast<size_t>(slot) * j.P + p) * j.Z + n0 + i] = acc[r];
    }
}

// ---- the head ---------------------------------------------------------------------------------------------------------------------------

struct OkWorldHeadParams
{
    OkDeviceState      st;
    ok_world_shape     s;
    const float       *enc, *ctrl, *part;
    const int         *list, *count;
    float              throttle, steer_scale;
    okenv_world_record rec;
};

// A wave per list slot.  Lane l holds the state's entries l, l + 64 and l + 128 (okCtrlLayer's input layout with a group of 64).
__global__ __launch_bounds__(64 * kWorldHeadSlots) void okWorldHeadKernel(const OkWorldHeadParams p)
{
    const int lane = static_cast<int>(threadIdx.x) & 63, slot = static_cast<int>(blockIdx.x) * kWorldHeadSlots + (static_cast<int>(threadIdx.x) >> 6);
    if (slot >= p.count[0])
        return; // (the whole wave)
    const ok_world_layout at = ok_world_offsets(p.s);
    const int             Z = p.s.Z, h = p.s.h, h2 = h / 2, in = Z + 2, P = ok_world_side(p.s, 3) * ok_world_side(p.s, 3);
    const long            a = p.list[slot];
    float                 sn, cs;
    ok_sincosf(p.st.rot[a], &sn, &cs); // the stored degrees, as the reference passes them (okenv_world.h)
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const int e = lane + 64 * k;
        float     v = e == Z ? sn : (e == Z + 1 ? cs : 0.F);
        if (e < Z)
        {
            v = p.enc[at.mb + e];
            for (int q = 0; q < P; ++q)
                v = v + p.part[(static_cast<size_t>(slot) * P + q) * Z + e];
            if (p.rec.mu != nullptr)
                p.rec.mu[a * Z + e] = v;
        }
        if (e < in && p.rec.state != nullptr)
            p.rec.state[a * in + e] = v;
        x[k] = v;
    }
    const float *w1 = p.ctrl + a * ok_world_controller_params(p.s), *b1 = w1 + h * in, *w2 = b1 + h, *b2 = w2 + h2 * h, *w3 = b2 + h2, *b3 = w3 + h2;
    float        a1[1], a2[1], a3[1];
    okCtrlLayer<8>(a1, x, w1, b1, in, h, lane, 64);
    a1[0] = lane < h ? ok_tanhf(a1[0]) : 0.F;
    okCtrlLayer<8>(a2, a1, w2, b2, h, h2, lane, 64);
    a2[0] = lane < h2 ? ok_tanhf(a2[0]) : 0.F;
    okCtrlLayer<8>(a3, a2, w3, b3, h2, 1, lane, 64);
    if (lane != 0)
        return;
    const float y = ok_tanhf(a3[0]), steer = y * p.steer_scale;
    p.st.thr[a]   = p.throttle;
    p.st.steer[a] = steer;
    if (p.rec.out != nullptr)
        p.rec.out[a] = y;
    if (p.rec.action != nullptr)
    {
        p.rec.action[2 * a]     = p.throttle;
        p.rec.action[2 * a + 1] = steer;
    }
    okActAlive(p.st.crashed, p.rec.alive, a);
}

// ---- the score --------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void okWorldScoreKernel(const OkDeviceState st, const int N, const float *cx, const float *cy, const float *w_left,
                                                          const float *w_right, const int P, float *fitness)
{
    const int a = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (a >= N)
        return;
    fitness[a] = ok_world_score(fitness[a], st.crashed[a], st.timed_out[a], cx, cy, w_left, w_right, P, st.pos_x[a], st.pos_y[a]);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okWorldCheckConfig(const okenv_world_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_world_shape_bad(okWorldShape(*c)))
        return "shape outside the limits (image_size a multiple of 16 in 16 .. 128; channels multiples of 16 in 16 .. 512; latent a "
               "multiple of 16 in 16 .. 128; at most 32768 features; hidden even in 2 .. 64)";
    if (okWorldLdsBytes(okWorldShape(*c)) > kWorldLdsBudget)
        return "the kernels' LDS (okenv_world_lds_bytes) does not fit 160 KB";
    if (!std::isfinite(c->throttle) || !std::isfinite(c->steer_scale))
        return "throttle / steer_scale must be finite";
    if (c->skip_crashed != 0 && c->skip_crashed != 1)
        return "skip_crashed must be 0 or 1";
    return nullptr;
}

// The action of n agents on host arrays; every output may be nullptr.  With skip_crashed the entries of crashed agents are left as they are.
inline void okWorldActHost(const okenv_world_config &c, const float *encoder, const float *controllers, const int n, const uint8_t *frames,
                           const float *rot, const uint8_t *crashed, float *mu, float *state, float *out, float *throttle, float *steer,
                           uint8_t *alive)
{
    const ok_world_shape s = okWorldShape(c);
    std::vector<float>   work(static_cast<size_t>(ok_world_work_floats(s))), x(static_cast<size_t>(s.Z) + 2U);
    const size_t         frame = static_cast<size_t>(s.S) * s.S * 4U, cp = static_cast<size_t>(ok_world_controller_params(s));
    for (int a = 0; a < n; ++a)
    {
        const bool gone = crashed != nullptr && crashed[a] != 0;
        if (gone && c.skip_crashed != 0)
            continue;
        float y = 0.F;
        ok_world_forward(s, encoder, controllers + a * cp, frames + a * frame, rot[a], work.data(), x.data(), &y);
        if (mu != nullptr)
            std::copy(x.begin(), x.begin() + s.Z, mu + static_cast<size_t>(a) * s.Z);
        if (state != nullptr)
            std::copy(x.begin(), x.end(), state + static_cast<size_t>(a) * (s.Z + 2));
        if (out != nullptr)
            out[a] = y;
        if (throttle != nullptr)
            throttle[a] = c.throttle;
        if (steer != nullptr)
            steer[a] = y * c.steer_scale;
        if (alive != nullptr)
            alive[a] = gone ? 0 : 1;
    }
}

inline void okWorldScoreHost(const float *cx, const float *cy, const float *w_left, const float *w_right, const int P, const int n, const float *x,
                             const float *y, const uint8_t *crashed, const uint8_t *timed_out, float *fitness)
{
    for (int a = 0; a < n; ++a)
        fitness[a] = ok_world_score(fitness[a], crashed[a], timed_out[a], cx, cy, w_left, w_right, P, x[a], y[a]);
}

#endif // OK_WORLD_H
