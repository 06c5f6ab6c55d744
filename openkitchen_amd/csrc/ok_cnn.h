// ok_cnn.h -- the behavioural-cloning image policy on the device: BehavioralCloning's PolicyCNN (env_train_bc.py)
// driven as main.cpp drives it, from the camera's RGBA8 frames to the action fields, for every agent of a handle.  The rule lives in
// include/okenv_cnn.h (ok_bev_pixel, ok_cnn_conv_at, ok_cnn_hidden_at, ok_cnn_action on top of ok_lidar_dot) and is shared with
// okCnnActHost below, so the device and the host entry agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  All matrix work runs on v_mfma_f32_16x16x4_f32 with the accumulator
// started from the bias: rows are output pixels (the convolutions) or agents (the hidden layer), columns output channels, k runs over
// the rule's chain, four terms an instruction; B comes from the weights as okCnnPackKernel laid them out at set_params.
//   okCnnConvKernel     one frame per workgroup of 8 waves.  The frame's bytes, layer 0's output and layer 1's output live in LDS
//                       (channels last; the frame's room is layer 1's once layer 0 is done); layer 2 writes the [N][F] features,
//                       channels last, to global memory.  No layer is tiled: a valid convolution of a whole frame has no halo.
//   okCnnHeadKernel<CT> 16 agents per workgroup of 8 waves: the hidden layer as a GEMM whose rows are agents, the features staged
//                       through LDS 256 k's at a time, a wave owning CT tiles of 16 columns; then the output layer, the tanh and the
//                       action, one agent per thread.  Rows of a partial last workgroup repeat the last agent and are never stored.
#ifndef OK_CNN_H
#define OK_CNN_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_cnn.h"
#include "ok_lidar.h"

constexpr int    kCnnThreads   = 512; // 8 waves
constexpr int    kCnnWaves     = kCnnThreads / 64;
constexpr int    kCnnRowBlock  = 2;   // row tiles a wave carries through one pass over a weight tile
constexpr int    kCnnAgents    = 16;  // agents per workgroup of the head: the rows of one MFMA tile
constexpr int    kCnnChunk     = 256; // features the head stages at a time
constexpr int    kCnnMaxColTiles = OK_CNN_MAX_HIDDEN / 16 / kCnnWaves; // 4
constexpr size_t kCnnLdsBudget = 160U * 1024U;

__host__ __device__ inline ok_cnn_shape okCnnShape(const okenv_cnn_config &c)
{
    ok_cnn_shape s;
    s.S = c.image_size;
    for (int l = 0; l < 3; ++l)
    {
        s.k[l] = c.kernel[l];
        s.s[l] = c.stride[l];
        s.c[l] = c.channels[l];
    }
    s.H = c.hidden;
    return s;
}

// Groups of 16 k's in a chain: layer 0 has 4 k's a tap (R, G, B and the alpha slot) and filler taps up to a whole group; l = 3 is the
// hidden layer
__host__ __device__ inline int okCnnGroups(const ok_cnn_shape s, const int l)
{
    if (l == 0)
        return (s.k[0] * s.k[0] + 3) / 4;
    return l == 3 ? ok_cnn_features(s) / 16 : s.k[l] * s.k[l] * s.c[l - 1] / 16;
}

// The conv kernel's LDS, in floats: [lut | p | q].  lut: ok_bev_pixel of the 256 bytes.  p: the frame, S x S words of four bytes, and
// behind layer 0 layer 1's output, side_1^2 pixels of c1 + 1 floats.  q: layer 0's output, side_0^2 pixels of c0 + 1 floats (odd: the
// 16 pixels of an MFMA tile start on different banks).  The head's: [tile | hid], 16 rows of kCnnChunk + 4 and of H + 4 floats.
struct OkCnnPlaces
{
    int side[3], ld0, ld1, p, q, conv_end;
    int region; // what sizes p: 0 the frame, 1 layer 1's output
    int ct, ldt, ldh, hid, head_end;
    int pack[4], pack_total; // where each layer's packed weights begin, in floats (3: the hidden layer)
};

__host__ __device__ inline OkCnnPlaces okCnnPlaces(const ok_cnn_shape s)
{
    OkCnnPlaces at;
    for (int l = 0; l < 3; ++l)
        at.side[l] = ok_cnn_side(s, l);
    at.ld0 = s.c[0] + 1;
    at.ld1 = s.c[1] + 1;
    const int frame = s.S * s.S, out1 = at.side[1] * at.side[1] * at.ld1;
    at.region   = out1 > frame ? 1 : 0;
    at.p        = 256;
    at.q        = at.p + okLidarMax(frame, out1);
    at.conv_end = at.q + at.side[0] * at.side[0] * at.ld0;
    at.ct       = (s.H / 16 + kCnnWaves - 1) / kCnnWaves;
    at.ldt      = kCnnChunk + 4;
    at.ldh      = s.H + 4;
    at.hid      = kCnnAgents * at.ldt;
    at.head_end = at.hid + kCnnAgents * at.ldh;
    int o = 0;
    for (int l = 0; l < 4; ++l)
    {
        at.pack[l] = o;
        o += okCnnGroups(s, l) * (l == 3 ? s.H : s.c[l]) * 16;
    }
    at.pack_total = o;
    return at;
}

inline size_t okCnnLdsBytes(const ok_cnn_shape s)
{
    if (ok_cnn_shape_bad(s))
        return 0U;
    const OkCnnPlaces at = okCnnPlaces(s);
    return sizeof(float) * static_cast<size_t>(okLidarMax(at.conv_end, at.head_end));
}

// ---- the weights as the kernels read them ----------------------------------------------------------------------------------------------

// A layer's B matrix [K][Cout] in groups of 16 k's, k the place in the rule's chain: the convolutions' k = tap * Cin' + ch
// (tap = ty * k + tx; Cin' = Cin, layer 0: 4), the hidden layer's k = (y * side_2 + x) * c2 + ch:
// pack[((k / 16) * Cout + n) * 16 + (k % 4) * 4 + (k % 16) / 4] -- the four floats a lane (column n, k-lane g = k % 4) feeds to the four
// instructions of a group lie side by side, one 16-byte load, and a wave's 64 loads are 1 KB in a row.  Layer 0's alpha slot and
// filler taps are 0.0f.
struct OkCnnPackParams
{
    ok_cnn_shape s;
    const float *params;
    float       *pack;
};

__global__ __launch_bounds__(256) void okCnnPackKernel(const OkCnnPackParams p)
{
    const ok_cnn_layout at = ok_cnn_offsets(p.s);
    const OkCnnPlaces   pl = okCnnPlaces(p.s);
    const int           e  = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= pl.pack_total)
        return;
    const int l    = e >= pl.pack[3] ? 3 : (e >= pl.pack[2] ? 2 : (e >= pl.pack[1] ? 1 : 0));
    const int base = l == 3 ? pl.pack[3] : (l == 2 ? pl.pack[2] : (l == 1 ? pl.pack[1] : 0)); // (no array indexed by l: it would live in scratch)
    const int Cout = l == 3 ? p.s.H : (l == 2 ? p.s.c[2] : (l == 1 ? p.s.c[1] : p.s.c[0]));
    const int idx = e - base, grp = idx / (Cout * 16), rem = idx - grp * Cout * 16, n = rem >> 4, g = (rem & 15) >> 2, q = rem & 3;
    const int kk = grp * 16 + 4 * q + g;
    float     v  = 0.F;
    if (l == 0)
    {
        const int taps = p.s.k[0] * p.s.k[0], tap = kk >> 2, ch = kk & 3;
        if (tap < taps && ch < 3)
            v = p.params[at.w[0] + (n * 3 + ch) * taps + tap];
    }
    else if (l == 3)
    {
        const int c2 = p.s.c[2], P = pl.side[2] * pl.side[2], pos = kk / c2, ch = kk - pos * c2;
        v = p.params[at.hw + n * (c2 * P) + ch * P + pos];
    }
    else
    {
        const int Cin = l == 2 ? p.s.c[1] : p.s.c[0], k = l == 2 ? p.s.k[2] : p.s.k[1], tap = kk / Cin, ch = kk - tap * Cin;
        v = p.params[(l == 2 ? at.w[2] : at.w[1]) + (n * Cin + ch) * k * k + tap];
    }
    p.pack[e] = v;
}

// ---- the convolution piece -------------------------------------------------------------------------------------------------------------

// One convolution of a whole image: M output pixels, W to a row, times Cout channels.  Input pixel (y, x) lies in LDS at
// in + y * rs + x * ps, its channel ch at + ch (kFirst: one word of four bytes); the output pixel (oy, ox) reads the input pixels
// (stride oy + ty, stride ox + tx), all of them inside the input.  Output pixel number `row` goes to out + row * ldo + channel, LDS or
// global.
struct OkCnnConvJob
{
    int          in, ps, rs, k, stride, Cin, W, M, Cout;
    const float *w, *bias; // packed weights of the layer, its bias
    float       *out;
    int          ldo;
};

// A wave owns 16 columns and kCnnRowBlock row tiles of 16 pixels at a time.  Lane l holds A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15]; accumulator register r is D[row 4 (l >> 4) + r][col l & 15] (ok_lidar.h).  Rows past M repeat the last
// pixel and are not stored.  kFirst: layer 0 -- a k-step is one tap, lane group g reads byte g of the pixel (3: the alpha byte against
// the alpha slot's 0.0f) through the table of ok_bev_pixel at the start of LDS; the filler taps read the last tap.
template <bool kFirst>
__device__ __forceinline__ void okCnnConv(const OkCnnConvJob &j)
{
    constexpr int RB = kCnnRowBlock;
    const int lane = static_cast<int>(threadIdx.x) & 63, i = lane & 15, g = lane >> 4, wave = static_cast<int>(threadIdx.x) >> 6;
    const int Nt = j.Cout >> 4, Mb = (j.M + 16 * RB - 1) / (16 * RB), units = Nt * Mb;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(ok_actor_lds);
    for (int u = wave; u < units; u += kCnnWaves)
    {
        const int  mb = u / Nt, n0 = (u - mb * Nt) << 4;
        int        abase[RB];
        okLidarAcc acc[RB];
#pragma unroll
        for (int m = 0; m < RB; ++m)
        {
            const int row = okLidarMin((mb * RB + m) * 16 + i, j.M - 1), oy = row / j.W, ox = row - oy * j.W;
            abase[m]      = j.in + j.stride * oy * j.rs + j.stride * ox * j.ps + (kFirst ? 0 : g);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[m][r] = j.bias[n0 + i];
        }
        const float4 *wp = reinterpret_cast<const float4 *>(j.w) + (n0 + i) * 4 + g;
        const int     gstride = j.Cout * 4; // float4's between groups
        int           ty = 0, tx = 0, c0 = 0;
        if constexpr (kFirst)
        {
            const int groups = (j.k * j.k + 3) >> 2;
            for (int grp = 0; grp < groups; ++grp)
            {
                const float4 bv = wp[grp * gstride];
                float        a[4][RB];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
                    const int toff = ty * j.rs + tx * j.ps;
#pragma unroll
                    for (int m = 0; m < RB; ++m)
                        a[q][m] = ok_actor_lds[(words[abase[m] + toff] >> (8 * g)) & 255U];
                    if (ty != j.k - 1 || tx != j.k - 1) // (the filler taps stay on the last tap)
                        if (++tx == j.k)
                            tx = 0, ++ty;
                }
                const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
#pragma unroll
                    for (int m = 0; m < RB; ++m)
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][m], b[q], acc[m], 0, 0, 0);
                }
            }
        }
        else
        {
            // group grp = (tap (ty, tx), channels c0 .. c0 + 15)
            const int groups = j.k * j.k * (j.Cin >> 4);
            for (int grp = 0; grp < groups; ++grp)
            {
                const float4 bv   = wp[grp * gstride];
                const int    toff = ty * j.rs + tx * j.ps + c0;
                float        a[4][RB];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
#pragma unroll
                    for (int m = 0; m < RB; ++m)
                        a[q][m] = ok_actor_lds[abase[m] + toff + 4 * q];
                }
                const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
#pragma unroll
                    for (int m = 0; m < RB; ++m)
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][m], b[q], acc[m], 0, 0, 0);
                }
                c0 += 16;
                if (c0 == j.Cin)
                {
                    c0 = 0;
                    if (++tx == j.k)
                        tx = 0, ++ty;
                }
            }
        }
#pragma unroll
        for (int m = 0; m < RB; ++m)
        {
#pragma unroll
            for (int r = 0; r < 4; ++r)
            {
                const int row = (mb * RB + m) * 16 + 4 * g + r;
                if (row < j.M)
                    j.out[static_cast<long>(row) * j.ldo + n0 + i] = ok_lidar_relu(acc[m][r]);
            }
        }
    }
}

struct OkCnnActParams
{
    OkDeviceState    st;
    int              N;
    ok_cnn_shape     s;
    const uint8_t   *frames; // [N][S][S][4]
    const float     *params, *pack;
    float           *feat; // layer 2's output, [N][side_2][side_2][c2]: the features in the hidden layer's chain order
    float            throttle, steer_scale;
    okenv_cnn_record rec;
};

__global__ __launch_bounds__(kCnnThreads) void okCnnConvKernel(const OkCnnActParams p)
{
    const ok_cnn_shape  sh = p.s;
    const ok_cnn_layout at = ok_cnn_offsets(sh);
    const OkCnnPlaces   pl = okCnnPlaces(sh);
    const int           S = sh.S, tid = static_cast<int>(threadIdx.x);
    const size_t        n = blockIdx.x;

    if (tid < 256)
        ok_actor_lds[tid] = ok_bev_pixel(static_cast<uint8_t>(tid));
    const uint32_t *frame = reinterpret_cast<const uint32_t *>(p.frames) + n * static_cast<size_t>(S * S);
    uint32_t       *words = reinterpret_cast<uint32_t *>(ok_actor_lds) + pl.p;
    for (int e = tid; e < S * S; e += kCnnThreads)
        words[e] = frame[e];
    __syncthreads();

    OkCnnConvJob j;
    j.in = pl.p, j.ps = 1, j.rs = S, j.k = sh.k[0], j.stride = sh.s[0], j.Cin = 4, j.W = pl.side[0], j.M = pl.side[0] * pl.side[0], j.Cout = sh.c[0];
    j.w = p.pack + pl.pack[0], j.bias = p.params + at.b[0];
    j.out = ok_actor_lds + pl.q, j.ldo = pl.ld0;
    okCnnConv<true>(j);
    __syncthreads();

    j.in = pl.q, j.ps = pl.ld0, j.rs = pl.side[0] * pl.ld0, j.k = sh.k[1], j.stride = sh.s[1], j.Cin = sh.c[0], j.W = pl.side[1];
    j.M = pl.side[1] * pl.side[1], j.Cout = sh.c[1];
    j.w = p.pack + pl.pack[1], j.bias = p.params + at.b[1];
    j.out = ok_actor_lds + pl.p, j.ldo = pl.ld1;
    okCnnConv<false>(j);
    __syncthreads();

    j.in = pl.p, j.ps = pl.ld1, j.rs = pl.side[1] * pl.ld1, j.k = sh.k[2], j.stride = sh.s[2], j.Cin = sh.c[1], j.W = pl.side[2];
    j.M = pl.side[2] * pl.side[2], j.Cout = sh.c[2];
    j.w = p.pack + pl.pack[2], j.bias = p.params + at.b[2];
    j.out = p.feat + n * static_cast<size_t>(j.M * sh.c[2]), j.ldo = sh.c[2];
    okCnnConv<false>(j);
}

template <int CT>
__global__ __launch_bounds__(kCnnThreads) void okCnnHeadKernel(const OkCnnActParams p)
{
    const ok_cnn_shape  sh = p.s;
    const ok_cnn_layout at = ok_cnn_offsets(sh);
    const OkCnnPlaces   pl = okCnnPlaces(sh);
    const int           H = sh.H, F = ok_cnn_features(sh), Nt = H >> 4, tid = static_cast<int>(threadIdx.x);
    const int           lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
    const long          a0 = static_cast<long>(blockIdx.x) * kCnnAgents;
    float              *hid = ok_actor_lds + pl.hid;

    okLidarAcc acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
    {
        const int t = okLidarMin(wave + kCnnWaves * c, Nt - 1); // (a wave without a tile of its own repeats the last one and stores nothing)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[c][r] = p.params[at.hb + 16 * t + i];
    }
    const float4 *wp = reinterpret_cast<const float4 *>(p.pack + pl.pack[3]) + i * 4 + g;
    const int     gstride = H * 4; // float4's between groups
    for (int k0 = 0; k0 < F; k0 += kCnnChunk)
    {
        const int kc = okLidarMin(kCnnChunk, F - k0), kc4 = kc >> 2;
        for (int e = tid; e < kCnnAgents * kc4; e += kCnnThreads)
        {
            const int    r = e / kc4, c4 = e - r * kc4;
            const long   a = okLidarMin(static_cast<int>(a0) + r, p.N - 1);
            const float4 v = reinterpret_cast<const float4 *>(p.feat + a * F + k0)[c4];
            *reinterpret_cast<float4 *>(ok_actor_lds + r * pl.ldt + 4 * c4) = v;
        }
        __syncthreads();
        for (int grp = 0; grp < (kc >> 4); ++grp)
        {
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                a[q] = ok_actor_lds[i * pl.ldt + 16 * grp + 4 * q + g];
#pragma unroll
            for (int c = 0; c < CT; ++c)
            {
                const int    t  = okLidarMin(wave + kCnnWaves * c, Nt - 1);
                const float4 bv = wp[((k0 >> 4) + grp) * gstride + t * 64];
                const float  b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[q], acc[c], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < CT; ++c)
    {
        const int t = wave + kCnnWaves * c;
        if (t < Nt)
        {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                hid[(4 * g + r) * pl.ldh + 16 * t + i] = ok_lidar_relu(acc[c][r]);
        }
    }
    __syncthreads();

    const long a = a0 + tid;
    if (tid >= kCnnAgents || a >= p.N)
        return;
    float out[3];
    ok_cnn_action(ok_lidar_dot(hid + tid * pl.ldh, p.params + at.ow, H, p.params[at.ob]), p.throttle, p.steer_scale, out);
    p.st.thr[a]   = out[1];
    p.st.steer[a] = out[2];
    if (p.rec.out != nullptr)
        p.rec.out[a] = out[0];
    if (p.rec.action != nullptr)
    {
        p.rec.action[2 * a]     = out[1];
        p.rec.action[2 * a + 1] = out[2];
    }
    okActAlive(p.st.crashed, p.rec.alive, a);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okCnnCheckConfig(const okenv_cnn_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_cnn_shape_bad(okCnnShape(*c)))
        return "shape outside the limits (image_size 16 .. 128; kernel 1 .. 8; stride 1 .. 4 and at most the kernel; every layer's side "
               "at least 1; channels multiples of 16 in 16 .. 128; at most 8192 features; hidden a multiple of 16 in 16 .. 512)";
    if (okCnnLdsBytes(okCnnShape(*c)) > kCnnLdsBudget)
        return "the conv kernel's LDS (okenv_cnn_lds_bytes) does not fit 160 KB";
    if (!std::isfinite(c->throttle) || !std::isfinite(c->steer_scale))
        return "throttle / steer_scale must be finite";
    return nullptr;
}

// The action of n agents on host arrays; every output may be nullptr
inline void okCnnActHost(const okenv_cnn_config &c, const float *params, const int n, const uint8_t *frames, const uint8_t *crashed,
                         float *throttle, float *steer, float *out, uint8_t *alive)
{
    const ok_cnn_shape s = okCnnShape(c);
    std::vector<float> work(static_cast<size_t>(ok_cnn_work_floats(s)));
    const size_t       frame = static_cast<size_t>(s.S) * s.S * 4U;
    for (int a = 0; a < n; ++a)
    {
        float o = 0.F, act[3];
        ok_cnn_forward(s, params, frames + static_cast<size_t>(a) * frame, work.data(), &o);
        ok_cnn_action(o, c.throttle, c.steer_scale, act);
        if (out != nullptr)
            out[a] = act[0];
        if (throttle != nullptr)
            throttle[a] = act[1];
        if (steer != nullptr)
            steer[a] = act[2];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

#endif // OK_CNN_H
