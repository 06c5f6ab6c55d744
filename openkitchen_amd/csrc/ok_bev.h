// ok_bev.h -- the flow driver's image encoder on the device: FlowMatching's BEVEncoder (flow_matching_model.py)
// from the camera's RGBA8 frames to the condition vectors okenv_flow_act takes, for every agent of a handle.  The rule lives in
// include/okenv_bev.h (ok_bev_pixel, ok_bev_conv_at, ok_bev_pool on top of ok_lidar_dot) and is shared with okBevEncodeHost below, so the
// device and the host entry agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  Every convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32
// (ok_conv.h's okConv, with the next group's operands prefetched): rows are output pixels of a tile, columns output channels, k runs
// over (tap row, tap column, input channel) with the channel innermost, A comes from an activation tile in LDS, B from the weights as
// okBevPackKernel laid them out at set_params, and the accumulator starts from the bias -- the rule's chain, four terms an
// instruction.  The lane mapping, the packed-weight layout, the unit loop and the walk of layers 1 and 2 are ok_conv.h's; this
// family's own are layer 0's planar loader (OkBevPlanarTaps) and the store of a tile that may reach past the image (OkBevTileStore).
//   okBevFrontKernel<T>  one T x T tile of layer 1's output of one frame per workgroup of 4 waves: the frame's patch as floats in LDS
//                        (planar), layer 0 on it into an LDS tile (channels last) with its halo recomputed, layer 1 from that tile to
//                        global memory (channels last).  Layer 0's output never leaves the CU.
//   okBevBackKernel<T>   one T x T tile of layer 2's output: its patch of layer 1's output into LDS, layer 2 to global memory.
//   okBevHeadKernel      one frame per workgroup: the pool in the rule's order, one channel per thread, and the projection.
// T is 8 where that tile's LDS fits and the layer's output is wider than 4 pixels, else 4 (okBevPlaces); tiles at an image's edge and
// images smaller than a tile run the same code with their stores guarded.
#ifndef OK_BEV_H
#define OK_BEV_H

#include <cstring>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_bev.h"
#include "ok_conv.h"
#include "ok_lidar.h"

constexpr int    kBevThreads   = 256; // 4 waves
constexpr int    kBevWaves     = kBevThreads / 64;
constexpr size_t kBevLdsBudget = 160U * 1024U;

__host__ __device__ inline ok_bev_shape okBevShape(const okenv_bev_config &c)
{
    ok_bev_shape s;
    s.S = c.image_size;
    for (int l = 0; l < 3; ++l)
    {
        s.k[l] = c.kernel[l];
        s.c[l] = c.channels[l];
    }
    s.E = c.embed_dim;
    return s;
}

// Floats between the rows of an LDS tile whose pixels are ld floats apart: at least side * ld, and 8 mod 16, so that with ld = 1 mod 16
// the 16 rows of an MFMA tile (8 pixels of one image row, 2 apart, and the row 2 below) start on 16 even banks of ds_read_b32's 32 and
// the two k's of a lane group fill the odd ones
__host__ __device__ inline int okBevRowStride(const int side, const int ld)
{
    return ((side * ld + 7) / 16) * 16 + 8;
}

// The two conv kernels' LDS, in floats.  Front: [in0 | tile1]: in0 the frame's patch, 3 planes of p0 x p0 floats (p0 odd, so a plane
// is: the two channels of a lane group fall on even and odd banks); tile1 layer 0's output, p1 x p1 pixels of c0 + 1 floats.  Back:
// [tile2], p2 x p2 pixels of c1 + 1 floats.  ta, tb: the tiles' sides.
struct OkBevPlaces
{
    int ta, p1, p0, plane0, ldc1, ldr1, tile1, front_end;
    int tb, p2, ldc2, ldr2, back_end;
    int pack[3], pack_total; // where each layer's packed weights begin, in floats
};

__host__ __device__ inline int okBevFrontFloats(const ok_bev_shape s, const int t)
{
    const int p1 = 2 * (t - 1) + s.k[1], p0 = 2 * (p1 - 1) + s.k[0];
    return 3 * p0 * p0 + p1 * okBevRowStride(p1, s.c[0] + 1);
}

__host__ __device__ inline int okBevBackFloats(const ok_bev_shape s, const int t)
{
    const int p2 = 2 * (t - 1) + s.k[2];
    return p2 * okBevRowStride(p2, s.c[1] + 1);
}

// Groups of 16 k's in a layer's chain: layer 0 has 4 k's a tap (R, G, B and the alpha slot) and filler taps up to a whole group
__host__ __device__ inline int okBevGroups(const ok_bev_shape s, const int l)
{
    return l == 0 ? (s.k[0] * s.k[0] + 3) / 4 : s.k[l] * s.k[l] * s.c[l - 1] / 16;
}

__host__ __device__ inline OkBevPlaces okBevPlaces(const ok_bev_shape s)
{
    OkBevPlaces  at;
    const size_t budget = kBevLdsBudget / sizeof(float);
    at.ta        = (ok_bev_side(s, 1) > 4 && static_cast<size_t>(okBevFrontFloats(s, 8)) <= budget) ? 8 : 4;
    at.p1        = 2 * (at.ta - 1) + s.k[1];
    at.p0        = 2 * (at.p1 - 1) + s.k[0];
    at.plane0    = at.p0 * at.p0;
    at.ldc1      = s.c[0] + 1;
    at.ldr1      = okBevRowStride(at.p1, at.ldc1);
    at.tile1     = 3 * at.plane0;
    at.front_end = at.tile1 + at.p1 * at.ldr1;
    at.tb        = (ok_bev_side(s, 2) > 4 && static_cast<size_t>(okBevBackFloats(s, 8)) <= budget) ? 8 : 4;
    at.p2        = 2 * (at.tb - 1) + s.k[2];
    at.ldc2      = s.c[1] + 1;
    at.ldr2      = okBevRowStride(at.p2, at.ldc2);
    at.back_end  = at.p2 * at.ldr2;
    int o = 0;
    for (int l = 0; l < 3; ++l)
    {
        at.pack[l] = o;
        o += okBevGroups(s, l) * s.c[l] * 16;
    }
    at.pack_total = o;
    return at;
}

inline size_t okBevLdsBytes(const ok_bev_shape s)
{
    if (ok_bev_shape_bad(s))
        return 0U;
    const OkBevPlaces at = okBevPlaces(s);
    return sizeof(float) * static_cast<size_t>(okLidarMax(at.front_end, at.back_end));
}

// ---- the weights as the conv kernels read them ---------------------------------------------------------------------------------------

// ok_conv.h's layout; k = tap * Cin' + ch (tap = ty * k + tx; Cin' = Cin, layer 0: 4), layer 0's alpha slot and filler taps 0.0f
struct OkBevPackParams
{
    ok_bev_shape s;
    const float *params;
    float       *pack;
};

__global__ __launch_bounds__(kBevThreads) void okBevPackKernel(const OkBevPackParams p)
{
    const ok_bev_layout at = ok_bev_offsets(p.s);
    const OkBevPlaces   pl = okBevPlaces(p.s);
    const int           e  = static_cast<int>(blockIdx.x) * kBevThreads + static_cast<int>(threadIdx.x);
    if (e >= pl.pack_total)
        return;
    const int  l = e >= pl.pack[2] ? 2 : (e >= pl.pack[1] ? 1 : 0);
    const auto of = [l](const int *v) { return l == 2 ? v[2] : (l == 1 ? v[1] : v[0]); }; // (no array indexed by l: it would live in scratch)
    const int  k = of(p.s.k), taps = k * k;
    const auto [n, kk] = okConvPackAt(e - of(pl.pack), of(p.s.c));
    float      v       = 0.F;
    if (l == 0)
    {
        const int tap = kk >> 2, ch = kk & 3;
        if (tap < taps && ch < 3)
            v = p.params[at.w[0] + (n * 3 + ch) * taps + tap];
    }
    else
        v = p.params[of(at.w) + okConvWeightAt(n, kk, l == 2 ? p.s.c[1] : p.s.c[0], taps)];
    p.pack[e] = v;
}

// ---- the convolutions ------------------------------------------------------------------------------------------------------------------

// Layer 0's A operands for okConv: the patch is planar, three planes of rs x rs floats; a k-step is one tap, lane group g reads plane g
// (3: the blue plane against the alpha slot's 0.0f); the filler taps read the last tap.
struct OkBevPlanarTaps
{
    int s = 0; // the group's first k-step

    __device__ __forceinline__ OkBevPlanarTaps(const OkConvJob &, const int) {}

    __device__ __forceinline__ static int groups(const OkConvJob &j)
    {
        return (j.k * j.k + 3) >> 2;
    }

    __device__ __forceinline__ static int lane(const OkConvJob &j, const int g)
    {
        return okLidarMin(g, 2) * j.rs * j.rs;
    }

    template <int RB>
    __device__ __forceinline__ void load(const OkConvJob &j, const int (&abase)[RB], float (&a)[4][RB], const bool first = false)
    {
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
            const int tap = okLidarMin((first ? 0 : s) + q, j.k * j.k - 1), ty = j.k == 3 ? tap / 3 : tap / 5; // (divisions by constants: k is 3 or 5)
            const int toff = ty * j.rs + (tap - ty * j.k) * j.ps;
#pragma unroll
            for (int m = 0; m < RB; ++m)
                a[q][m] = ok_actor_lds[abase[m] + toff];
        }
        s += 4;
    }
};

// The store of a tile: output pixel (oy, ox), image position (gy0 + oy, gx0 + ox) of `side`, goes to out + oy * ors + ox * ops + channel,
// LDS or global; outside the image nothing is stored, or 0.0f (zero_outside: the next layer's padding)
struct OkBevTileStore
{
    float *out;
    long   ops, ors;
    int    gy0, gx0, side;
    bool   zero_outside;

    __device__ __forceinline__ void put(const int oy, const int ox, const int n0, const int i, const float v) const
    {
        const int  gy = gy0 + oy, gx = gx0 + ox; // (0 <= gy < side as one unsigned compare, and no branch between the two: the stores of a
                                                 // row tile stay under one mask)
        const bool inside = (static_cast<unsigned>(gy) < static_cast<unsigned>(side)) & (static_cast<unsigned>(gx) < static_cast<unsigned>(side));
        if (inside || zero_outside)
            out[oy * ors + ox * ops + n0 + i] = inside ? v : 0.F;
    }
};

struct OkBevEncodeParams
{
    int            N;
    ok_bev_shape   s;
    const uint8_t *frames; // [N][S][S][4]
    const float   *params, *pack;
    float         *act1, *act2; // layer 1's and layer 2's outputs, [N][side][side][c], channels last
    float         *out;         // [N][E]
};

template <int T>
__global__ __launch_bounds__(kBevThreads) void okBevFrontKernel(const OkBevEncodeParams p)
{
    const ok_bev_shape  sh = p.s;
    const ok_bev_layout at = ok_bev_offsets(sh);
    const OkBevPlaces   pl = okBevPlaces(sh);
    const int           S = sh.S, side0 = S >> 1, side1 = S >> 2, tiles = (side1 + T - 1) / T;
    const int           tid = static_cast<int>(threadIdx.x);
    const int           b = static_cast<int>(blockIdx.x), n = b / (tiles * tiles), t = b - n * tiles * tiles, ty = t / tiles, tx = t - ty * tiles;
    // the tile's origin in layer 1's output, the origin of the region of layer 0's output it reads, and of the frame's patch that reads
    const int y1 = T * ty, x1 = T * tx, y0 = 2 * y1 - sh.k[1] / 2, x0 = 2 * x1 - sh.k[1] / 2, yf = 2 * y0 - sh.k[0] / 2, xf = 2 * x0 - sh.k[0] / 2;

    const uint32_t *frame = reinterpret_cast<const uint32_t *>(p.frames) + static_cast<size_t>(n) * S * S;
    for (int e = tid; e < pl.plane0; e += kBevThreads)
    {
        const int  py = e / pl.p0, px = e - py * pl.p0, y = yf + py, x = xf + px;
        const bool inside = y >= 0 && y < S && x >= 0 && x < S;
        const uint32_t rgba = inside ? frame[y * S + x] : 0U;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            ok_actor_lds[ch * pl.plane0 + e] = inside ? ok_bev_pixel(static_cast<uint8_t>(rgba >> (8 * ch))) : 0.F;
    }
    __syncthreads();

    OkConvJob      j;
    OkBevTileStore to;
    j.in = 0, j.ps = 1, j.rs = pl.p0, j.k = sh.k[0], j.stride = 2, j.Cin = 4, j.W = pl.p1, j.M = pl.p1 * pl.p1, j.Cout = sh.c[0];
    j.w = p.pack + pl.pack[0], j.bias = p.params + at.b[0];
    to.out = ok_actor_lds + pl.tile1, to.ops = pl.ldc1, to.ors = pl.ldr1;
    to.gy0 = y0, to.gx0 = x0, to.side = side0, to.zero_outside = true;
    okConv<OkBevPlanarTaps, 4, kBevWaves, true>(j, to);
    __syncthreads();

    j.in = pl.tile1, j.ps = pl.ldc1, j.rs = pl.ldr1, j.k = sh.k[1], j.Cin = sh.c[0], j.W = T, j.M = T * T, j.Cout = sh.c[1];
    j.w = p.pack + pl.pack[1], j.bias = p.params + at.b[1];
    to.ops = sh.c[1], to.ors = static_cast<long>(side1) * sh.c[1];
    to.out = p.act1 + (static_cast<size_t>(n) * side1 * side1 + static_cast<size_t>(y1) * side1 + x1) * sh.c[1];
    to.gy0 = y1, to.gx0 = x1, to.side = side1, to.zero_outside = false;
    okConv<OkConvWalk, T * T / 16, kBevWaves, true>(j, to);
}

template <int T>
__global__ __launch_bounds__(kBevThreads) void okBevBackKernel(const OkBevEncodeParams p)
{
    const ok_bev_shape  sh = p.s;
    const ok_bev_layout at = ok_bev_offsets(sh);
    const OkBevPlaces   pl = okBevPlaces(sh);
    const int           side1 = sh.S >> 2, side2 = sh.S >> 3, tiles = (side2 + T - 1) / T, c1 = sh.c[1], c14 = c1 >> 2;
    const int           tid = static_cast<int>(threadIdx.x);
    const int           b = static_cast<int>(blockIdx.x), n = b / (tiles * tiles), t = b - n * tiles * tiles, ty = t / tiles, tx = t - ty * tiles;
    const int           y2 = T * ty, x2 = T * tx, y1 = 2 * y2 - sh.k[2] / 2, x1 = 2 * x2 - sh.k[2] / 2;

    // the patch of layer 1's output, 16 bytes of a pixel's channels per thread; outside the image it is the padding's 0.0f
    const float4 *src = reinterpret_cast<const float4 *>(p.act1 + static_cast<size_t>(n) * side1 * side1 * c1);
    for (int e = tid; e < pl.p2 * pl.p2 * c14; e += kBevThreads)
    {
        const int  pix = e / c14, c4 = e - pix * c14, py = pix / pl.p2, px = pix - py * pl.p2, y = y1 + py, x = x1 + px;
        const bool inside = y >= 0 && y < side1 && x >= 0 && x < side1;
        const float4 v = inside ? src[(y * side1 + x) * c14 + c4] : make_float4(0.F, 0.F, 0.F, 0.F);
        float       *d = ok_actor_lds + py * pl.ldr2 + px * pl.ldc2 + 4 * c4;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    __syncthreads();

    OkConvJob      j;
    OkBevTileStore to;
    j.in = 0, j.ps = pl.ldc2, j.rs = pl.ldr2, j.k = sh.k[2], j.stride = 2, j.Cin = c1, j.W = T, j.M = T * T, j.Cout = sh.c[2];
    j.w = p.pack + pl.pack[2], j.bias = p.params + at.b[2];
    to.ops = sh.c[2], to.ors = static_cast<long>(side2) * sh.c[2];
    to.out = p.act2 + (static_cast<size_t>(n) * side2 * side2 + static_cast<size_t>(y2) * side2 + x2) * sh.c[2];
    to.gy0 = y2, to.gx0 = x2, to.side = side2, to.zero_outside = false;
    okConv<OkConvWalk, T * T / 16, kBevWaves, true>(j, to);
}

constexpr int kBevPoolBatch = 8; // loads a thread issues before it adds the first of them

__global__ __launch_bounds__(kBevThreads) void okBevHeadKernel(const OkBevEncodeParams p)
{
    __shared__ float    mean[OK_BEV_MAX_CHANNELS];
    const ok_bev_shape  sh = p.s;
    const ok_bev_layout at = ok_bev_offsets(sh);
    const int           side2 = sh.S >> 3, P = side2 * side2, c2 = sh.c[2], tid = static_cast<int>(threadIdx.x);
    const size_t        n = blockIdx.x;
    const float        *a = p.act2 + n * P * c2;
    if (tid < c2) // ok_bev_pool: p ascending from 0.0f
    {
        float sum = 0.F;
        for (int p0 = 0; p0 < P; p0 += kBevPoolBatch)
        {
            float v[kBevPoolBatch];
#pragma unroll
            for (int u = 0; u < kBevPoolBatch; ++u)
                v[u] = a[okLidarMin(p0 + u, P - 1) * c2 + tid]; // (every load goes out; one past the end re-reads the last position)
#pragma unroll
            for (int u = 0; u < kBevPoolBatch; ++u)
                if (p0 + u < P)
                    sum = sum + v[u];
        }
        mean[tid] = sum / static_cast<float>(P);
    }
    __syncthreads();
    for (int e = tid; e < sh.E; e += kBevThreads)
        p.out[n * sh.E + e] = ok_lidar_dot(mean, p.params + at.pw + e * c2, c2, p.params[at.pb + e]);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okBevCheckConfig(const okenv_bev_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_bev_shape_bad(okBevShape(*c)))
        return "shape outside the limits (image_size a multiple of 8 in 16 .. 128; kernel 3 or 5; channels multiples of 16 in 16 .. 128; "
               "embed_dim a multiple of 16 in 16 .. 512)";
    if (okBevLdsBytes(okBevShape(*c)) > kBevLdsBudget)
        return "the conv kernels' LDS (okenv_bev_lds_bytes) does not fit 160 KB";
    return nullptr;
}

// The embeddings of n frames on host arrays
inline void okBevEncodeHost(const okenv_bev_config &c, const float *params, const int n, const uint8_t *frames, float *out)
{
    const ok_bev_shape s = okBevShape(c);
    std::vector<float> work(static_cast<size_t>(ok_bev_work_floats(s)));
    const size_t       frame = static_cast<size_t>(s.S) * s.S * 4U;
    for (int a = 0; a < n; ++a)
        ok_bev_forward(s, params, frames + static_cast<size_t>(a) * frame, work.data(), out + static_cast<size_t>(a) * s.E);
}

#endif // OK_BEV_H
