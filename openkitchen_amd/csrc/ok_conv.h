// ok_conv.h -- what the image encoders share on the device: the flow driver's (ok_bev.h), the image policy
// (ok_cnn.h, section 26), the image Q-network (ok_qcnn.h, section 29) and the world model's encoder and memory (ok_world.h, ok_memory.h,
// sections 27 and 28).  All of it runs on v_mfma_f32_16x16x4_f32 with the accumulator started from the bias, so that every chain is
// the rule's.  Rows are output pixels (the convolutions) or agents (the hidden layer), columns output channels, k runs over the rule's
// chain, four terms an instruction; B comes from the packed weights.
//   okConvPackAt, okConvWeightAt  the packed-weight layout: from an element of a pack to its column and place in the chain, and from
//                  there into a conv weight
//   okConvPack     a four-layer pack (three convolutions and a hidden layer), a family supplying layer 0's value
//   okConvMfma     the 4 x RB instructions of one group of 16 k's: the only place that names the instruction
//   okConv<Taps, RB, Waves, Prefetch>  one convolution of an image in LDS; Taps fetches a group's A operands: OkConvWalk for layers 1
//                  and 2, a family's own loader for layer 0; the caller's store says where an output pixel goes
//   okConvFc1      the hidden layer as a GEMM whose rows are agents, into LDS
// Nothing here knows which family calls it.
#ifndef OK_CONV_H
#define OK_CONV_H

#include "../../include/okenv_cnn.h"
#include "ok_lidar.h"

constexpr int    kConvThreads     = 512; // 8 waves
constexpr int    kConvWaves       = kConvThreads / 64;
constexpr int    kConvRowBlock    = 2;   // row tiles a wave carries through one pass over a weight tile (the convolutions)
constexpr int    kConvAgents      = 16;  // agents per row tile of the head: the rows of one MFMA tile
constexpr int    kConvChunk       = 256; // features the head stages at a time
constexpr int    kConvMaxColTiles = OK_CNN_MAX_HIDDEN / 16 / kConvWaves; // 4
constexpr size_t kConvLdsBudget   = 160U * 1024U;

// The head's LDS, in floats: [tile | hid], 16 rows of kConvChunk + 4 and of H + 4 floats; and where each layer's packed weights begin
// (3: the hidden layer).  A family's places derive from this.
struct OkConvHeadPlaces
{
    int ct, ldt, ldh, hid, head_end;
    int pack[4], pack_total;
};

// groups[l], cout[l]: layer l's groups of 16 k's and its columns
__host__ __device__ inline void okConvHeadPlaces(OkConvHeadPlaces &at, const int H, const int (&groups)[4], const int (&cout)[4])
{
    at.ct       = (H / 16 + kConvWaves - 1) / kConvWaves;
    at.ldt      = kConvChunk + 4;
    at.ldh      = H + 4;
    at.hid      = kConvAgents * at.ldt;
    at.head_end = at.hid + kConvAgents * at.ldh;
    int o = 0;
    for (int l = 0; l < 4; ++l)
    {
        at.pack[l] = o;
        o += groups[l] * cout[l] * 16;
    }
    at.pack_total = o;
}

// ---- the weights as the kernels read them ----------------------------------------------------------------------------------------------

// A layer's B matrix [K][Cout] in groups of 16 k's, k the place in the rule's chain:
// pack[((k / 16) * Cout + n) * 16 + (k % 4) * 4 + (k % 16) / 4] -- the four floats a lane (column n, k-lane g = k % 4) feeds to the four
// instructions of a group lie side by side, one 16-byte load, and a wave's 64 loads are 1 KB in a row.  Every pack kernel walks its
// pack's elements and asks these two where an element comes from.
struct OkConvPackAt
{
    int n, kk; // column, place in the chain
};

// Element idx of a layer's pack of Cout columns
__host__ __device__ inline OkConvPackAt okConvPackAt(const int idx, const int Cout)
{
    const int grp = idx / (Cout * 16), rem = idx - grp * Cout * 16, g = (rem & 15) >> 2, q = rem & 3;
    return {rem >> 4, grp * 16 + 4 * q + g};
}

// Where a conv weight [n][Cin][taps] holds column n's k = tap * Cin + ch (tap = ty * k + tx)
__host__ __device__ inline int okConvWeightAt(const int n, const int kk, const int Cin, const int taps)
{
    const int tap = kk / Cin, ch = kk - tap * Cin;
    return (n * Cin + ch) * taps + tap;
}

// Three convolutions and a hidden layer: layer 0's k as its family says, layers 1 and 2's as okConvWeightAt's, the hidden layer's
// k = (y * side_2 + x) * c2 + ch.  Element blockIdx.x * 256 + threadIdx.x of the pack; layer0(n, k) is layer 0's B[k][n].  Shape, Layout
// and Places are a family's ok_*_shape, ok_*_layout and Ok*Places.
template <class Shape, class Layout, class Places, class Layer0>
__device__ __forceinline__ void okConvPack(const Shape &s, const Layout &at, const Places &pl, const float *params, float *pack, const Layer0 layer0)
{
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= pl.pack_total)
        return;
    const int l    = e >= pl.pack[3] ? 3 : (e >= pl.pack[2] ? 2 : (e >= pl.pack[1] ? 1 : 0));
    const int base = l == 3 ? pl.pack[3] : (l == 2 ? pl.pack[2] : (l == 1 ? pl.pack[1] : 0)); // (no array indexed by l: it would live in scratch)
    const int Cout = l == 3 ? s.H : (l == 2 ? s.c[2] : (l == 1 ? s.c[1] : s.c[0]));
    const auto [n, kk] = okConvPackAt(e - base, Cout);
    float      v;
    if (l == 0)
        v = layer0(n, kk);
    else if (l == 3)
    {
        const int c2 = s.c[2], P = pl.side[2] * pl.side[2], pos = kk / c2, ch = kk - pos * c2;
        v = params[at.hw + n * (c2 * P) + ch * P + pos];
    }
    else
    {
        const int k = l == 2 ? s.k[2] : s.k[1];
        v = params[(l == 2 ? at.w[2] : at.w[1]) + okConvWeightAt(n, kk, l == 2 ? s.c[1] : s.c[0], k * k)];
    }
    pack[e] = v;
}

// ---- the convolution piece -------------------------------------------------------------------------------------------------------------

// One group of 16 k's on RB row tiles against one tile of 16 columns: bv is the lane's 16-byte load from the pack
template <int RB>
__device__ __forceinline__ void okConvMfma(const float (&a)[4][RB], const float4 bv, okLidarAcc (&acc)[RB])
{
    const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
#pragma unroll
        for (int m = 0; m < RB; ++m)
            acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][m], b[q], acc[m], 0, 0, 0);
    }
}

// ... on one row tile
__device__ __forceinline__ void okConvMfma(const float (&a)[4], const float4 bv, okLidarAcc &acc)
{
    const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[q], acc, 0, 0, 0);
}

// One convolution of an image in LDS: M output pixels, W to a row, times Cout channels.  Input pixel (y, x) lies at
// in + y * rs + x * ps, its channel ch at + ch unless the Taps say otherwise (a border the rule pads with is part of the image: +0.0f
// in LDS); the output pixel (oy, ox) reads the input pixels (stride oy + ty, stride ox + tx), all of them inside the input.  Where an
// output pixel goes, the caller's store says.
struct OkConvJob
{
    int          in, ps, rs, k, stride, Cin, W, M, Cout;
    const float *w, *bias; // packed weights of the layer, its bias
};

// The store of a whole image: pixel (oy, ox) goes to out + ((oy + opad) * orow + ox + opad) * ldo + channel n0 + i -- LDS, inside a
// border of opad pixels in rows of orow, or global (opad = 0, orow = W)
struct OkConvBordered
{
    float *out;
    int    ldo, opad, orow;

    __device__ __forceinline__ void put(const int oy, const int ox, const int n0, const int i, const float v) const
    {
        out[static_cast<long>((oy + opad) * orow + ox + opad) * ldo + n0 + i] = v;
    }
};

// Layers 1 and 2's A operands: group grp = (tap (ty, tx), channels c0 .. c0 + 15), lane group g reads channel c0 + 4 q + g
struct OkConvWalk
{
    int ty = 0, tx = 0, c0 = 0;

    __device__ __forceinline__ OkConvWalk(const OkConvJob &, const int) {}

    __device__ __forceinline__ static int groups(const OkConvJob &j)
    {
        return j.k * j.k * (j.Cin >> 4);
    }

    __device__ __forceinline__ static int lane(const OkConvJob &, const int g)
    {
        return g;
    }

    template <int RB>
    __device__ __forceinline__ void load(const OkConvJob &j, const int (&abase)[RB], float (&a)[4][RB], const bool first = false)
    {
        const int off = first ? 0 : ty * j.rs + tx * j.ps + c0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
#pragma unroll
            for (int m = 0; m < RB; ++m)
                a[q][m] = ok_actor_lds[abase[m] + off + 4 * q];
        }
        c0 += 16;
        if (c0 == j.Cin)
        {
            c0 = 0;
            if (++tx == j.k)
                tx = 0, ++ty;
        }
    }
};

// A workgroup of Waves waves; a wave owns 16 columns and RB row tiles of 16 pixels at a time: RB independent accumulator chains.
// Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; accumulator register r is D[row 4 (l >> 4) + r][col l & 15]
// (ok_lidar.h).  Rows past M repeat the last pixel and are not stored.  Taps(j, g) starts a unit's chain for lane group g; groups(j) is
// the chain's length in groups of 16 k's; lane(j, g) is where lane group g's first k lies behind a window's first pixel (kept in abase,
// out of the walk); load(j, abase, a) fills a[q][m], the lane's A operand of the group's instruction q on row tile m, from the window
// at abase[m], and moves on to the next group; load(j, abase, a, true) fetches the unit's first group instead, wherever the walk stands,
// and is the unit's last load.  to.put(oy, ox, n0, i, v) stores channel n0 + i of an output pixel (apart: n0 is the wave's, i the
// lane's, and a store adds them in that order to the pixel's place).
// Prefetch: the next group's operands are loaded before this group's instructions are issued, so that the LDS's latency passes behind
// them where the waves of a SIMD are too few to hide it; the last group loads the first one again, so that every load goes out -- as
// an offset of 0 chosen in place of the walk's, which the compiler makes a branch that keeps the loads in front of the instructions
// (resetting the walk instead cost the flow encoder 3 %, docs/HISTORY.md section 46).
template <class Taps, int RB, int Waves, bool Prefetch, class Store>
__device__ __forceinline__ void okConv(const OkConvJob &j, const Store &to)
{
    const int lane = static_cast<int>(threadIdx.x) & 63, i = lane & 15, g = lane >> 4, wave = static_cast<int>(threadIdx.x) >> 6;
    const int Nt = j.Cout >> 4, Mb = (j.M + 16 * RB - 1) / (16 * RB), units = Nt * Mb, groups = Taps::groups(j);
    for (int u = wave; u < units; u += Waves)
    {
        const int  mb = u / Nt, n0 = (u - mb * Nt) << 4;
        int        abase[RB];
        okLidarAcc acc[RB];
#pragma unroll
        for (int m = 0; m < RB; ++m)
        {
            const int row = okLidarMin((mb * RB + m) * 16 + i, j.M - 1), oy = row / j.W, ox = row - oy * j.W;
            abase[m]      = j.in + j.stride * oy * j.rs + j.stride * ox * j.ps + Taps::lane(j, g);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[m][r] = j.bias[n0 + i];
        }
        const float4 *wp = reinterpret_cast<const float4 *>(j.w) + (n0 + i) * 4 + g;
        const int     gstride = j.Cout * 4; // float4's between groups
        Taps          taps(j, g);
        if constexpr (Prefetch)
        {
            float  a[4][RB];
            float4 bv = wp[0];
            taps.load(j, abase, a);
            for (int grp = 0; grp < groups; ++grp)
            {
                const int    next = grp + 1 < groups ? grp + 1 : 0;
                const float4 bn   = wp[next * gstride];
                float        an[4][RB];
                taps.load(j, abase, an, next == 0);
                okConvMfma(a, bv, acc);
                bv = bn;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
#pragma unroll
                    for (int m = 0; m < RB; ++m)
                        a[q][m] = an[q][m];
                }
            }
        }
        else
        {
            for (int grp = 0; grp < groups; ++grp)
            {
                const float4 bv = wp[grp * gstride];
                float        a[4][RB];
                taps.load(j, abase, a);
                okConvMfma(a, bv, acc);
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
                {
                    const int oy = row / j.W, ox = row - oy * j.W;
                    to.put(oy, ox, n0, i, ok_lidar_relu(acc[m][r]));
                }
            }
        }
    }
}

// ---- the hidden layer ------------------------------------------------------------------------------------------------------------------

// relu(feat W^T + bias) of agents a0 .. a0 + 16 RT - 1 into LDS, for a workgroup of 8 waves: the features [N][F] staged through LDS
// kConvChunk k's at a time, rows of ldt floats; a wave owns CT tiles of 16 of the H columns for RT row tiles of 16 agents, so w, the
// layer's packed weights, is read once per workgroup.  Rows past N repeat the last agent.  Returns the hidden activations, rows of ldh
// floats behind the staged tile, every thread past the barrier behind their last store.
template <int CT, int RT>
__device__ __forceinline__ const float *okConvFc1(const float *feat, const int N, const int F, const int H, const long a0, const float *w, const float *bias,
                                                  const int ldt, const int ldh)
{
    constexpr int kAgents = kConvAgents * RT;
    const int     Nt = H >> 4, tid = static_cast<int>(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
    float        *hid = ok_actor_lds + kAgents * ldt;

    okLidarAcc acc[CT][RT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
    {
        const int t = okLidarMin(wave + kConvWaves * c, Nt - 1); // (a wave without a tile of its own repeats the last one and stores nothing)
#pragma unroll
        for (int m = 0; m < RT; ++m)
        {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[c][m][r] = bias[16 * t + i];
        }
    }
    const float4 *wp = reinterpret_cast<const float4 *>(w) + i * 4 + g;
    const int     gstride = H * 4; // float4's between groups
    for (int k0 = 0; k0 < F; k0 += kConvChunk)
    {
        const int kc = okLidarMin(kConvChunk, F - k0), kc4 = kc >> 2;
        for (int e = tid; e < kAgents * kc4; e += kConvThreads)
        {
            const int    r = e / kc4, c4 = e - r * kc4;
            const long   a = okLidarMin(static_cast<int>(a0) + r, N - 1);
            const float4 v = reinterpret_cast<const float4 *>(feat + a * F + k0)[c4];
            *reinterpret_cast<float4 *>(ok_actor_lds + r * ldt + 4 * c4) = v;
        }
        __syncthreads();
        for (int grp = 0; grp < (kc >> 4); ++grp)
        {
            float a[4][RT];
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
#pragma unroll
                for (int m = 0; m < RT; ++m)
                    a[q][m] = ok_actor_lds[(16 * m + i) * ldt + 16 * grp + 4 * q + g];
            }
#pragma unroll
            for (int c = 0; c < CT; ++c)
            {
                const int t = okLidarMin(wave + kConvWaves * c, Nt - 1);
                okConvMfma(a, wp[((k0 >> 4) + grp) * gstride + t * 64], acc[c]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < CT; ++c)
    {
        const int t = wave + kConvWaves * c;
        if (t < Nt)
        {
#pragma unroll
            for (int m = 0; m < RT; ++m)
            {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    hid[(16 * m + 4 * g + r) * ldh + 16 * t + i] = ok_lidar_relu(acc[c][m][r]);
            }
        }
    }
    __syncthreads();
    return hid;
}

#endif // OK_CONV_H
