// ok_memory.h -- the world-model racers' memory on the device: WorldModelVaeRnn's GRUDynamics (train_rnn.py) and
// the [mu | h_top] controllers of main.cpp's CmaEsAgent::runVaeRnn, for every agent of a handle that has okenv_world_create's racers.
// The rule lives in include/okenv_memory.h and is shared with okMemoryActHost below, so the device and the host entry agree bit for bit.
// The first recurrent driver: every agent's hidden state [L][H] lives in the handle and persists from act to act.
//
// The encoder is ok_world.h's, unchanged: okWorldListKernel, the four conv launches and okWorldLatentKernel leave the list and fc_mu's
// partial chains in the world's workspace.  Behind them, the matrix work on v_mfma_f32_16x16x4_f32: the running sums start from the
// bias, and each K block's product is accumulated from zero and added on, which is the rule's blocked chain (ok_memory_dot):
//   okMemoryInputKernel     a thread per (list slot, input): the partial chains joined into mu in the world head's order; mu and the
//                           normalised x0 = [(mu - z_mean) / z_std | (a - a_mean) / a_std], a the agent's stored throttle and steering.
//   okMemoryLayerKernel     one GRU layer, launched L times.  Rows are list slots, a tile of 16 per wave, 128 per workgroup; columns are
//                           hidden units, kMemCols = 32 per workgroup (two column tiles).  K runs in the rule's blocks of 64: the block's A
//                           tile (the rows' inputs, or in the second pass their h_prev) and the block's weight tiles of all three gates
//                           are staged in LDS, and all eight waves -- eight row tiles -- read the same weight tiles from there.  A wave
//                           carries the three gi accumulators and, with carry, the three gh accumulators of both column tiles, does the
//                           gate arithmetic in registers and writes h'.  With carry == 0 the Whh matrices are never read.
//   okMemoryHeadKernel      a wave per list slot: the device-side copy of the slot's new hidden state into the agent's (see below), the
//                           prediction (only if recorded), the controller on [mu | h_top], the action, the record, okActAlive.
//   okMemoryResetKernel     zeroes every agent's hidden state.
//
// THE HIDDEN UPDATE IS NOT IN PLACE.  With carry, workgroups that own different column blocks of a layer all read the whole h_prev of
// their rows, so no workgroup may overwrite it.  The layers read the agents' state `hidden` [N][L][H] and write `fresh` [slot][L][H], a
// second buffer indexed by list slot; the head kernel, which runs behind all layers, copies fresh -> hidden for the listed agents.  The
// two buffers never change roles: nothing alternates in host variables or kernel arguments, so a captured graph replays the same work,
// and a crashed agent under skip_crashed is in no slot and keeps its state.
#ifndef OK_MEMORY_H
#define OK_MEMORY_H

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_memory.h"
#include "ok_world.h"

constexpr int kMemThreads   = 512;                // 8 waves, a row tile each
constexpr int kMemWaves     = kMemThreads / 64;
constexpr int kMemRows      = 16 * kMemWaves;     // list slots of a workgroup
constexpr int kMemColTiles  = 2;                  // column tiles (16 hidden units) of a workgroup: a wave's column block
constexpr int kMemCols      = 16 * kMemColTiles;
constexpr int kMemChunk     = OK_MEMORY_BLOCK;    // k's of a K block: the rule's block, whose partial sum a K block's MFMAs give
constexpr int kMemLda       = kMemChunk + 2;      // floats between the A tile's rows (ok_world.h: kWorldLda)
constexpr int kMemATile     = kMemRows * kMemLda; // floats; a multiple of 4, so that the weight tiles behind it are 16-byte aligned
constexpr int kMemWTile     = 3 * kMemCols * kMemChunk;
constexpr int kMemHeadSlots = 4;                  // list slots per workgroup of the head kernel, a wave each
constexpr int kMemPlan      = 8;                  // ints of okMemoryPlan

__host__ __device__ inline ok_memory_shape okMemoryShape(const okenv_world_config &w, const okenv_memory_config &c)
{
    ok_memory_shape s;
    s.Z     = w.latent;
    s.H     = c.hidden;
    s.L     = c.layers;
    s.h     = c.ctrl_hidden;
    s.carry = c.carry;
    return s;
}

// k's of layer l's input that run on the matrix cores: layer 0's two action columns are added by hand behind them
__host__ __device__ inline int okMemoryKin(const ok_memory_shape s, const int l)
{
    return l == 0 ? s.Z : s.H;
}

__host__ __device__ inline int okMemoryPitch(const ok_memory_shape s)
{
    return s.Z + 4; // of x0's rows: [Z | 2 | 2 unused], so that every row begins 16-byte aligned
}

// Where the packed matrices begin, in floats (Wih and Whh of every layer), and the workspace of N agents, in 4-byte words:
// [pack | controllers | mu | x0 | fresh | hidden], every piece 16-byte aligned
struct OkMemoryPlaces
{
    int    ih[OK_MEMORY_MAX_LAYERS], hh[OK_MEMORY_MAX_LAYERS], pack_total;
    size_t ctrl, mu, x0, fresh, hidden, words;
};

__host__ __device__ inline OkMemoryPlaces okMemoryPlaces(const ok_memory_shape s, const size_t N)
{
    OkMemoryPlaces at;
    int            o = 0;
    for (int l = 0; l < OK_MEMORY_MAX_LAYERS; ++l)
    {
        at.ih[l] = o;
        o += l < s.L ? 3 * s.H * okMemoryKin(s, l) : 0;
        at.hh[l] = o;
        o += l < s.L ? 3 * s.H * s.H : 0;
    }
    at.pack_total    = o;
    const auto round = [](const size_t w) { return (w + 3U) & ~static_cast<size_t>(3U); };
    size_t     w     = static_cast<size_t>(o);
    at.ctrl          = w;
    w                = round(w + N * static_cast<size_t>(ok_memory_controller_params(s)));
    at.mu            = w;
    w += N * static_cast<size_t>(s.Z);
    at.x0 = w;
    w += N * static_cast<size_t>(okMemoryPitch(s));
    at.fresh = w;
    w += N * static_cast<size_t>(s.L * s.H);
    at.hidden = w;
    at.words  = w + N * static_cast<size_t>(s.L * s.H);
    return at;
}

// The layer kernel's dynamic LDS: the A tile and the three gates' weight tiles of one K block.  The same for every shape.
inline size_t okMemoryLdsBytes(const ok_memory_shape s)
{
    return ok_memory_shape_bad(s) ? 0U : sizeof(float) * static_cast<size_t>(kMemATile + kMemWTile);
}

// What names the kernels' paths for a shape: the column blocks of a layer and the live column tiles of the last one (1: its second
// tile idles), the K blocks of layer 0's input and the k's of the last one, the K blocks of a chain over H and the k's of the last one,
// whether the Whh pass runs, and the launches of the layer kernel
inline void okMemoryPlan(const ok_memory_shape s, int32_t *plan)
{
    plan[0] = (s.H + kMemCols - 1) / kMemCols;
    plan[1] = (s.H - (plan[0] - 1) * kMemCols) / 16;
    plan[2] = (s.Z + kMemChunk - 1) / kMemChunk;
    plan[3] = s.Z - (plan[2] - 1) * kMemChunk;
    plan[4] = (s.H + kMemChunk - 1) / kMemChunk;
    plan[5] = s.H - (plan[4] - 1) * kMemChunk;
    plan[6] = s.carry;
    plan[7] = s.L;
}

// ---- the weights as the layer kernel reads them ------------------------------------------------------------------------------------------

// One matrix [cols][stride], of which the first K columns are packed: B [K][cols] in ok_conv.h's layout
struct OkMemoryPackJob
{
    const float *src;
    float       *dst;
    int          cols, K, stride;
};

__global__ __launch_bounds__(256) void okMemoryPackKernel(const OkMemoryPackJob j)
{
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= j.cols * j.K)
        return;
    const auto [n, kk] = okConvPackAt(e, j.cols);
    j.dst[e]           = j.src[n * j.stride + kk];
}

// ---- the state --------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void okMemoryResetKernel(float *hidden, const long words)
{
    const long e = static_cast<long>(blockIdx.x) * 256 + static_cast<long>(threadIdx.x);
    if (e < words)
        hidden[e] = 0.F;
}

// ---- the input --------------------------------------------------------------------------------------------------------------------------

struct OkMemoryInputJob
{
    OkDeviceState st;
    const float  *enc_bias, *part; // fc_mu's bias; the latent kernel's partial chains [slot][P][Z]
    const float  *z_mean, *z_std, *a_mean, *a_std;
    float        *mu, *x0; // [slot][Z], [slot][Z + 4]
    const int    *list, *count;
    int           Z, P;
};

__global__ __launch_bounds__(256) void okMemoryInputKernel(const OkMemoryInputJob j)
{
    const int  in = j.Z + OK_MEMORY_ACTIONS;
    const long t  = static_cast<long>(blockIdx.x) * 256 + static_cast<long>(threadIdx.x);
    const long slot = t / in;
    const int  e    = static_cast<int>(t - slot * in);
    if (slot >= j.count[0])
        return;
    float *x = j.x0 + slot * (j.Z + 4);
    if (e < j.Z)
    {
        float v = j.enc_bias[e];
        for (int q = 0; q < j.P; ++q)
            v = v + j.part[(static_cast<size_t>(slot) * j.P + q) * j.Z + e];
        j.mu[slot * j.Z + e] = v;
        x[e]                 = ok_memory_normalise(v, j.z_mean[e], j.z_std[e]);
    }
    else
    {
        const long  a = j.list[slot];
        const int   k = e - j.Z;
        const float v = k == 0 ? j.st.thr[a] : j.st.steer[a]; // as stored: the action of the step before
        x[e]          = ok_memory_normalise(v, j.a_mean[k], j.a_std[k]);
    }
}

// ---- one GRU layer ----------------------------------------------------------------------------------------------------------------------

struct OkMemoryLayerJob
{
    const float *x;      // the input's rows [slot][x_pitch]: x0, or the layer below's fresh state
    const float *hidden; // this layer's h_prev of AGENT a at hidden + a * LH
    float       *fresh;  // this layer's h' of list SLOT s at fresh + s * LH
    const float *wih, *whh;   // packed
    const float *tail;        // layer 0: Wih [3H][Z + 2] as set, for the two action columns; otherwise nullptr
    const float *bih, *bhh;
    const int   *list, *count;
    int          x_pitch, Kin, H, LH, carry;
};

// One pass over a chain of K k's: per K block, acc[t][gate] += A[rows][block] B[block][the gate's columns of tile t], the block's
// product accumulated from zero (ok_memory_dot's blocks).  kHidden: the rows are the agents'
// h_prev (through the list); otherwise the input's rows.  Every wave stages and waits; a wave multiplies for its live column tiles.
template <bool kHidden>
__device__ __forceinline__ void okMemoryPass(const OkMemoryLayerJob &j, const int K, const float *pack, const int m0, const int j0, const int count,
                                             okLidarAcc (&acc)[kMemColTiles][3])
{
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
    float    *A = ok_actor_lds;
    float4   *W = reinterpret_cast<float4 *>(ok_actor_lds + kMemATile);
    const float4 *pack4 = reinterpret_cast<const float4 *>(pack);
    const int     H = j.H;
    for (int k0 = 0; k0 < K; k0 += kMemChunk)
    {
        const int kc = okLidarMin(kMemChunk, K - k0), ngrp = kc >> 4, kc4 = kc >> 2;
        for (int e = tid; e < kMemRows * kc4; e += kMemThreads)
        {
            const int row = e / kc4, c4 = e - row * kc4, slot = m0 + row;
            float4    v = make_float4(0.F, 0.F, 0.F, 0.F);
            if (slot < count)
            {
                const float *src = kHidden ? j.hidden + static_cast<size_t>(j.list[slot]) * j.LH : j.x + static_cast<size_t>(slot) * j.x_pitch;
                v                = *reinterpret_cast<const float4 *>(src + k0 + 4 * c4);
            }
            float2 *d = reinterpret_cast<float2 *>(A + row * kMemLda + 4 * c4);
            d[0]      = make_float2(v.x, v.y);
            d[1]      = make_float2(v.z, v.w);
        }
        // the weight tiles: per (group of 16 k's, gate) the 16 floats of each of the block's 32 columns, as they lie in the pack
        for (int e = tid; e < ngrp * 3 * kMemCols * 4; e += kMemThreads)
        {
            const int f = e & 3, n = (e >> 2) & (kMemCols - 1), gg = e >> 7, grp = gg / 3, gate = gg - 3 * grp, unit = j0 + n;
            float4    v = make_float4(0.F, 0.F, 0.F, 0.F);
            if (unit < H)
                v = pack4[(static_cast<size_t>((k0 >> 4) + grp) * (3 * H) + gate * H + unit) * 4 + f];
            W[e] = v;
        }
        __syncthreads();
        okLidarAcc part[kMemColTiles][3];
#pragma unroll
        for (int t = 0; t < kMemColTiles; ++t)
        {
#pragma unroll
            for (int gate = 0; gate < 3; ++gate)
                part[t][gate] = okLidarAcc{0.F, 0.F, 0.F, 0.F};
        }
        for (int grp = 0; grp < ngrp; ++grp)
        {
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                a[q] = A[(16 * wave + i) * kMemLda + 16 * grp + 4 * q + g];
#pragma unroll
            for (int t = 0; t < kMemColTiles; ++t)
            {
                if (j0 + 16 * t < H)
                {
#pragma unroll
                    for (int gate = 0; gate < 3; ++gate)
                        okConvMfma(a, W[((grp * 3 + gate) * kMemCols + 16 * t + i) * 4 + g], part[t][gate]);
                }
            }
        }
        // the block's partial sums onto the running ones: one rounded addition each (the rule's acc = acc + part)
#pragma unroll
        for (int t = 0; t < kMemColTiles; ++t)
        {
#pragma unroll
            for (int gate = 0; gate < 3; ++gate)
                acc[t][gate] = acc[t][gate] + part[t][gate];
        }
        __syncthreads();
    }
}

// Lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; accumulator register r is D[row 4 (l >> 4) + r][col l & 15]
// (ok_lidar.h).  Grid (slots / 128, H / 32), both rounded up and sized for every agent: workgroups past the list's end leave at once.
__global__ __launch_bounds__(kMemThreads) void okMemoryLayerKernel(const OkMemoryLayerJob j)
{
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
    const int count = j.count[0], m0 = static_cast<int>(blockIdx.x) * kMemRows, j0 = static_cast<int>(blockIdx.y) * kMemCols, H = j.H;
    if (m0 >= count)
        return; // (the whole workgroup)
    okLidarAcc gi[kMemColTiles][3], gh[kMemColTiles][3];
#pragma unroll
    for (int t = 0; t < kMemColTiles; ++t)
    {
        const int unit = j0 + 16 * t < H ? j0 + 16 * t + i : 0;
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
        {
            const float bi = j.bih[gate * H + unit], bh = j.bhh[gate * H + unit];
#pragma unroll
            for (int r = 0; r < 4; ++r)
            {
                gi[t][gate][r] = bi;
                gh[t][gate][r] = bh; // (with carry == 0 this is gh itself)
            }
        }
    }
    okMemoryPass<false>(j, j.Kin, j.wih, m0, j0, count, gi);
    if (j.carry != 0)
        okMemoryPass<true>(j, H, j.whh, m0, j0, count, gh);
#pragma unroll
    for (int t = 0; t < kMemColTiles; ++t)
    {
        if (j0 + 16 * t >= H)
            continue;
        const int unit = j0 + 16 * t + i;
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const int slot = m0 + 16 * wave + 4 * g + r;
            if (slot >= count)
                continue;
            float s[3] = {gi[t][0][r], gi[t][1][r], gi[t][2][r]};
            if (j.tail != nullptr)
            {
                // layer 0's two action columns, the chain's last block
                const float *xa = j.x + static_cast<size_t>(slot) * j.x_pitch + j.Kin;
#pragma unroll
                for (int gate = 0; gate < 3; ++gate)
                {
                    const float *w = j.tail + static_cast<size_t>(gate * H + unit) * (j.Kin + OK_MEMORY_ACTIONS) + j.Kin;
                    s[gate]        = s[gate] + ok_memory_action_part(xa, w);
                }
            }
            const float before = j.carry != 0 ? j.hidden[static_cast<size_t>(j.list[slot]) * j.LH + unit] : 0.F;
            j.fresh[static_cast<size_t>(slot) * j.LH + unit] = ok_memory_gate(s[0], s[1], s[2], gh[t][0][r], gh[t][1][r], gh[t][2][r], before);
        }
    }
}

// ---- the head ---------------------------------------------------------------------------------------------------------------------------

struct OkMemoryHeadParams
{
    OkDeviceState       st;
    ok_memory_shape     s;
    const float        *net, *ctrl, *mu, *fresh; // the network vector as set; [N][controller]; [slot][Z]; [slot][L][H]
    float              *hidden;                  // [N][L][H]
    const int          *list, *count;
    float               throttle, steer_scale;
    okenv_memory_record rec;
};

// A wave per list slot.  The controller's first layer has up to 640 inputs, more than okCtrlLayer places in a wave's registers, so it
// is written anew: lane u evaluates unit u as one sequential non-fused chain over the inputs in ascending order, the inputs read at
// wave-uniform addresses.  The two narrow layers behind it are okCtrlLayer's.
__global__ __launch_bounds__(64 * kMemHeadSlots) void okMemoryHeadKernel(const OkMemoryHeadParams p)
{
    const int lane = static_cast<int>(threadIdx.x) & 63, slot = static_cast<int>(blockIdx.x) * kMemHeadSlots + (static_cast<int>(threadIdx.x) >> 6);
    if (slot >= p.count[0])
        return; // (the whole wave)
    const ok_memory_layout at = ok_memory_offsets(p.s);
    const int              Z = p.s.Z, H = p.s.H, LH = p.s.L * H, h = p.s.h, h2 = h / 2, in = Z + H;
    const long             a = p.list[slot];
    const float           *mu = p.mu + static_cast<size_t>(slot) * Z, *all = p.fresh + static_cast<size_t>(slot) * LH, *top = all + LH - H;
    // the agent's state becomes the slot's fresh one: the copy that makes the update safe (see the file's head)
    for (int e = lane; e < LH; e += 64)
        p.hidden[a * LH + e] = all[e];
    for (int e = lane; e < Z; e += 64)
    {
        if (p.rec.mu != nullptr)
            p.rec.mu[a * Z + e] = mu[e];
        if (p.rec.state != nullptr)
            p.rec.state[a * in + e] = mu[e];
    }
    for (int e = lane; e < H; e += 64)
    {
        if (p.rec.hidden != nullptr)
            p.rec.hidden[a * H + e] = top[e];
        if (p.rec.state != nullptr)
            p.rec.state[a * in + Z + e] = top[e];
    }
    if (p.rec.prediction != nullptr)
    {
        for (int e = lane; e < Z; e += 64)
        {
            const float *w  = p.net + at.hw + static_cast<size_t>(e) * H;
            const float  zn = ok_memory_dot(top, w, H, p.net[at.hb + e]);
            p.rec.prediction[a * Z + e] = zn * p.net[at.z_std + e] + p.net[at.z_mean + e];
        }
    }
    const float *w1 = p.ctrl + a * ok_memory_controller_params(p.s), *b1 = w1 + h * in, *w2 = b1 + h, *b2 = w2 + h2 * h, *w3 = b2 + h2, *b3 = w3 + h2;
    const int    u  = lane < h ? lane : h - 1;
    const float *wu = w1 + u * in;
    float        acc = b1[u];
    for (int k0 = 0; k0 < Z; k0 += 8)
    {
        float w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            w[k] = wu[k0 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            acc = acc + w[k] * mu[k0 + k];
    }
    wu += Z;
    for (int k0 = 0; k0 < H; k0 += 8)
    {
        float w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            w[k] = wu[k0 + k];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            acc = acc + w[k] * top[k0 + k];
    }
    float a1[1], a2[1], a3[1];
    a1[0] = lane < h ? ok_tanhf(acc) : 0.F;
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

// ---- host side (no GPU) -----------------------------------------------------------------------------------------------------------------

inline const char *okMemoryCheckConfig(const okenv_world_config *w, const okenv_memory_config *c)
{
    if (w == nullptr || c == nullptr)
        return "config is NULL";
    if (const char *why = okWorldCheckConfig(w))
        return why;
    if (c->carry != 0 && c->carry != 1)
        return "carry must be 0 or 1";
    if (ok_memory_shape_bad(okMemoryShape(*w, *c)))
        return "shape outside the limits (hidden a multiple of 16 in 16 .. 512; layers 1 .. 4; ctrl_hidden even in 2 .. 64)";
    if (!std::isfinite(c->throttle) || !std::isfinite(c->steer_scale))
        return "throttle / steer_scale must be finite";
    return nullptr;
}

// One act of n agents on host arrays: hidden [n][L][H], throttle and steer [n] in and out (the stored action in, the new one out); the
// record's members are host pointers, each may be nullptr.  With skip_crashed everything of a crashed agent is left as it is.
inline void okMemoryActHost(const okenv_world_config &wc, const okenv_memory_config &mc, const float *encoder, const float *network,
                            const float *controllers, const int n, const uint8_t *frames, const uint8_t *crashed, float *hidden, float *throttle,
                            float *steer, const okenv_memory_record &rec)
{
    const ok_world_shape  w = okWorldShape(wc);
    const ok_memory_shape s = okMemoryShape(wc, mc);
    std::vector<float>    work(static_cast<size_t>(ok_memory_work_floats(w, s))), x(static_cast<size_t>(s.Z + s.H)), pred(static_cast<size_t>(s.Z));
    const size_t          frame = static_cast<size_t>(w.S) * w.S * 4U, cp = static_cast<size_t>(ok_memory_controller_params(s));
    const size_t          LH = static_cast<size_t>(s.L) * s.H, Z = static_cast<size_t>(s.Z), H = static_cast<size_t>(s.H);
    for (int a = 0; a < n; ++a)
    {
        const bool gone = crashed != nullptr && crashed[a] != 0;
        if (gone && wc.skip_crashed != 0)
            continue;
        const float action[2] = {throttle[a], steer[a]};
        float       y         = 0.F;
        ok_memory_forward(w, s, encoder, network, controllers + a * cp, frames + a * frame, action, hidden + a * LH, work.data(), x.data(),
                          rec.prediction != nullptr ? pred.data() : nullptr, &y);
        if (rec.mu != nullptr)
            std::copy(x.begin(), x.begin() + s.Z, rec.mu + a * Z);
        if (rec.hidden != nullptr)
            std::copy(x.begin() + s.Z, x.end(), rec.hidden + a * H);
        if (rec.prediction != nullptr)
            std::copy(pred.begin(), pred.end(), rec.prediction + a * Z);
        if (rec.state != nullptr)
            std::copy(x.begin(), x.end(), rec.state + a * (Z + H));
        if (rec.out != nullptr)
            rec.out[a] = y;
        throttle[a] = mc.throttle;
        steer[a]    = y * mc.steer_scale;
        if (rec.action != nullptr)
        {
            rec.action[2 * a]     = throttle[a];
            rec.action[2 * a + 1] = steer[a];
        }
        if (rec.alive != nullptr)
            rec.alive[a] = gone ? 0 : 1;
    }
}

#endif // OK_MEMORY_H
