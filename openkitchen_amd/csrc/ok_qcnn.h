// ok_qcnn.h -- the Deep-Q image racers on the device: RLRacers/DQN_CNN's padded conv Q-network driven as
// dq_cnn_racer_sim.cpp drives it, from the camera's RGBA8 frames to the action fields, for every agent of a handle, and the ring of
// frame transitions with its push and its batch gather.  The rule lives in include/okenv_qcnn.h (ok_qcnn_grey, ok_qcnn_conv_at,
// ok_cnn_hidden_at, ok_lidar_dot, ok_actor_argmax, ok_actor_eps_greedy, ok_qcnn_push, ok_qcnn_batch) and is shared with the host
// entries below, so the device and the host agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  The lane mapping, the packed-weight layout, the unit loop of a
// convolution, the walk of layers 1 and 2 and fc1's GEMM are ok_conv.h's; what is this family's own:
//   okQcnnPackKernel      at set_params: the four weight matrices in groups of 16 k's (layer 0: 16 taps a group, filler taps 0.0f)
//   OkQcnnGreyTaps        layer 0's A operands: the grey plane, one float a tap
//   okQcnnConvKernel      one frame per workgroup of 8 waves, every layer in LDS, channels last.  The grey plane and the outputs of
//                         layers 0 and 1 lie INSIDE A BORDER OF +0.0f as wide as the next layer's padding: every tap of every
//                         window is an ordinary in-range LDS read (the rule's ZERO TERMS).  Layer 2 writes the [N][F] features,
//                         channels last, to global memory.
//   okQcnnHeadKernel<CT,RT> 16 RT agents per workgroup of 8 waves: fc1 (okConvFc1, a wave owning CT tiles of 16 columns for RT row
//                         tiles); then fc2, the choice, the action fields and the record, 8 lanes an agent (lane k: q_k).  The act
//                         runs RT = 1; RT = 2 (32 agents, fc1.weight read half as often) was measured slower and is kept behind
//                         okenv_debug_qcnn_stages only.
//   okReplayCountKernel<OkQcnnPushParams>, okQcnnRankKernel, okQcnnFramesKernel<Vec>
//                         the push: ok_dqn.h's count, its rank piece (slot per agent, action / reward / done, the counter), then both
//                         frames' grey planes into the survivors' slots, several workgroups a frame
//   okQcnnBatchKernel<Vec> the gather: the ring's size read on the device, the slot drawn or walked per position, the planes copied
// Vec: the planes move as 16-byte vectors; S S must be a multiple of 4 for every plane to start on 16 bytes.
#ifndef OK_QCNN_H
#define OK_QCNN_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_qcnn.h"
#include "ok_conv.h"
#include "ok_dqn.h"
#include "ok_lidar.h"

static_assert(OKENV_QCNN_BATCH_UNIFORM == OK_QCNN_BATCH_UNIFORM && OKENV_QCNN_BATCH_SEQUENTIAL == OK_QCNN_BATCH_SEQUENTIAL, "the ABI's modes are the rule's");

constexpr int kQcnnCopyThreads = 256;

__host__ __device__ inline ok_qcnn_shape okQcnnShape(const okenv_qcnn_config &c)
{
    ok_qcnn_shape s;
    s.S = c.image_size;
    for (int l = 0; l < 3; ++l)
    {
        s.k[l] = c.kernel[l];
        s.s[l] = c.stride[l];
        s.p[l] = c.padding[l];
        s.c[l] = c.channels[l];
    }
    s.H = c.hidden;
    s.A = c.num_actions;
    return s;
}

// Groups of 16 k's in a chain: layer 0 has one k a tap and filler taps up to a whole group; l = 3 is fc1
__host__ __device__ inline int okQcnnGroups(const ok_qcnn_shape s, const int l)
{
    if (l == 0)
        return (s.k[0] * s.k[0] + 15) / 16;
    return l == 3 ? ok_qcnn_features(s) / 16 : s.k[l] * s.k[l] * s.c[l - 1] / 16;
}

// The conv kernel's LDS, in floats: [p | q].  p: the grey plane inside its border, pin x pin floats, and behind layer 0 layer 1's
// output inside its border, pad1^2 pixels of c1 + 1 floats.  q: layer 0's output inside its border, pad0^2 pixels of c0 + 1 floats
// (odd: the 16 pixels of an MFMA tile start on different banks).  The head's LDS and the pack's places are OkConvHeadPlaces'.
struct OkQcnnPlaces : OkConvHeadPlaces
{
    int side[3], pin, pad0, pad1, ld0, ld1, p, q, conv_end;
    int region; // what sizes p: 0 the grey plane, 1 layer 1's output
    int vec;    // the push and the gather move planes as 16-byte vectors
};

__host__ __device__ inline OkQcnnPlaces okQcnnPlaces(const ok_qcnn_shape s)
{
    OkQcnnPlaces at;
    for (int l = 0; l < 3; ++l)
        at.side[l] = ok_qcnn_side(s, l);
    at.pin  = s.S + 2 * s.p[0];
    at.pad0 = at.side[0] + 2 * s.p[1];
    at.pad1 = at.side[1] + 2 * s.p[2];
    at.ld0  = s.c[0] + 1;
    at.ld1  = s.c[1] + 1;
    const int plane = at.pin * at.pin, out1 = at.pad1 * at.pad1 * at.ld1;
    at.region   = out1 > plane ? 1 : 0;
    at.p        = 0;
    at.q        = at.p + okLidarMax(plane, out1);
    at.conv_end = at.q + at.pad0 * at.pad0 * at.ld0;
    at.vec      = (s.S * s.S) % 4 == 0 ? 1 : 0;
    const int groups[4] = {okQcnnGroups(s, 0), okQcnnGroups(s, 1), okQcnnGroups(s, 2), okQcnnGroups(s, 3)}, cout[4] = {s.c[0], s.c[1], s.c[2], s.H};
    okConvHeadPlaces(at, s.H, groups, cout);
    return at;
}

inline size_t okQcnnLdsBytes(const ok_qcnn_shape s)
{
    if (ok_qcnn_shape_bad(s))
        return 0U;
    const OkQcnnPlaces at = okQcnnPlaces(s);
    return sizeof(float) * static_cast<size_t>(okLidarMax(at.conv_end, at.head_end));
}

// ---- the weights as the kernels read them ----------------------------------------------------------------------------------------------

// okConvPack's layout; layer 0's k = tap (tap = ty * k0 + tx), its filler taps 0.0f
struct OkQcnnPackParams
{
    ok_qcnn_shape s;
    const float  *params;
    float        *pack;
};

__global__ __launch_bounds__(256) void okQcnnPackKernel(const OkQcnnPackParams p)
{
    const ok_qcnn_layout at = ok_qcnn_offsets(p.s);
    okConvPack(p.s, at, okQcnnPlaces(p.s), p.params, p.pack, [&](const int n, const int kk) {
        const int taps = p.s.k[0] * p.s.k[0];
        return kk < taps ? p.params[at.w[0] + n * taps + kk] : 0.F;
    });
}

// ---- the convolutions ------------------------------------------------------------------------------------------------------------------

// Layer 0's A operands for okConv: one input channel, a k-step is four taps, lane group g reads tap 16 grp + 4 q + g; the filler taps
// read the last tap against their 0.0f weight.
struct OkQcnnGreyTaps
{
    const int g, last;
    int       ty, tx; // this lane group's tap, four further every k-step

    __device__ __forceinline__ OkQcnnGreyTaps(const OkConvJob &j, const int g_) : g(g_), last((j.k - 1) * (j.rs + j.ps)), ty(g / j.k), tx(g - ty * j.k) {}

    __device__ __forceinline__ static int groups(const OkConvJob &j)
    {
        return (j.k * j.k + 15) >> 4;
    }

    __device__ __forceinline__ static int lane(const OkConvJob &, const int)
    {
        return 0;
    }

    template <int RB>
    __device__ __forceinline__ void load(const OkConvJob &j, const int (&abase)[RB], float (&a)[4][RB], const bool first = false)
    {
        if (first)
            ty = g / j.k, tx = g - ty * j.k;
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
            const int toff = ty >= j.k ? last : ty * j.rs + tx * j.ps;
#pragma unroll
            for (int m = 0; m < RB; ++m)
                a[q][m] = ok_actor_lds[abase[m] + toff];
            tx += 4;
            while (tx >= j.k)
                tx -= j.k, ++ty;
        }
    }
};

struct OkQcnnActParams
{
    OkDeviceState     st;
    int               N;
    ok_qcnn_shape     s;
    const uint8_t    *frames; // [N][S][S][4]
    const float      *params, *pack;
    float            *feat; // layer 2's output, [N][side_2][side_2][c2]: the features in fc1's chain order
    OkActDrawWords    draw;
    okenv_qcnn_config cfg;
    okenv_qcnn_record rec;
};

__global__ __launch_bounds__(kConvThreads) void okQcnnConvKernel(const OkQcnnActParams p)
{
    const ok_qcnn_shape  sh = p.s;
    const ok_qcnn_layout at = ok_qcnn_offsets(sh);
    const OkQcnnPlaces   pl = okQcnnPlaces(sh);
    const int            S = sh.S, tid = static_cast<int>(threadIdx.x);
    const size_t         n = blockIdx.x;

    // the grey plane inside its border, and +0.0f all over layer 0's place (its border stays)
    const uint32_t *frame = reinterpret_cast<const uint32_t *>(p.frames) + n * static_cast<size_t>(S * S);
    for (int e = tid; e < pl.pin * pl.pin; e += kConvThreads)
    {
        const int y = e / pl.pin - sh.p[0], x = e - (y + sh.p[0]) * pl.pin - sh.p[0];
        float     v = 0.F;
        if (y >= 0 && y < S && x >= 0 && x < S)
        {
            const uint32_t w = frame[y * S + x];
            v                = ok_qcnn_grey(static_cast<uint8_t>(w & 255U), static_cast<uint8_t>((w >> 8) & 255U), static_cast<uint8_t>((w >> 16) & 255U));
        }
        ok_actor_lds[pl.p + e] = v;
    }
    if (sh.p[1] > 0)
        for (int e = tid; e < pl.pad0 * pl.pad0 * pl.ld0; e += kConvThreads)
            ok_actor_lds[pl.q + e] = 0.F;
    __syncthreads();

    OkConvJob      j;
    OkConvBordered to;
    j.in = pl.p, j.ps = 1, j.rs = pl.pin, j.k = sh.k[0], j.stride = sh.s[0], j.Cin = 1, j.W = pl.side[0], j.M = pl.side[0] * pl.side[0], j.Cout = sh.c[0];
    j.w = p.pack + pl.pack[0], j.bias = p.params + at.b[0];
    to.out = ok_actor_lds + pl.q, to.ldo = pl.ld0, to.opad = sh.p[1], to.orow = pl.pad0;
    okConv<OkQcnnGreyTaps, kConvRowBlock, kConvWaves, false>(j, to);
    __syncthreads();

    // (the grey plane is done with: +0.0f all over layer 1's place)
    if (sh.p[2] > 0)
    {
        for (int e = tid; e < pl.pad1 * pl.pad1 * pl.ld1; e += kConvThreads)
            ok_actor_lds[pl.p + e] = 0.F;
        __syncthreads();
    }
    j.in = pl.q, j.ps = pl.ld0, j.rs = pl.pad0 * pl.ld0, j.k = sh.k[1], j.stride = sh.s[1], j.Cin = sh.c[0], j.W = pl.side[1];
    j.M = pl.side[1] * pl.side[1], j.Cout = sh.c[1];
    j.w = p.pack + pl.pack[1], j.bias = p.params + at.b[1];
    to.out = ok_actor_lds + pl.p, to.ldo = pl.ld1, to.opad = sh.p[2], to.orow = pl.pad1;
    okConv<OkConvWalk, kConvRowBlock, kConvWaves, false>(j, to);
    __syncthreads();

    j.in = pl.p, j.ps = pl.ld1, j.rs = pl.pad1 * pl.ld1, j.k = sh.k[2], j.stride = sh.s[2], j.Cin = sh.c[1], j.W = pl.side[2];
    j.M = pl.side[2] * pl.side[2], j.Cout = sh.c[2];
    j.w = p.pack + pl.pack[2], j.bias = p.params + at.b[2];
    to.out = p.feat + n * static_cast<size_t>(j.M * sh.c[2]), to.ldo = sh.c[2], to.opad = 0, to.orow = j.W;
    okConv<OkConvWalk, kConvRowBlock, kConvWaves, false>(j, to);
}

// CT: tiles of 16 hidden units a wave owns; RT: row tiles of 16 agents a workgroup carries (fc1.weight is read once per workgroup): 1 in
// the act, 2 for measurement ("The head's tiling")
template <int CT, int RT>
__global__ __launch_bounds__(kConvThreads) void okQcnnHeadKernel(const OkQcnnActParams p)
{
    constexpr int        kAgents = kConvAgents * RT;
    const ok_qcnn_shape  sh = p.s;
    const ok_qcnn_layout at = ok_qcnn_offsets(sh);
    const OkQcnnPlaces   pl = okQcnnPlaces(sh);
    const int            H = sh.H, A = sh.A, tid = static_cast<int>(threadIdx.x);
    const long           a0 = static_cast<long>(blockIdx.x) * kAgents;
    const float         *hid = okConvFc1<CT, RT>(p.feat, p.N, ok_qcnn_features(sh), H, a0, p.pack + pl.pack[3], p.params + at.hb, pl.ldt, pl.ldh);

    // fc2 and the choice: 8 lanes an agent, lane k holds q_k (whole waves leave here, so the shuffles below are complete)
    if (tid >= kAgents * OK_ACTOR_LANES)
        return;
    const int   row = tid / OK_ACTOR_LANES, k = tid & (OK_ACTOR_LANES - 1);
    const bool  valid = a0 + row < p.N;
    const long  a = valid ? a0 + row : static_cast<long>(p.N) - 1;
    const float mine = k < A ? ok_lidar_dot(hid + row * pl.ldh, p.params + at.ow + k * H, H, p.params[at.ob + k]) : 0.F;
    float       z[OK_ACTOR_MAX_ACTIONS];
#pragma unroll
    for (int q = 0; q < OK_ACTOR_MAX_ACTIONS; ++q)
        z[q] = __shfl(mine, q, OK_ACTOR_LANES);
    const int best   = ok_actor_argmax(z, A);
    int       action = best;
    if (p.cfg.mode == OKENV_ACTOR_EPS_GREEDY)
        action = ok_actor_eps_greedy(p.cfg.epsilon, p.cfg.seed, p.cfg.agent_base + static_cast<uint32_t>(a), okActDraw(p.draw), A, best);
    const float value = __shfl(mine, action, OK_ACTOR_LANES);
    if (!valid)
        return;
    if (p.rec.q != nullptr && k < A)
        p.rec.q[a * A + k] = mine;
    if (k != 0)
        return;
    float thr = p.cfg.action_table[0][0], steer = p.cfg.action_table[0][1];
#pragma unroll
    for (int q = 1; q < OK_ACTOR_MAX_ACTIONS; ++q)
        if (q == action)
        {
            thr   = p.cfg.action_table[q][0];
            steer = p.cfg.action_table[q][1];
        }
    p.st.thr[a]   = thr;
    p.st.steer[a] = steer;
    if (p.rec.action != nullptr)
        p.rec.action[a] = action;
    if (p.rec.value != nullptr)
        p.rec.value[a] = value;
    okActAlive(p.st.crashed, p.rec.alive, a);
}

// ---- the push ------------------------------------------------------------------------------------------------------------------------

// (okReplayCountKernel / okReplaySelected of ok_dqn.h take this struct: N, flags, rec.alive, counts, snapshot, pushed)
struct OkQcnnPushParams
{
    int               N, R, S;
    uint32_t          flags;
    uint64_t          capacity;
    okenv_qcnn_ring   ring;
    uint64_t         *pushed, *snapshot;
    uint32_t         *counts;  // [workgroups of the count]
    long long        *slots;   // [N] the slot of the agent's transition, or -1
    okenv_qcnn_record rec;
    const uint8_t    *frames, *next_frames; // [N][S][S][4]
    const uint8_t    *crashed;
    const float      *dist;    // OKENV_F_DIST after the step
    const float      *reward;  // or nullptr: the clearance rule
};

// okReplayScatterKernel's rank piece: each workgroup re-sums the counts in front of it, ranks its agents by ballot prefixes and writes
// the survivors' slot, action, done and reward; the last workgroup advances `pushed`
__global__ __launch_bounds__(kReplayThreads) void okQcnnRankKernel(const OkQcnnPushParams p)
{
    __shared__ uint32_t wave_count[kReplayWaves];
    __shared__ uint32_t before_part[kReplayThreads], total_part[kReplayThreads];
    const int  wv = static_cast<int>(threadIdx.x) / kReplayWave, lane = static_cast<int>(threadIdx.x) % kReplayWave;
    const long a  = static_cast<long>(blockIdx.x) * kReplayThreads + threadIdx.x;
    uint32_t   before = 0, total = 0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += kReplayThreads)
    {
        const uint32_t c = p.counts[b];
        total += c;
        if (b < blockIdx.x)
            before += c;
    }
    before_part[threadIdx.x] = before;
    total_part[threadIdx.x]  = total;
    const bool               sel = okReplaySelected(p, a);
    const unsigned long long b   = __ballot(sel);
    const uint32_t           pre = static_cast<uint32_t>(__popcll(b & ((1ULL << lane) - 1ULL)));
    if (lane == 0)
        wave_count[wv] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    for (int h = kReplayThreads / 2; h >= 1; h >>= 1)
    {
        if (static_cast<int>(threadIdx.x) < h)
        {
            before_part[threadIdx.x] += before_part[threadIdx.x + h];
            total_part[threadIdx.x] += total_part[threadIdx.x + h];
        }
        __syncthreads();
    }
    const uint64_t n = total_part[0], start = p.snapshot[0];
    uint64_t       k = before_part[0] + pre;
    for (int w = 0; w < wv; ++w)
        k += wave_count[w];
    long long slot = -1;
    if (sel && ok_dqn_survives(k, n, p.capacity))
    {
        slot                = static_cast<long long>(ok_dqn_slot(start + k, p.capacity));
        const int crash     = p.crashed[a] != 0;
        p.ring.action[slot] = p.rec.action[a];
        p.ring.done[slot]   = crash ? 1.F : 0.F;
        p.ring.reward[slot] = p.reward != nullptr ? p.reward[a] : ok_dqn_reward(crash, p.dist + a * p.R, p.R);
    }
    if (a < p.N)
        p.slots[a] = slot;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        p.pushed[0] = start + n;
}

__device__ __forceinline__ float okQcnnGreyWord(const uint32_t w)
{
    return ok_qcnn_grey(static_cast<uint8_t>(w & 255U), static_cast<uint8_t>((w >> 8) & 255U), static_cast<uint8_t>((w >> 16) & 255U));
}

// Both frames of agent blockIdx.x into its slot: workgroup blockIdx.y takes kQcnnCopyThreads pixels (Vec: four times as many)
template <bool Vec>
__global__ __launch_bounds__(kQcnnCopyThreads) void okQcnnFramesKernel(const OkQcnnPushParams p)
{
    const long long slot = p.slots[blockIdx.x];
    if (slot < 0)
        return;
    const size_t px = static_cast<size_t>(p.S) * static_cast<size_t>(p.S), src = blockIdx.x * px, dst = static_cast<size_t>(slot) * px;
    const size_t e  = static_cast<size_t>(blockIdx.y) * kQcnnCopyThreads + threadIdx.x;
    if constexpr (Vec)
    {
        if (4U * e >= px)
            return;
        const uint4 s = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint32_t *>(p.frames) + src)[e];
        const uint4 t = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint32_t *>(p.next_frames) + src)[e];
        reinterpret_cast<float4 *>(p.ring.state + dst)[e] = make_float4(okQcnnGreyWord(s.x), okQcnnGreyWord(s.y), okQcnnGreyWord(s.z), okQcnnGreyWord(s.w));
        reinterpret_cast<float4 *>(p.ring.next_state + dst)[e] = make_float4(okQcnnGreyWord(t.x), okQcnnGreyWord(t.y), okQcnnGreyWord(t.z), okQcnnGreyWord(t.w));
    }
    else
    {
        if (e >= px)
            return;
        p.ring.state[dst + e]      = okQcnnGreyWord(reinterpret_cast<const uint32_t *>(p.frames)[src + e]);
        p.ring.next_state[dst + e] = okQcnnGreyWord(reinterpret_cast<const uint32_t *>(p.next_frames)[src + e]);
    }
}

// ---- the batch gather ------------------------------------------------------------------------------------------------------------------

struct OkQcnnBatchParams
{
    int                  S, B, mode;
    uint32_t             seed;
    uint64_t             capacity, start_or_draw;
    const uint64_t      *pushed;
    okenv_qcnn_ring      ring;
    okenv_qcnn_batch_out out;
};

// Position blockIdx.x of the batch; workgroup blockIdx.y copies kQcnnCopyThreads floats of each plane (Vec: four times as many), the
// first of them the scalars too
template <bool Vec>
__global__ __launch_bounds__(kQcnnCopyThreads) void okQcnnBatchKernel(const OkQcnnBatchParams p)
{
    const uint64_t pushed = p.pushed[0], size = ok_dqn_size(pushed, p.capacity);
    const uint32_t q      = blockIdx.x;
    const bool     live   = size != 0U;
    const size_t   slot   = live ? static_cast<size_t>(ok_qcnn_batch_slot(p.mode, p.seed, p.start_or_draw, q, pushed, size, p.capacity)) : 0U;
    const size_t   px = static_cast<size_t>(p.S) * static_cast<size_t>(p.S), src = slot * px, dst = q * px;
    const size_t   e  = static_cast<size_t>(blockIdx.y) * kQcnnCopyThreads + threadIdx.x;
    if (blockIdx.y == 0 && threadIdx.x == 0)
    {
        if (p.out.action != nullptr)
            p.out.action[q] = live ? p.ring.action[slot] : 0;
        if (p.out.reward != nullptr)
            p.out.reward[q] = live ? p.ring.reward[slot] : 0.F;
        if (p.out.done != nullptr)
            p.out.done[q] = live ? p.ring.done[slot] : 0.F;
        if (p.out.index != nullptr)
            p.out.index[q] = static_cast<int32_t>(slot);
    }
    if constexpr (Vec)
    {
        if (4U * e >= px)
            return;
        const float4 zero = make_float4(0.F, 0.F, 0.F, 0.F);
        if (p.out.state != nullptr)
            reinterpret_cast<float4 *>(p.out.state + dst)[e] = live ? reinterpret_cast<const float4 *>(p.ring.state + src)[e] : zero;
        if (p.out.next_state != nullptr)
            reinterpret_cast<float4 *>(p.out.next_state + dst)[e] = live ? reinterpret_cast<const float4 *>(p.ring.next_state + src)[e] : zero;
    }
    else
    {
        if (e >= px)
            return;
        if (p.out.state != nullptr)
            p.out.state[dst + e] = live ? p.ring.state[src + e] : 0.F;
        if (p.out.next_state != nullptr)
            p.out.next_state[dst + e] = live ? p.ring.next_state[src + e] : 0.F;
    }
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okQcnnCheckShape(const ok_qcnn_shape s)
{
    if (ok_qcnn_shape_bad(s))
        return "shape outside the limits (image_size 16 .. 128; kernel 1 .. 8; stride 1 .. 4 and at most the kernel; padding 0 .. 3 and below "
               "the kernel; every layer's side at least 1; channels multiples of 16 in 16 .. 128; at most 16384 features; hidden a multiple "
               "of 16 in 16 .. 512; 2 .. 8 actions)";
    if (okQcnnLdsBytes(s) > kConvLdsBudget)
        return "the conv kernel's LDS (okenv_qcnn_lds_bytes) does not fit 160 KB";
    return nullptr;
}

inline const char *okQcnnCheckConfig(const okenv_qcnn_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (const char *why = okQcnnCheckShape(okQcnnShape(*c)))
        return why;
    if (c->mode != OKENV_ACTOR_GREEDY && c->mode != OKENV_ACTOR_EPS_GREEDY)
        return "unknown mode (OKENV_ACTOR_GREEDY / _EPS_GREEDY)";
    if (!(c->epsilon >= 0.F && c->epsilon <= 1.F))
        return "epsilon outside [0, 1]";
    for (int a = 0; a < OK_ACTOR_MAX_ACTIONS; ++a)
        if (!std::isfinite(c->action_table[a][0]) || !std::isfinite(c->action_table[a][1]))
            return "the action table must be finite";
    return nullptr;
}

inline ok_qcnn_ring okQcnnRing(const okenv_qcnn_ring &r)
{
    return ok_qcnn_ring{r.state, r.next_state, r.action, r.reward, r.done};
}

// The action of n agents on host arrays; every output may be nullptr
inline void okQcnnActHost(const okenv_qcnn_config &c, const float *params, const int n, const uint8_t *frames, const uint8_t *crashed,
                          const uint32_t draw_index, float *throttle, float *steer, float *q_out, int64_t *action, float *value, uint8_t *alive)
{
    const ok_qcnn_shape s = okQcnnShape(c);
    std::vector<float>  work(static_cast<size_t>(ok_qcnn_work_floats(s)));
    const size_t        frame = static_cast<size_t>(s.S) * s.S * 4U;
    for (int a = 0; a < n; ++a)
    {
        float q[OK_ACTOR_MAX_ACTIONS] = {};
        ok_qcnn_forward(s, params, frames + static_cast<size_t>(a) * frame, work.data(), q);
        const int act = ok_qcnn_choose(c.mode, c.epsilon, c.seed, c.agent_base + static_cast<uint32_t>(a), draw_index, q, s.A);
        if (q_out != nullptr)
            for (int k = 0; k < s.A; ++k)
                q_out[static_cast<size_t>(a) * s.A + k] = q[k];
        if (throttle != nullptr)
            throttle[a] = c.action_table[act][0];
        if (steer != nullptr)
            steer[a] = c.action_table[act][1];
        if (action != nullptr)
            action[a] = act;
        if (value != nullptr)
            value[a] = q[act];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

#endif // OK_QCNN_H
