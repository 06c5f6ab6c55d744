// ok_flow.h -- the flow-matching driver on the device: the Euler sampler of FlowMatching's ActionFlowTrunk
// (flow_matching_model.py; main_flow_control.cpp:68-102) for every agent of a handle, all S evaluations of the trunk in ONE kernel.
// The rule lives in include/okenv_flow.h (ok_flow_noise, ok_flow_hidden1, ok_flow_euler, ok_flow_clamp, ok_flow_action on top of
// ok_lidar_dot) and is shared with okFlowActHost below, so the device and the host entry agree bit for bit.
//
// This is NOT a step kernel and adds no step-kernel launch site.
//   okFlowActKernel  kFlowAgents agents per workgroup of 4 waves.  cond, the condition's share of layer 1 (pre), both hidden layers
//                    and x stay in LDS over the whole loop.  pre and layer 2 run through ok_lidar.h's okLidarLinear on
//                    v_mfma_f32_16x16x4_f32 from a bias-initialised accumulator (the rule's chain); layer 3 is the same instruction
//                    on a tile whose columns 2 .. 15 are zero weights nobody stores; layer 1's three terms, the Euler update and the
//                    end run on the VALU.  Rows of a partial last workgroup repeat the last agent and are never stored.
// The weights are read from global memory (L2 / Infinity Cache) in torch's layout by every workgroup.  W2, read once per Euler step,
// passes through LDS in blocks of columns where the LDS has room for them (okFlowPlaces: stage_cols).
#ifndef OK_FLOW_H
#define OK_FLOW_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_flow.h"
#include "ok_lidar.h"

// Row tiles of 16 agents a workgroup owns (at most kLidarRowBlock = 4: one okLidarUnit covers them).  ONE: the populations this
// driver serves (1024 .. 4096 agents) then make 64 .. 256 workgroups, at most one per CU, and the act's length is one workgroup's
// critical path.  More tiles would give a wave independent accumulator chains (the instruction issues every 32 cycles, a dependent one
// every 40) and read W2 fewer times, but leave three quarters of the CUs idle and make every wave's chain of work kFlowTiles times as
// long.
constexpr int kFlowTiles  = 1;
constexpr int kFlowAgents = 16 * kFlowTiles; // agents per workgroup
static_assert(kFlowTiles >= 1 && kFlowTiles <= kLidarRowBlock && kFlowTiles <= kLidarWaves, "one okLidarUnit, one wave per tile in layer 3");

__host__ __device__ inline ok_flow_shape okFlowShape(const okenv_flow_config &c)
{
    ok_flow_shape s;
    s.C = c.cond_dim;
    s.H = c.hidden;
    s.S = c.steps;
    return s;
}

constexpr size_t kFlowLdsBudget = 160U * 1024U;
constexpr int    kFlowStageCols = 64; // rows of W2 (columns of layer 2) staged in LDS at a time, at most: one 16-column tile per wave
constexpr int    kFlowStageBatch = 8; // 16-byte loads a thread issues before it stores the first of them

// The act kernel's LDS, in floats: [cond | pre | h1 | h2 | x | w1x | w3s | w2s].  Rows of cond are C + pad long, rows of pre, h1, h2 H + pad
// (ok_lidar.h's padding: the 16 rows of a tile start 4 banks apart); x is [rows][2]; w1x [H][3] holds layer 1's columns of x_0, x_1, t;
// w3s W3's two rows, H + pad apart;
// w2s is stage_cols rows of W2, H + pad long like the activations' (the 16 rows of a B tile start 4 banks apart as well): as many
// whole tiles as fit behind the rest, at most kFlowStageCols and at most H; 0 when not even one tile fits -- layer 2 then reads W2 from
// global memory.
struct OkFlowPlaces
{
    int rows, ldc, ldh, stage_cols;
    int cond, pre, h1, h2, x, w1x, w3s, w2s, end;
};

__host__ __device__ inline OkFlowPlaces okFlowPlaces(const ok_flow_shape sh)
{
    OkFlowPlaces at;
    at.rows = kFlowAgents;
    at.ldc  = sh.C + kLidarPad;
    at.ldh  = sh.H + kLidarPad;
    at.cond = 0;
    at.pre  = at.cond + at.rows * at.ldc;
    at.h1   = at.pre + at.rows * at.ldh;
    at.h2   = at.h1 + at.rows * at.ldh;
    at.x    = at.h2 + at.rows * at.ldh;
    at.w1x  = at.x + 2 * at.rows;
    at.w3s  = at.w1x + 3 * sh.H;
    at.w2s  = (at.w3s + 2 * at.ldh + 3) & ~3; // (16-byte stores)
    const int room = (static_cast<int>(kFlowLdsBudget / sizeof(float)) - at.w2s) / at.ldh;
    at.stage_cols  = okLidarMin(okLidarMin(kFlowStageCols, sh.H), room < 0 ? 0 : room & ~15);
    at.end  = at.w2s + at.stage_cols * at.ldh;
    return at;
}

inline size_t okFlowLdsBytes(const ok_flow_shape s)
{
    return ok_flow_shape_bad(s) ? 0U : sizeof(float) * static_cast<size_t>(okFlowPlaces(s).end);
}

struct OkFlowActParams
{
    OkDeviceState     st;
    int               N;
    ok_flow_shape     s;
    const float      *params, *cond; // cond [N][C]
    OkActDrawWords    draw;
    float             lo[2], hi[2];
    int               noise;
    uint32_t          seed, agent_base;
    okenv_flow_record rec;
};

// Layer 3 and the Euler update of the row tile from row r0 on, by one wave: v = W3 h2 + b3 as an MFMA tile whose columns 0 and 1 are
// W3's rows and whose columns 2 .. 15 are zeros (their accumulators stay at the bias and are dropped); k ascends from the bias, four
// terms an instruction.  Accumulator register r of lane l is D[row 4 (l >> 4) + r][col l & 15] (ok_lidar.h).
__device__ __forceinline__ void okFlowVelocity(const int h2o, const int w3o, const int ldh, const int r0, const int H, const float *__restrict__ b3,
                                               const float dt, float *X)
{
    const int    lane = static_cast<int>(threadIdx.x) & 63, i = lane & 15, g = lane >> 4;
    const bool   col  = i < 2;
    const float *h    = ok_actor_lds + h2o + (r0 + i) * ldh + g;
    const float *w    = ok_actor_lds + w3o + (col ? i : 0) * ldh + g; // W3's rows in LDS (w3s)
    okLidarAcc   acc;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        acc[r] = b3[col ? i : 0];
    for (int k0 = 0; k0 < H; k0 += 16)
    {
        float b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
            const float wv = w[k0 + 4 * q]; // (every lane reads inside w3s: the columns past 1 read row 0 and use 0)
            b[q]           = col ? wv : 0.F;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h[k0 + 4 * q], b[q], acc, 0, 0, 0);
    }
    if (!col)
        return;
#pragma unroll
    for (int r = 0; r < 4; ++r)
    {
        const int at = 2 * (r0 + 4 * g + r) + i;
        X[at]        = ok_flow_euler(X[at], dt, acc[r]);
    }
}

// Rows n0 .. n0 + nb of W2 [H][H] (global, 16-byte aligned: the pieces in front of it are a multiple of four floats) into w2s, rows
// ldh apart: consecutive threads on consecutive 16 bytes, kFlowStageBatch loads in flight per thread.  The caller's barrier follows.
__device__ __forceinline__ void okFlowStageW2(float *w2s, const int ldh, const float *__restrict__ w2, const int H, const int n0, const int nb)
{
    const int     q = H >> 2, total = nb * q;
    const float4 *src = reinterpret_cast<const float4 *>(w2 + static_cast<long>(n0) * H);
    for (int base = static_cast<int>(threadIdx.x); base < total; base += kLidarThreads * kFlowStageBatch)
    {
        float4 v[kFlowStageBatch];
#pragma unroll
        for (int u = 0; u < kFlowStageBatch; ++u)
        {
            const int e = base + u * kLidarThreads;
            v[u]        = src[e < total ? e : total - 1]; // (every load goes out; one past the block re-reads its last element)
        }
#pragma unroll
        for (int u = 0; u < kFlowStageBatch; ++u)
        {
            const int e = base + u * kLidarThreads;
            if (e < total)
            {
                const int r = e / q, c = e - r * q;
                *reinterpret_cast<float4 *>(w2s + r * ldh + 4 * c) = v[u];
            }
        }
    }
}

__global__ __launch_bounds__(kLidarThreads) void okFlowActKernel(const OkFlowActParams p)
{
    const ok_flow_shape  sh = p.s;
    const ok_flow_layout at = ok_flow_offsets(sh);
    const OkFlowPlaces   pl = okFlowPlaces(sh);
    const int            C = sh.C, H = sh.H, S = sh.S, rows = pl.rows;
    const int            tid = static_cast<int>(threadIdx.x);
    float               *Cond = ok_actor_lds + pl.cond, *Pre = ok_actor_lds + pl.pre, *H1 = ok_actor_lds + pl.h1, *X = ok_actor_lds + pl.x;
    float               *W1x = ok_actor_lds + pl.w1x, *W2s = ok_actor_lds + pl.w2s;
    const float         *prm = p.params;
    const long           a0  = static_cast<long>(blockIdx.x) * kFlowAgents;

    // the conditions of the workgroup's agents, consecutive threads on consecutive floats; layer 1's first three columns; W3
    for (int e = tid; e < rows * C; e += kLidarThreads)
    {
        const int  r = e / C, k = e - r * C;
        const long a_raw = a0 + r, a = a_raw < p.N ? a_raw : static_cast<long>(p.N) - 1;
        Cond[r * pl.ldc + k] = p.cond[a * C + k];
    }
    for (int e = tid; e < 3 * H; e += kLidarThreads)
    {
        const int j = e / 3, c = e - 3 * j;
        W1x[e]      = prm[at.w1 + j * at.ld1 + c];
    }
    for (int e = tid; e < 2 * H; e += kLidarThreads)
    {
        const int k = e / H, j = e - k * H;
        ok_actor_lds[pl.w3s + k * pl.ldh + j] = prm[at.w3 + e];
    }
    // the noise, one agent per thread
    if (tid < rows)
    {
        const long a_raw = a0 + tid, a = a_raw < p.N ? a_raw : static_cast<long>(p.N) - 1;
        float      xa = 0.F, xb = 0.F;
        if (p.noise != 0)
            ok_flow_noise(p.seed, p.agent_base + static_cast<uint32_t>(a), okActDraw(p.draw), &xa, &xb);
        X[2 * tid]     = xa;
        X[2 * tid + 1] = xb;
        if (a_raw < p.N && p.rec.x0 != nullptr)
        {
            p.rec.x0[2 * a]     = xa;
            p.rec.x0[2 * a + 1] = xb;
        }
    }
    __syncthreads();
    // the condition's share of layer 1: the weight rows start behind the columns of x_0, x_1 and t
    okLidarLinear(pl.cond, pl.ldc, C, 0, kFlowTiles, C, prm + at.w1 + 3, at.ld1, prm + at.b1, H, false, false, pl.pre, pl.ldh, 0);
    __syncthreads();

    const float dt = 1.0F / static_cast<float>(S);
    for (int step = 0; step < S; ++step)
    {
        const float t = static_cast<float>(step) / static_cast<float>(S);
        for (int e = tid; e < rows * H; e += kLidarThreads)
        {
            const int r = e / H, j = e - r * H;
            H1[r * pl.ldh + j] = ok_flow_hidden1(Pre[r * pl.ldh + j], W1x + 3 * j, X[2 * r], X[2 * r + 1], t);
        }
        __syncthreads();
        if (pl.stage_cols == 0)
        {
            okLidarLinear(pl.h1, pl.ldh, H, 0, kFlowTiles, H, prm + at.w2, H, prm + at.b2, H, true, false, pl.h2, pl.ldh, 0);
            __syncthreads();
        }
        else
            for (int n0 = 0; n0 < H; n0 += pl.stage_cols) // a block of W2's rows through LDS, then the block's columns of h2
            {
                const int nb = okLidarMin(pl.stage_cols, H - n0);
                okFlowStageW2(W2s, pl.ldh, prm + at.w2, H, n0, nb);
                __syncthreads();
                okLidarLinear(pl.h1, pl.ldh, H, 0, kFlowTiles, H, W2s, pl.ldh, prm + at.b2 + n0, nb, true, false, pl.h2 + n0, pl.ldh, 0);
                __syncthreads();
            }
        if ((tid >> 6) < kFlowTiles) // (the same for every lane of a wave)
            okFlowVelocity(pl.h2, pl.w3s, pl.ldh, 16 * (tid >> 6), H, prm + at.b3, dt, X);
        __syncthreads();
    }

    if (tid >= 2 * rows)
        return;
    const int  r = tid >> 1, k = tid & 1;
    const long a = a0 + r;
    if (a >= p.N)
        return;
    const float x   = ok_flow_clamp(X[tid], -1.0F, 1.0F);
    const float act = ok_flow_action(x, k ? p.lo[1] : p.lo[0], k ? p.hi[1] : p.hi[0]);
    (k ? p.st.steer : p.st.thr)[a] = act;
    if (p.rec.x != nullptr)
        p.rec.x[2 * a + k] = x;
    if (p.rec.action != nullptr)
        p.rec.action[2 * a + k] = act;
    if (k == 0)
        okActAlive(p.st.crashed, p.rec.alive, a);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okFlowCheckConfig(const okenv_flow_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_flow_shape_bad(okFlowShape(*c)))
        return "shape outside the limits (cond_dim and hidden multiples of 16 in 16 .. 512; steps 1 .. 256)";
    if (okFlowLdsBytes(okFlowShape(*c)) > kFlowLdsBudget)
        return "the act kernel's LDS (okenv_flow_lds_bytes) does not fit 160 KB";
    if (c->noise != 0 && c->noise != 1)
        return "noise must be 0 or 1";
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(c->action_lo[k]) || !std::isfinite(c->action_hi[k]))
            return "action_lo / action_hi must be finite";
    return nullptr;
}

// The action of n agents on host arrays; every output may be nullptr
inline void okFlowActHost(const okenv_flow_config &c, const float *params, const int n, const float *cond, const uint8_t *crashed,
                          const uint32_t draw_index, float *throttle, float *steer, float *x0_out, float *x_out, uint8_t *alive)
{
    const ok_flow_shape s = okFlowShape(c);
    std::vector<float>  work(static_cast<size_t>(ok_flow_work_floats(s)));
    for (int a = 0; a < n; ++a)
    {
        const size_t sa = static_cast<size_t>(a);
        float        x0[2] = {0.F, 0.F}, x[2];
        if (c.noise != 0)
            ok_flow_noise(c.seed, c.agent_base + static_cast<uint32_t>(a), draw_index, &x0[0], &x0[1]);
        ok_flow_forward(s, params, cond + sa * static_cast<size_t>(s.C), x0, work.data(), x);
        if (throttle != nullptr)
            throttle[a] = ok_flow_action(x[0], c.action_lo[0], c.action_hi[0]);
        if (steer != nullptr)
            steer[a] = ok_flow_action(x[1], c.action_lo[1], c.action_hi[1]);
        for (int k = 0; k < 2; ++k)
        {
            if (x0_out != nullptr)
                x0_out[2 * sa + k] = x0[k];
            if (x_out != nullptr)
                x_out[2 * sa + k] = x[k];
        }
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

#endif // OK_FLOW_H
