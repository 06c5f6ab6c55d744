/*
 * okenv_flow.h -- the rule of the flow-matching driver (FlowMatching/flow_matching_model.py: ActionFlowTrunk;
 * main_flow_control.cpp:68-102): the Euler sampler of the trunk, x += dt * v(x, t, embedding) from x ~ N(0, I), clamped and
 * denormalised, evaluated for every agent of a handle.  Shared bit for bit by the HIP kernel (openkitchen_amd/csrc/ok_flow.h) and the
 * host entry okenv_flow_act_host.  The image encoder is not part of it: the rule starts from its output, the
 * condition vector, which does not change over the steps of one act.
 *
 * THE RULE
 *
 * Shape.  Condition width C and hidden width H (multiples of 16 in 16 .. OK_FLOW_MAX_WIDTH), S Euler steps (1 .. OK_FLOW_MAX_STEPS),
 * 2 actions.  The reference: C = 128, H = 256, S = 32.  The device kernel's LDS plan (okenv_flow_lds_bytes) must fit 160 KB as well.
 *
 * Parameter vector (ok_flow_offsets): torch's parameters() order for the reference's ActionFlowTrunk, every matrix row-major:
 *     net.0.weight [H][3 + C]   (columns: x_0, x_1, t, then the C embedding columns)
 *     net.0.bias   [H]
 *     net.2.weight [H][H], net.2.bias [H]
 *     net.4.weight [2][H], net.4.bias [2]
 *
 * Forward of one agent with condition cond [C], fp32 throughout, nothing fused but the fmaf's written here.
 *     noise     one Philox4x32-10 block, counter = (g, draw, OK_FLOW_STREAM, 0), key = (seed, "oken"); g the global agent id, draw
 *               the act's draw index (okenv_gauss_act's contract); (x_0, x_1) = ok_gauss_normal_pair(word 0, word 1)  (ok_flow_noise).
 *               config.noise == 0: x = (0, 0), nothing is drawn.
 *     pre       the condition's share of layer 1, once:  pre_j = ok_lidar_dot(cond, W1[j] + 3, C, b1[j])  -- the fused chain over the
 *               embedding columns, k ascending, starting from the bias.
 *     Euler     for i = 0 .. S - 1, t = (float)i / (float)S, dt = 1.0f / (float)S:
 *                   h1_j = relu(fmaf(t, W1[j][2], fmaf(x_1, W1[j][1], fmaf(x_0, W1[j][0], pre_j))))          (ok_flow_hidden1)
 *                   h2_j = relu(ok_lidar_dot(h1, W2[j], H, b2[j]))
 *                   v_k  = ok_lidar_dot(h2, W3[k], H, b3[k])
 *                   x_k  = x_k + dt * v_k                                            two roundings           (ok_flow_euler)
 *     end       x_k = x_k < -1.0f ? -1.0f : (x_k > 1.0f ? 1.0f : x_k)                                        (ok_flow_clamp)
 *               a_k = ok_lidar_output(x_k, lo_k, hi_k), then clamped into [lo_k, hi_k] the same way; k = 0 throttle, 1 steering
 *
 * Against torch's Linear on cat([x, t, embedding]) the embedding columns come FIRST in layer 1's chain and x_0, x_1, t behind them:
 * a difference of rounding only, and what lets pre be computed once instead of S times.
 *
 * Philox stream 13 (counter word 2) is used by nothing else; the list of streams is in okenv_math.h.
 *
 * Only fmaf, +, *, /, comparisons and ok_gauss_normal_pair are used; compile with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_FLOW_H
#define OKENV_FLOW_H

#include "okenv_lidar.h"

#define OK_FLOW_MAX_WIDTH 512
#define OK_FLOW_MAX_STEPS 256
#define OK_FLOW_STREAM 13u

typedef struct ok_flow_shape {
    int C, H, S;
} ok_flow_shape;

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_flow_shape_bad(const ok_flow_shape s)
{
    if (s.C < 16 || s.C > OK_FLOW_MAX_WIDTH || s.C % 16 != 0) return 1;
    if (s.H < 16 || s.H > OK_FLOW_MAX_WIDTH || s.H % 16 != 0) return 1;
    if (s.S < 1 || s.S > OK_FLOW_MAX_STEPS) return 1;
    return 0;
}

/* Where the pieces of the parameter vector begin, in floats; ld1 = 3 + C is the row length of w1 */
typedef struct ok_flow_layout {
    int w1, b1, w2, b2, w3, b3, total, ld1;
} ok_flow_layout;

OK_HDI ok_flow_layout ok_flow_offsets(const ok_flow_shape s)
{
    ok_flow_layout at;
    at.ld1   = 3 + s.C;
    at.w1    = 0;
    at.b1    = at.w1 + s.H * at.ld1;
    at.w2    = at.b1 + s.H;
    at.b2    = at.w2 + s.H * s.H;
    at.w3    = at.b2 + s.H;
    at.b3    = at.w3 + 2 * s.H;
    at.total = at.b3 + 2;
    return at;
}

/* x ~ N(0, I) of (seed, global agent id, draw index) */
OK_HD void ok_flow_noise(const uint32_t seed, const uint32_t agent, const uint32_t draw, float *x0, float *x1)
{
    const ok_u32x4 b = ok_philox4x32(agent, draw, OK_FLOW_STREAM, 0u, seed, 0x6F6B656Eu);
    ok_gauss_normal_pair(b.v[0], b.v[1], x0, x1);
}

/* One unit of layer 1 behind the hoisted chain: w = W1[j], the row's first three columns */
OK_HDI float ok_flow_hidden1(const float pre, const float *w, const float x0, const float x1, const float t)
{
    return ok_lidar_relu(__builtin_fmaf(t, w[2], __builtin_fmaf(x1, w[1], __builtin_fmaf(x0, w[0], pre))));
}

OK_HDI float ok_flow_euler(const float x, const float dt, const float v)
{
    return x + dt * v;
}

OK_HDI float ok_flow_clamp(const float x, const float lo, const float hi)
{
    return x < lo ? lo : (x > hi ? hi : x);
}

/* The action from the clamped normalised sample */
OK_HDI float ok_flow_action(const float x, const float lo, const float hi)
{
    return ok_flow_clamp(ok_lidar_output(x, lo, hi), lo, hi);
}

/* Floats of work space ok_flow_forward needs: [pre | h1 | h2] */
OK_HDI int ok_flow_work_floats(const ok_flow_shape s)
{
    return 3 * s.H;
}

/* The whole sampler of one agent on the host: cond [C], x0 [2] (the noise) -> x [2], the clamped normalised sample */
OK_HD void ok_flow_forward(const ok_flow_shape s, const float *params, const float *cond, const float *x0, float *work, float *x)
{
    const ok_flow_layout at = ok_flow_offsets(s);
    const int   H = s.H;
    float      *pre = work, *h1 = pre + H, *h2 = h1 + H;
    const float dt = 1.0f / (float)s.S;
    float       xa = x0[0], xb = x0[1];
    for (int j = 0; j < H; ++j) pre[j] = ok_lidar_dot(cond, params + at.w1 + j * at.ld1 + 3, s.C, params[at.b1 + j]);
    for (int i = 0; i < s.S; ++i) {
        const float t = (float)i / (float)s.S;
        for (int j = 0; j < H; ++j) h1[j] = ok_flow_hidden1(pre[j], params + at.w1 + j * at.ld1, xa, xb, t);
        for (int j = 0; j < H; ++j) h2[j] = ok_lidar_relu(ok_lidar_dot(h1, params + at.w2 + j * H, H, params[at.b2 + j]));
        const float va = ok_lidar_dot(h2, params + at.w3, H, params[at.b3]);
        const float vb = ok_lidar_dot(h2, params + at.w3 + H, H, params[at.b3 + 1]);
        xa = ok_flow_euler(xa, dt, va);
        xb = ok_flow_euler(xb, dt, vb);
    }
    x[0] = ok_flow_clamp(xa, -1.0f, 1.0f);
    x[1] = ok_flow_clamp(xb, -1.0f, 1.0f);
}

#endif /* OKENV_FLOW_H */
