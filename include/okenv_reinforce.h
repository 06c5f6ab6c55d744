/*
 * okenv_reinforce.h -- the rule of REINFORCE's network and update (RLRacers/Reinforce/Policy.hpp:22-29, ReinforceAgent.hpp:71-123),
 * shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_actor.h, ok_reinforce.h) and the host entries
 * okenv_actor_act_dropout_host and okenv_reinforce_update_host.  It stands on the actor's rule (okenv_math.h,
 * ok_actor_*) and the learner's (okenv_learn.h, ok_learn_*).
 *
 * THE RULE
 *
 * Dropout.  Policy::forward is affine1 -> Dropout(0.6) -> relu -> affine2 -> softmax, in training mode while acting and in the update.
 * Parameters: p in [0, 1) and a dropout_seed; the scale is s = 1.0f / (1.0f - p), one IEEE fp32 division (ok_reinforce_scale).  The
 * mask covers the hidden units of the POLICY network only, never a value network, and belongs to a (global agent id g, draw index d):
 * while acting d is the actor's draw index, in the update it is recomputed from the sample's flat index, never stored.
 *     hidden unit j:  one Philox4x32-10 block with counter = (g, d, 9, b(j)), key = (dropout_seed, "oken"),
 *                     b(j) = (j mod 8) + 8 * (j div 32); the word used is (j div 8) mod 4; kept iff ok_u01(word) >= p.
 * Stream 9 is used by nothing else (the list is in okenv_math.h).  The layout is the one the actor's interleave of 8 lanes per
 * sample wants: lane l owns the units l, l + 8, ... and needs one block per four of them, block l + 8 n for its units 4 n .. 4 n + 3
 * (ok_reinforce_kept_lane; ok_reinforce_kept is the same thing by j).  It depends on j only, on no launch shape and not on H.
 *     pre_j  = b1[j] + w1[j][0] * x[0] + ... ascending: section 14's sum (ok_learn_pre's expression)
 *     h_j    = kept ? relu(pre_j * s) : 0.0f          one fp32 multiplication; relu(v) = v > 0 ? v : 0
 * Everything behind the hidden layer is the actor's rule unchanged: the 8 interleaved partial sums, their tree, the softmax through
 * ok_expf, the clamp, the draw on stream 6, the action table.  With p == 0 no mask is evaluated and the result is section 14's, bit
 * for bit (s is 1.0f and pre_j * 1.0f is pre_j).
 *
 * The loss and its seed (ok_reinforce_seed).  Sample k has action a, normalised return G and the softmax q of its state, recomputed
 * with the sample's own mask from the current parameters: before the first step q_a equals the recorded probability bit for bit.
 *     term   = -(ok_logf(clamp(q_a)) * G)                 clamp to [1e-8f, 1.0f]: ok_actor_clamp_prob
 *     ind_i  = i == a ? 1.0f : 0.0f;  diff_i = ind_i - q_i;  prod_i = G * diff_i;  dz_i = -prod_i        q_i = e_i / S, unclamped
 * A probability q_a that the clamp moved contributes dz = 0 for every i (section 16's convention), its term stays finite.  The
 * reference takes the logarithm of the unclamped softmax (ReinforceAgent.hpp:79); the clamp is the shared actor's.
 *     layer 2:  dW2[k][j] = dz_k * h_j,  db2[k] = dz_k;   dh_j = w2[0][j] * dz_0 + w2[1][j] * dz_1 + ... ascending k
 *     hidden:   dpre_j = (kept && pre_j * s > 0) ? dh_j * s : 0.0f
 *     layer 1:  dW1[j][i] = dpre_j * x_i,  db1[j] = dpre_j
 * All fp32, a separate multiplication and addition per term, nothing fused.
 *
 * Sums.  Section 16's: chunks of OK_LEARN_CHUNK consecutive positions, acc = 0.0f; acc = acc + term ascending within a chunk
 * (ok_learn_term), ok_learn_tree over the chunk partials.  The loss term is one more column behind the parameters.
 *
 * Slices.  The M samples (position q is sample order[q], or q without an order; an index outside 0 .. M-1 counts as the nearest valid
 * one) are cut into ceil(M / B) slices of B consecutive positions, the last one shorter.  A slice's column sums are formed as above
 * with the parameters of the moment.
 *     accumulate != 0 (the reference: one optimiser step per updatePolicy): an fp32 accumulator column starts at 0.0f and takes
 *                     acc = acc + slice_sum in ascending slice order; after the last slice ONE Adam step with count = M.
 *     accumulate == 0 (minibatch REINFORCE): one Adam step after every slice with count = the slice's length.
 *     reduce          OK_REINFORCE_SUM: gradient and loss are the sums (the reference's loss +=);
 *                     OK_REINFORCE_MEAN: each divided once by (float)count after the join, one IEEE division.
 * Adam is ok_learn_adam with the host's fp64 factors of step number t (ok_learn_factors); t, m and v are the section 16 learner's.
 *
 * Only +, -, *, /, comparisons, ok_expf and ok_logf are used; compile with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_REINFORCE_H
#define OKENV_REINFORCE_H

#include "okenv_learn.h"

#define OK_REINFORCE_STREAM 9u
#define OK_REINFORCE_SUM 0
#define OK_REINFORCE_MEAN 1

/* Whose mask: p, its scale, the key and the counter's first two words */
typedef struct ok_reinforce_mask {
    float    p, s;
    uint32_t seed, agent, draw;
} ok_reinforce_mask;

OK_HDI float ok_reinforce_scale(const float p)
{
    return 1.0f / (1.0f - p);
}

/* Whether the lane-l unit number i (hidden unit j = l + 8 i) is kept; r holds the lane's current block and is refilled every four
 * units, so a lane walks its units in ascending i.  With p == 0 nothing is evaluated. */
OK_HDI int ok_reinforce_kept_lane(const ok_reinforce_mask m, ok_u32x4 *r, const int l, const int i)
{
    if (!(m.p > 0.0f)) return 1;
    const int w = i & 3;
    if (w == 0) *r = ok_philox4x32(m.agent, m.draw, OK_REINFORCE_STREAM, (uint32_t)(l + 8 * (i >> 2)), m.seed, 0x6F6B656Eu);
    const uint32_t word = w == 0 ? r->v[0] : (w == 1 ? r->v[1] : (w == 2 ? r->v[2] : r->v[3]));
    return ok_u01(word) >= m.p;
}

/* The same by hidden unit j */
OK_HD int ok_reinforce_kept(const ok_reinforce_mask m, const int j)
{
    if (!(m.p > 0.0f)) return 1;
    const ok_u32x4 r = ok_philox4x32(m.agent, m.draw, OK_REINFORCE_STREAM, (uint32_t)((j % 8) + 8 * (j / 32)), m.seed, 0x6F6B656Eu);
    return ok_u01(r.v[(j / 8) % 4]) >= m.p;
}

OK_HDI float ok_reinforce_hidden(const float pre, const int kept, const float s)
{
    const float v = pre * s;
    return (kept && v > 0.0f) ? v : 0.0f;
}

/* ok_actor_partial with the mask: the partial sums of interleave lane l for every output */
OK_HDI void ok_reinforce_partial(const float *w1, const int w1_stride, const float *b1, const float *w2, const int in, const int hidden, const int out,
                                 const float *x, const int l, const ok_reinforce_mask m, float *part)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < out) part[k] = 0.0f;
    ok_u32x4 r;
    r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0u;
    for (int j = l, i = 0; j < hidden; j += OK_ACTOR_LANES, ++i) {
        const int kept = ok_reinforce_kept_lane(m, &r, l, i);
        const float h = ok_reinforce_hidden(ok_learn_pre(w1, w1_stride, b1, in, x, j), kept, m.s);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
            if (k < out) part[k] = part[k] + w2[k * hidden + j] * h;
    }
}

/* dpre_j from the output seeds dz[0 .. out-1] (dz has OK_ACTOR_MAX_ACTIONS entries) and the pre-activation of unit j */
OK_HDI float ok_reinforce_back_hidden(const float *w2, const int hidden, const int out, const float *dz, const int j, const float pre, const int kept,
                                      const float s)
{
    float d = w2[j] * dz[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < out) d = d + w2[k * hidden + j] * dz[k];
    return (kept && pre * s > 0.0f) ? d * s : 0.0f;
}

/* From the logits of one sample to the seeds dz[0 .. n-1] and the loss term.  z and dz have OK_ACTOR_MAX_ACTIONS entries; `action` is
 * already inside 0 .. n-1. */
OK_HDI void ok_reinforce_seed(const float *z, const int n, const int action, const float G, float *dz, float *term)
{
    float e[OK_ACTOR_MAX_ACTIONS];
    float m = z[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n && z[k] > m) m = z[k];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        e[k] = k < n ? ok_expf(z[k] - m) : 0.0f;
    float qa; /* the actor's clamped probability of `action` */
    (void)ok_actor_pick(e, n, 0.0f, action, &qa);
    float s = e[0]; /* ok_actor_pick's sum */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n) s = s + e[k];
    float ya = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k == action) ya = e[k] / s;
    *term = -(ok_logf(qa) * G);
    const int passes = ya >= OK_ACTOR_PROB_MIN && ya <= OK_ACTOR_PROB_MAX;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k) {
        const float ind = k == action ? 1.0f : 0.0f;
        const float diff = ind - e[k] / s;
        const float prod = G * diff;
        dz[k] = (k < n && passes) ? -prod : 0.0f;
    }
}

/* The gradient (or loss) of a step from its joined sum */
OK_HDI float ok_reinforce_reduce(const float sum, const int reduce, const float count)
{
    return reduce == OK_REINFORCE_MEAN ? sum / count : sum;
}

#endif /* OKENV_REINFORCE_H */
