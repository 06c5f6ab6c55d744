/*
 * okenv_vithead.h -- the rule of the training of the image transformer driver's policy head (DinoControl/train_dino_control.py: the
 * backbone is frozen, its embeddings are computed once, and the 384-128-64-1 head alone is trained with a weighted squared error and
 * Adam).  Shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_vithead.h) and the host entries okenv_vit_head_update_host /
 * okenv_vit_head_eval_host.
 *
 * THE RULE
 *
 * Data.  M samples: embedding [M][D], what okenv_vit_act records (the class token behind the final LayerNorm), and steer [M], the
 * recorded steering delta.  The head is D -> H1 -> H2 -> 1 with ReLU between, its parameters the tail of the driver's parameter vector
 * (ok_vithead_offsets; okenv_vit.h's hw0 .. hb2):  W1 [H1][D], b1 [H1], W2 [H2][H1], b2 [H2], w3 [1][H2], b3 [1].
 *
 * Label and weight (ok_vithead_label, ok_vithead_weight).
 *     y = steer / steer_scale (one IEEE division), then y < -1 ? -1 : (y > 1 ? 1 : y)        a NaN passes through
 *     w = |y| > threshold ? weight : 1.0f                                                     |y| exactly at the threshold: 1
 * The reference's values: weight 5, threshold 0.1, batch 512, Adam 1e-4, no shuffle, 50 epochs.
 *
 * Minibatches.  okenv_learn.h's: epoch e cuts the M samples into ceil(M / B) minibatches; minibatch k holds the B_k = min(B, M - k B)
 * positions q = 0 .. B_k - 1, and position q is sample order[e][k B + q], or k B + q without an order.  An index outside 0 .. M-1
 * counts as the nearest valid one (ok_learn_clamp_index).  One Adam step per minibatch; every forward of a minibatch uses the
 * parameters from before its step.
 *
 * Forward.  The act's head and nothing else (okenv_vit.h): ok_lidar_dot's chain from the bias, k ascending, fused; ok_lidar_relu.
 *     s1_j = dot(e, W1[j], b1[j]),  h1_j = relu(s1_j);   s2_k = dot(h1, W2[k], b2[k]),  h2_k = relu(s2_k);   o = dot(h2, w3, b3)
 * An embedding evaluated with unchanged parameters therefore reproduces the act's recorded `output` bit for bit.
 *
 * Loss and seeds (ok_vithead_seed), nothing fused here.
 *     t    = w * ((o - y) * (o - y))                      the position's loss term
 *     do   = (2.0f * w) * (o - y)
 *     d2_k = s2_k > 0 ? w3[k] * do : 0.0f                 ReLU's derivative at 0 is 0
 *     d1_j = s1_j > 0 ? chain : 0.0f,  chain: acc = +0.0f;  acc = fmaf(W2[k][j], d2_k, acc) for k = 0 .. H2-1 ascending
 *
 * Sums.  The order belongs to the rule, never to a launch.  A minibatch's positions are cut into chunks of OK_VITHEAD_CHUNK = 64
 * consecutive positions.  Within a chunk every parameter's partial is ONE chain from +0.0f, ascending in position:
 *     weights   acc = fmaf(delta_q, a_q, acc)     (delta, a) = (d1_j, e_i) for W1[j][i], (d2_k, h1_j) for W2[k][j], (do, h2_k) for w3[k]
 *     biases    acc = acc + delta_q               which is fmaf(delta_q, 1.0f, acc) bit for bit: the device computes it so
 *     loss      acc = acc + t_q
 * The chunk partials are joined by plain additions ascending in chunk, starting from chunk 0's partial: ((p_0 + p_1) + p_2) + ...
 * The factor 1 / B_k is applied ONCE, after the join: gradient = joined / (float)B_k, loss = joined / (float)B_k, each one IEEE
 * division.
 *     ZERO TERMS.  The last chunk of a minibatch whose B_k is no multiple of 64 is filled up to 64 positions with filler positions
 *     whose delta, t and a are +0.0f (a is 1.0f in a bias's chain).  A filler term is acc + (+0.0f): it leaves every acc as it was,
 *     with one exception, acc = -0.0f becomes +0.0f (a chain from +0.0f reaches -0.0f only when a product underflows to it).  The
 *     fillers belong to the rule: a partial chunk's partials end with one addition of +0.0f (ok_vithead_fill), which is what any
 *     number of filler terms amounts to; a full chunk has none.
 *
 * Adam.  ok_learn_adam with ok_learn_factors (okenv_learn.h), unchanged; t, m and v persist across calls.
 *
 * Eval.  The same per-minibatch loss with no update (the reference's validation loop); sequential order.
 *
 * Only fmaf, +, -, *, /, comparisons and the correctly rounded square root are used; compile with -ffp-contract=off.
 * Plain C99 / C++ / HIP.
 */
#ifndef OKENV_VITHEAD_H
#define OKENV_VITHEAD_H

#include "okenv_learn.h"
#include "okenv_lidar.h"

#define OK_VITHEAD_CHUNK 64

/* Where the head's pieces begin, in floats from its first weight (okenv_vit.h's hw0) */
typedef struct ok_vithead_layout {
    int w1, b1, w2, b2, w3, b3, total;
} ok_vithead_layout;

OK_HDI ok_vithead_layout ok_vithead_offsets(const int D, const int H1, const int H2)
{
    ok_vithead_layout at;
    at.w1    = 0;
    at.b1    = at.w1 + H1 * D;
    at.w2    = at.b1 + H1;
    at.b2    = at.w2 + H2 * H1;
    at.w3    = at.b2 + H2;
    at.b3    = at.w3 + H2;
    at.total = at.b3 + 1;
    return at;
}

/* 0 when the head's widths are inside okenv_vit.h's limits */
OK_HDI int ok_vithead_shape_bad(const int D, const int H1, const int H2)
{
    if (D < 16 || D > 768 || D % 16 != 0) return 1;
    if (H1 < 16 || H1 > 2048 || H1 % 16 != 0) return 1;
    if (H2 < 16 || H2 > 2048 || H2 % 16 != 0) return 1;
    return 0;
}

OK_HDI float ok_vithead_label(const float steer, const float steer_scale)
{
    const float y = steer / steer_scale;
    return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y);
}

OK_HDI float ok_vithead_weight(const float y, const float threshold, const float weight)
{
    const float a = y < 0.0f ? -y : y;
    return a > threshold ? weight : 1.0f;
}

/* The position's loss term and the output's seed */
OK_HDI void ok_vithead_seed(const float o, const float y, const float w, float *t, float *d_o)
{
    const float e = o - y;
    *t   = w * (e * e);
    *d_o = (2.0f * w) * e;
}

/* h2k: relu(s2_k), which is > 0 exactly where s2_k is */
OK_HDI float ok_vithead_d2(const float h2k, const float w3k, const float d_o)
{
    return h2k > 0.0f ? w3k * d_o : 0.0f;
}

/* d1_j from d2 [H2]; h1j: relu(s1_j) */
OK_HDI float ok_vithead_d1(const float h1j, const float *w2, const int H1, const int H2, const float *d2, const int j)
{
    float acc = 0.0f;
    for (int k = 0; k < H2; ++k) acc = __builtin_fmaf(w2[k * H1 + j], d2[k], acc);
    return h1j > 0.0f ? acc : 0.0f;
}

/* What the fillers of a partial chunk leave of a partial */
OK_HDI float ok_vithead_fill(const float acc)
{
    return acc + 0.0f;
}

/* One position: embedding row e [D] and its steering -> h1 [H1], h2 [H2], d1 [H1], d2 [H2], *d_o, *t; returns the output o */
OK_HD float ok_vithead_position(const float *head, const int D, const int H1, const int H2, const float *e, const float steer, const float steer_scale,
                                const float weight, const float threshold, float *h1, float *h2, float *d1, float *d2, float *d_o, float *t)
{
    const ok_vithead_layout at = ok_vithead_offsets(D, H1, H2);
    for (int j = 0; j < H1; ++j) h1[j] = ok_lidar_relu(ok_lidar_dot(e, head + at.w1 + (long)j * D, D, head[at.b1 + j]));
    for (int k = 0; k < H2; ++k) h2[k] = ok_lidar_relu(ok_lidar_dot(h1, head + at.w2 + (long)k * H1, H1, head[at.b2 + k]));
    const float o = ok_lidar_dot(h2, head + at.w3, H2, head[at.b3]);
    const float y = ok_vithead_label(steer, steer_scale);
    ok_vithead_seed(o, y, ok_vithead_weight(y, threshold, weight), t, d_o);
    for (int k = 0; k < H2; ++k) d2[k] = ok_vithead_d2(h2[k], head[at.w3 + k], *d_o);
    for (int j = 0; j < H1; ++j) d1[j] = ok_vithead_d1(h1[j], head + at.w2, H1, H2, d2, j);
    return o;
}

#endif /* OKENV_VITHEAD_H */
