/*
 * okenv_lidar.h -- the rule of the lidar transformer driver (ImitationLearningTransformer/laser_transformer.py: LidarTransformer,
 * infer_torch_traced_main.cpp:19-43, 138-148): a point embedding, post-norm transformer encoder layers and a control head, evaluated
 * for every agent of a handle.  Shared bit for bit by the HIP kernel (openkitchen_amd/csrc/ok_lidar.h) and the host entry
 * okenv_lidar_act_host.  Inference only: dropout has no part here.
 *
 * THE RULE
 *
 * Shape.  R points (1 .. 16), d_model d, feed-forward width F, head widths H1, H2 (multiples of 16 up to the OK_LIDAR_MAX_* below),
 * nhead dividing d (head width dh = d / nhead), L layers (1 .. 8).  The device kernel's LDS plan (okenv_lidar_lds_bytes) must fit
 * 160 KB as well.
 *
 * Parameter vector (ok_lidar_offsets): torch's parameters() order for the reference module, then the positional table:
 *     point_embedding.weight [d][2], .bias [d]
 *     per layer: self_attn.in_proj_weight [3 d][d] (rows: q, k, v), in_proj_bias [3 d], self_attn.out_proj.weight [d][d], .bias [d],
 *                linear1.weight [F][d], .bias [F], linear2.weight [d][F], .bias [d], norm1.weight, .bias [d], norm2.weight, .bias [d]
 *     control_head.0.weight [H1][R d], .bias [H1], control_head.2.weight [H2][H1], .bias [H2], control_head.4.weight [2][H2], .bias [2]
 *     pos [R][d]
 * All matrices row-major as torch holds them: y = W x + b.
 *
 * Forward of one agent, fp32 throughout.
 *     input     in_{t,0} = ok_lidar_input(rel_x[t]), in_{t,1} = ok_lidar_input(rel_y[t]):  2.0f * (x - lo) / (hi - lo) - 1.0f with
 *               lo = -sensor_range, hi = sensor_range, evaluated left to right: ((2 (x - lo)) / (hi - lo)) - 1
 *     linear    every linear layer, the embedding (K = 2) included (ok_lidar_dot): ONE fused chain, k ascending, starting from the bias:
 *                   y_j = fmaf(x_{K-1}, w_{j,K-1}, ... fmaf(x_1, w_{j,1}, fmaf(x_0, w_{j,0}, b_j)))
 *               This is what an f32-input MFMA accumulating from a bias-initialised C gives.
 *     embedding x_t = linear(in_t) + pos[t]                                                      (one rounded addition)
 *     attention (ok_lidar_attend), per head h on the columns [h dh, (h + 1) dh) of q, k, v = linear(x) with the in_proj rows:
 *                   s_{tq,tk} = chain(q_tq . k_tk) * scale,  chain: fmaf over c = 0 .. dh - 1 ascending from 0.0f,
 *                                                            scale = (float)(1.0 / sqrt((double)dh))
 *                   m = max_tk s;  e_tk = ok_expf(s_tk - m);  sum = e_0 + e_1 + ... ascending from the first term;  p_tk = e_tk / sum
 *                   ctx_{tq,c} = fmaf(p_{R-1}, v_{R-1,c}, ... fmaf(p_0, v_{0,c}, 0.0f))
 *               y = linear(ctx) with out_proj
 *     post-norm x = norm1(x + y);  h = relu(linear1(x));  y = linear2(h);  x = norm2(x + y)          relu(v) = v > 0 ? v : 0
 *     LayerNorm over the d values v_c of a row (ok_lidar_sum_part, ok_lidar_sq_part, ok_lidar_den, ok_lidar_norm):
 *                   part_l = 0.0f; part_l = part_l + v_c for c = l, l + 8, ... ascending  (l = 0 .. 7);   mean = ok_gauss_tree(part) / (float)d
 *                   part_l = 0.0f; part_l = part_l + (v_c - mean) * (v_c - mean), unfused;                var  = ok_gauss_tree(part) / (float)d
 *                   out_c  = (v_c - mean) / sqrtf(var + 1e-5f) * g_c + b_c          correctly rounded divide and root, nothing fused
 *     head      z = [x_0 | x_1 | ... | x_{R-1}] (R d values);  o = linear(relu(linear(relu(linear(z)))))
 *     output    a_k = (o_k + 1.f) / 2.f * (hi_k - lo_k) + lo_k  (ok_lidar_output), nothing fused; k = 0 throttle, 1 steering
 *
 * The positional table is only added; how it is filled is the exporter's business (openkitchen_amd/imitation.py).
 *
 * Only fmaf, +, -, *, /, comparisons, the correctly rounded square root and ok_expf are used; compile with -ffp-contract=off.
 * Plain C99 / C++ / HIP.
 */
#ifndef OKENV_LIDAR_H
#define OKENV_LIDAR_H

#include "okenv_gauss.h"

#define OK_LIDAR_MAX_POINTS 16
#define OK_LIDAR_MAX_DMODEL 512
#define OK_LIDAR_MAX_FF 4096
#define OK_LIDAR_MAX_HEAD 2048
#define OK_LIDAR_MAX_LAYERS 8

typedef struct ok_lidar_shape {
    int R, d, ff, h1, h2, nhead, layers;
} ok_lidar_shape;

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_lidar_shape_bad(const ok_lidar_shape s)
{
    if (s.R < 1 || s.R > OK_LIDAR_MAX_POINTS || s.layers < 1 || s.layers > OK_LIDAR_MAX_LAYERS) return 1;
    if (s.d < 16 || s.d > OK_LIDAR_MAX_DMODEL || s.d % 16 != 0) return 1;
    if (s.ff < 16 || s.ff > OK_LIDAR_MAX_FF || s.ff % 16 != 0) return 1;
    if (s.h1 < 16 || s.h1 > OK_LIDAR_MAX_HEAD || s.h1 % 16 != 0) return 1;
    if (s.h2 < 16 || s.h2 > OK_LIDAR_MAX_HEAD || s.h2 % 16 != 0) return 1;
    if (s.nhead < 1 || s.nhead > s.d || s.d % s.nhead != 0) return 1;
    return 0;
}

/* Where the pieces of the parameter vector begin, in floats.  The pieces of layer i lie at layer0 + i * layer_stride + the in-layer
 * offsets in_w .. n2_b. */
typedef struct ok_lidar_layout {
    int emb_w, emb_b, layer0, layer_stride;
    int in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_g, n1_b, n2_g, n2_b;
    int hw0, hb0, hw1, hb1, hw2, hb2, pos, total;
} ok_lidar_layout;

OK_HDI ok_lidar_layout ok_lidar_offsets(const ok_lidar_shape s)
{
    ok_lidar_layout at;
    const int d = s.d;
    at.emb_w  = 0;
    at.emb_b  = 2 * d;
    at.layer0 = 3 * d;
    at.in_w   = 0;
    at.in_b   = at.in_w + 3 * d * d;
    at.out_w  = at.in_b + 3 * d;
    at.out_b  = at.out_w + d * d;
    at.l1_w   = at.out_b + d;
    at.l1_b   = at.l1_w + s.ff * d;
    at.l2_w   = at.l1_b + s.ff;
    at.l2_b   = at.l2_w + d * s.ff;
    at.n1_g   = at.l2_b + d;
    at.n1_b   = at.n1_g + d;
    at.n2_g   = at.n1_b + d;
    at.n2_b   = at.n2_g + d;
    at.layer_stride = at.n2_b + d;
    at.hw0    = at.layer0 + s.layers * at.layer_stride;
    at.hb0    = at.hw0 + s.h1 * s.R * d;
    at.hw1    = at.hb0 + s.h1;
    at.hb1    = at.hw1 + s.h2 * s.h1;
    at.hw2    = at.hb1 + s.h2;
    at.hb2    = at.hw2 + 2 * s.h2;
    at.pos    = at.hb2 + 2;
    at.total  = at.pos + s.R * d;
    return at;
}

OK_HDI float ok_lidar_input(const float x, const float range)
{
    const float lo = -range, hi = range;
    return 2.0f * (x - lo) / (hi - lo) - 1.0f;
}

OK_HDI float ok_lidar_output(const float o, const float lo, const float hi)
{
    return (o + 1.f) / 2.f * (hi - lo) + lo;
}

OK_HDI float ok_lidar_relu(const float v)
{
    return v > 0.0f ? v : 0.0f;
}

/* One output of a linear layer: the fused chain over k ascending from the bias */
OK_HDI float ok_lidar_dot(const float *x, const float *w, const int K, const float bias)
{
    float acc = bias;
    for (int k = 0; k < K; ++k) acc = __builtin_fmaf(x[k], w[k], acc);
    return acc;
}

/* One head's attention for one query: q [dh]; k, v: token t's [dh] at k + t * tstride; p [R] is work space; out [dh] */
OK_HDI void ok_lidar_attend(const float *q, const float *k, const float *v, const int tstride, const int R, const int dh, const float scale, float *p,
                            float *out)
{
    float m = 0.0f;
    for (int t = 0; t < R; ++t) {
        const float s = ok_lidar_dot(q, k + t * tstride, dh, 0.0f) * scale;
        p[t] = s;
        m = (t == 0 || s > m) ? s : m;
    }
    float sum = 0.0f;
    for (int t = 0; t < R; ++t) {
        const float e = ok_expf(p[t] - m);
        p[t] = e;
        sum = t == 0 ? e : sum + e;
    }
    for (int t = 0; t < R; ++t) p[t] = p[t] / sum;
    for (int c = 0; c < dh; ++c) {
        float acc = 0.0f;
        for (int t = 0; t < R; ++t) acc = __builtin_fmaf(p[t], v[t * tstride + c], acc);
        out[c] = acc;
    }
}

/* LayerNorm's partial sums of lane l over a row v [n] */
OK_HDI float ok_lidar_sum_part(const float *v, const int n, const int l)
{
    float s = 0.0f;
    for (int c = l; c < n; c += OK_ACTOR_LANES) s = s + v[c];
    return s;
}

OK_HDI float ok_lidar_sq_part(const float *v, const int n, const int l, const float mean)
{
    float s = 0.0f;
    for (int c = l; c < n; c += OK_ACTOR_LANES) {
        const float dv = v[c] - mean;
        s = s + dv * dv;
    }
    return s;
}

/* sqrtf(var + eps): the fp64 root rounded once is the correctly rounded fp32 root */
OK_HDI float ok_lidar_den(const float var)
{
    return (float)__builtin_sqrt((double)(var + 1e-5f));
}

OK_HDI float ok_lidar_norm(const float v, const float mean, const float den, const float g, const float b)
{
    return (v - mean) / den * g + b;
}

/* (float)(1.0 / sqrt((double)dh)) */
OK_HD float ok_lidar_scale(const int dh)
{
    return (float)(1.0 / __builtin_sqrt((double)dh));
}

/* x [R][d] = LayerNorm(x + y) in place, row by row */
OK_HD void ok_lidar_add_norm(float *x, const float *y, const int R, const int d, const float *g, const float *b)
{
    for (int t = 0; t < R; ++t) {
        float *row = x + t * d;
        float part[OK_ACTOR_LANES];
        for (int c = 0; c < d; ++c) row[c] = row[c] + y[t * d + c];
        for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = ok_lidar_sum_part(row, d, l);
        const float mean = ok_gauss_tree(part) / (float)d;
        for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = ok_lidar_sq_part(row, d, l, mean);
        const float den = ok_lidar_den(ok_gauss_tree(part) / (float)d);
        for (int c = 0; c < d; ++c) row[c] = ok_lidar_norm(row[c], mean, den, g[c], b[c]);
    }
}

/* Floats of work space ok_lidar_forward needs: x, y, q, k, v [R][d]; h, first the attention's context [R][d], then the feed-forward's
 * hidden layer [R][ff] (ff may be smaller than d); p [R]; the head's hidden layers */
OK_HDI int ok_lidar_hidden_floats(const ok_lidar_shape s)
{
    return s.R * (s.ff > s.d ? s.ff : s.d);
}

OK_HDI int ok_lidar_work_floats(const ok_lidar_shape s)
{
    return 5 * s.R * s.d + ok_lidar_hidden_floats(s) + s.R + s.h1 + s.h2;
}

/* The whole forward of one agent on the host: in [R][2] (normalised points) -> o [2] (normalised controls) */
OK_HD void ok_lidar_forward(const ok_lidar_shape s, const float *params, const float *in, float *work, float *o)
{
    const ok_lidar_layout at = ok_lidar_offsets(s);
    const int R = s.R, d = s.d, dh = s.d / s.nhead;
    float *x = work, *y = x + R * d, *q = y + R * d, *k = q + R * d, *v = k + R * d, *h = v + R * d, *p = h + ok_lidar_hidden_floats(s), *g1 = p + R, *g2 = g1 + s.h1;
    const float scale = ok_lidar_scale(dh);
    for (int t = 0; t < R; ++t)
        for (int c = 0; c < d; ++c)
            x[t * d + c] = ok_lidar_dot(in + 2 * t, params + at.emb_w + 2 * c, 2, params[at.emb_b + c]) + params[at.pos + t * d + c];
    for (int i = 0; i < s.layers; ++i) {
        const float *lp = params + at.layer0 + i * at.layer_stride;
        for (int t = 0; t < R; ++t)
            for (int c = 0; c < d; ++c) {
                q[t * d + c] = ok_lidar_dot(x + t * d, lp + at.in_w + c * d, d, lp[at.in_b + c]);
                k[t * d + c] = ok_lidar_dot(x + t * d, lp + at.in_w + (d + c) * d, d, lp[at.in_b + d + c]);
                v[t * d + c] = ok_lidar_dot(x + t * d, lp + at.in_w + (2 * d + c) * d, d, lp[at.in_b + 2 * d + c]);
            }
        /* the context goes to h (free until the feed-forward) */
        for (int t = 0; t < R; ++t)
            for (int hd = 0; hd < s.nhead; ++hd) ok_lidar_attend(q + t * d + hd * dh, k + hd * dh, v + hd * dh, d, R, dh, scale, p, h + t * d + hd * dh);
        for (int t = 0; t < R; ++t)
            for (int c = 0; c < d; ++c) y[t * d + c] = ok_lidar_dot(h + t * d, lp + at.out_w + c * d, d, lp[at.out_b + c]);
        ok_lidar_add_norm(x, y, R, d, lp + at.n1_g, lp + at.n1_b);
        for (int t = 0; t < R; ++t)
            for (int f = 0; f < s.ff; ++f) h[t * s.ff + f] = ok_lidar_relu(ok_lidar_dot(x + t * d, lp + at.l1_w + f * d, d, lp[at.l1_b + f]));
        for (int t = 0; t < R; ++t)
            for (int c = 0; c < d; ++c) y[t * d + c] = ok_lidar_dot(h + t * s.ff, lp + at.l2_w + c * s.ff, s.ff, lp[at.l2_b + c]);
        ok_lidar_add_norm(x, y, R, d, lp + at.n2_g, lp + at.n2_b);
    }
    for (int j = 0; j < s.h1; ++j) g1[j] = ok_lidar_relu(ok_lidar_dot(x, params + at.hw0 + j * R * d, R * d, params[at.hb0 + j]));
    for (int j = 0; j < s.h2; ++j) g2[j] = ok_lidar_relu(ok_lidar_dot(g1, params + at.hw1 + j * s.h1, s.h1, params[at.hb1 + j]));
    for (int j = 0; j < 2; ++j) o[j] = ok_lidar_dot(g2, params + at.hw2 + j * s.h2, s.h2, params[at.hb2 + j]);
}

#endif /* OKENV_LIDAR_H */
