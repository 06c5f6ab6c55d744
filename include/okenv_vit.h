/*
 * okenv_vit.h -- the rule of the image transformer driver (DinoControl/: a frozen vision transformer, timm's
 * vit_small_patch8_224.dino, and a 384-128-64-1 policy head on its class token, driven as main_dino_control.cpp:80-89 drives them): the
 * camera's RGBA8 frame of an agent -> its steering.  Shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_vit.h) and the host
 * entry okenv_vit_act_host.  Inference only.
 *
 * THE RULE
 *
 * Shape.  Square frames of side S, patches of side P in {4, 8, 16}, S a multiple of P; T = (S / P)^2 + 1 tokens, at most 1024; width
 * D (a multiple of 16, 16 .. 768); `heads` heads of dh = D / heads (a multiple of 16, at most 64); depth 1 .. 12 pre-norm blocks;
 * feed-forward F (a multiple of 16, 16 .. 4 D); head widths H1, H2 (multiples of 16, 16 .. 2048).  The device's LDS plan
 * (okenv_vit_lds_bytes) must fit 160 KB as well.  The reference: S 224, P 8, D 384, 6 heads, depth 12, F 1536, head 128 / 64.
 *
 * Parameter vector (ok_vit_offsets): torch's parameters() order of openkitchen_amd/dino.py's ViT (timm's names):
 *     cls_token [1][1][D], pos_embed [1][T][D], patch_embed.proj.weight [D][3][P][P], patch_embed.proj.bias [D]
 *     per block: norm1.weight, norm1.bias [D], attn.qkv.weight [3 D][D], attn.qkv.bias [3 D], attn.proj.weight [D][D], attn.proj.bias [D],
 *                norm2.weight, norm2.bias [D], mlp.fc1.weight [F][D], mlp.fc1.bias [F], mlp.fc2.weight [D][F], mlp.fc2.bias [D]
 *     norm.weight, norm.bias [D]
 *     head.net.0.weight [H1][D], .bias [H1], head.net.2.weight [H2][H1], .bias [H2], head.output_layer.weight [1][H2], .bias [1]
 * All matrices row-major as torch holds them: y = W x + b.  Every weight must be finite.
 *
 * Forward of one frame [S][S][4] uint8 (R, G, B, A; row 0 first), fp32 throughout, nothing fused but the fmaf's written here.
 *     input     ok_vit_input: (ok_bev_pixel(byte) - mean_c) / std_c, the IEEE division twice.  Alpha is not an input.  The frames are
 *               rendered at S; no resize is part of the rule.
 *     patches   token 1 + py (S / P) + px: for every column n, ONE fused chain from patch_embed.proj.bias[n] over k = (c P + r) P + col
 *               ascending (torch's Conv2d weight order: channel, row, column), K = 3 P P terms, of input(c, py P + r, px P + col)
 *               times weight[n][k]; then one rounded addition of pos_embed[token][n].  Token 0 is cls_token[n] + pos_embed[0][n].
 *     linear    every linear layer is ok_lidar_dot's chain: bias first, k ascending, fused.
 *     block     x = x + proj(attn(LN1(x)));  x = x + fc2(gelu(fc1(LN2(x)))): each residual one rounded addition.
 *     attention per head h on the columns of qkv = linear(LN1(x)) split as timm's reshape(T, 3, heads, dh): q at h dh, k at D + h dh,
 *               v at 2 D + h dh (ok_vit_attend; ok_lidar_attend's definitions but for the sum):
 *                   s_{tq,tk} = chain(q_tq . k_tk) * scale,  chain: fmaf over c = 0 .. dh - 1 ascending from 0.0f,
 *                                                            scale = (float)(1.0 / sqrt((double)dh))  (ok_lidar_scale)
 *                   m = max_tk s;  e_tk = ok_expf(s_tk - m)
 *                   sum: OK_ACTOR_LANES = 8 interleaved partials, part_l = 0.0f; part_l = part_l + e_tk for tk = l, l + 8, ... ascending;
 *                        sum = ok_gauss_tree(part)  -- NOT one sequential chain: with up to 1024 keys eight lanes share a row
 *                   p_tk = e_tk / sum  (IEEE)
 *                   ctx_{tq,c} = fmaf(p_{T-1}, v_{T-1,c}, ... fmaf(p_0, v_{0,c}, 0.0f))
 *               ZERO TERMS.  The device's context chain contains, behind key T - 1, up to 15 filler keys with p = 0.0f and v = -0.0f: each
 *               is fmaf(0.0f, -0.0f, acc) = acc + (-0) = acc for every acc, the sign of a zero included.
 *     LayerNorm section 22's partial sums (ok_lidar_sum_part, ok_lidar_sq_part, ok_lidar_norm) with the config's eps inside the root
 *               (ok_vit_den): mean = tree(part) / (float)D;  var = tree(part) / (float)D;  (v - mean) / sqrtf(var + eps) * g + b
 *     GELU      ok_vit_gelu, five rounded operations in this order, nothing fused:
 *                   t = x * 0.70710678f;  t = ok_erff(t);  t = 1.0f + t;  t = x * t;  t = 0.5f * t
 *     final     LayerNorm (norm) of the class token's row only: the embedding [D]
 *     head      o = linear(relu(linear(relu(linear(embedding)))))  with ok_lidar_relu, widths H1, H2, 1
 *     action    throttle_delta = throttle;  steering_delta = clamp(o * steer_scale, -steer_scale, steer_scale) (ok_vit_steer):
 *               v = o * steer_scale; v < -steer_scale ? -steer_scale : (v > steer_scale ? steer_scale : v); a NaN passes through
 *
 * Only fmaf, +, -, *, /, comparisons, the correctly rounded square root, ok_expf and ok_erff are used; compile with -ffp-contract=off.
 * Plain C99 / C++ / HIP.
 */
#ifndef OKENV_VIT_H
#define OKENV_VIT_H

#include "okenv_bev.h"
#include "okenv_lidar.h"

#define OK_VIT_MAX_TOKENS 1024
#define OK_VIT_MAX_DIM 768
#define OK_VIT_MAX_HEAD_DIM 64
#define OK_VIT_MAX_DEPTH 12
#define OK_VIT_MAX_HEAD 2048

typedef struct ok_vit_shape {
    int S, P, D, heads, depth, ff, h1, h2;
} ok_vit_shape;

/* What the forward needs of the config beside the shape */
typedef struct ok_vit_consts {
    float mean[3], std[3], eps, throttle, steer_scale;
} ok_vit_consts;

OK_HDI int ok_vit_side(const ok_vit_shape s)
{
    return s.S / s.P;
}

OK_HDI int ok_vit_tokens(const ok_vit_shape s)
{
    return ok_vit_side(s) * ok_vit_side(s) + 1;
}

OK_HDI int ok_vit_patch_k(const ok_vit_shape s)
{
    return 3 * s.P * s.P;
}

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_vit_shape_bad(const ok_vit_shape s)
{
    if (s.P != 4 && s.P != 8 && s.P != 16) return 1;
    if (s.S < s.P || s.S > 16 * OK_VIT_MAX_TOKENS || s.S % s.P != 0) return 1;
    if (ok_vit_side(s) > 32 || ok_vit_tokens(s) > OK_VIT_MAX_TOKENS) return 1;
    if (s.D < 16 || s.D > OK_VIT_MAX_DIM || s.D % 16 != 0) return 1;
    if (s.heads < 1 || s.heads > s.D || s.D % s.heads != 0) return 1;
    if ((s.D / s.heads) % 16 != 0 || s.D / s.heads > OK_VIT_MAX_HEAD_DIM) return 1;
    if (s.depth < 1 || s.depth > OK_VIT_MAX_DEPTH) return 1;
    if (s.ff < 16 || s.ff > 4 * s.D || s.ff % 16 != 0) return 1;
    if (s.h1 < 16 || s.h1 > OK_VIT_MAX_HEAD || s.h1 % 16 != 0) return 1;
    if (s.h2 < 16 || s.h2 > OK_VIT_MAX_HEAD || s.h2 % 16 != 0) return 1;
    return 0;
}

/* Where the pieces of the parameter vector begin, in floats.  The pieces of block i lie at block0 + i * block_stride + the in-block
 * offsets n1_g .. fc2_b.  (The largest shape has 86 million parameters: int holds them.) */
typedef struct ok_vit_layout {
    int cls, pos, pe_w, pe_b, block0, block_stride;
    int n1_g, n1_b, qkv_w, qkv_b, proj_w, proj_b, n2_g, n2_b, fc1_w, fc1_b, fc2_w, fc2_b;
    int norm_g, norm_b, hw0, hb0, hw1, hb1, hw2, hb2, total;
} ok_vit_layout;

OK_HDI ok_vit_layout ok_vit_offsets(const ok_vit_shape s)
{
    ok_vit_layout at;
    const int D = s.D, T = ok_vit_tokens(s);
    at.cls    = 0;
    at.pos    = D;
    at.pe_w   = at.pos + T * D;
    at.pe_b   = at.pe_w + D * ok_vit_patch_k(s);
    at.block0 = at.pe_b + D;
    at.n1_g   = 0;
    at.n1_b   = at.n1_g + D;
    at.qkv_w  = at.n1_b + D;
    at.qkv_b  = at.qkv_w + 3 * D * D;
    at.proj_w = at.qkv_b + 3 * D;
    at.proj_b = at.proj_w + D * D;
    at.n2_g   = at.proj_b + D;
    at.n2_b   = at.n2_g + D;
    at.fc1_w  = at.n2_b + D;
    at.fc1_b  = at.fc1_w + s.ff * D;
    at.fc2_w  = at.fc1_b + s.ff;
    at.fc2_b  = at.fc2_w + D * s.ff;
    at.block_stride = at.fc2_b + D;
    at.norm_g = at.block0 + s.depth * at.block_stride;
    at.norm_b = at.norm_g + D;
    at.hw0    = at.norm_b + D;
    at.hb0    = at.hw0 + s.h1 * D;
    at.hw1    = at.hb0 + s.h1;
    at.hb1    = at.hw1 + s.h2 * s.h1;
    at.hw2    = at.hb1 + s.h2;
    at.hb2    = at.hw2 + s.h2;
    at.total  = at.hb2 + 1;
    return at;
}

OK_HDI float ok_vit_input(const uint8_t byte, const float mean, const float std)
{
    return (ok_bev_pixel(byte) - mean) / std;
}

/* Term k of a patch's chain: the input of frame [S][S][4] at patch (py, px), k = (c P + r) P + col */
OK_HDI float ok_vit_patch_input(const uint8_t *frame, const int S, const int P, const int py, const int px, const int k, const float *mean,
                                const float *std)
{
    const int c = k / (P * P), r = (k / P) % P, col = k % P;
    return ok_vit_input(frame[((py * P + r) * S + px * P + col) * 4 + c], mean[c], std[c]);
}

OK_HDI float ok_vit_gelu(const float x)
{
    float t = x * 0.70710678f;
    t = ok_erff(t);
    t = 1.0f + t;
    t = x * t;
    t = 0.5f * t;
    return t;
}

/* sqrtf(var + eps): the fp64 root rounded once is the correctly rounded fp32 root */
OK_HDI float ok_vit_den(const float var, const float eps)
{
    return (float)__builtin_sqrt((double)(var + eps));
}

OK_HDI float ok_vit_steer(const float o, const float steer_scale)
{
    const float v = o * steer_scale;
    return v < -steer_scale ? -steer_scale : (v > steer_scale ? steer_scale : v);
}

/* The softmax sum's partial of lane l over e [T] */
OK_HDI float ok_vit_sum_part(const float *e, const int T, const int l)
{
    float s = 0.0f;
    for (int t = l; t < T; t += OK_ACTOR_LANES) s = s + e[t];
    return s;
}

/* One head's attention for one query: q [dh]; k, v: token t's [dh] at k + t * tstride; p [T] is work space; out [dh] */
OK_HD void ok_vit_attend(const float *q, const float *k, const float *v, const long tstride, const int T, const int dh, const float scale, float *p,
                         float *out)
{
    float m = 0.0f;
    for (int t = 0; t < T; ++t) {
        const float s = ok_lidar_dot(q, k + t * tstride, dh, 0.0f) * scale;
        p[t] = s;
        m = (t == 0 || s > m) ? s : m;
    }
    for (int t = 0; t < T; ++t) p[t] = ok_expf(p[t] - m);
    float part[OK_ACTOR_LANES];
    for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = ok_vit_sum_part(p, T, l);
    const float sum = ok_gauss_tree(part);
    for (int t = 0; t < T; ++t) p[t] = p[t] / sum;
    for (int c = 0; c < dh; ++c) {
        float acc = 0.0f;
        for (int t = 0; t < T; ++t) acc = __builtin_fmaf(p[t], v[t * tstride + c], acc);
        out[c] = acc;
    }
}

/* out [D] = LayerNorm(row [D]) */
OK_HD void ok_vit_norm_row(const float *row, const int D, const float *g, const float *b, const float eps, float *out)
{
    float part[OK_ACTOR_LANES];
    for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = ok_lidar_sum_part(row, D, l);
    const float mean = ok_gauss_tree(part) / (float)D;
    for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = ok_lidar_sq_part(row, D, l, mean);
    const float den = ok_vit_den(ok_gauss_tree(part) / (float)D, eps);
    for (int c = 0; c < D; ++c) out[c] = ok_lidar_norm(row[c], mean, den, g[c], b[c]);
}

/* Floats of the activations of one agent: x, n (a LayerNorm's output), ctx [T][D]; qkv [T][3 D]; hid [T][F].  The device's workspace
 * holds this much per agent of a pass; the host forward needs the softmax row [T] and the head's hidden layers behind it. */
OK_HDI size_t ok_vit_agent_floats(const ok_vit_shape s)
{
    return (size_t)ok_vit_tokens(s) * (size_t)(6 * s.D + s.ff);
}

OK_HDI size_t ok_vit_work_floats(const ok_vit_shape s)
{
    return ok_vit_agent_floats(s) + (size_t)ok_vit_tokens(s) + (size_t)(s.D + s.h1 + s.h2);
}

/* The whole network of one frame on the host: frame [S][S][4] uint8 -> embedding [D] (may be NULL) and *out, the head's output */
OK_HD void ok_vit_forward(const ok_vit_shape s, const ok_vit_consts kc, const float *params, const uint8_t *frame, float *work, float *embedding,
                          float *out)
{
    const ok_vit_layout at = ok_vit_offsets(s);
    const int T = ok_vit_tokens(s), D = s.D, F = s.ff, dh = D / s.heads, side = ok_vit_side(s), K = ok_vit_patch_k(s);
    float *x = work, *n = x + (size_t)T * D, *ctx = n + (size_t)T * D, *qkv = ctx + (size_t)T * D, *hid = qkv + (size_t)T * 3 * D;
    float *p = hid + (size_t)T * F, *emb = p + T, *g1 = emb + D, *g2 = g1 + s.h1;
    const float scale = ok_lidar_scale(dh);
    for (int c = 0; c < D; ++c) x[c] = params[at.cls + c] + params[at.pos + c];
    for (int py = 0; py < side; ++py)
        for (int px = 0; px < side; ++px) {
            const int t = 1 + py * side + px;
            for (int c = 0; c < D; ++c) {
                const float *w = params + at.pe_w + (size_t)c * K;
                float acc = params[at.pe_b + c];
                for (int k = 0; k < K; ++k) acc = __builtin_fmaf(ok_vit_patch_input(frame, s.S, s.P, py, px, k, kc.mean, kc.std), w[k], acc);
                x[(size_t)t * D + c] = acc + params[at.pos + (size_t)t * D + c];
            }
        }
    for (int i = 0; i < s.depth; ++i) {
        const float *bp = params + at.block0 + (size_t)i * at.block_stride;
        for (int t = 0; t < T; ++t) ok_vit_norm_row(x + (size_t)t * D, D, bp + at.n1_g, bp + at.n1_b, kc.eps, n + (size_t)t * D);
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < 3 * D; ++c) qkv[(size_t)t * 3 * D + c] = ok_lidar_dot(n + (size_t)t * D, bp + at.qkv_w + (size_t)c * D, D, bp[at.qkv_b + c]);
        for (int t = 0; t < T; ++t)
            for (int hd = 0; hd < s.heads; ++hd)
                ok_vit_attend(qkv + (size_t)t * 3 * D + hd * dh, qkv + D + hd * dh, qkv + 2 * D + hd * dh, 3L * D, T, dh, scale, p, ctx + (size_t)t * D + hd * dh);
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < D; ++c)
                x[(size_t)t * D + c] = x[(size_t)t * D + c] + ok_lidar_dot(ctx + (size_t)t * D, bp + at.proj_w + (size_t)c * D, D, bp[at.proj_b + c]);
        for (int t = 0; t < T; ++t) ok_vit_norm_row(x + (size_t)t * D, D, bp + at.n2_g, bp + at.n2_b, kc.eps, n + (size_t)t * D);
        for (int t = 0; t < T; ++t)
            for (int f = 0; f < F; ++f) hid[(size_t)t * F + f] = ok_vit_gelu(ok_lidar_dot(n + (size_t)t * D, bp + at.fc1_w + (size_t)f * D, D, bp[at.fc1_b + f]));
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < D; ++c)
                x[(size_t)t * D + c] = x[(size_t)t * D + c] + ok_lidar_dot(hid + (size_t)t * F, bp + at.fc2_w + (size_t)c * F, F, bp[at.fc2_b + c]);
    }
    ok_vit_norm_row(x, D, params + at.norm_g, params + at.norm_b, kc.eps, emb);
    if (embedding)
        for (int c = 0; c < D; ++c) embedding[c] = emb[c];
    for (int j = 0; j < s.h1; ++j) g1[j] = ok_lidar_relu(ok_lidar_dot(emb, params + at.hw0 + (size_t)j * D, D, params[at.hb0 + j]));
    for (int j = 0; j < s.h2; ++j) g2[j] = ok_lidar_relu(ok_lidar_dot(g1, params + at.hw1 + (size_t)j * s.h1, s.h1, params[at.hb1 + j]));
    *out = ok_lidar_dot(g2, params + at.hw2, s.h2, params[at.hb2]);
}

#endif /* OKENV_VIT_H */
