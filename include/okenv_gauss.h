/*
 * okenv_gauss.h -- the rule of the continuous REINFORCE learner (RLRacers/ReinforceContinuous/Policy.hpp:17-53,
 * ReinforceAgent.hpp:49-146): a two-hidden-layer network with a Gaussian head, its normal draw and its update, shared bit for bit by
 * the HIP kernels (openkitchen_amd/csrc/ok_gauss.h) and the host entries okenv_gauss_act_host and okenv_gauss_update_host (DESIGN.md
 * section 20).  It stands on the actor's rule (okenv_math.h) and the learner's (okenv_learn.h).
 *
 * THE RULE
 *
 * Network (Choice 1).  R -> H1 -> H2 -> A, ReLU behind both hidden layers (relu(v) = v > 0 ? v : 0), and one free vector
 * log_std [A].  1 <= R <= 64, 1 <= H1, H2 <= OK_GAUSS_MAX_HIDDEN = 128, 1 <= A <= OK_ACTOR_MAX_ACTIONS (the learner uses A = 2; a value
 * network is A = 1).  The parameter vector is in the order of torch's parameters() for a module that owns log_std and the children
 * fc1, fc2, mean -- a module's own parameters come before its children's:
 *     log_std [A], fc1.weight [H1][R] row-major, fc1.bias [H1], fc2.weight [H2][H1], fc2.bias [H2], mean.weight [A][H2], mean.bias [A]
 * (ok_gauss_layout).  All sums are fp32 with a separate multiplication and addition per term, nothing fused.
 *     layer 1:  pre1_i = ok_learn_pre: b1[i] + w1[i][0] * x[0] + ... ascending;  h1_i = relu(pre1_i)
 *     layer 2:  the actor's OUTPUT-layer rule, for every unit j (ok_gauss_pre):
 *                   part_l = 0.0f; part_l = part_l + w2[j][i] * h1[i] for i = l, l + 8, ... < H1 ascending          (l = 0 .. 7)
 *                   pre2_j = b2[j] + (((part_0 + part_4) + (part_2 + part_6)) + ((part_1 + part_5) + (part_3 + part_7)))
 *               (ok_actor_join's tree; there is no limit of 8 outputs here);  h2_j = relu(pre2_j)
 *     layer 3:  the same rule over h2:  mu_k = b3[k] + tree(part_l over j = l, l + 8, ... < H2 of w3[k][j] * h2[j])
 * Backward, from the output seeds dz[0 .. A-1]:
 *     dh2_j   = w3[0][j] * dz_0 + w3[1][j] * dz_1 + ... ascending k (ok_learn_back_hidden);   dpre2_j = pre2_j > 0 ? dh2_j : 0
 *     dh1_i   = tree(part_l), part_l = 0.0f; part_l = part_l + w2[j][i] * dpre2_j for j = l, l + 8, ... < H2 ascending (ok_gauss_back);
 *     dpre1_i = pre1_i > 0 ? dh1_i : 0
 * (pre > 0 is tested as relu(pre) > 0: the same truth value, NaN included.)  The term of parameter p for one sample
 * (ok_gauss_decode / ok_gauss_term) is
 *     log_std[a]: dls[a];   fc1: dpre1[a] * x[b], dpre1[a];   fc2: dpre2[a] * h1[b], dpre2[a];   mean: dz[a] * h2[b], dz[a]
 *
 * The normal draw (Choice 2, ok_gauss_normal_pair / ok_gauss_eps).  One Philox4x32-10 block per (seed, global agent id g, draw index
 * d, block n): counter = (g, d, 10, n), key = (seed, "oken").  Stream 10 is used by nothing else (the list is in okenv_math.h).
 * Box-Muller on words 0 and 1 of block n gives the components 2 n and 2 n + 1:
 *     u1 = 1.0f - ok_u01(w0)                       in (0, 1], exact
 *     r  = (float)sqrt((double)(-2.0f * ok_logf(u1)))   the fp64 square root rounded once: the correctly rounded fp32 root
 *     (s, c) = ok_sincosf(6.2831855f * ok_u01(w1))
 *     eps_{2n} = r * c,  eps_{2n+1} = r * s
 * so |eps| <= sqrt(48 ln 2) = 5.77.  Words 2 and 3 are not used.  The draw index is section 14's: the handle's step count plus the
 * caller-owned draw-offset word.  Greedy acting draws nothing.
 *
 * The sample (Choice 3, ok_gauss_component, ok_gauss_logp, ok_gauss_action).  For component k with mean mu_k:
 *     std_k = ok_expf(log_std_k)
 *     se_k  = std_k * eps_k;   pre_k = mu_k + se_k         (greedy: pre_k = mu_k, and z_k = 0.0f below)
 *     t_k   = ok_tanhf(pre_k)
 *     a_k   = t_k * scale_k + bias_k                       section 18's form; config defaults (50, 50) and (10, 0).  The reference writes
 *                                                          ((t_0 + 1) * 0.5) * 100 and t_1 * 10: the throttle differs by rounding only
 *     u_k   = 1.0f - t_k * t_k
 *     n_k   = ((-0.5f * z_k) * z_k - log_std_k) - 0.9189385f        z_k = eps_k; log_std_k stands for log(exp(log_std_k))
 *     l_k   = ok_logf(u_k + 1e-6f)
 *     logp  = (n_0 + n_1 + ...) - (l_0 + l_1 + ...)        both sums ascending, each starting from its first term
 * The loss term of a sample with normalised return G is -(logp * G).
 *
 * Two gradient modes (ok_gauss_seed), chosen per update:
 *                        OK_GAUSS_GRAD_REFERENCE (0, default)                      OK_GAUSS_GRAD_SCORE (1)
 *     reads              the recorded eps                                          the recorded pre
 *     pre, t             recomputed from the current parameters as above           the recorded pre and t = ok_tanhf(pre): constants
 *     z_k                eps_k                                                     (pre_k - mu_k) / std_k
 *     seed on mu_k       -(G * c_k),  c_k = ((2.0f * t_k) * u_k) / (u_k + 1e-6f)    -(G * (z_k / std_k))
 *     seed on log_std_k  -(G * (c_k * se_k - 1.0f))                                -(G * (z_k * z_k - 1.0f))
 * REFERENCE is what autograd gives for the reference's graph, in which pre is NOT detached: (pre - mu) / std is eps there, the normal
 * term gives mu no gradient and log_std only the -1 of -log(std), and everything else flows through the tanh correction.  It is not
 * the score-function estimator; SCORE is (pre detached).  In REFERENCE mode, before the first optimiser step, the recomputed logp
 * equals the recorded one bit for bit: the same expressions on the same numbers.
 *
 * Sums, slices, accumulate, reduce, Adam (Choice 4): okenv_reinforce.h's, unchanged.  Chunks of OK_LEARN_CHUNK positions ascending,
 * ok_learn_tree over the chunk partials, the loss term one more column behind the parameters, slices of B positions,
 * `accumulate` / `reduce` / `order` with their meanings there, ok_learn_adam with the host's fp64 factors; log_std is stepped like
 * any other parameter.
 *
 * Only +, -, *, /, comparisons, the correctly rounded square root, ok_expf, ok_logf, ok_tanhf and ok_sincosf are used; compile with
 * -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_GAUSS_H
#define OKENV_GAUSS_H

#include "okenv_learn.h"

#define OK_GAUSS_STREAM 10u
#define OK_GAUSS_MAX_HIDDEN 128
#define OK_GAUSS_GRAD_REFERENCE 0
#define OK_GAUSS_GRAD_SCORE 1

/* Where the pieces of the parameter vector begin, in floats */
typedef struct ok_gauss_layout {
    int log_std, w1, b1, w2, b2, w3, b3, total;
} ok_gauss_layout;

/* The layout of a vector with `nls` floats of log_std in front: at.log_std = 0 and at.w1 = nls */
OK_HDI ok_gauss_layout ok_gauss_offsets_nls(const int in, const int h1, const int h2, const int out, const int nls)
{
    ok_gauss_layout at;
    at.log_std = 0;
    at.w1 = nls;
    at.b1 = at.w1 + h1 * in;
    at.w2 = at.b1 + h1;
    at.b2 = at.w2 + h2 * h1;
    at.w3 = at.b2 + h2;
    at.b3 = at.w3 + out * h2;
    at.total = at.b3 + out;
    return at;
}

/* This learner's vector: one log_std per output */
OK_HDI ok_gauss_layout ok_gauss_offsets(const int in, const int h1, const int h2, const int out) { return ok_gauss_offsets_nls(in, h1, h2, out, out); }

OK_HDI int ok_gauss_num_params(const int in, const int h1, const int h2, const int out)
{
    return out + h1 * in + h1 + h2 * h1 + h2 + out * h2 + out;
}

/* ok_actor_join's tree without the bias */
OK_HDI float ok_gauss_tree(const float *p)
{
    return ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]));
}

/* Pre-activation of unit j of a layer over n inputs h: the 8 interleaved partial sums, their tree, the bias.  The rows of w lie
 * `stride` floats apart. */
OK_HDI float ok_gauss_pre(const float *w, const int stride, const float *b, const int n, const float *h, const int j)
{
    const float *row = w + j * stride;
    float part[OK_ACTOR_LANES];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = 0.0f;
    int i = 0;
    for (; i + OK_ACTOR_LANES <= n; i += OK_ACTOR_LANES) { /* whole rounds of the interleave: no test, the loads go out together */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = part[l] + row[i + l] * h[i + l];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        if (i + l < n) part[l] = part[l] + row[i + l] * h[i + l];
    return ok_actor_join(part, b[j]);
}

/* dh_i of a layer with n outputs from their seeds d[0 .. n-1]: partials over the output units j = l, l + 8, ..., the forward's tree */
OK_HDI float ok_gauss_back(const float *w, const int stride, const int n, const float *d, const int i)
{
    float part[OK_ACTOR_LANES];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = 0.0f;
    int j = 0;
    for (; j + OK_ACTOR_LANES <= n; j += OK_ACTOR_LANES) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int l = 0; l < OK_ACTOR_LANES; ++l) part[l] = part[l] + w[(j + l) * stride + i] * d[j + l];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        if (j + l < n) part[l] = part[l] + w[(j + l) * stride + i] * d[j + l];
    return ok_gauss_tree(part);
}

/* The two normals of one Philox block */
OK_HD void ok_gauss_normal_pair(const uint32_t w0, const uint32_t w1, float *e0, float *e1)
{
    const float u1 = 1.0f - ok_u01(w0);
    const float r = (float)__builtin_sqrt((double)(-2.0f * ok_logf(u1)));
    float s, c;
    ok_sincosf(6.2831855f * ok_u01(w1), &s, &c);
    *e0 = r * c;
    *e1 = r * s;
}

/* eps_k of (seed, global agent id, draw index) */
OK_HD float ok_gauss_eps(const uint32_t seed, const uint32_t agent, const uint32_t draw, const int k)
{
    const ok_u32x4 b = ok_philox4x32(agent, draw, OK_GAUSS_STREAM, (uint32_t)(k >> 1), seed, 0x6F6B656Eu);
    float e0, e1;
    ok_gauss_normal_pair(b.v[0], b.v[1], &e0, &e1);
    return (k & 1) ? e1 : e0;
}

/* One component of the sample */
typedef struct ok_gauss_comp {
    float std, se, pre, t, u, n, l;
} ok_gauss_comp;

/* From mu, log_std and either eps (use_pre == 0: pre = mu + std * eps, z = eps) or a given pre (use_pre != 0: z = (pre - mu) / std).
 * `greedy` (with use_pre == 0): pre = mu, z = 0. */
OK_HD ok_gauss_comp ok_gauss_component(const float mu, const float log_std, const float eps, const float pre_in, const int use_pre, const int greedy,
                                       float *z_out)
{
    ok_gauss_comp c;
    c.std = ok_expf(log_std);
    float z;
    if (use_pre) {
        c.se = 0.0f;
        c.pre = pre_in;
        z = (pre_in - mu) / c.std;
    } else if (greedy) {
        c.se = 0.0f;
        c.pre = mu;
        z = 0.0f;
    } else {
        c.se = c.std * eps;
        c.pre = mu + c.se;
        z = eps;
    }
    c.t = ok_tanhf(c.pre);
    c.u = 1.0f - c.t * c.t;
    c.n = ((-0.5f * z) * z - log_std) - 0.9189385f;
    c.l = ok_logf(c.u + 1e-6f);
    *z_out = z;
    return c;
}

/* logp from the components' n and l (arrays of OK_ACTOR_MAX_ACTIONS entries, `out` of them used) */
OK_HDI float ok_gauss_logp(const float *n, const float *l, const int out)
{
    float sn = n[0], sl = l[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < out) {
            sn = sn + n[k];
            sl = sl + l[k];
        }
    return sn - sl;
}

OK_HDI float ok_gauss_action(const float t, const float scale, const float bias)
{
    return t * scale + bias;
}

/* The seeds of one component on mu_k and log_std_k */
OK_HD void ok_gauss_seed(const int mode, const ok_gauss_comp c, const float z, const float G, float *dmu, float *dls)
{
    if (mode == OK_GAUSS_GRAD_SCORE) {
        *dmu = -(G * (z / c.std));
        *dls = -(G * (z * z - 1.0f));
    } else {
        const float cc = ((2.0f * c.t) * c.u) / (c.u + 1e-6f);
        *dmu = -(G * cc);
        *dls = -(G * (cc * c.se - 1.0f));
    }
}

/* Parameter index p as the term it sums: kind 0: dls[a]; 1: dpre1[a] * x[b]; 2: dpre1[a]; 3: dpre2[a] * h1[b]; 4: dpre2[a];
 * 5: dz[a] * h2[b]; 6: dz[a].  The vector begins with `nls` log_std entries. */
OK_HDI ok_learn_slot ok_gauss_decode_nls(int p, const int in, const int h1, const int h2, const int out, const int nls)
{
    ok_learn_slot s;
    s.b = 0;
    if (p < nls) { s.kind = 0; s.a = p; return s; }
    p -= nls;
    if (p < h1 * in) { s.kind = 1; s.a = p / in; s.b = p - s.a * in; return s; }
    p -= h1 * in;
    if (p < h1) { s.kind = 2; s.a = p; return s; }
    p -= h1;
    if (p < h2 * h1) { s.kind = 3; s.a = p / h1; s.b = p - s.a * h1; return s; }
    p -= h2 * h1;
    if (p < h2) { s.kind = 4; s.a = p; return s; }
    p -= h2;
    if (p < out * h2) { s.kind = 5; s.a = p / h2; s.b = p - s.a * h2; return s; }
    s.kind = 6;
    s.a = p - out * h2;
    return s;
}

OK_HDI ok_learn_slot ok_gauss_decode(const int p, const int in, const int h1, const int h2, const int out) { return ok_gauss_decode_nls(p, in, h1, h2, out, out); }

/* The term of one sample from its rows */
OK_HDI float ok_gauss_term(const ok_learn_slot s, const float *x, const float *h1, const float *h2, const float *d1, const float *d2, const float *dz,
                           const float *dls)
{
    switch (s.kind) {
    case 0: return dls[s.a];
    case 1: return d1[s.a] * x[s.b];
    case 2: return d1[s.a];
    case 3: return d2[s.a] * h1[s.b];
    case 4: return d2[s.a];
    case 5: return dz[s.a] * h2[s.b];
    default: return dz[s.a];
    }
}

#endif /* OKENV_GAUSS_H */
