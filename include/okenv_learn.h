/*
 * okenv_learn.h -- the rule of PPO's update (RLRacers/PPO/PPOAgent.hpp:104-154: the minibatch loop of updatePolicy), shared bit for
 * bit by the HIP kernels (openkitchen_amd/csrc/ok_learn.h) and the host entry okenv_ppo_update_host.
 *
 * THE RULE
 *
 * Input.  M samples as okenv_batch_prepare leaves them dense: state [M][R], action [M] (int64), prob [M] (the recorded clamped
 * probability, NOT its logarithm), ret [M] and optionally adv [M].  The networks and their limits are the actor's (okenv_math.h):
 * policy R -> H -> A, value R -> Hv -> 1, ReLU, parameters in the order of torch's parameters().
 *
 * Minibatches.  Epoch e cuts the M samples into ceil(M / B) minibatches; minibatch k holds the B_k = min(B, M - k B) positions
 * q = 0 .. B_k-1, and position q is sample order[e][k B + q], or k B + q without an order (ExperienceBuffer::sample(batch_size, i)).
 * An index outside 0 .. M-1 counts as the nearest valid one, an action outside 0 .. A-1 likewise: device data is not validated.
 * Both networks step once per minibatch, the actor first; every forward of a minibatch uses the parameters from before either step.
 *
 * Forward.  The actor's rule and nothing else: ok_actor_partial / ok_actor_join for the logits z and the value v, ok_expf(z_k - max z)
 * and ok_actor_pick for the clamped probability p_new of the recorded action.  A recorded state evaluated with unchanged parameters
 * therefore reproduces the recorded probability bit for bit.  The hidden pre-activation s_j the backward pass needs is
 * ok_learn_pre: ok_actor_partial's own expression, so the same bits.
 *
 * Sample (ok_learn_policy_seed, ok_learn_value_seed).
 *     adv    = adv[s] when given, else ret[s] - v                    (v detached, PPOAgent.hpp:125)
 *     r      = p_new / p_old                                         one IEEE division; the reference's exp(log p_new - log p_old) differs
 *                                                                    from it by rounding only, and r is exactly 1 on the first minibatch
 *     rc     = r < lo ? lo : (r > hi ? hi : r)                       lo = (float)(1 - (double)clip), hi = (float)(1 + (double)clip)
 *     s1     = r * adv,  s2 = rc * adv,  surr = s1 < s2 ? s1 : s2    (PPOAgent.hpp:137-139)
 *     clipped = r < lo || r > hi
 *     e      = v - ret,  the critic's term is e * e                  (PPOAgent.hpp:141)
 * Gradient conventions: torch autograd's.
 *     min    the smaller side takes the gradient; on a tie (neither s1 < s2 nor s2 < s1) each side takes half
 *     clamp  passes the gradient on its closed range [lo, hi], nothing outside
 *     d surr / d r = w1 * adv + w2 * (lo <= r <= hi ? adv : 0),  (w1, w2) = (1, 0), (0, 1) or (.5, .5): exact products
 *     d r / d p_new = 1 / p_old, so g_p = -(d surr / d r) / p_old    (the minus of actor_loss = -mean(surr) goes in here: exact)
 *     a probability the clamp to [1e-8f, 1.0f] moved contributes no policy gradient; on the closed range it passes
 *     softmax y_k = e_k / S (S as ok_actor_pick sums it):  t = g_p * y_a,  dz_k = t * ((k == a ? 1.0f : 0.0f) - y_k)
 *     value:  dz = 2.0f * e
 *     layer 2:  dW2[k][j] = dz_k * h_j,  db2[k] = dz_k;   dh_j = w2[0][j] * dz_0 + w2[1][j] * dz_1 + ... ascending k
 *     ReLU's derivative at 0 is 0:  ds_j = s_j > 0 ? dh_j : 0
 *     layer 1:  dW1[j][i] = ds_j * x_i,  db1[j] = ds_j
 * All fp32, a separate multiplication and addition per term, nothing fused.
 *
 * Sums.  The order belongs to the rule, never to a launch.  A minibatch is cut into chunks of OK_LEARN_CHUNK = 32 consecutive
 * positions.  Within a chunk a parameter's partial is acc = 0.0f; acc = acc + term in ascending position (ok_learn_term gives the term
 * of parameter index p).  The chunk partials are joined by ok_learn_tree: section 15's fixed tree in fp32 (pad to a power of two,
 * x[i] += x[i + h] for h = P/2 .. 1).  The two losses are two more columns summed the same way (surr and e * e per position); the
 * clip count is an integer sum.  The factor 1 / B_k is applied ONCE, after the join: gradient = joined sum / (float)B_k,
 * actor_loss = -(joined surr / (float)B_k), critic_loss = joined e * e / (float)B_k, each one IEEE division.
 *
 * Adam (ok_learn_adam): torch's defaults and formulation, no weight decay, no amsgrad, fp32 state.
 *     m = beta1 * m + (1 - beta1) * g;   v = beta2 * v + ((1 - beta2) * g) * g;      1 - beta as (float)(1 - (double)beta)
 *     p = p - step * (m / (sqrt(v) / bc2 + eps))
 * with step = lr / (1 - beta1^t) and bc2 = sqrt(1 - beta2^t) evaluated in fp64 on the host from the step number t (ok_learn_factors),
 * rounded once to fp32 and passed by value.  sqrt(v) is the fp64 square root rounded to fp32, which is the correctly rounded fp32
 * square root (53 >= 2 * 24 + 2 bits).  t, m and v persist across calls; actor and critic have their own m and v and share t.
 *
 * Only +, -, *, /, sqrt, comparisons and ok_expf are used, all IEEE-exact on x86-64 and on gfx950, provided the translation unit is
 * compiled with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_LEARN_H
#define OKENV_LEARN_H

#include "okenv_math.h"

#define OK_LEARN_CHUNK 32

/* Pre-activation of hidden unit j: the expression of ok_actor_partial, so the same bits */
OK_HDI float ok_learn_pre(const float *w1, const int w1_stride, const float *b1, const int in, const float *x, const int j)
{
    const float *row = w1 + j * w1_stride;
    float s = b1[j];
    for (int i = 0; i < in; ++i) s = s + row[i] * x[i];
    return s;
}

/* ds_j from the output seeds dz[0 .. out-1] (dz has OK_ACTOR_MAX_ACTIONS entries) and the pre-activation s of unit j */
OK_HDI float ok_learn_back_hidden(const float *w2, const int hidden, const int out, const float *dz, const int j, const float s)
{
    float d = w2[j] * dz[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < out) d = d + w2[k * hidden + j] * dz[k];
    return s > 0.0f ? d : 0.0f;
}

OK_HDI int ok_learn_clamp_index(const long long i, const int n)
{
    return i < 0 ? 0 : (i >= (long long)n ? n - 1 : (int)i);
}

/* From the logits of one sample to the seeds dz[0 .. n-1] of the actor's loss, its surrogate term and whether the ratio was clipped.
 * z and dz have OK_ACTOR_MAX_ACTIONS entries; `action` is already inside 0 .. n-1. */
OK_HDI void ok_learn_policy_seed(const float *z, const int n, const int action, const float p_old, const float adv, const float lo, const float hi,
                                 float *dz, float *surr, int *clipped)
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
    float p_new;
    (void)ok_actor_pick(e, n, 0.0f, action, &p_new); /* the actor's clamped probability of `action` */
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
    const float r = p_new / p_old;
    const float rc = r < lo ? lo : (r > hi ? hi : r);
    const float s1 = r * adv, s2 = rc * adv;
    *surr = s1 < s2 ? s1 : s2;
    *clipped = (r < lo || r > hi) ? 1 : 0;
    const float w1 = s1 < s2 ? 1.0f : (s2 < s1 ? 0.0f : 0.5f);
    const float w2 = 1.0f - w1;
    const float in_range = (r >= lo && r <= hi) ? adv : 0.0f;
    const float g_r = w1 * adv + w2 * in_range;
    const float g_p = (ya >= OK_ACTOR_PROB_MIN && ya <= OK_ACTOR_PROB_MAX) ? -g_r / p_old : 0.0f;
    const float t = g_p * ya;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        dz[k] = k < n ? t * ((k == action ? 1.0f : 0.0f) - e[k] / s) : 0.0f;
}

/* The critic's term and seed of one sample */
OK_HDI void ok_learn_value_seed(const float v, const float ret, float *dz, float *sq)
{
    const float e = v - ret;
    *sq = e * e;
    *dz = 2.0f * e;
}

/* Parameter index p of a network in -> hidden -> out as the term it sums: kind 0: ds[a] * x[b], 1: ds[a], 2: dz[a] * h[b], 3: dz[a] */
typedef struct ok_learn_slot {
    int kind, a, b;
} ok_learn_slot;

OK_HDI ok_learn_slot ok_learn_decode(int p, const int in, const int hidden, const int out)
{
    ok_learn_slot s;
    s.b = 0;
    if (p < hidden * in) { s.kind = 0; s.a = p / in; s.b = p - s.a * in; return s; }
    p -= hidden * in;
    if (p < hidden) { s.kind = 1; s.a = p; return s; }
    p -= hidden;
    if (p < out * hidden) { s.kind = 2; s.a = p / hidden; s.b = p - s.a * hidden; return s; }
    s.kind = 3;
    s.a = p - out * hidden;
    return s;
}

/* The term of one sample: x, h, ds, dz are that sample's rows */
OK_HDI float ok_learn_term(const ok_learn_slot s, const float *x, const float *h, const float *ds, const float *dz)
{
    switch (s.kind) {
    case 0: return ds[s.a] * x[s.b];
    case 1: return ds[s.a];
    case 2: return dz[s.a] * h[s.b];
    default: return dz[s.a];
    }
}

/* Section 15's fixed tree in fp32 over n partials that lie `stride` floats apart; x[0] is the result, x is overwritten */
OK_HDI float ok_learn_tree(float *x, const long long stride, const uint32_t n)
{
    uint32_t w = 1u;
    while (w < n) w <<= 1;
    for (uint32_t h = w >> 1; h >= 1u; h >>= 1)
        for (uint32_t i = 0u; i < h; ++i)
            if (i + h < n) x[(long long)i * stride] = x[(long long)i * stride] + x[(long long)(i + h) * stride];
    return x[0];
}

typedef struct ok_learn_adam_consts {
    float beta1, omb1, beta2, omb2, eps; /* omb = (float)(1 - (double)beta) */
    float step, bc2;                     /* of this step number: ok_learn_factors */
} ok_learn_adam_consts;

/* One Adam step of one parameter with gradient g */
OK_HDI void ok_learn_adam(float *p, float *m, float *v, const float g, const ok_learn_adam_consts c)
{
    const float m1 = c.beta1 * *m;
    const float m2 = c.omb1 * g;
    const float mn = m1 + m2;
    const float v1 = c.beta2 * *v;
    const float v2 = (c.omb2 * g) * g;
    const float vn = v1 + v2;
    const float root = (float)__builtin_sqrt((double)vn);
    const float den = root / c.bc2 + c.eps;
    const float upd = c.step * (mn / den);
    *m = mn;
    *v = vn;
    *p = *p - upd;
}

/* step = lr / (1 - beta1^t) and bc2 = sqrt(1 - beta2^t) for step number t >= 1: fp64 (the power by repeated squaring, so that no
 * libm decides a bit), each rounded once to fp32.  Host functions. */
static inline double ok_learn_powi(double b, long long t)
{
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r = r * b;
        b = b * b;
        t >>= 1;
    }
    return r;
}

static inline void ok_learn_factors(const float lr, const float beta1, const float beta2, const long long t, float *step, float *bc2)
{
    *step = (float)((double)lr / (1.0 - ok_learn_powi((double)beta1, t)));
    *bc2 = (float)__builtin_sqrt(1.0 - ok_learn_powi((double)beta2, t));
}

#endif /* OKENV_LEARN_H */
