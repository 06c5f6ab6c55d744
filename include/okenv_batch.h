/*
 * okenv_batch.h -- the rule that turns a recorded episode into the learner's batch, shared bit for bit by the HIP kernels
 * (openkitchen_amd/csrc/ok_batch.h) and the host entry okenv_batch_prepare_host.
 *
 * It is the data side of the reference's updatePolicy: ExperienceBuffer::calculateDiscountedRewards + ::sample
 * (RLRacers/PPO/ExperienceBuffer.hpp:15-68), ReinforceAgent.hpp:94-106 and GCLAgent.hpp:75-84,137-148, stated for a record of
 * N agent columns and T step rows in which `alive[t][i]` marks the samples an agent produced while it was driving.
 *
 * THE RULE
 *
 * Walk.  Every agent column is walked on its own from t = T-1 down to 0 with ok_batch_walk_row; the state it carries is
 * ok_batch_walk.  Where alive[t][i] is set:
 *     c = reward + gamma * c                      one fp32 multiply, then one fp32 add (ExperienceBuffer.hpp:59);  G[t][i] = c
 *     delta = (reward + gamma * v_next) - value   (only with a value plane)
 *     a = delta + gl * a                          gl = (float)(gamma * lambda), rounded once on the host;          A[t][i] = a
 *     v_next = value
 * where it is not, G[t][i] = A[t][i] = 0 and c = a = v_next = 0: a dead row is an episode boundary and a terminal state, so with
 * auto-reset on nothing leaks from one episode of a column into the one before it.  At the start c = a = 0 and v_next is
 * last_value[i] when that is given (an episode cut by max_steps bootstraps from the critic), else 0.
 *
 * Statistics.  Over the alive samples: the count M and, in fp64, the sum S and the sum of squares Q of G (and of A).  The order is
 * part of the rule and no launch shape can change it: per column in walk order (t = T-1 .. 0; the square of an fp32 value is
 * exact in fp64, so each sample costs two fp64 additions), then the N column partials are joined by ok_batch_tree's fixed tree over
 * the agent index.  ok_batch_finish turns (M, S, Q) into mean = S / M and the unbiased standard deviation
 * sqrt(max(Q - S * mean, 0) / (M - 1)) (what torch's std() estimates), both evaluated in fp64 and rounded once to fp32.
 * M = 0 gives mean = 0 and std = 0; M = 1 gives mean = the sample and std = 0, so its normalised value is 0 / FLT_EPSILON = 0:
 * never NaN or inf.
 *
 * Normalisation.  ok_batch_normalize: (x - mean) / (std + FLT_EPSILON) in fp32, the sum formed once, an IEEE division
 * (ExperienceBuffer.hpp:67).  Only the dense outputs are normalised; the [T][N] planes keep the raw G and A.
 *
 * Sample order.  The alive samples in step-major, agent-minor order (the order of the reference's buffer, ppo_sim.cpp:63-80);
 * sample k carries the flat index t * N + i.
 *
 * Only +, -, *, / , sqrt and conversions are used, all IEEE-exact on x86-64 and on gfx950, provided the translation unit is
 * compiled with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_BATCH_H
#define OKENV_BATCH_H

#include "okenv_math.h"

#define OK_BATCH_EPS 1.1920928955078125e-07f /* FLT_EPSILON = torch.finfo(torch.float32).eps */

typedef struct ok_batch_walk {
    float    c, a, v_next;        /* running return, running advantage, the value the next older row bootstraps from */
    double   s_g, q_g, s_a, q_a;  /* column partials: sum and sum of squares of G and of A                           */
    uint32_t m;                   /* alive samples of the column                                                      */
} ok_batch_walk;

OK_HDI void ok_batch_walk_init(ok_batch_walk *w, const float last_value)
{
    w->c      = 0.0f;
    w->a      = 0.0f;
    w->v_next = last_value;
    w->s_g = w->q_g = w->s_a = w->q_a = 0.0;
    w->m                              = 0u;
}

/* One row of one column; has_value: a value plane is given.  *g_out / *a_out receive G[t][i] / A[t][i] (a_out only with a value). */
OK_HDI void ok_batch_walk_row(ok_batch_walk *w, const int alive, const float reward, const float value, const int has_value, const float gamma,
                              const float gl, float *g_out, float *a_out)
{
    if (!alive)
    {
        w->c = w->a = w->v_next = 0.0f;
        *g_out                  = 0.0f;
        *a_out                  = 0.0f;
        return;
    }
    const float gc = gamma * w->c;
    w->c           = reward + gc;
    *g_out         = w->c;
    const double g = (double)w->c;
    w->s_g         = w->s_g + g;
    w->q_g         = w->q_g + g * g;
    w->m += 1u;
    if (has_value)
    {
        const float gv    = gamma * w->v_next;
        const float tgt   = reward + gv;
        const float delta = tgt - value;
        const float ga    = gl * w->a;
        w->a              = delta + ga;
        w->v_next         = value;
        const double a    = (double)w->a;
        w->s_a            = w->s_a + a;
        w->q_a            = w->q_a + a * a;
    }
    *a_out = w->a;
}

/* The tree's width for n columns: the smallest power of two >= n. */
OK_HDI uint32_t ok_batch_tree_width(const uint32_t n)
{
    uint32_t p = 1u;
    while (p < n)
        p <<= 1;
    return p;
}

/* The fixed tree over the agent index: the n partials are padded with zeros to P = ok_batch_tree_width(n); for h = P/2, P/4, .. 1
 * every x[i], i < h, becomes x[i] + x[i + h].  x[0] is the result; x is overwritten.  (A partial is never -0, so leaving out the
 * additions of the padding changes nothing.) */
OK_HD double ok_batch_tree(double *x, const uint32_t n)
{
    for (uint32_t h = ok_batch_tree_width(n) >> 1; h >= 1u; h >>= 1)
        for (uint32_t i = 0u; i < h; ++i)
            if (i + h < n)
                x[i] = x[i] + x[i + h];
    return x[0];
}

/* (M, S, Q) -> mean and unbiased standard deviation, fp64 throughout, each rounded once to fp32 */
OK_HDI void ok_batch_finish(const uint32_t m, const double s, const double q, float *mean_out, float *std_out)
{
    double mean = 0.0, sd = 0.0;
    if (m >= 1u)
        mean = s / (double)m;
    if (m >= 2u)
    {
        double ss = q - s * mean;
        if (!(ss > 0.0))
            ss = 0.0;
        sd = __builtin_sqrt(ss / (double)(m - 1u));
    }
    *mean_out = (float)mean;
    *std_out  = (float)sd;
}

OK_HDI float ok_batch_normalize(const float x, const float mean, const float sd)
{
    const float den = sd + OK_BATCH_EPS;
    return (x - mean) / den;
}

#endif /* OKENV_BATCH_H */
