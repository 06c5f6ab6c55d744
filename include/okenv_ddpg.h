/*
 * okenv_ddpg.h -- the rule of DDPG (RLRacers/DDPG/ddpg_sim.cpp:55-95, DDPGAgent.hpp:60-170, Actor.hpp:30-39, Critic.hpp:27-33,
 * common/ReplayBuffer.hpp): the continuous actor, the critic on [state, action], the replay ring with a two-float action, the two
 * target networks and one update iteration, shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_ddpg.h) and the host
 * entries okenv_ddpg_act_host / okenv_ddpg_replay_push_host / okenv_ddpg_update_host.  Written on top of the
 * actor's forward and ok_tanhf (okenv_math.h), the learner's backward, sums and Adam (okenv_learn.h) and the ring's rules, sampling
 * and target (okenv_dqn.h).
 *
 * THE RULE
 *
 * The networks.  One hidden layer each and ReLU, parameters in the order of torch's parameters() (l1.weight row-major, l1.bias,
 * l2.weight, l2.bias); the reference's 400-300 stacks are GEMM kernels, a different design.
 *     actor    R -> H -> 2
 *     critic   (R + 2) -> Hc -> 1; its input row is the state followed by the two action components: torch::cat({state, action}, 1)
 *              (Critic.hpp:27).  The action is the raw one (Critic.hpp's kOut*Max are unused in the reference too).
 *     limits   1 <= R <= 62 (OK_DDPG_MAX_RAYS: R + 2 stays inside OK_ACTOR_MAX_RAYS), 1 <= H, Hc <= 256
 * Both forwards are the actor's rule and nothing else (ok_actor_partial / ok_actor_join): a hidden unit starts at its bias and adds
 * in ascending input order, an output is eight interleaved partial sums joined by the fixed tree.
 *
 * The action (Actor.hpp:30-39).  z = actor(x), x = dist / 200.0f as section 14 made it;
 *     t_k = ok_tanhf(z_k),   a_k = t_k * scale_k + bias_k        one fp32 multiplication, one addition (ok_ddpg_action)
 * scale and bias belong to the config; the reference's are (50, 5) and (50, 0).  a_0 is throttle_delta, a_1 steering_delta.
 *
 * Exploration (ok_ddpg_explore).  The reference has none: noise = (0, 0) is the default and then no draw changes a bit.  A component
 * with noise_k > 0 becomes
 *     a_k = a_k + noise_k * (2.0f * u_k - 1.0f)      each operation rounded on its own (the doubling is exact)
 *     a_k = a_k < lo_k ? lo_k : (a_k > hi_k ? hi_k : a_k),   lo_k = bias_k - scale_k, hi_k = bias_k + scale_k
 * with u_k = ok_u01(word k) of Philox4x32-10(counter = (global agent id, draw index, 8, 0), key = (seed, "oken")): one block per
 * agent and draw on stream 8, which nothing else uses (okenv_math.h lists the streams).  A component with noise_k == 0 is left
 * exactly as ok_ddpg_action made it: no addition, no clamp.  The draw index is section 14's Choice 2: the handle's step count plus
 * the caller's draw-offset word, if one is registered.  No new transcendental.
 *
 * The ring.  Section 17's rules unchanged: the transition with push rank p lives in slot ok_dqn_slot(p, C), size = ok_dqn_size(pushed,
 * C), the selected agents are appended in ascending agent order AS IF pushed one by one, and only the last C of one push survive
 * (ok_dqn_survives).  Selected: the record's `alive` byte, or every agent with OK_REPLAY_PUSH_ALL.
 *     state, action    the record of the act that preceded the step; action is [C][2] floats
 *     next_state[i]    dist[i] / 200.0f on the distances after the step
 *     done             crashed_ after the step: 1.0f or 0.0f
 *     reward           the caller's reward[a], or 1.0f without an array (ddpg_sim.cpp:73)
 *
 * One update iteration (DDPGAgent.hpp:127-170).  Iteration i reads draw d = draw_base + i with `resample`, else d = draw_base every
 * time; position q = 0 .. B-1 reads slot ok_dqn_sample(sample_seed, q, d, size).  Both steps of an iteration read the same slots.
 *   1. Target.  a' = the action of actor_target(s'), without noise; q' = critic_target([s', a']);
 *          y = ok_dqn_target(r, done, gamma, q', OK_DQN_MASK_DONE)     the done mask is always on (:146); y is a constant (.detach())
 *   2. Critic.  e = critic([s, a]) - y.  mse_loss = sum e^2 / B; the seed that enters the sums is e, the factor is applied once after
 *      the join.  Backward and sums are okenv_learn.h's with `in` = R + 2 (section 16's Choice 2: chunks of 32 positions, ascending,
 *      a separate multiplication and addition, ok_learn_tree):
 *          gradient = (2.0f * sum) / (float)B,   loss = (sum of e * e) / (float)B,   then ok_learn_adam with lr_critic
 *   3. Actor.  Uses the critic from AFTER step 2: the reference steps the critic first and then forms -critic(s, actor(s)).mean().
 *          z = actor(s), t_k = ok_tanhf(z_k), a_k = t_k * scale_k + bias_k, q = critic([s, a]) with pre-activations s_j
 *          the seed on q is 1:  dh_j = s_j > 0 ? w2c[j] : 0                                    (w2c[j] * 1.0f: the same bits)
 *          da_k = sum_j w1c[j][R + k] * dh_j in the join order of the forward: hidden unit j goes to partial j mod 8
 *                 (part = 0.0f; part = part + w1c[j][R + k] * dh_j for j ascending), the eight partials joined by the fixed tree
 *                 ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7))                                     (ok_ddpg_critic_lane, ok_ddpg_join)
 *          dz_k = (da_k * scale_k) * (1.0f - t_k * t_k)          autograd's tanh derivative on the rounded output (ok_ddpg_seed)
 *      then okenv_learn.h's backward through the actor (out = 2) and the same sums;
 *          gradient = -(sum) / (float)B,   loss = -((sum of q) / (float)B),   then ok_learn_adam with lr_actor
 *      The gradients this backward would leave on the critic are not computed: the reference discards them at the next zero_grad.
 *   4. Soft updates (:123).  omt = 1.0f - tau evaluated once in fp32;
 *          target = (tau * p) + (omt * target)                   two multiplications and one addition (ok_ddpg_soft)
 *      for both target networks, after both steps.  The kernels fuse each soft update into its own network's step: the thread that
 *      has just stepped parameter p updates target p from the new value.  That gives the same values, because the critic's target is
 *      read only in step 1 of an iteration and the actor's target is read only in step 1, so nothing reads either target between the
 *      critic's step and the end of the iteration, and the value of p that the soft update reads is final once its own step is done.
 * Both Adams share one step number t (both step once per iteration); the host evaluates both pairs of factors (ok_learn_factors).
 *
 * With size == 0 there is nothing to read: every position counts as an all-zero transition with e = 0, a zero seed on q and a zero q
 * term, so both gradients and both losses are zeros, Adam steps, and from zero moments that leaves every online parameter bit for
 * bit (section 17).  The soft update still runs.
 *
 * Only +, -, *, /, sqrt, comparisons and ok_tanhf decide a bit; nothing is fused outside ok_tanhf.  IEEE-exact on x86-64 and gfx950
 * under -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_DDPG_H
#define OKENV_DDPG_H

#include "okenv_dqn.h"

#define OK_DDPG_MAX_RAYS (OK_ACTOR_MAX_RAYS - 2)
#define OK_DDPG_STREAM 8u

OK_HD int ok_ddpg_critic_params(const int rays, const int hidden)
{
    return ok_actor_num_params(rays + 2, hidden, 1);
}

OK_HD float ok_ddpg_action(const float z, const float scale, const float bias, float *t_out)
{
    const float t = ok_tanhf(z);
    const float ts = t * scale;
    *t_out = t;
    return ts + bias;
}

OK_HDI ok_u32x4 ok_ddpg_draw(const uint32_t seed, const uint32_t agent, const uint32_t draw)
{
    return ok_philox4x32(agent, draw, OK_DDPG_STREAM, 0u, seed, 0x6F6B656Eu);
}

/* One component; `word` is word k of the agent's block (read only when noise > 0) */
OK_HD float ok_ddpg_explore(const float a, const float noise, const uint32_t word, const float scale, const float bias)
{
    if (!(noise > 0.0f)) return a;
    const float twice = 2.0f * ok_u01(word);
    const float d = twice - 1.0f;
    const float nd = noise * d;
    const float b = a + nd;
    const float lo = bias - scale, hi = bias + scale;
    return b < lo ? lo : (b > hi ? hi : b);
}

/* The fixed tree of ok_actor_join without a bias */
OK_HDI float ok_ddpg_join(const float *p)
{
    return ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]));
}

/* Interleave lane l of the critic for the actor's step: over the hidden units j = l, l + 8, ... the partial of q (ok_actor_partial's
 * expression, so the same bits) and the partials of da_0, da_1 with the seed `seed` (1.0f, or 0.0f on an empty ring) on q.
 * x is the row [state, a_0, a_1] of in = rays + 2 entries; w1's rows lie w1_stride floats apart. */
OK_HDI void ok_ddpg_critic_lane(const float *w1, const int w1_stride, const float *b1, const float *w2, const int in, const int hidden, const float *x,
                                const int l, const float seed, float *part_q, float *part_da)
{
    float pq = 0.0f, d0 = 0.0f, d1 = 0.0f;
    for (int j = l; j < hidden; j += OK_ACTOR_LANES) {
        const float *row = w1 + j * w1_stride;
        float s = b1[j];
        for (int i = 0; i < in; ++i) s = s + row[i] * x[i];
        const float h = s > 0.0f ? s : 0.0f;
        pq = pq + w2[j] * h;
        const float dh = s > 0.0f ? w2[j] * seed : 0.0f;
        d0 = d0 + row[in - 2] * dh;
        d1 = d1 + row[in - 1] * dh;
    }
    *part_q = pq;
    part_da[0] = d0;
    part_da[1] = d1;
}

/* dz_k of the actor's output from da_k and the rounded tanh */
OK_HD float ok_ddpg_seed(const float da, const float scale, const float t)
{
    const float g = da * scale;
    const float tt = t * t;
    const float d = 1.0f - tt;
    return g * d;
}

OK_HD float ok_ddpg_soft(const float p, const float target, const float tau, const float omt)
{
    const float a = tau * p;
    const float b = omt * target;
    return a + b;
}

/* (2 sum) / B for the critic, -(sum) / B for the actor; the losses sum / B and -(sum / B) */
OK_HD float ok_ddpg_scale_grad(const float sum, const float count, const int actor)
{
    return actor ? (-sum) / count : ok_dqn_scale_grad(sum, count);
}

OK_HD float ok_ddpg_scale_loss(const float sum, const float count, const int actor)
{
    const float l = sum / count;
    return actor ? -l : l;
}

#endif /* OKENV_DDPG_H */
