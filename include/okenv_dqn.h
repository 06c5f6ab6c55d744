/*
 * okenv_dqn.h -- the rule of Deep-Q learning (RLRacers/Deep_Q_Learning/dq_racer_sim.cpp:81-132, DQAgent.hpp:106-181,
 * common/ReplayBuffer.hpp): the replay ring, the uniform sampling and the temporal-difference update, shared bit for bit by the HIP
 * kernels (openkitchen_amd/csrc/ok_dqn.h) and the host entries okenv_replay_push_host / okenv_dqn_update_host.
 * Written on top of the actor's forward (okenv_math.h: ok_actor_*) and the learner's backward, sums and Adam (okenv_learn.h:
 * ok_learn_*).
 *
 * THE RULE
 *
 * The network.  The actor's R -> H -> A with one hidden layer and ReLU, in the order of torch's parameters().  The reference's
 * 400-300 stack is not carried over: it is a GEMM kernel, a different design.
 *
 * The replay ring.  Capacity C >= 1 slots of state [C][R], next_state [C][R], action [C] (int64), reward [C], done [C] (float, 1.0f or
 * 0.0f), and ONE 64-bit word `pushed` that counts every transition ever pushed.  The transition with push rank p (0, 1, 2, ...) lives in
 * slot ok_dqn_slot(p, C) = p mod C; size = min(pushed, C) (ok_dqn_size).  The reference's buffer is an unbounded deque; a bounded ring
 * that forgets the oldest is what a device store can be.
 *
 * One push.  After `act` and `step`, the selected agents' transitions are appended in ascending agent order: selected are the agents
 * whose record byte `alive` is non-zero (they entered the step alive: the project's "live" convention), or every agent with
 * OK_REPLAY_PUSH_ALL (the reference's loop pushes crashed agents' frozen observations too).  The k-th selected agent (k = 0 .. n-1) has
 * push rank pushed + k; afterwards pushed = pushed + n.  The result is AS IF they were pushed one by one: when n > C only the last C
 * survive (k >= n - C: ok_dqn_survives), so no slot is written twice by one push.
 *     state, action   the actor record of the act that preceded the step (x = dist / 200.0f as section 14 made it; the index)
 *     next_state[i]   dist[i] / 200.0f on the distances after the step: the IEEE division of the actor's rule
 *     done            crashed_ after the step: 1.0f or 0.0f
 *     reward          ok_dqn_reward: crashed_ ? -200.0f : min(200.0f, dist_0, dist_1, ...) taken as m = 200.0f; if (m > dist_i) m = dist_i
 *                     for i ascending (DQAgent.hpp:162-181; a NaN distance is never taken), or the caller's reward[a] when an array
 *                     is given (the tracker's progress, or the +1 of dq_racer_sim.cpp:100)
 *
 * Sampling.  Position q = 0 .. B-1 of draw d reads slot idx = (uint32)(((uint64)w * size) >> 32), w the first word of
 * Philox4x32-10(counter = (q, d, 7, 0), key = (seed, "oken")) (ok_dqn_sample).  Stream 7 is used by nothing else (0 .. 6: see
 * okenv_math.h).  Iteration i of an update draws d = draw_base + i with `resample`, else d = draw_base for every iteration
 * (DQAgent.hpp:113 draws once; :117 is the commented alternative).  With size == 0 there is nothing to read: every position counts
 * as an all-zero transition with e = 0, so the gradient and the loss are +0, Adam steps, and from zero moments that leaves the
 * parameters bit for bit (m = v = 0, the update is step * (0 / eps) = 0).
 *
 * Target (ok_dqn_target).  q' = net'(s') with the actor's forward (ok_actor_partial / ok_actor_join), net' the online parameters or,
 * with a target network, a frozen copy; m = max_k q'_k (m = q'_0; if (q'_k > m) m = q'_k ascending: a NaN never wins);
 *     y = r + gamma * m                              one fp32 multiplication, one addition, nothing fused (DQAgent.hpp:133)
 *     y = r + ((1.0f - done) * gamma) * m            with OK_DQN_MASK_DONE (DQAgent.hpp:134)
 * y is a constant of the backward pass (.detach()).
 *
 * Gradient.  q = net(s), a = the action clamped into 0 .. A-1, e = q_a - y.  The reference's target tensor is q with y at a, so
 * mse_loss(q, target) = sum_b e_b^2 / (B A) and its seed on the outputs is (2 / (B A)) e on output a and 0 on the others.  The seed
 * that enters the sums is e itself (ok_dqn_seed); the factor is applied once after the join:
 *     backward     okenv_learn.h's: dW2[k][j] = dz_k h_j, db2[k] = dz_k, ds_j = s_j > 0 ? sum_k w2[k][j] dz_k : 0, dW1[j][i] = ds_j x_i
 *     sums         section 16's Choice 2 exactly: chunks of OK_LEARN_CHUNK = 32 consecutive positions, acc = 0.0f; acc = acc + term in
 *                  ascending position (a separate multiplication and addition), the chunk partials joined by ok_learn_tree
 *     gradient     (2.0f * sum) / (float)(B * A)    the doubling is exact, then one IEEE division (ok_dqn_scale_grad)
 *     loss         (sum of e * e, summed the same way) / (float)(B * A)
 *     Adam         ok_learn_adam with ok_learn_factors' constants from the host; t, m and v are the learner's (section 16)
 * The forward of s' and of s in one iteration both see the parameters from before that iteration's step.
 *
 * Only +, -, *, /, sqrt and comparisons are used, IEEE-exact on x86-64 and gfx950 under -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_DQN_H
#define OKENV_DQN_H

#include "okenv_learn.h"

#define OK_REPLAY_PUSH_ALL 1u
#define OK_DQN_MASK_DONE 1u
#define OK_DQN_STREAM 7u
#define OK_DQN_CRASH_REWARD (-200.0f)

OK_HD uint64_t ok_dqn_slot(const uint64_t rank, const uint64_t capacity)
{
    return rank % capacity;
}

OK_HD uint64_t ok_dqn_size(const uint64_t pushed, const uint64_t capacity)
{
    return pushed < capacity ? pushed : capacity;
}

/* Does the k-th of n transitions of one push outlive that push in a ring of `capacity` slots? */
OK_HD int ok_dqn_survives(const uint64_t k, const uint64_t n, const uint64_t capacity)
{
    return n - k <= capacity;
}

/* DQLearnAgent::calculateReward on the distances after the step */
OK_HD float ok_dqn_reward(const int crashed, const float *dist, const int num_rays)
{
    if (crashed) return OK_DQN_CRASH_REWARD;
    float m = OK_SENSOR_RANGE;
    for (int i = 0; i < num_rays; ++i)
        if (m > dist[i]) m = dist[i];
    return m;
}

/* Slot of position q in draw d; size >= 1 */
OK_HDI uint32_t ok_dqn_sample(const uint32_t seed, const uint32_t q, const uint32_t d, const uint32_t size)
{
    const ok_u32x4 r = ok_philox4x32(q, d, OK_DQN_STREAM, 0u, seed, 0x6F6B656Eu);
    return ok_index_from_word(r.v[0], size);
}

/* max over q'[0 .. n-1] (OK_ACTOR_MAX_ACTIONS entries) */
OK_HDI float ok_dqn_max(const float *z, const int n)
{
    float m = z[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n && z[k] > m) m = z[k];
    return m;
}

OK_HDI float ok_dqn_target(const float reward, const float done, const float gamma, const float m, const uint32_t flags)
{
    const float g = (flags & OK_DQN_MASK_DONE) != 0u ? (1.0f - done) * gamma : gamma;
    const float gm = g * m;
    return reward + gm;
}

/* From the chosen output za = q_a of one sample to the seeds dz[0 .. OK_ACTOR_MAX_ACTIONS-1] and the squared error; `action` inside
 * 0 .. n-1.  `live` = 0 (an empty ring): e counts as 0.  (The caller looks q_a up: the kernel takes it from the lane that holds it
 * rather than index a register array.) */
OK_HDI void ok_dqn_seed(const float za, const int action, const float y, const int live, float *dz, float *sq)
{
    const float e = live ? za - y : 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        dz[k] = k == action ? e : 0.0f;
    *sq = e * e;
}

/* (float)(B * A): B * A < 2^31 is the callers' to check */
OK_HD float ok_dqn_count(const int batch, const int num_actions)
{
    return (float)((long long)batch * (long long)num_actions);
}

OK_HD float ok_dqn_scale_grad(const float sum, const float count)
{
    const float twice = 2.0f * sum;
    return twice / count;
}

OK_HD float ok_dqn_scale_loss(const float sum, const float count)
{
    return sum / count;
}

#endif /* OKENV_DQN_H */
