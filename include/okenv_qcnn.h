/*
 * okenv_qcnn.h -- the rule of the Deep-Q image racers (RLRacers/DQN_CNN: CNN.hpp, DQCNNAgent.hpp, dq_cnn_racer_sim.cpp): the camera's
 * RGBA8 frame of an agent -> one grey plane -> the Q-values of A actions -> an epsilon-greedy action, and the ring of frame
 * transitions the learner reads its batches from.  Shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_qcnn.h) and the host
 * entries okenv_qcnn_act_host / okenv_qcnn_push_host / okenv_qcnn_batch_host.
 *
 * THE RULE
 *
 * Shape.  Square frames of side S (16 .. 128), three PADDED convolutions l = 0, 1, 2 of kernel k_l (1 .. 8), stride s_l (1 .. 4,
 * s_l <= k_l) and padding p_l (0 .. 3, p_l < k_l): side_l = (side_{l-1} + 2 p_l - k_l) / s_l + 1 with the integer division (torch's
 * flooring; rows and columns at the far edge that no window reaches are unused), every side_l >= 1; c_l output channels (multiples of
 * 16 in 16 .. 128), ONE input channel; F = c_2 side_2^2 <= 16384 features; a hidden layer of H (a multiple of 16 in 16 .. 512); A
 * outputs (2 .. 8, OK_ACTOR_MAX_ACTIONS).  The reference's layers on the camera at S = 96: k = (8, 4, 3), s = (4, 2, 1), p = (2, 1, 1),
 * c = (32, 64, 64), H = 512, A = 5: sides 24 / 12 / 12, F = 9216, 4 793 509 parameters.  (The reference feeds a quarter-scale screen
 * grab of 350 x 400; as in okenv_cnn.h a resize is not part of the rule: the frames are rendered at the network's own size.)
 *
 * Parameter vector (ok_qcnn_offsets): torch's parameters() order of the reference module, every tensor in torch's layout:
 *     conv1.weight [c0][1][k0][k0],  conv1.bias [c0]
 *     conv2.weight [c1][c0][k1][k1], conv2.bias [c1]
 *     conv3.weight [c2][c1][k2][k2], conv3.bias [c2]
 *     fc1.weight [H][F], F indexed (ch side_2 + y) side_2 + x (torch's flatten),  fc1.bias [H]
 *     fc2.weight [A][H],             fc2.bias [A]
 * Every weight must be finite (see the zero terms below).
 *
 * Forward of one frame [S][S][4] uint8 (R, G, B, A; row 0 first), fp32 throughout, nothing fused but the fmaf's written here.
 *     grey      r, g, b = ok_bev_pixel of the three bytes ((float)byte / 255.0f, the IEEE division); then, as
 *               DQCNNAgent::imageToTensor evaluates it elementwise in torch, separate multiplications and additions:
 *                   t = r * 0.2989f;  t = t + g * 0.5870f;  t = t + b * 0.1140f          (ok_qcnn_grey)
 *               Alpha is not an input.
 *     conv      one output (channel n at (oy, ox)) is ok_lidar_relu of ONE fused chain started from the bias (ok_qcnn_conv_at), in
 *               ok_cnn_conv_at's order -- tap row, tap column, input channel, the channel innermost:
 *                   acc = bias[n];  for ty = 0 .. k-1, for tx = 0 .. k-1, for ch = 0 .. Cin-1:
 *                       acc = fmaf(in[ch](s oy + ty - p, s ox + tx - p), w[n][ch][ty][tx], acc)
 *               where a tap that falls into the padding reads +0.0f.
 *               ZERO TERMS.  A padding tap's term is fmaf(+0.0f, w, acc).  The host leaves it out; the device keeps it (its layers
 *               lie in LDS inside a border of +0.0f as wide as the next layer's padding, so that every tap is an ordinary read).
 *               With finite weights the product is +-0 and leaves acc's value unchanged; only the sign of a zero accumulator can
 *               differ, and the ReLU behind every convolution removes it.  This is okenv_cnn.h's argument for its alpha slot and
 *               filler taps carried to the border; the device's layer 0 also has those filler taps (weight 0.0f on a finite input)
 *               behind the last tap, up to a multiple of 16 terms.
 *     hidden    h[j] = ok_lidar_relu of ONE fused chain from the bias over the features in the order (y, x, channel)
 *               (ok_cnn_hidden_at), the weight read at torch's index [j][(ch side_2 + y) side_2 + x].
 *     Q-values  q[a] = ok_lidar_dot(h, fc2.weight[a], H, fc2.bias[a]).  No activation.
 *
 * Choice.  The shared-network actor's rule unchanged: best = ok_actor_argmax(q, A) (the lowest index wins a tie, a NaN never wins);
 * OK_ACTOR_GREEDY takes it, OK_ACTOR_EPS_GREEDY takes ok_actor_eps_greedy(epsilon, seed, agent_base + agent, draw, A, best).  An
 * image learner and a lidar learner with the same key so explore on the same steps with the same random indices.  The action fields
 * come from the table [8][2] of (throttle_delta, steering_delta) per index.
 *
 * Frame ring.  Capacity C >= 1 slots of state [C][S][S], next_state [C][S][S] (fp32 grey planes: what the learner's network takes),
 * action [C] (int64), reward [C], done [C] (1.0f or 0.0f) and the 64-bit word `pushed`.  okenv_dqn.h's ring: the transition with push
 * rank p lives in slot ok_dqn_slot(p, C), size = ok_dqn_size(pushed, C).  One push (ok_qcnn_push) selects and ranks as okenv_dqn.h's:
 * the agents whose `alive` byte of the act's record is non-zero, or every agent with OK_REPLAY_PUSH_ALL, in ascending agent order, AS
 * IF pushed one by one (ok_dqn_survives: of n > C only the last C are written, no slot twice; an agent whose transition does not
 * survive writes nothing).  state = grey of the frame the act saw, next_state = grey of the frame after the step, action = the
 * record's index, done = crashed_ after the step, reward = the caller's reward[a], or without an array ok_dqn_reward on the distances
 * after the step.
 *
 * Batch (ok_qcnn_batch).  B positions q = 0 .. B-1 are read from the ring into dense arrays; `index` receives the slot.
 *     OK_QCNN_BATCH_UNIFORM     slot ok_dqn_sample(seed, q, draw, size): stream 7, the lidar ring's draw
 *     OK_QCNN_BATCH_SEQUENTIAL  the transition with push rank first + ((start + q) mod size), first = pushed - size: the reference's
 *                               updateDQN walks its buffer in order, batch after batch.  THE ONE DIFFERENCE: the reference's last,
 *                               short batch ends at the buffer's end; here it wraps round to the oldest transitions, so that every
 *                               batch has B rows.
 * With size == 0 every output is zero and the index is 0.
 *
 * Only fmaf, +, *, /, and comparisons are used; compile with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_QCNN_H
#define OKENV_QCNN_H

#include "okenv_cnn.h"
#include "okenv_dqn.h"

#define OK_QCNN_MAX_PADDING 3
#define OK_QCNN_MAX_FEATURES 16384
#define OK_QCNN_BATCH_UNIFORM 0
#define OK_QCNN_BATCH_SEQUENTIAL 1

typedef struct ok_qcnn_shape {
    int S, k[3], s[3], p[3], c[3], H, A;
} ok_qcnn_shape;

OK_HDI int ok_qcnn_cin(const ok_qcnn_shape s, const int l)
{
    return l == 0 ? 1 : s.c[l - 1];
}

/* Output side of layer l (<= 0 when a kernel does not fit its padded input; -1 is the frame itself) */
OK_HDI int ok_qcnn_side(const ok_qcnn_shape s, const int l)
{
    int side = s.S;
    for (int i = 0; i <= l && i < 3; ++i) side = side + 2 * s.p[i] < s.k[i] ? 0 : (side + 2 * s.p[i] - s.k[i]) / s.s[i] + 1;
    return side;
}

OK_HDI int ok_qcnn_features(const ok_qcnn_shape s)
{
    return s.c[2] * ok_qcnn_side(s, 2) * ok_qcnn_side(s, 2);
}

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_qcnn_shape_bad(const ok_qcnn_shape s)
{
    if (s.S < OK_CNN_MIN_SIDE || s.S > OK_CNN_MAX_SIDE) return 1;
    for (int l = 0; l < 3; ++l) {
        if (s.k[l] < 1 || s.k[l] > OK_CNN_MAX_KERNEL) return 1;
        if (s.s[l] < 1 || s.s[l] > OK_CNN_MAX_STRIDE || s.s[l] > s.k[l]) return 1;
        if (s.p[l] < 0 || s.p[l] > OK_QCNN_MAX_PADDING || s.p[l] >= s.k[l]) return 1;
        if (s.c[l] < 16 || s.c[l] > OK_CNN_MAX_CHANNELS || s.c[l] % 16 != 0) return 1;
    }
    for (int l = 0; l < 3; ++l)
        if (ok_qcnn_side(s, l) < 1) return 1;
    if (ok_qcnn_features(s) > OK_QCNN_MAX_FEATURES) return 1;
    if (s.H < 16 || s.H > OK_CNN_MAX_HIDDEN || s.H % 16 != 0) return 1;
    if (s.A < 2 || s.A > OK_ACTOR_MAX_ACTIONS) return 1;
    return 0;
}

/* Where the pieces of the parameter vector begin, in floats */
typedef struct ok_qcnn_layout {
    int w[3], b[3], hw, hb, ow, ob, total;
} ok_qcnn_layout;

OK_HDI ok_qcnn_layout ok_qcnn_offsets(const ok_qcnn_shape s)
{
    ok_qcnn_layout at;
    int            o = 0;
    for (int l = 0; l < 3; ++l) {
        at.w[l] = o;
        o += s.c[l] * ok_qcnn_cin(s, l) * s.k[l] * s.k[l];
        at.b[l] = o;
        o += s.c[l];
    }
    at.hw    = o;
    at.hb    = at.hw + s.H * ok_qcnn_features(s);
    at.ow    = at.hb + s.H;
    at.ob    = at.ow + s.A * s.H;
    at.total = at.ob + s.A;
    return at;
}

/* One pixel's grey from its R, G and B bytes */
OK_HDI float ok_qcnn_grey(const uint8_t r, const uint8_t g, const uint8_t b)
{
    float       t  = ok_bev_pixel(r) * 0.2989f;
    const float tg = ok_bev_pixel(g) * 0.5870f;
    t              = t + tg;
    const float tb = ok_bev_pixel(b) * 0.1140f;
    t              = t + tb;
    return t;
}

/* One output of a padded convolution before its ReLU: in [Cin][side_in][side_in] (planar), w = weight[n] [Cin][k][k].  The padding's
 * taps are left out (ZERO TERMS above). */
OK_HD float ok_qcnn_conv_at(const float *in, const int Cin, const int side_in, const float *w, const int k, const int stride, const int pad,
                            const float bias, const int oy, const int ox)
{
    float acc = bias;
    for (int ty = 0; ty < k; ++ty) {
        const int y = stride * oy + ty - pad;
        if (y < 0 || y >= side_in) continue;
        for (int tx = 0; tx < k; ++tx) {
            const int x = stride * ox + tx - pad;
            if (x < 0 || x >= side_in) continue;
            for (int ch = 0; ch < Cin; ++ch) acc = __builtin_fmaf(in[(ch * side_in + y) * side_in + x], w[(ch * k + ty) * k + tx], acc);
        }
    }
    return acc;
}

/* Floats of work space ok_qcnn_forward needs: the grey plane, the three layers' outputs (planar) and the hidden layer */
OK_HDI int ok_qcnn_work_floats(const ok_qcnn_shape s)
{
    int n = s.S * s.S + s.H;
    for (int l = 0; l < 3; ++l) n += s.c[l] * ok_qcnn_side(s, l) * ok_qcnn_side(s, l);
    return n;
}

/* The network on one grey plane [S][S]: q[0 .. A-1].  work: ok_qcnn_work_floats(s) - S S floats. */
OK_HD void ok_qcnn_forward_plane(const ok_qcnn_shape s, const float *params, const float *plane, float *work, float *q)
{
    const ok_qcnn_layout at = ok_qcnn_offsets(s);
    const float         *in = plane;
    float               *o  = work;
    int                  side_in = s.S;
    for (int l = 0; l < 3; ++l) {
        const int Cin = ok_qcnn_cin(s, l), side = ok_qcnn_side(s, l), k = s.k[l];
        for (int n = 0; n < s.c[l]; ++n)
            for (int oy = 0; oy < side; ++oy)
                for (int ox = 0; ox < side; ++ox)
                    o[(n * side + oy) * side + ox] = ok_lidar_relu(ok_qcnn_conv_at(in, Cin, side_in, params + at.w[l] + n * Cin * k * k, k, s.s[l],
                                                                                  s.p[l], params[at.b[l] + n], oy, ox));
        in = o;
        o += s.c[l] * side * side;
        side_in = side;
    }
    const int F = s.c[2] * side_in * side_in;
    float    *h = o;
    for (int j = 0; j < s.H; ++j) h[j] = ok_lidar_relu(ok_cnn_hidden_at(in, s.c[2], side_in, params + at.hw + j * F, params[at.hb + j]));
    for (int a = 0; a < s.A; ++a) q[a] = ok_lidar_dot(h, params + at.ow + a * s.H, s.H, params[at.ob + a]);
}

/* The grey plane [S][S] of one frame [S][S][4] */
OK_HD void ok_qcnn_grey_plane(const int S, const uint8_t *frame, float *plane)
{
    for (int p = 0; p < S * S; ++p) plane[p] = ok_qcnn_grey(frame[4 * p], frame[4 * p + 1], frame[4 * p + 2]);
}

/* The whole network of one frame on the host: frame [S][S][4] uint8 -> q[0 .. A-1] */
OK_HD void ok_qcnn_forward(const ok_qcnn_shape s, const float *params, const uint8_t *frame, float *work, float *q)
{
    ok_qcnn_grey_plane(s.S, frame, work);
    ok_qcnn_forward_plane(s, params, work, work + s.S * s.S, q);
}

/* The action of one agent from its Q-values q[0 .. A-1]; mode OK_ACTOR_GREEDY or OK_ACTOR_EPS_GREEDY */
OK_HD int ok_qcnn_choose(const int mode, const float epsilon, const uint32_t seed, const uint32_t agent, const uint32_t draw, const float *q, const int A)
{
    float z[OK_ACTOR_MAX_ACTIONS];
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k) z[k] = k < A ? q[k] : 0.0f;
    const int best = ok_actor_argmax(z, A);
    return mode == OK_ACTOR_EPS_GREEDY ? ok_actor_eps_greedy(epsilon, seed, agent, draw, A, best) : best;
}

/* ---- the frame ring ---- */

typedef struct ok_qcnn_ring {
    float   *state, *next_state; /* [C][S][S] */
    int64_t *action;             /* [C] */
    float   *reward, *done;      /* [C] */
} ok_qcnn_ring;

/* One push of n agents.  action [n]; alive [n] (may be NULL with OK_REPLAY_PUSH_ALL); frames, next_frames [n][S][S][4]; crashed [n] after
 * the step; reward [n], or NULL: ok_dqn_reward on dist [n][num_rays]. */
OK_HD void ok_qcnn_push(const ok_qcnn_ring ring, const uint64_t capacity, const int S, uint64_t *pushed, const uint32_t flags, const int n_agents,
                        const int64_t *action, const uint8_t *alive, const uint8_t *frames, const uint8_t *next_frames, const uint8_t *crashed,
                        const float *reward, const float *dist, const int num_rays)
{
    const int    all = (flags & OK_REPLAY_PUSH_ALL) != 0u;
    const size_t px  = (size_t)S * (size_t)S;
    uint64_t     n = 0, k = 0;
    for (int a = 0; a < n_agents; ++a) n += (all || alive[a] != 0) ? 1u : 0u;
    for (int a = 0; a < n_agents; ++a) {
        if (!(all || alive[a] != 0)) continue;
        if (ok_dqn_survives(k, n, capacity)) {
            const size_t slot  = (size_t)ok_dqn_slot(*pushed + k, capacity);
            const int    crash = crashed[a] != 0;
            ok_qcnn_grey_plane(S, frames + (size_t)a * px * 4u, ring.state + slot * px);
            ok_qcnn_grey_plane(S, next_frames + (size_t)a * px * 4u, ring.next_state + slot * px);
            ring.action[slot] = action[a];
            ring.done[slot]   = crash ? 1.0f : 0.0f;
            ring.reward[slot] = reward != 0 ? reward[a] : ok_dqn_reward(crash, dist + (size_t)a * (size_t)num_rays, num_rays);
        }
        ++k;
    }
    *pushed += n;
}

/* Where a batch goes: each pointer may be NULL */
typedef struct ok_qcnn_batch_out {
    float   *state, *next_state; /* [B][S][S] */
    int64_t *action;             /* [B] */
    float   *reward, *done;      /* [B] */
    int32_t *index;              /* [B] the slot */
} ok_qcnn_batch_out;

/* The slot of position q of a batch; size >= 1 */
OK_HDI uint64_t ok_qcnn_batch_slot(const int mode, const uint32_t seed, const uint64_t start_or_draw, const uint32_t q, const uint64_t pushed,
                                   const uint64_t size, const uint64_t capacity)
{
    if (mode == OK_QCNN_BATCH_UNIFORM) return ok_dqn_sample(seed, q, (uint32_t)start_or_draw, (uint32_t)size);
    const uint64_t first = pushed - size, at = (start_or_draw % size + q) % size;
    return ok_dqn_slot(first + at, capacity);
}

OK_HD void ok_qcnn_batch(const ok_qcnn_ring ring, const uint64_t capacity, const int S, const uint64_t pushed, const uint32_t seed, const int B,
                         const int mode, const uint64_t start_or_draw, const ok_qcnn_batch_out out)
{
    const uint64_t size = ok_dqn_size(pushed, capacity);
    const size_t   px   = (size_t)S * (size_t)S;
    for (int q = 0; q < B; ++q) {
        const size_t slot = size != 0u ? (size_t)ok_qcnn_batch_slot(mode, seed, start_or_draw, (uint32_t)q, pushed, size, capacity) : 0u;
        for (size_t i = 0; i < px; ++i) {
            if (out.state != 0) out.state[(size_t)q * px + i] = size != 0u ? ring.state[slot * px + i] : 0.0f;
            if (out.next_state != 0) out.next_state[(size_t)q * px + i] = size != 0u ? ring.next_state[slot * px + i] : 0.0f;
        }
        if (out.action != 0) out.action[q] = size != 0u ? ring.action[slot] : 0;
        if (out.reward != 0) out.reward[q] = size != 0u ? ring.reward[slot] : 0.0f;
        if (out.done != 0) out.done[q] = size != 0u ? ring.done[slot] : 0.0f;
        if (out.index != 0) out.index[q] = (int32_t)slot;
    }
}

#endif /* OKENV_QCNN_H */
