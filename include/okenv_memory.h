/*
 * okenv_memory.h -- the rule of the world-model racers' memory (WorldModelVaeRnn: the GRUDynamics network of train_rnn.py and
 * main.cpp:156-218, CmaEsAgent::runVaeRnn): the camera's frame of an agent -> the conv-VAE encoder's mu (okenv_world.h, unchanged) ->
 * a stacked GRU on [mu | last action] -> the agent's own controller on [mu | h_top] -> its steering.  The first recurrent driver: every
 * agent carries a hidden state [L][H] from act to act.  Shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_memory.h) and
 * the host entry okenv_memory_act_host.
 *
 * THE RULE
 *
 * Shape.  Z, the latent width, is the world shape's; A = 2 action values; the memory's width H (a multiple of 16 in 16 .. 512), its
 * layers L (1 .. 4), the controller's hidden width h (even, 2 .. OK_CTRL_MAX_HIDDEN), carry (0 or 1).  The reference: H = 512, L = 3,
 * h = 16.
 *
 * Parameters.  Two vectors.  The NETWORK vector (ok_memory_offsets), shared by all agents, in the order of torch's state_dict of
 * GRUDynamics, every tensor in torch's layout:
 *     for l = 0 .. L-1:  gru.weight_ih_l [3H][in_l] (in_0 = Z + 2, in_l = H),  gru.weight_hh_l [3H][H],  gru.bias_ih_l [3H],
 *                        gru.bias_hh_l [3H]                     -- the gate rows in torch's order: r, z, n
 *     head.weight [Z][H],  head.bias [Z]
 *     z_mean [Z],  z_std [Z],  a_mean [2],  a_std [2]            -- train_rnn.py's stats.npz
 * Every value must be finite and every std > 0 (ok_memory_params_bad).  The CONTROLLERS: [N][ok_controller_num_params(Z + H, h, 1)],
 * one row per agent, in the controller rule's order (okenv_math.h).
 *
 * One act of one agent, fp32 throughout, nothing fused but the fmaf's written here.
 *     mu        exactly okenv_world.h's (the conv chains, ok_world_mu).
 *     input     x0 = [(mu_j - z_mean_j) / z_std_j for j < Z,  (a_k - a_mean_k) / a_std_k for k < 2];  a = the agent's OKENV_F_THROTTLE /
 *               OKENV_F_STEER as stored when the act begins: the action of the step before, which runVaeRnn reads from
 *               current_action_ before updateAction overwrites it.
 *     chain     every sum over inputs (ok_memory_dot) runs in BLOCKS of OK_MEMORY_BLOCK = 64 k's: acc = bias; for each block in
 *               ascending order: part = +0.0f; for k ascending in the block: part = fmaf(x_k, w_k, part); then acc = acc + part (one
 *               rounded addition).  A block's partial sum is what an f32 MFMA accumulating from a zero C gives over one K block of
 *               the kernel; see the third departure below for why the chain is not one run from the bias.
 *     layer l   for unit j and gate g (0: r, 1: z, 2: n), x the layer's input (x0, or the layer below's NEW hidden state):
 *                   gi_g = ok_memory_dot(x, Wih[g H + j], H, bih[g H + j])           in layers l > 0
 *                   gi_g = ok_memory_dot(x0, Wih[g H + j], Z, bih[g H + j]) + pa     in layer 0: the Z latent columns in their
 *                          blocks, and the two action columns as a last block of their own, pa = fmaf(x0_{Z+1}, w_{Z+1},
 *                          fmaf(x0_Z, w_Z, +0.0f)) (a kernel runs the latent columns on the matrix cores, K a multiple of 4 with no
 *                          padding terms, and these two by hand, as ok_flow_hidden1 does)
 *                   gh_g = ok_memory_dot(h_prev, Whh[g H + j], H, bhh[g H + j])      with carry == 1
 *                   gh_g = bhh[g H + j]                                             with carry == 0: the rule itself leaves the chain
 *                          out, on the host and on the device alike, so no argument about zero terms is needed
 *                   r = sig(gi_0 + gh_0);  u = sig(gi_1 + gh_1);  n = ok_tanhf(gi_2 + r * gh_2)
 *                   h'_j = (1.0f - u) * n + u * h_prev_j          two multiplies and one add; with carry == 0, h_prev_j = +0.0f
 *                   sig(v) = 0.5f * ok_tanhf(0.5f * v) + 0.5f     no new transcendental: ok_tanhf is one set of bits everywhere
 *               Layer l + 1 reads layer l's h'.  The agent's hidden state becomes h' in every layer (also with carry == 0, where the
 *               next act does not read it).
 *     predict   (a record member only)  zn_j = ok_memory_dot(h_top, head.w[j], H, head.b[j]);  z_next_j = zn_j * z_std_j + z_mean_j
 *     control   x = [mu | h_top] (main.cpp:215; no heading terms), in = Z + H, through the controller rule (ok_world_controller);
 *               steering_delta = y * steer_scale;  throttle_delta = throttle.
 *
 * THREE DELIBERATE DEPARTURES from the reference and from the plainest reading of it.  (1) The latent is mu, not the reparameterised
 * draw mu + eps * exp(logvar / 2) the reference's runVaeRnn feeds: the encoder vector has no fc_logvar.  (2) carry.  carry == 0 is the
 * reference AS WRITTEN: rnn_model_.forward({x_seq}) with SEQ_LEN = 1 and no hidden argument starts from zero on every call, so its
 * "memory" never remembers.  carry == 1 is the memory the reference's Readme describes: h persists from act to act until it is reset.
 * (3) The chains are blocked.  One fused chain of 512 terms run from the bias (ok_lidar_dot) deviates from float64 about six times
 * more than torch's fp32 linear does (3.8e-07 against 6.3e-08 on sums of size 0.4): every term is rounded at the size of the running
 * sum.  Over four acts that put the hidden state of an H = 512 memory 5.8 x further from the float64 nn.GRU than the fp32 nn.GRU is;
 * with blocks of 64 it is 1.1 x (1.8 x with four layers).  The blocks cost the kernel one vector addition per accumulator and K block.
 *
 * Only fmaf, +, -, *, /, comparisons and ok_tanhf are used on top of okenv_world.h; compile with -ffp-contract=off.
 * Plain C99 / C++ / HIP.
 */
#ifndef OKENV_MEMORY_H
#define OKENV_MEMORY_H

#include "okenv_world.h"

#define OK_MEMORY_MAX_HIDDEN 512
#define OK_MEMORY_MAX_LAYERS 4
#define OK_MEMORY_ACTIONS 2
#define OK_MEMORY_BLOCK 64

typedef struct ok_memory_shape {
    int Z, H, L, h, carry;
} ok_memory_shape;

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_memory_shape_bad(const ok_memory_shape s)
{
    if (s.Z < 16 || s.Z > OK_WORLD_MAX_LATENT || s.Z % 16 != 0) return 1;
    if (s.H < 16 || s.H > OK_MEMORY_MAX_HIDDEN || s.H % 16 != 0) return 1;
    if (s.L < 1 || s.L > OK_MEMORY_MAX_LAYERS) return 1;
    if (s.h < 2 || s.h > OK_CTRL_MAX_HIDDEN || s.h % 2 != 0) return 1;
    if (s.carry != 0 && s.carry != 1) return 1;
    return 0;
}

/* Inputs of layer l */
OK_HDI int ok_memory_in(const ok_memory_shape s, const int l)
{
    return l == 0 ? s.Z + OK_MEMORY_ACTIONS : s.H;
}

/* Where the pieces of the network vector begin, in floats */
typedef struct ok_memory_layout {
    int wih[OK_MEMORY_MAX_LAYERS], whh[OK_MEMORY_MAX_LAYERS], bih[OK_MEMORY_MAX_LAYERS], bhh[OK_MEMORY_MAX_LAYERS];
    int hw, hb, z_mean, z_std, a_mean, a_std, total;
} ok_memory_layout;

OK_HDI ok_memory_layout ok_memory_offsets(const ok_memory_shape s)
{
    ok_memory_layout at;
    int              o = 0;
    for (int l = 0; l < OK_MEMORY_MAX_LAYERS; ++l) {
        const int live = l < s.L;
        at.wih[l] = o;
        o += live ? 3 * s.H * ok_memory_in(s, l) : 0;
        at.whh[l] = o;
        o += live ? 3 * s.H * s.H : 0;
        at.bih[l] = o;
        o += live ? 3 * s.H : 0;
        at.bhh[l] = o;
        o += live ? 3 * s.H : 0;
    }
    at.hw     = o;
    at.hb     = at.hw + s.Z * s.H;
    at.z_mean = at.hb + s.Z;
    at.z_std  = at.z_mean + s.Z;
    at.a_mean = at.z_std + s.Z;
    at.a_std  = at.a_mean + OK_MEMORY_ACTIONS;
    at.total  = at.a_std + OK_MEMORY_ACTIONS;
    return at;
}

OK_HDI int ok_memory_controller_params(const ok_memory_shape s)
{
    return ok_controller_num_params(s.Z + s.H, s.h, 1);
}

/* 0 when every value of a network vector is finite and every std > 0 */
OK_HD int ok_memory_params_bad(const ok_memory_shape s, const float *params)
{
    const ok_memory_layout at = ok_memory_offsets(s);
    for (int i = 0; i < at.total; ++i)
        if (!(params[i] - params[i] == 0.0f)) return 1;
    for (int i = at.z_std; i < at.z_std + s.Z; ++i)
        if (!(params[i] > 0.0f)) return 1;
    for (int i = at.a_std; i < at.a_std + OK_MEMORY_ACTIONS; ++i)
        if (!(params[i] > 0.0f)) return 1;
    return 0;
}

OK_HDI float ok_memory_sig(const float v)
{
    return 0.5f * ok_tanhf(0.5f * v) + 0.5f;
}

/* One sum over K inputs: blocks of OK_MEMORY_BLOCK k's, each a fused chain from +0.0f, added onto the bias in ascending order */
OK_HDI float ok_memory_dot(const float *x, const float *w, const int K, const float bias)
{
    float acc = bias;
    for (int k0 = 0; k0 < K; k0 += OK_MEMORY_BLOCK) {
        const int end  = k0 + OK_MEMORY_BLOCK < K ? k0 + OK_MEMORY_BLOCK : K;
        float     part = 0.0f;
        for (int k = k0; k < end; ++k) part = __builtin_fmaf(x[k], w[k], part);
        acc = acc + part;
    }
    return acc;
}

/* Layer 0's last block: the two action columns */
OK_HDI float ok_memory_action_part(const float *xa, const float *wa)
{
    return __builtin_fmaf(xa[1], wa[1], __builtin_fmaf(xa[0], wa[0], 0.0f));
}

/* One unit's new hidden value from its six gate sums */
OK_HDI float ok_memory_gate(const float gi_r, const float gi_z, const float gi_n, const float gh_r, const float gh_z, const float gh_n,
                            const float h_prev)
{
    const float r = ok_memory_sig(gi_r + gh_r), u = ok_memory_sig(gi_z + gh_z);
    const float n = ok_tanhf(gi_n + r * gh_n);
    const float keep = u * h_prev, fresh = (1.0f - u) * n;
    return fresh + keep;
}

/* One entry of the normalised input */
OK_HDI float ok_memory_normalise(const float v, const float mean, const float std)
{
    return (v - mean) / std;
}

/* Floats of work space ok_memory_step needs: the input [Z + 2] and one layer's new hidden state [H] */
OK_HDI int ok_memory_step_floats(const ok_memory_shape s)
{
    return s.Z + OK_MEMORY_ACTIONS + s.H;
}

/* Floats of work space ok_memory_forward needs: the encoder's and, behind them, the step's */
OK_HDI int ok_memory_work_floats(const ok_world_shape w, const ok_memory_shape s)
{
    return ok_world_work_floats(w) + ok_memory_step_floats(s);
}

/* One act of the memory on given mu [Z] and action [2] (throttle, steering as stored): hidden [L][H] in place; prediction [Z] or NULL;
 * work: ok_memory_step_floats floats */
OK_HD void ok_memory_step(const ok_memory_shape s, const float *params, const float *mu, const float *action, float *hidden, float *work,
                          float *prediction)
{
    const ok_memory_layout at = ok_memory_offsets(s);
    const int              H = s.H, Z = s.Z;
    float                 *x0 = work, *fresh = work + Z + OK_MEMORY_ACTIONS;
    for (int j = 0; j < Z; ++j) x0[j] = ok_memory_normalise(mu[j], params[at.z_mean + j], params[at.z_std + j]);
    for (int k = 0; k < OK_MEMORY_ACTIONS; ++k) x0[Z + k] = ok_memory_normalise(action[k], params[at.a_mean + k], params[at.a_std + k]);
    const float *x = x0;
    for (int l = 0; l < s.L; ++l) {
        const int    in  = ok_memory_in(s, l);
        const float *wih = params + at.wih[l], *whh = params + at.whh[l], *bih = params + at.bih[l], *bhh = params + at.bhh[l];
        float       *h   = hidden + l * H;
        for (int j = 0; j < H; ++j) {
            float gi[3], gh[3];
            for (int g = 0; g < 3; ++g) {
                const int row = g * H + j;
                gi[g] = ok_memory_dot(x, wih + row * in, l == 0 ? Z : H, bih[row]);
                if (l == 0) gi[g] = gi[g] + ok_memory_action_part(x + Z, wih + row * in + Z);
                gh[g] = s.carry ? ok_memory_dot(h, whh + row * H, H, bhh[row]) : bhh[row];
            }
            fresh[j] = ok_memory_gate(gi[0], gi[1], gi[2], gh[0], gh[1], gh[2], s.carry ? h[j] : 0.0f);
        }
        for (int j = 0; j < H; ++j) h[j] = fresh[j];
        x = h;
    }
    if (prediction) {
        const float *top = hidden + (s.L - 1) * H;
        for (int j = 0; j < Z; ++j)
            prediction[j] = ok_memory_dot(top, params + at.hw + j * H, H, params[at.hb + j]) * params[at.z_std + j] + params[at.z_mean + j];
    }
}

/* One agent on the host: frame [S][S][4] uint8, action [2] as stored, hidden [L][H] in place -> state [Z + H] (mu first), prediction [Z]
 * or NULL, and *out, the controller's output.  w.Z must be s.Z (w.h is not read).  work: ok_memory_work_floats floats */
OK_HD void ok_memory_forward(const ok_world_shape w, const ok_memory_shape s, const float *encoder, const float *network, const float *controller,
                             const uint8_t *frame, const float *action, float *hidden, float *work, float *state, float *prediction, float *out)
{
    const ok_world_layout at = ok_world_offsets(w);
    float                *in = work;
    for (int ch = 0; ch < 3; ++ch)
        for (int p = 0; p < w.S * w.S; ++p) in[ch * w.S * w.S + p] = ok_bev_pixel(frame[4 * p + ch]);
    int side_in = w.S;
    for (int l = 0; l < 4; ++l) {
        const int Cin = ok_world_cin(w, l), side = ok_world_side(w, l);
        float    *o = in + Cin * side_in * side_in;
        for (int n = 0; n < w.c[l]; ++n)
            for (int oy = 0; oy < side; ++oy)
                for (int ox = 0; ox < side; ++ox)
                    o[(n * side + oy) * side + ox] =
                        ok_lidar_relu(ok_world_conv_at(in, Cin, side_in, encoder + at.w[l] + n * Cin * 16, encoder[at.b[l] + n], oy, ox));
        in      = o;
        side_in = side;
    }
    const int F = w.c[3] * side_in * side_in;
    for (int j = 0; j < s.Z; ++j) state[j] = ok_world_mu(in, w.c[3], side_in, encoder + at.mw + j * F, encoder[at.mb + j]);
    ok_memory_step(s, network, state, action, hidden, work + ok_world_work_floats(w), prediction);
    for (int j = 0; j < s.H; ++j) state[s.Z + j] = hidden[(s.L - 1) * s.H + j];
    *out = ok_world_controller(controller, s.Z + s.H, s.h, state);
}

#endif /* OKENV_MEMORY_H */
