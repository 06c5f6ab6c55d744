/*
 * okenv_world.h -- the rule of the world-model racers (WorldModelVaeRnn/main.cpp: CmaEsAgent::runVaeOnly and updateAction, with the
 * encoder of train_vae.py): the camera's RGBA8 frame of an agent -> the conv-VAE encoder's mu -> the agent's own controller -> its
 * steering, and the fitness main.cpp:329-342 accumulates.  Shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_world.h) and
 * the host entries okenv_world_act_host / okenv_world_score_host.
 *
 * THE RULE
 *
 * Shape.  Square frames of side S (a multiple of 16 in 16 .. 128), four convolutions l = 0 .. 3 of kernel 4, stride 2 and padding 1,
 * all fixed -- the sides halve to S/2, S/4, S/8, S/16 -- with c_l output channels (multiples of 16 in 16 .. 512), 3 input channels;
 * the latent width Z (a multiple of 16 in 16 .. 128); F = c_3 (S/16)^2 <= 32768 features; the controller's hidden width h (even,
 * 2 .. OK_CTRL_MAX_HIDDEN).  The reference: S = 128, c = (64, 128, 256, 512), Z = 32, h = 16.
 *
 * Parameters.  Two vectors.  The ENCODER vector (ok_world_offsets), shared by all agents, every tensor in torch's layout:
 *     net.0.weight [c0][3][4][4],  net.0.bias [c0]
 *     net.2.weight [c1][c0][4][4], net.2.bias [c1]        (eval-mode BatchNorm net.3 folded in)
 *     net.5.weight [c2][c1][4][4], net.5.bias [c2]        (net.6 folded in)
 *     net.8.weight [c3][c2][4][4], net.8.bias [c3]        (net.9 folded in)
 *     fc_mu.weight [Z][F], F indexed (ch side_3 + y) side_3 + x (torch's flatten),  fc_mu.bias [Z]
 * fc_logvar is not part of it: the driver reads mu only.  The CONTROLLERS: [N][ok_controller_num_params(Z + 2, h, 1)], one row per
 * agent, in the controller rule's order (okenv_math.h).  Every weight must be finite (see the zero terms below).
 *
 * Forward of one frame [S][S][4] uint8 (R, G, B, A; row 0 first), fp32 throughout, nothing fused but the fmaf's written here.
 *     pixel     ok_bev_pixel: (float)byte / 255.0f.  Alpha is not an input.
 *     conv      one output (channel n at (oy, ox)) is ok_lidar_relu of ONE fused chain started from the bias (ok_world_conv_at):
 *                   acc = bias[n];  for ty = 0 .. 3, for tx = 0 .. 3, for ch = 0 .. Cin-1:
 *                       acc = fmaf(in[ch](2 oy + ty - 1, 2 ox + tx - 1), w[n][ch][ty][tx], acc)
 *               -- tap row, tap column, input channel, the channel innermost.  Taps outside the input are left out.
 *               ZERO TERMS (okenv_bev.h's argument, restated).  The device's chain contains, at their place in this order, terms the
 *               host leaves out: the padding taps (input 0.0f) and layer 0's fourth channel behind every tap (the frame's alpha slot:
 *               input 0.0f, weight 0.0f).  With finite weights each is fmaf(x, w, acc) with x w = +-0 and leaves acc's value
 *               unchanged; only the sign of a zero accumulator can differ, and the ReLU behind every convolution removes it.
 *     mu[j]     one partial chain per position, then a sequential sum (ok_world_mu).  For p = y side_3 + x ascending:
 *                   part_p = +0.0f;  for ch = 0 .. c3-1:  part_p = fmaf(a[ch][y][x], w[j][(ch side_3 + y) side_3 + x], part_p)
 *               then mu = bias[j];  for p ascending: mu = mu + part_p.  The order is fixed this way so that a kernel may run the
 *               (S/16)^2 partial chains in parallel and still agree bit for bit.
 *     state     x = [mu_0 .. mu_{Z-1}, s, c] with ok_sincosf(rot, &s, &c), rot the agent's OKENV_F_ROT value AS STORED, in degrees:
 *               the reference calls std::sin(rot_) / std::cos(rot_) on the degree value (main.cpp:231).  That is the reference's
 *               behaviour and is kept.
 *     control   the controller rule (okenv_math.h: every unit starts from its bias and adds w * x in ascending input order, one
 *               multiply and one add per term, no FMA; ok_tanhf after each of the three layers) with in = Z + 2 and out = 1
 *               (ok_world_controller);  steering_delta = y * steer_scale;  throttle_delta = throttle.
 *
 * Score (main.cpp:329-342), per agent (ok_world_score): if not crashed, fitness += 1.0f - d, d = RaceTrack::getDistanceToLaneCenter:
 * the squared distance to every centre-line point is ddx*ddx + ddy*ddy without FMA, the first minimum in ascending index wins,
 * d = sqrtf(min) / (w_left[i] + w_right[i]).  Otherwise, if timed out, fitness = 0.
 *
 * Against torch the chains' order differs: rounding only.  A resize of the frame is not part of the rule: the frames are rendered at
 * the encoder's own size.
 *
 * Only fmaf, +, *, /, sqrtf, comparisons, ok_sincosf and ok_tanhf are used; compile with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_WORLD_H
#define OKENV_WORLD_H

#include <float.h>

#include "okenv_bev.h"

#define OK_WORLD_MIN_SIDE 16
#define OK_WORLD_MAX_SIDE 128
#define OK_WORLD_MAX_CHANNELS 512
#define OK_WORLD_MAX_LATENT 128
#define OK_WORLD_MAX_FEATURES 32768

typedef struct ok_world_shape {
    int S, c[4], Z, h;
} ok_world_shape;

/* Input channels and output side of layer l */
OK_HDI int ok_world_cin(const ok_world_shape s, const int l)
{
    return l == 0 ? 3 : s.c[l - 1];
}

OK_HDI int ok_world_side(const ok_world_shape s, const int l)
{
    return s.S >> (l + 1);
}

OK_HDI int ok_world_features(const ok_world_shape s)
{
    return s.c[3] * ok_world_side(s, 3) * ok_world_side(s, 3);
}

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_world_shape_bad(const ok_world_shape s)
{
    if (s.S < OK_WORLD_MIN_SIDE || s.S > OK_WORLD_MAX_SIDE || s.S % 16 != 0) return 1;
    for (int l = 0; l < 4; ++l)
        if (s.c[l] < 16 || s.c[l] > OK_WORLD_MAX_CHANNELS || s.c[l] % 16 != 0) return 1;
    if (s.Z < 16 || s.Z > OK_WORLD_MAX_LATENT || s.Z % 16 != 0) return 1;
    if (ok_world_features(s) > OK_WORLD_MAX_FEATURES) return 1;
    if (s.h < 2 || s.h > OK_CTRL_MAX_HIDDEN || s.h % 2 != 0) return 1;
    return 0;
}

/* Where the pieces of the encoder vector begin, in floats */
typedef struct ok_world_layout {
    int w[4], b[4], mw, mb, total;
} ok_world_layout;

OK_HDI ok_world_layout ok_world_offsets(const ok_world_shape s)
{
    ok_world_layout at;
    int             o = 0;
    for (int l = 0; l < 4; ++l) {
        at.w[l] = o;
        o += s.c[l] * ok_world_cin(s, l) * 16;
        at.b[l] = o;
        o += s.c[l];
    }
    at.mw    = o;
    at.mb    = at.mw + s.Z * ok_world_features(s);
    at.total = at.mb + s.Z;
    return at;
}

OK_HDI int ok_world_controller_params(const ok_world_shape s)
{
    return ok_controller_num_params(s.Z + 2, s.h, 1);
}

/* One output of a convolution before its ReLU: in [Cin][side_in][side_in] (planar), w = weight[n] [Cin][4][4] */
OK_HD float ok_world_conv_at(const float *in, const int Cin, const int side_in, const float *w, const float bias, const int oy, const int ox)
{
    float acc = bias;
    for (int ty = 0; ty < 4; ++ty) {
        const int y = 2 * oy + ty - 1;
        if (y < 0 || y >= side_in) continue;
        for (int tx = 0; tx < 4; ++tx) {
            const int x = 2 * ox + tx - 1;
            if (x < 0 || x >= side_in) continue;
            for (int ch = 0; ch < Cin; ++ch) acc = __builtin_fmaf(in[(ch * side_in + y) * side_in + x], w[(ch * 4 + ty) * 4 + tx], acc);
        }
    }
    return acc;
}

/* One latent: a [C][side][side] (planar: torch's flatten), w = fc_mu.weight[j] [C side side] */
OK_HD float ok_world_mu(const float *a, const int C, const int side, const float *w, const float bias)
{
    const int P  = side * side;
    float     mu = bias;
    for (int p = 0; p < P; ++p) {
        float part = 0.0f;
        for (int ch = 0; ch < C; ++ch) part = __builtin_fmaf(a[ch * P + p], w[ch * P + p], part);
        mu = mu + part;
    }
    return mu;
}

/* One layer of the controller rule: out[u] = tanh(b[u] + sum of w[u][i] * x[i], i ascending, no FMA) */
OK_HD void ok_world_ctrl_layer(const float *w, const float *b, const int n_in, const int n_out, const float *x, float *out)
{
    for (int u = 0; u < n_out; ++u) {
        float acc = b[u];
        for (int i = 0; i < n_in; ++i) acc = acc + w[u * n_in + i] * x[i];
        out[u] = ok_tanhf(acc);
    }
}

/* One agent's controller on its state x [Z + 2]: prm in the controller rule's order; the output behind its tanh */
OK_HD float ok_world_controller(const float *prm, const int in, const int h, const float *x)
{
    const int    h2 = h / 2;
    const float *w1 = prm, *b1 = w1 + h * in, *w2 = b1 + h, *b2 = w2 + h2 * h, *w3 = b2 + h2, *b3 = w3 + h2;
    float        a1[OK_CTRL_MAX_HIDDEN], a2[OK_CTRL_MAX_HIDDEN / 2], y;
    ok_world_ctrl_layer(w1, b1, in, h, x, a1);
    ok_world_ctrl_layer(w2, b2, h, h2, a1, a2);
    ok_world_ctrl_layer(w3, b3, h2, 1, a2, &y);
    return y;
}

/* Floats of work space ok_world_forward needs: the input and the four layers' outputs, planar */
OK_HDI int ok_world_work_floats(const ok_world_shape s)
{
    int n = 3 * s.S * s.S;
    for (int l = 0; l < 4; ++l) n += s.c[l] * ok_world_side(s, l) * ok_world_side(s, l);
    return n;
}

/* One agent on the host: frame [S][S][4] uint8, rot in degrees as stored -> state [Z + 2] (mu first) and *out, the controller's output */
OK_HD void ok_world_forward(const ok_world_shape s, const float *encoder, const float *controller, const uint8_t *frame, const float rot,
                            float *work, float *state, float *out)
{
    const ok_world_layout at = ok_world_offsets(s);
    float                *in = work;
    for (int ch = 0; ch < 3; ++ch)
        for (int p = 0; p < s.S * s.S; ++p) in[ch * s.S * s.S + p] = ok_bev_pixel(frame[4 * p + ch]);
    int side_in = s.S;
    for (int l = 0; l < 4; ++l) {
        const int Cin = ok_world_cin(s, l), side = ok_world_side(s, l);
        float    *o = in + Cin * side_in * side_in;
        for (int n = 0; n < s.c[l]; ++n)
            for (int oy = 0; oy < side; ++oy)
                for (int ox = 0; ox < side; ++ox)
                    o[(n * side + oy) * side + ox] =
                        ok_lidar_relu(ok_world_conv_at(in, Cin, side_in, encoder + at.w[l] + n * Cin * 16, encoder[at.b[l] + n], oy, ox));
        in      = o;
        side_in = side;
    }
    const int F = s.c[3] * side_in * side_in;
    for (int j = 0; j < s.Z; ++j) state[j] = ok_world_mu(in, s.c[3], side_in, encoder + at.mw + j * F, encoder[at.mb + j]);
    ok_sincosf(rot, &state[s.Z], &state[s.Z + 1]);
    *out = ok_world_controller(controller, s.Z + 2, s.h, state);
}

/* RaceTrack::getDistanceToLaneCenter of (x, y) */
OK_HD float ok_world_lane_distance(const float *cx, const float *cy, const float *w_left, const float *w_right, const int P, const float x,
                                   const float y)
{
    float best = FLT_MAX;
    int   at   = 0;
    for (int i = 0; i < P; ++i) {
        const float ddx = x - cx[i], ddy = y - cy[i];
        const float d2 = ddx * ddx + ddy * ddy;
        if (d2 < best) {
            best = d2;
            at   = i;
        }
    }
    return __builtin_sqrtf(best) / (w_left[at] + w_right[at]);
}

/* One agent's fitness after one step of the loop (main.cpp:329-342) */
OK_HD float ok_world_score(const float fitness, const int crashed, const int timed_out, const float *cx, const float *cy, const float *w_left,
                           const float *w_right, const int P, const float x, const float y)
{
    if (!crashed) return fitness + (1.0f - ok_world_lane_distance(cx, cy, w_left, w_right, P, x, y));
    return timed_out ? 0.0f : fitness;
}

#endif /* OKENV_WORLD_H */
