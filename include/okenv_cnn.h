/*
 * okenv_cnn.h -- the rule of the behavioural-cloning image policy (BehavioralCloning/env_train_bc.py: PolicyCNN, driven as main.cpp
 * drives it): the camera's RGBA8 frame of an agent -> its steering.  Shared bit for bit by the HIP kernels
 * (openkitchen_amd/csrc/ok_cnn.h) and the host entry okenv_cnn_act_host.
 *
 * THE RULE
 *
 * Shape.  Square frames of side S (16 .. 128), three VALID convolutions l = 0, 1, 2 of kernel k_l (1 .. 8) and stride s_l (1 .. 4,
 * s_l <= k_l), no padding: side_l = (side_{l-1} - k_l) / s_l + 1 with the integer division (torch's flooring; rows and columns at the
 * far edge that no window reaches are unused), every side_l >= 1; c_l output channels (multiples of 16 in 16 .. 128), 3 input channels;
 * F = c_2 side_2^2 <= 8192 features; a hidden layer of H (a multiple of 16 in 16 .. 512); one output.  The reference: S = 96,
 * k = (8, 4, 3), s = (4, 2, 1), c = (32, 64, 64), H = 256: sides 23 / 10 / 8, F = 4096.
 *
 * Parameter vector (ok_cnn_offsets): torch's parameters() order of the reference module, every tensor in torch's layout:
 *     encoder.0.weight [c0][3][k0][k0],  encoder.0.bias [c0]
 *     encoder.2.weight [c1][c0][k1][k1], encoder.2.bias [c1]
 *     encoder.4.weight [c2][c1][k2][k2], encoder.4.bias [c2]
 *     steering_head.0.weight [H][F], F indexed (ch side_2 + y) side_2 + x (torch's flatten),  steering_head.0.bias [H]
 *     steering_head.2.weight [1][H],     steering_head.2.bias [1]
 * Every weight must be finite (see the zero terms below).
 *
 * Forward of one frame [S][S][4] uint8 (R, G, B, A; row 0 first), fp32 throughout, nothing fused but the fmaf's written here.
 *     pixel     ok_bev_pixel: (float)byte / 255.0f, the IEEE division.  Alpha is not an input.
 *     conv      one output (channel n at (oy, ox)) is ok_lidar_relu of ONE fused chain started from the bias (ok_cnn_conv_at):
 *                   acc = bias[n];  for ty = 0 .. k-1, for tx = 0 .. k-1, for ch = 0 .. Cin-1:
 *                       acc = fmaf(in[ch](s oy + ty, s ox + tx), w[n][ch][ty][tx], acc)
 *               -- tap row, tap column, input channel, the channel innermost; ok_bev_conv_at's order with nothing left out.
 *               ZERO TERMS.  The device's chain contains, at their place in this order, terms the host leaves out: layer 0's fourth
 *               channel behind every tap (the frame's alpha slot, weight 0.0f, a finite input) and filler taps behind the last one that
 *               round layer 0's chain up to a multiple of 16 terms (weight 0.0f, a finite input).  With finite weights and inputs each
 *               is fmaf(x, w, acc) with x w = +-0 and leaves acc's value unchanged; only the sign of a zero accumulator can differ, and
 *               the ReLU behind every convolution removes it.
 *     hidden    h[j] = ok_lidar_relu of ONE fused chain from the bias over the features in the order (y, x, channel), the channel
 *               innermost (ok_cnn_hidden_at) -- the conv chains' order, NOT torch's flatten order; the weight is still read at torch's
 *               index [j][(ch side_2 + y) side_2 + x].  Layer 2's output can so stay channels-last on the device, and four consecutive
 *               terms are four channels of one position.
 *     output    o = ok_lidar_dot(h, w2, H, b2);  y = ok_tanhf(o);  steering_delta = y * steer_scale;  throttle_delta = throttle.
 *
 * Against torch only the chains' order differs: rounding only.  A resize of the frame is not part of the rule: the frames are rendered
 * at the policy's own size.
 *
 * Only fmaf, +, *, /, comparisons and ok_tanhf are used; compile with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_CNN_H
#define OKENV_CNN_H

#include "okenv_bev.h"

#define OK_CNN_MIN_SIDE 16
#define OK_CNN_MAX_SIDE 128
#define OK_CNN_MAX_KERNEL 8
#define OK_CNN_MAX_STRIDE 4
#define OK_CNN_MAX_CHANNELS 128
#define OK_CNN_MAX_FEATURES 8192
#define OK_CNN_MAX_HIDDEN 512

typedef struct ok_cnn_shape {
    int S, k[3], s[3], c[3], H;
} ok_cnn_shape;

/* Input channels and output side of layer l (the side is <= 0 when a kernel does not fit its input; -1 is the frame itself) */
OK_HDI int ok_cnn_cin(const ok_cnn_shape s, const int l)
{
    return l == 0 ? 3 : s.c[l - 1];
}

OK_HDI int ok_cnn_side(const ok_cnn_shape s, const int l)
{
    int side = s.S;
    for (int i = 0; i <= l && i < 3; ++i) side = side < s.k[i] ? 0 : (side - s.k[i]) / s.s[i] + 1;
    return side;
}

OK_HDI int ok_cnn_features(const ok_cnn_shape s)
{
    return s.c[2] * ok_cnn_side(s, 2) * ok_cnn_side(s, 2);
}

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_cnn_shape_bad(const ok_cnn_shape s)
{
    if (s.S < OK_CNN_MIN_SIDE || s.S > OK_CNN_MAX_SIDE) return 1;
    for (int l = 0; l < 3; ++l) {
        if (s.k[l] < 1 || s.k[l] > OK_CNN_MAX_KERNEL) return 1;
        if (s.s[l] < 1 || s.s[l] > OK_CNN_MAX_STRIDE || s.s[l] > s.k[l]) return 1;
        if (s.c[l] < 16 || s.c[l] > OK_CNN_MAX_CHANNELS || s.c[l] % 16 != 0) return 1;
    }
    for (int l = 0; l < 3; ++l)
        if (ok_cnn_side(s, l) < 1) return 1;
    if (ok_cnn_features(s) > OK_CNN_MAX_FEATURES) return 1;
    if (s.H < 16 || s.H > OK_CNN_MAX_HIDDEN || s.H % 16 != 0) return 1;
    return 0;
}

/* Where the pieces of the parameter vector begin, in floats */
typedef struct ok_cnn_layout {
    int w[3], b[3], hw, hb, ow, ob, total;
} ok_cnn_layout;

OK_HDI ok_cnn_layout ok_cnn_offsets(const ok_cnn_shape s)
{
    ok_cnn_layout at;
    int           o = 0;
    for (int l = 0; l < 3; ++l) {
        at.w[l] = o;
        o += s.c[l] * ok_cnn_cin(s, l) * s.k[l] * s.k[l];
        at.b[l] = o;
        o += s.c[l];
    }
    at.hw    = o;
    at.hb    = at.hw + s.H * ok_cnn_features(s);
    at.ow    = at.hb + s.H;
    at.ob    = at.ow + s.H;
    at.total = at.ob + 1;
    return at;
}

/* One output of a convolution before its ReLU: in [Cin][side_in][side_in] (planar), w = weight[n] [Cin][k][k] */
OK_HD float ok_cnn_conv_at(const float *in, const int Cin, const int side_in, const float *w, const int k, const int stride, const float bias,
                           const int oy, const int ox)
{
    float acc = bias;
    for (int ty = 0; ty < k; ++ty) {
        const int y = stride * oy + ty;
        for (int tx = 0; tx < k; ++tx) {
            const int x = stride * ox + tx;
            for (int ch = 0; ch < Cin; ++ch) acc = __builtin_fmaf(in[(ch * side_in + y) * side_in + x], w[(ch * k + ty) * k + tx], acc);
        }
    }
    return acc;
}

/* One unit of the hidden layer before its ReLU: a [C][side][side] (planar: torch's flatten), w = weight[j] [C side side] */
OK_HD float ok_cnn_hidden_at(const float *a, const int C, const int side, const float *w, const float bias)
{
    float acc = bias;
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x)
            for (int ch = 0; ch < C; ++ch) {
                const int at = (ch * side + y) * side + x;
                acc          = __builtin_fmaf(a[at], w[at], acc);
            }
    return acc;
}

/* The action from the network's output o: out[0] = tanh(o), out[1] = throttle_delta, out[2] = steering_delta */
OK_HDI void ok_cnn_action(const float o, const float throttle, const float steer_scale, float *out)
{
    const float y = ok_tanhf(o);
    out[0] = y;
    out[1] = throttle;
    out[2] = y * steer_scale;
}

/* Floats of work space ok_cnn_forward needs: the input and the three layers' outputs, planar, and the hidden layer */
OK_HDI int ok_cnn_work_floats(const ok_cnn_shape s)
{
    int n = 3 * s.S * s.S + s.H;
    for (int l = 0; l < 3; ++l) n += s.c[l] * ok_cnn_side(s, l) * ok_cnn_side(s, l);
    return n;
}

/* The whole network of one frame on the host: frame [S][S][4] uint8 -> *out, the output layer's o (in front of the tanh) */
OK_HD void ok_cnn_forward(const ok_cnn_shape s, const float *params, const uint8_t *frame, float *work, float *out)
{
    const ok_cnn_layout at = ok_cnn_offsets(s);
    float              *in = work;
    for (int ch = 0; ch < 3; ++ch)
        for (int p = 0; p < s.S * s.S; ++p) in[ch * s.S * s.S + p] = ok_bev_pixel(frame[4 * p + ch]);
    int side_in = s.S;
    for (int l = 0; l < 3; ++l) {
        const int Cin = ok_cnn_cin(s, l), side = ok_cnn_side(s, l), k = s.k[l];
        float    *o = in + Cin * side_in * side_in;
        for (int n = 0; n < s.c[l]; ++n)
            for (int oy = 0; oy < side; ++oy)
                for (int ox = 0; ox < side; ++ox)
                    o[(n * side + oy) * side + ox] = ok_lidar_relu(
                        ok_cnn_conv_at(in, Cin, side_in, params + at.w[l] + n * Cin * k * k, k, s.s[l], params[at.b[l] + n], oy, ox));
        in      = o;
        side_in = side;
    }
    const int F = s.c[2] * side_in * side_in;
    float    *h = in + F;
    for (int j = 0; j < s.H; ++j) h[j] = ok_lidar_relu(ok_cnn_hidden_at(in, s.c[2], side_in, params + at.hw + j * F, params[at.hb + j]));
    *out = ok_lidar_dot(h, params + at.ow, s.H, params[at.ob]);
}

#endif /* OKENV_CNN_H */
