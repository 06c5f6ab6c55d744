/*
 * okenv_bev.h -- the rule of the flow driver's image encoder (FlowMatching/flow_matching_model.py: BEVEncoder): the camera's RGBA8 frame
 * of an agent -> the condition vector okenv_flow_act takes.  Shared bit for bit by the HIP kernels (openkitchen_amd/csrc/ok_bev.h) and
 * the host entry okenv_bev_encode_host.
 *
 * THE RULE
 *
 * Shape.  Square frames of side S (a multiple of 8 in 16 .. 128), three convolutions l = 0, 1, 2 of kernel k_l (3 or 5), stride 2 and
 * padding k_l / 2 -- the sides halve to S/2, S/4, S/8 -- with c_l output channels (multiples of 16 in 16 .. 128), 3 input channels, and
 * the embedding width E (a multiple of 16 in 16 .. 512).  The reference: S = 128, k = (5, 3, 3), c = (32, 64, 128), E = 128.
 *
 * Parameter vector (ok_bev_offsets): torch's parameters() order of the reference module, every tensor in torch's layout:
 *     conv.0.weight [c0][3][k0][k0],  conv.0.bias [c0]
 *     conv.2.weight [c1][c0][k1][k1], conv.2.bias [c1]
 *     conv.4.weight [c2][c1][k2][k2], conv.4.bias [c2]
 *     proj.weight   [E][c2],          proj.bias   [E]
 * Every weight must be finite (see the zero terms below).
 *
 * Forward of one frame [S][S][4] uint8 (R, G, B, A; row 0 first), fp32 throughout, nothing fused but the fmaf's written here.
 *     pixel     (float)byte / 255.0f, the IEEE division (ok_bev_pixel).  Alpha is not an input.
 *     conv      one output (channel n at (oy, ox)) is ok_lidar_relu of ONE fused chain started from the bias (ok_bev_conv_at):
 *                   acc = bias[n];  for ty = 0 .. k-1, for tx = 0 .. k-1, for ch = 0 .. Cin-1:
 *                       acc = fmaf(in[ch](2 oy + ty - k/2, 2 ox + tx - k/2), w[n][ch][ty][tx], acc)
 *               -- tap row, tap column, input channel, the channel innermost.  Taps outside the input are left out.
 *               ZERO TERMS.  The device's chain contains, at their place in this order, terms the host leaves out: the padding taps
 *               (input 0.0f), layer 0's fourth channel behind every tap (the frame's alpha slot, weight 0.0f) and filler taps behind
 *               the last one that round layer 0's chain up to a multiple of 16 terms (weight 0.0f, a finite input).  With finite
 *               weights and inputs each is fmaf(x, w, acc) with x w = +-0 and leaves acc's value unchanged; only the sign of a zero
 *               accumulator can differ, and the ReLU behind every convolution removes it.
 *     pool      per channel: sum = 0.0f; for p = 0 .. P - 1 ascending (p = y (S/8) + x): sum = sum + a[p];  mean = sum / (float)P,
 *               P = (S/8)^2  (ok_bev_pool).  One sequential chain: no atomics, nothing that depends on scheduling.
 *     proj      out[e] = ok_lidar_dot(mean, proj.weight[e], c2, proj.bias[e])
 *
 * Against torch the chain's order and the pool's differ: rounding only.  A resize of the frame is not part of the rule: the frames
 * are rendered at the encoder's own size.
 *
 * Only fmaf, +, /, comparisons are used; compile with -ffp-contract=off.  Plain C99 / C++ / HIP.
 */
#ifndef OKENV_BEV_H
#define OKENV_BEV_H

#include "okenv_lidar.h"

#define OK_BEV_MIN_SIDE 16
#define OK_BEV_MAX_SIDE 128
#define OK_BEV_MAX_CHANNELS 128
#define OK_BEV_MAX_EMBED 512

typedef struct ok_bev_shape {
    int S, k[3], c[3], E;
} ok_bev_shape;

/* 0 when the shape is inside the rule's limits */
OK_HDI int ok_bev_shape_bad(const ok_bev_shape s)
{
    if (s.S < OK_BEV_MIN_SIDE || s.S > OK_BEV_MAX_SIDE || s.S % 8 != 0) return 1;
    for (int l = 0; l < 3; ++l) {
        if (s.k[l] != 3 && s.k[l] != 5) return 1;
        if (s.c[l] < 16 || s.c[l] > OK_BEV_MAX_CHANNELS || s.c[l] % 16 != 0) return 1;
    }
    if (s.E < 16 || s.E > OK_BEV_MAX_EMBED || s.E % 16 != 0) return 1;
    return 0;
}

/* Input channels and output side of layer l */
OK_HDI int ok_bev_cin(const ok_bev_shape s, const int l)
{
    return l == 0 ? 3 : s.c[l - 1];
}

OK_HDI int ok_bev_side(const ok_bev_shape s, const int l)
{
    return s.S >> (l + 1);
}

/* Where the pieces of the parameter vector begin, in floats */
typedef struct ok_bev_layout {
    int w[3], b[3], pw, pb, total;
} ok_bev_layout;

OK_HDI ok_bev_layout ok_bev_offsets(const ok_bev_shape s)
{
    ok_bev_layout at;
    int           o = 0;
    for (int l = 0; l < 3; ++l) {
        at.w[l] = o;
        o += s.c[l] * ok_bev_cin(s, l) * s.k[l] * s.k[l];
        at.b[l] = o;
        o += s.c[l];
    }
    at.pw    = o;
    at.pb    = at.pw + s.E * s.c[2];
    at.total = at.pb + s.E;
    return at;
}

OK_HDI float ok_bev_pixel(const uint8_t byte)
{
    return (float)byte / 255.0f;
}

/* One output of a convolution before its ReLU: in [Cin][side_in][side_in] (planar), w = weight[n] [Cin][k][k] */
OK_HD float ok_bev_conv_at(const float *in, const int Cin, const int side_in, const float *w, const int k, const float bias, const int oy,
                           const int ox)
{
    float acc = bias;
    for (int ty = 0; ty < k; ++ty) {
        const int y = 2 * oy + ty - k / 2;
        if (y < 0 || y >= side_in) continue;
        for (int tx = 0; tx < k; ++tx) {
            const int x = 2 * ox + tx - k / 2;
            if (x < 0 || x >= side_in) continue;
            for (int ch = 0; ch < Cin; ++ch) acc = __builtin_fmaf(in[(ch * side_in + y) * side_in + x], w[(ch * k + ty) * k + tx], acc);
        }
    }
    return acc;
}

/* The mean of one channel's P values, a [P] */
OK_HDI float ok_bev_pool(const float *a, const int P)
{
    float sum = 0.0f;
    for (int p = 0; p < P; ++p) sum = sum + a[p];
    return sum / (float)P;
}

/* Floats of work space ok_bev_forward needs: the input and the three layers' outputs, planar, and the pooled vector */
OK_HDI int ok_bev_work_floats(const ok_bev_shape s)
{
    int n = 3 * s.S * s.S + s.c[2];
    for (int l = 0; l < 3; ++l) n += s.c[l] * ok_bev_side(s, l) * ok_bev_side(s, l);
    return n;
}

/* The whole encoder of one frame on the host: frame [S][S][4] uint8 -> out [E] */
OK_HD void ok_bev_forward(const ok_bev_shape s, const float *params, const uint8_t *frame, float *work, float *out)
{
    const ok_bev_layout at = ok_bev_offsets(s);
    float              *in = work;
    for (int ch = 0; ch < 3; ++ch)
        for (int p = 0; p < s.S * s.S; ++p) in[ch * s.S * s.S + p] = ok_bev_pixel(frame[4 * p + ch]);
    int side_in = s.S;
    for (int l = 0; l < 3; ++l) {
        const int Cin = ok_bev_cin(s, l), side = ok_bev_side(s, l), k = s.k[l];
        float    *o = in + Cin * side_in * side_in;
        for (int n = 0; n < s.c[l]; ++n)
            for (int oy = 0; oy < side; ++oy)
                for (int ox = 0; ox < side; ++ox)
                    o[(n * side + oy) * side + ox] =
                        ok_lidar_relu(ok_bev_conv_at(in, Cin, side_in, params + at.w[l] + n * Cin * k * k, k, params[at.b[l] + n], oy, ox));
        in      = o;
        side_in = side;
    }
    const int P = side_in * side_in;
    float    *mean = in + s.c[2] * P;
    for (int n = 0; n < s.c[2]; ++n) mean[n] = ok_bev_pool(in + n * P, P);
    for (int e = 0; e < s.E; ++e) out[e] = ok_lidar_dot(mean, params + at.pw + e * s.c[2], s.c[2], params[at.pb + e]);
}

#endif /* OKENV_BEV_H */
