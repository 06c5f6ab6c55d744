// ok_cnn.h -- the behavioural-cloning image policy on the device: BehavioralCloning's PolicyCNN (env_train_bc.py)
// driven as main.cpp drives it, from the camera's RGBA8 frames to the action fields, for every agent of a handle.  The rule lives in
// include/okenv_cnn.h (ok_bev_pixel, ok_cnn_conv_at, ok_cnn_hidden_at, ok_cnn_action on top of ok_lidar_dot) and is shared with
// okCnnActHost below, so the device and the host entry agree bit for bit.
//
// These are NOT step kernels and add no step-kernel launch site.  The lane mapping, the packed-weight layout, the unit loop of a
// convolution, the walk of layers 1 and 2 and the hidden layer's GEMM are ok_conv.h's; what is this family's own:
//   okCnnPackKernel     at set_params: the four weight matrices in groups of 16 k's (layer 0: 4 k's a tap, R, G, B and an alpha slot)
//   OkCnnRgbaTaps       layer 0's A operands: a frame's bytes through the table of ok_bev_pixel
//   okCnnConvKernel     one frame per workgroup of 8 waves.  The frame's bytes, layer 0's output and layer 1's output live in LDS
//                       (channels last; the frame's room is layer 1's once layer 0 is done); layer 2 writes the [N][F] features,
//                       channels last, to global memory.  No layer is tiled: a valid convolution of a whole frame has no halo.
//   okCnnHeadKernel<CT> 16 agents per workgroup of 8 waves: the hidden layer (okConvFc1, a wave owning CT tiles of 16 columns); then the
//                       output layer, the tanh and the action, one agent per thread.
#ifndef OK_CNN_H
#define OK_CNN_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_cnn.h"
#include "ok_conv.h"
#include "ok_lidar.h"

__host__ __device__ inline ok_cnn_shape okCnnShape(const okenv_cnn_config &c)
{
    ok_cnn_shape s;
    s.S = c.image_size;
    for (int l = 0; l < 3; ++l)
    {
        s.k[l] = c.kernel[l];
        s.s[l] = c.stride[l];
        s.c[l] = c.channels[l];
    }
    s.H = c.hidden;
    return s;
}

// Groups of 16 k's in a chain: layer 0 has 4 k's a tap (R, G, B and the alpha slot) and filler taps up to a whole group; l = 3 is the
// hidden layer
__host__ __device__ inline int okCnnGroups(const ok_cnn_shape s, const int l)
{
    if (l == 0)
        return (s.k[0] * s.k[0] + 3) / 4;
    return l == 3 ? ok_cnn_features(s) / 16 : s.k[l] * s.k[l] * s.c[l - 1] / 16;
}

// The conv kernel's LDS, in floats: [lut | p | q].  lut: ok_bev_pixel of the 256 bytes.  p: the frame, S x S words of four bytes, and
// behind layer 0 layer 1's output, side_1^2 pixels of c1 + 1 floats.  q: layer 0's output, side_0^2 pixels of c0 + 1 floats (odd: the
// 16 pixels of an MFMA tile start on different banks).  The head's LDS and the pack's places are OkConvHeadPlaces'.
struct OkCnnPlaces : OkConvHeadPlaces
{
    int side[3], ld0, ld1, p, q, conv_end;
    int region; // what sizes p: 0 the frame, 1 layer 1's output
};

__host__ __device__ inline OkCnnPlaces okCnnPlaces(const ok_cnn_shape s)
{
    OkCnnPlaces at;
    for (int l = 0; l < 3; ++l)
        at.side[l] = ok_cnn_side(s, l);
    at.ld0 = s.c[0] + 1;
    at.ld1 = s.c[1] + 1;
    const int frame = s.S * s.S, out1 = at.side[1] * at.side[1] * at.ld1;
    at.region   = out1 > frame ? 1 : 0;
    at.p        = 256;
    at.q        = at.p + okLidarMax(frame, out1);
    at.conv_end = at.q + at.side[0] * at.side[0] * at.ld0;
    const int groups[4] = {okCnnGroups(s, 0), okCnnGroups(s, 1), okCnnGroups(s, 2), okCnnGroups(s, 3)}, cout[4] = {s.c[0], s.c[1], s.c[2], s.H};
    okConvHeadPlaces(at, s.H, groups, cout);
    return at;
}

inline size_t okCnnLdsBytes(const ok_cnn_shape s)
{
    if (ok_cnn_shape_bad(s))
        return 0U;
    const OkCnnPlaces at = okCnnPlaces(s);
    return sizeof(float) * static_cast<size_t>(okLidarMax(at.conv_end, at.head_end));
}

// ---- the weights as the kernels read them ----------------------------------------------------------------------------------------------

// okConvPack's layout; layer 0's k = tap * 4 + ch (tap = ty * k + tx), its alpha slot and filler taps 0.0f
struct OkCnnPackParams
{
    ok_cnn_shape s;
    const float *params;
    float       *pack;
};

__global__ __launch_bounds__(256) void okCnnPackKernel(const OkCnnPackParams p)
{
    const ok_cnn_layout at = ok_cnn_offsets(p.s);
    okConvPack(p.s, at, okCnnPlaces(p.s), p.params, p.pack, [&](const int n, const int kk) {
        const int taps = p.s.k[0] * p.s.k[0], tap = kk >> 2, ch = kk & 3;
        return tap < taps && ch < 3 ? p.params[at.w[0] + (n * 3 + ch) * taps + tap] : 0.F;
    });
}

// ---- the convolutions ------------------------------------------------------------------------------------------------------------------

// Layer 0's A operands for okConv: a pixel is one word of four bytes, a k-step is one tap, lane group g reads byte g of the pixel (3: the
// alpha byte against the alpha slot's 0.0f) through the table of ok_bev_pixel at the start of LDS; the filler taps read the last tap.
struct OkCnnRgbaTaps
{
    const int g;
    int       ty = 0, tx = 0;

    __device__ __forceinline__ OkCnnRgbaTaps(const OkConvJob &, const int g_) : g(g_) {}

    __device__ __forceinline__ static int groups(const OkConvJob &j)
    {
        return (j.k * j.k + 3) >> 2;
    }

    __device__ __forceinline__ static int lane(const OkConvJob &, const int)
    {
        return 0;
    }

    template <int RB>
    __device__ __forceinline__ void load(const OkConvJob &j, const int (&abase)[RB], float (&a)[4][RB], const bool first = false)
    {
        const uint32_t *words = reinterpret_cast<const uint32_t *>(ok_actor_lds);
        if (first)
            ty = 0, tx = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
            const int toff = ty * j.rs + tx * j.ps;
#pragma unroll
            for (int m = 0; m < RB; ++m)
                a[q][m] = ok_actor_lds[(words[abase[m] + toff] >> (8 * g)) & 255U];
            if (ty != j.k - 1 || tx != j.k - 1) // (the filler taps stay on the last tap)
                if (++tx == j.k)
                    tx = 0, ++ty;
        }
    }
};

struct OkCnnActParams
{
    OkDeviceState    st;
    int              N;
    ok_cnn_shape     s;
    const uint8_t   *frames; // [N][S][S][4]
    const float     *params, *pack;
    float           *feat; // layer 2's output, [N][side_2][side_2][c2]: the features in the hidden layer's chain order
    float            throttle, steer_scale;
    okenv_cnn_record rec;
};

__global__ __launch_bounds__(kConvThreads) void okCnnConvKernel(const OkCnnActParams p)
{
    const ok_cnn_shape  sh = p.s;
    const ok_cnn_layout at = ok_cnn_offsets(sh);
    const OkCnnPlaces   pl = okCnnPlaces(sh);
    const int           S = sh.S, tid = static_cast<int>(threadIdx.x);
    const size_t        n = blockIdx.x;

    if (tid < 256)
        ok_actor_lds[tid] = ok_bev_pixel(static_cast<uint8_t>(tid));
    const uint32_t *frame = reinterpret_cast<const uint32_t *>(p.frames) + n * static_cast<size_t>(S * S);
    uint32_t       *words = reinterpret_cast<uint32_t *>(ok_actor_lds) + pl.p;
    for (int e = tid; e < S * S; e += kConvThreads)
        words[e] = frame[e];
    __syncthreads();

    OkConvJob      j;
    OkConvBordered to;
    j.in = pl.p, j.ps = 1, j.rs = S, j.k = sh.k[0], j.stride = sh.s[0], j.Cin = 4, j.W = pl.side[0], j.M = pl.side[0] * pl.side[0], j.Cout = sh.c[0];
    j.w = p.pack + pl.pack[0], j.bias = p.params + at.b[0];
    to.out = ok_actor_lds + pl.q, to.ldo = pl.ld0, to.opad = 0, to.orow = j.W; // (no layer pads: no border anywhere)
    okConv<OkCnnRgbaTaps, kConvRowBlock, kConvWaves, false>(j, to);
    __syncthreads();

    j.in = pl.q, j.ps = pl.ld0, j.rs = pl.side[0] * pl.ld0, j.k = sh.k[1], j.stride = sh.s[1], j.Cin = sh.c[0], j.W = pl.side[1];
    j.M = pl.side[1] * pl.side[1], j.Cout = sh.c[1];
    j.w = p.pack + pl.pack[1], j.bias = p.params + at.b[1];
    to.out = ok_actor_lds + pl.p, to.ldo = pl.ld1, to.orow = j.W;
    okConv<OkConvWalk, kConvRowBlock, kConvWaves, false>(j, to);
    __syncthreads();

    j.in = pl.p, j.ps = pl.ld1, j.rs = pl.side[1] * pl.ld1, j.k = sh.k[2], j.stride = sh.s[2], j.Cin = sh.c[1], j.W = pl.side[2];
    j.M = pl.side[2] * pl.side[2], j.Cout = sh.c[2];
    j.w = p.pack + pl.pack[2], j.bias = p.params + at.b[2];
    to.out = p.feat + n * static_cast<size_t>(j.M * sh.c[2]), to.ldo = sh.c[2], to.orow = j.W;
    okConv<OkConvWalk, kConvRowBlock, kConvWaves, false>(j, to);
}

template <int CT>
__global__ __launch_bounds__(kConvThreads) void okCnnHeadKernel(const OkCnnActParams p)
{
    const ok_cnn_shape  sh = p.s;
    const ok_cnn_layout at = ok_cnn_offsets(sh);
    const OkCnnPlaces   pl = okCnnPlaces(sh);
    const int           H = sh.H, tid = static_cast<int>(threadIdx.x);
    const long          a0 = static_cast<long>(blockIdx.x) * kConvAgents;
    const float        *hid = okConvFc1<CT, 1>(p.feat, p.N, ok_cnn_features(sh), H, a0, p.pack + pl.pack[3], p.params + at.hb, pl.ldt, pl.ldh);

    const long a = a0 + tid;
    if (tid >= kConvAgents || a >= p.N)
        return;
    float out[3];
    ok_cnn_action(ok_lidar_dot(hid + tid * pl.ldh, p.params + at.ow, H, p.params[at.ob]), p.throttle, p.steer_scale, out);
    p.st.thr[a]   = out[1];
    p.st.steer[a] = out[2];
    if (p.rec.out != nullptr)
        p.rec.out[a] = out[0];
    if (p.rec.action != nullptr)
    {
        p.rec.action[2 * a]     = out[1];
        p.rec.action[2 * a + 1] = out[2];
    }
    okActAlive(p.st.crashed, p.rec.alive, a);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline const char *okCnnCheckConfig(const okenv_cnn_config *c)
{
    if (c == nullptr)
        return "config is NULL";
    if (ok_cnn_shape_bad(okCnnShape(*c)))
        return "shape outside the limits (image_size 16 .. 128; kernel 1 .. 8; stride 1 .. 4 and at most the kernel; every layer's side "
               "at least 1; channels multiples of 16 in 16 .. 128; at most 8192 features; hidden a multiple of 16 in 16 .. 512)";
    if (okCnnLdsBytes(okCnnShape(*c)) > kConvLdsBudget)
        return "the conv kernel's LDS (okenv_cnn_lds_bytes) does not fit 160 KB";
    if (!std::isfinite(c->throttle) || !std::isfinite(c->steer_scale))
        return "throttle / steer_scale must be finite";
    return nullptr;
}

// The action of n agents on host arrays; every output may be nullptr
inline void okCnnActHost(const okenv_cnn_config &c, const float *params, const int n, const uint8_t *frames, const uint8_t *crashed,
                         float *throttle, float *steer, float *out, uint8_t *alive)
{
    const ok_cnn_shape s = okCnnShape(c);
    std::vector<float> work(static_cast<size_t>(ok_cnn_work_floats(s)));
    const size_t       frame = static_cast<size_t>(s.S) * s.S * 4U;
    for (int a = 0; a < n; ++a)
    {
        float o = 0.F, act[3];
        ok_cnn_forward(s, params, frames + static_cast<size_t>(a) * frame, work.data(), &o);
        ok_cnn_action(o, c.throttle, c.steer_scale, act);
        if (out != nullptr)
            out[a] = act[0];
        if (throttle != nullptr)
            throttle[a] = act[1];
        if (steer != nullptr)
            steer[a] = act[2];
        if (alive != nullptr)
            alive[a] = (crashed != nullptr && crashed[a]) ? 0 : 1;
    }
}

#endif // OK_CNN_H
