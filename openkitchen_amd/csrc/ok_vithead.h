// ok_vithead.h -- the training of the image transformer driver's policy head on the device.  The rule lives in
// include/okenv_vithead.h and is shared with okVitHeadUpdateHost below, so the device and the host entries agree bit for bit.
//
// Two launches per minibatch, and whatever crosses workgroups crosses the launch boundary between them:
//   okVitHeadForwardKernel   16 positions a workgroup: the embedding rows into LDS, the head's forward (okLidarLinear), the seeds do, d2
//                            and d1 = d2 . W2; the rows [e | h1 | h2 | d1 | d2 | (do, t)] of every position go to a scratch in global
//                            memory, filler positions up to a whole chunk as +0.0f
//   okVitHeadGradKernel      a wave owns a 16 x 16 tile of one layer's gradient [W | b]: per chunk of 64 positions 16 steps of
//                            v_mfma_f32_16x16x4_f32 with k = the positions (the rule's chain from +0.0f; the bias is the column whose
//                            activation is 1.0f), the chunks joined in the rule's order in registers, the division by B_k, Adam in place.
//                            The loss is the row of t's against the 1.0f column of the last layer.  No LDS, no barrier.
// The eval is the forward kernel and the one wave of the gradient kernel that holds the loss.
#ifndef OK_VITHEAD_H
#define OK_VITHEAD_H

#include <cmath>
#include <vector>

#include "../../include/okenv.h"
#include "../../include/okenv_vithead.h"
#include "ok_learn.h"
#include "ok_vit.h"

constexpr int kVitHeadRows = 16; // positions of a workgroup of the forward kernel: the rows of one MFMA tile

// The forward kernel's LDS, in floats: [e 16 x (D + 4) | h1 16 x (H1 + 4) | h2 16 x (H2 + 4) | d2 16 x (H2 + 4) | do 16]
struct OkVitHeadPlaces
{
    int ldx, ld1, ld2, h1_at, h2_at, d2_at, o_at, end;
};

__host__ __device__ inline OkVitHeadPlaces okVitHeadPlaces(const int D, const int H1, const int H2)
{
    OkVitHeadPlaces at;
    at.ldx   = D + kLidarPad;
    at.ld1   = H1 + kLidarPad;
    at.ld2   = H2 + kLidarPad;
    at.h1_at = kVitHeadRows * at.ldx;
    at.h2_at = at.h1_at + kVitHeadRows * at.ld1;
    at.d2_at = at.h2_at + kVitHeadRows * at.ld2;
    at.o_at  = at.d2_at + kVitHeadRows * at.ld2;
    at.end   = at.o_at + kVitHeadRows;
    return at;
}

inline size_t okVitHeadLdsBytes(const int D, const int H1, const int H2)
{
    return ok_vithead_shape_bad(D, H1, H2) ? 0U : sizeof(float) * static_cast<size_t>(okVitHeadPlaces(D, H1, H2).end);
}

// The scratch of a minibatch of Qp positions (a multiple of 64), in floats: the rows of every position
struct OkVitHeadScratch
{
    float *e, *h1, *h2, *d1, *d2, *d3; // [Qp][D], [Qp][H1], [Qp][H2], [Qp][H1], [Qp][H2], [Qp][2]: (do, t)
};

inline size_t okVitHeadScratchFloats(const int D, const int H1, const int H2, const size_t Qp)
{
    return Qp * static_cast<size_t>(D + 2 * H1 + 2 * H2 + 2);
}

inline OkVitHeadScratch okVitHeadScratchAt(float *base, const int D, const int H1, const int H2, const size_t Qp)
{
    OkVitHeadScratch s;
    s.e  = base;
    s.h1 = s.e + Qp * D;
    s.h2 = s.h1 + Qp * H1;
    s.d1 = s.h2 + Qp * H2;
    s.d2 = s.d1 + Qp * H1;
    s.d3 = s.d2 + Qp * H2;
    return s;
}

struct OkVitHeadForwardParams
{
    int              D, H1, H2, M, Bk;
    long             base;  // the minibatch's first position in the epoch
    const float     *head;  // the head's parameters (ok_vithead_offsets)
    const float     *embedding, *steer;
    const int32_t   *order; // the epoch's row, or nullptr
    float            steer_scale, weight, threshold;
    OkVitHeadScratch out;
};

// Grid: Qp / 16 workgroups, Qp = Bk rounded up to whole chunks.  Positions from Bk on are filler: every row of theirs is +0.0f.
__global__ __launch_bounds__(kLidarThreads) void okVitHeadForwardKernel(const OkVitHeadForwardParams p)
{
    const int               D = p.D, H1 = p.H1, H2 = p.H2, tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const ok_vithead_layout at = ok_vithead_offsets(D, H1, H2);
    const OkVitHeadPlaces   pl = okVitHeadPlaces(D, H1, H2);
    float                  *X = ok_actor_lds, *A1 = X + pl.h1_at, *A2 = X + pl.h2_at, *D2 = X + pl.d2_at, *Do = X + pl.o_at;
    const long              q0 = static_cast<long>(blockIdx.x) * kVitHeadRows;
    const auto sample_of = [&p](const long q) {
        const long at_q = p.base + q;
        return ok_learn_clamp_index(p.order != nullptr ? static_cast<long long>(p.order[at_q]) : static_cast<long long>(at_q), p.M);
    };
    for (int r = 0; r < kVitHeadRows; ++r)
    {
        const long   q = q0 + r;
        const bool   live = q < p.Bk;
        const float *row = p.embedding + (live ? static_cast<long>(sample_of(q)) : 0L) * D;
        for (int c = tid; c < D; c += kLidarThreads)
        {
            const float v = live ? row[c] : 0.F;
            X[r * pl.ldx + c]  = v;
            p.out.e[q * D + c] = v;
        }
    }
    __syncthreads();
    okLidarLinear(0, pl.ldx, D, 0, 1, D, p.head + at.w1, D, p.head + at.b1, H1, true, false, pl.h1_at, pl.ld1, 0);
    __syncthreads();
    okLidarLinear(pl.h1_at, pl.ld1, H1, 0, 1, H1, p.head + at.w2, H1, p.head + at.b2, H2, true, false, pl.h2_at, pl.ld2, 0);
    __syncthreads();
    if (tid < kVitHeadRows)
    {
        const long q = q0 + tid;
        float      t = 0.F, d_o = 0.F;
        if (q < p.Bk)
        {
            const float o = ok_lidar_dot(A2 + tid * pl.ld2, p.head + at.w3, H2, p.head[at.b3]);
            const float y = ok_vithead_label(p.steer[sample_of(q)], p.steer_scale);
            ok_vithead_seed(o, y, ok_vithead_weight(y, p.threshold, p.weight), &t, &d_o);
        }
        Do[tid]             = d_o;
        p.out.d3[2 * q]     = d_o;
        p.out.d3[2 * q + 1] = t;
    }
    __syncthreads();
    for (int r = 0; r < kVitHeadRows; ++r)
    {
        const long q = q0 + r;
        const bool live = q < p.Bk;
        for (int k = tid; k < H2; k += kLidarThreads)
        {
            const float h = A2[r * pl.ld2 + k];
            const float v = live ? ok_vithead_d2(h, p.head[at.w3 + k], Do[r]) : 0.F;
            D2[r * pl.ld2 + k]   = v;
            p.out.d2[q * H2 + k] = v;
            p.out.h2[q * H2 + k] = live ? h : 0.F;
        }
        for (int j = tid; j < H1; j += kLidarThreads)
            p.out.h1[q * H1 + j] = live ? A1[r * pl.ld1 + j] : 0.F;
    }
    __syncthreads();
    // d1 = d2 . W2 behind ReLU's mask: a wave takes a 16-column tile of hidden layer 1; B[k][col] = W2[k][col], the chain from +0.0f
    const float *w2 = p.head + at.w2;
    for (int nt = wave; nt < H1 / 16; nt += kLidarWaves)
    {
        const int  n0 = nt * 16;
        okLidarAcc acc = {0.F, 0.F, 0.F, 0.F};
        for (int k0 = 0; k0 < H2; k0 += 16)
        {
            float b[4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                b[s] = w2[static_cast<long>(k0 + 4 * s + g) * H1 + n0 + i];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(D2[i * pl.ld2 + k0 + 4 * s + g], b[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const int  row = 4 * g + r;
            const long q = q0 + row;
            p.out.d1[q * H1 + n0 + i] = (q < p.Bk && A1[row * pl.ld1 + n0 + i] > 0.F) ? acc[r] : 0.F;
        }
    }
}

struct OkVitHeadGradParams
{
    int                  D, H1, H2, Bk, chunks;
    int                  first_unit; // 0; the eval: the unit that holds the loss (okVitHeadUnits - 1)
    OkVitHeadScratch     in;
    float               *head, *m, *v;
    ok_learn_adam_consts adam;
    float               *grad, *loss; // the minibatch's gradient [ok_vithead_offsets.total] and its loss, each may be nullptr
};

// Tiles of the three layers' gradients [W | b]: rows H1, H2 and 1 (the last layer's tile also carries the row of t's), columns
// D + 1, H1 + 1, H2 + 1
__host__ __device__ inline int okVitHeadUnits(const int D, const int H1, const int H2)
{
    return (H1 / 16) * (D / 16 + 1) + (H2 / 16) * (H1 / 16 + 1) + (H2 / 16 + 1);
}

// One wave per unit; kUpdate == false stores the loss only.  Lane l holds A[row l & 15][k = l >> 4] = delta of position k, and
// B[k = l >> 4][col l & 15] = the activation of position k (ok_lidar.h); accumulator register r is row 4 (l >> 4) + r, col l & 15.
template <bool kUpdate>
__global__ __launch_bounds__(kLidarThreads) void okVitHeadGradKernel(const OkVitHeadGradParams p)
{
    const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int D = p.D, H1 = p.H1, H2 = p.H2;
    const ok_vithead_layout at = ok_vithead_offsets(D, H1, H2);
    const int n0 = (H1 / 16) * (D / 16 + 1), n1 = (H2 / 16) * (H1 / 16 + 1), n2 = H2 / 16 + 1;
    int       u = p.first_unit + static_cast<int>(blockIdx.x) * kLidarWaves + wave;
    if (u >= n0 + n1 + n2)
        return;
    // the unit's layer: delta [Qp][ldd] with `rows` rows to read and `stored` to keep, the activation [Qp][width]
    const float *delta, *act;
    int          ldd, rows, stored, width, w_at, b_at, layer;
    if (u < n0)
        layer = 0, delta = p.in.d1, ldd = H1, rows = H1, stored = H1, act = p.in.e, width = D, w_at = at.w1, b_at = at.b1;
    else if (u < n0 + n1)
        layer = 1, u -= n0, delta = p.in.d2, ldd = H2, rows = H2, stored = H2, act = p.in.h1, width = H1, w_at = at.w2, b_at = at.b2;
    else
        layer = 2, u -= n0 + n1, delta = p.in.d3, ldd = 2, rows = 2, stored = 1, act = p.in.h2, width = H2, w_at = at.w3, b_at = at.b3;
    const int  cts = width / 16 + 1, rt = u / cts, ct = u - rt * cts;
    const int  row_a = 16 * rt + i, col_b = 16 * ct + i;
    const bool a_live = row_a < rows, b_live = col_b < width;
    const float b_fill = col_b == width ? 1.F : 0.F; // (the bias's column; the columns behind it are never stored)
    const float *ap = delta + (a_live ? row_a : 0), *bp = act + (b_live ? col_b : 0);
    okLidarAcc   joined = {0.F, 0.F, 0.F, 0.F};
    for (int c = 0; c < p.chunks; ++c)
    {
        const long q0 = static_cast<long>(c) * OK_VITHEAD_CHUNK + g;
        float      a[OK_VITHEAD_CHUNK / 4], b[OK_VITHEAD_CHUNK / 4];
#pragma unroll
        for (int s = 0; s < OK_VITHEAD_CHUNK / 4; ++s)
        {
            const long q = q0 + 4 * s;
            a[s] = a_live ? ap[q * ldd] : 0.F;
            b[s] = b_live ? bp[q * width] : b_fill;
        }
        okLidarAcc acc = {0.F, 0.F, 0.F, 0.F};
#pragma unroll
        for (int s = 0; s < OK_VITHEAD_CHUNK / 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
        if (c == 0)
            joined = acc;
        else
        {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                joined[r] = joined[r] + acc[r];
        }
    }
    const float count = static_cast<float>(p.Bk);
#pragma unroll
    for (int r = 0; r < 4; ++r)
    {
        const int   row = 16 * rt + 4 * g + r;
        const float mean = joined[r] / count;
        if (layer == 2 && row == 1 && col_b == width)
        {
            if (p.loss != nullptr)
                *p.loss = mean;
            continue;
        }
        if (!kUpdate || row >= stored || col_b > width)
            continue;
        const int at_p = b_live ? w_at + row * width + col_b : b_at + row;
        ok_learn_adam(p.head + at_p, p.m + at_p, p.v + at_p, mean, p.adam);
        if (p.grad != nullptr)
            p.grad[at_p] = mean;
    }
}

// okenv_vit_embed's last kernel: the final LayerNorm of the class token of every sequence of a pass, 8 lanes a row (okVitFinalKernel's
// expressions), x [count][T][D] -> out [count][D]
__global__ __launch_bounds__(kVitThreads) void okVitEmbedKernel(const int count, const int D, const long seq_stride, const float *__restrict__ x,
                                                               const float *__restrict__ gam, const float *__restrict__ bet, const float eps,
                                                               float *__restrict__ out)
{
    const int    lane = static_cast<int>(threadIdx.x) & (OK_ACTOR_LANES - 1);
    const long   r_raw = static_cast<long>(blockIdx.x) * kVitNormRows + static_cast<int>(threadIdx.x) / OK_ACTOR_LANES;
    const bool   live = r_raw < count; // (a group past the last row takes part in the shuffles and stores nothing)
    const float *row = x + (live ? r_raw : 0) * seq_stride;
    float        part[OK_ACTOR_LANES];
    const float  mine = live ? ok_lidar_sum_part(row, D, lane) : 0.F;
#pragma unroll
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        part[l] = __shfl(mine, l, OK_ACTOR_LANES);
    const float mean = ok_gauss_tree(part) / static_cast<float>(D);
    const float sq   = live ? ok_lidar_sq_part(row, D, lane, mean) : 0.F;
#pragma unroll
    for (int l = 0; l < OK_ACTOR_LANES; ++l)
        part[l] = __shfl(sq, l, OK_ACTOR_LANES);
    const float den = ok_vit_den(ok_gauss_tree(part) / static_cast<float>(D), eps);
    if (live)
        for (int c = lane; c < D; c += OK_ACTOR_LANES)
            out[r_raw * D + c] = ok_lidar_norm(row[c], mean, den, gam[c], bet[c]);
}

// ---- host side (no GPU) ----------------------------------------------------------------------------------------------------------

inline okenv_learner_params okVitHeadAdam(const okenv_vit_head_params &hp)
{
    okenv_learner_params lp{};
    lp.lr    = hp.lr;
    lp.clip  = 0.F;
    lp.beta1 = hp.beta1;
    lp.beta2 = hp.beta2;
    lp.eps   = hp.eps;
    return lp;
}

inline const char *okVitHeadCheckParams(const okenv_vit_head_params *hp)
{
    if (hp == nullptr)
        return "params is NULL";
    const okenv_learner_params lp = okVitHeadAdam(*hp);
    if (const char *why = okLearnCheckParams(&lp))
        return why;
    if (!std::isfinite(hp->weight) || !(hp->weight > 0.F))
        return "weight must be positive and finite";
    if (!std::isfinite(hp->threshold) || !(hp->threshold >= 0.F))
        return "threshold must be finite and not negative";
    return nullptr;
}

inline const char *okVitHeadCheckShape(const int D, const int H1, const int H2, const float steer_scale)
{
    if (ok_vithead_shape_bad(D, H1, H2))
        return "shape outside the limits (dim a multiple of 16 up to 768; head_hidden1/2 multiples of 16 up to 2048)";
    if (okVitHeadLdsBytes(D, H1, H2) > kLidarLdsBudget)
        return "the forward kernel's LDS (okenv_vit_head_lds_bytes) does not fit 160 KB";
    if (!std::isfinite(steer_scale) || !(steer_scale > 0.F))
        return "steer_scale must be finite and > 0 (the label divides by it)";
    return nullptr;
}

inline const char *okVitHeadCheckCall(const float *embedding, const float *steer, const int32_t M, const int32_t B, const int32_t epochs)
{
    if (embedding == nullptr || steer == nullptr)
        return "embedding and steer are required (NULL argument)";
    if (M < 1 || B < 1 || epochs < 1)
        return "M, B and epochs must be at least 1";
    if (static_cast<int64_t>(epochs) * M >= (INT64_C(1) << 31))
        return "epochs * M must stay below 2^31";
    return nullptr;
}

// One minibatch on the host: the joined sums over its Bk positions divided by Bk -> grad [total] and *loss.  `order`: the epoch's row.
inline void okVitHeadMinibatchHost(const float *head, const int D, const int H1, const int H2, const float steer_scale, const okenv_vit_head_params &hp,
                                   const float *embedding, const float *steer, const int M, const int32_t *order, const long base, const int Bk,
                                   std::vector<float> &grad, float *loss)
{
    const ok_vithead_layout at = ok_vithead_offsets(D, H1, H2);
    std::vector<float>      part(static_cast<size_t>(at.total)), h1(H1), h2(H2), d1(H1), d2(H2);
    float                   l_joined = 0.F;
    for (int c0 = 0; c0 < Bk; c0 += OK_VITHEAD_CHUNK)
    {
        const int n = std::min(OK_VITHEAD_CHUNK, Bk - c0);
        std::fill(part.begin(), part.end(), 0.F);
        float l_part = 0.F;
        for (int q = c0; q < c0 + n; ++q)
        {
            const int    s = ok_learn_clamp_index(order != nullptr ? static_cast<long long>(order[base + q]) : static_cast<long long>(base + q), M);
            const float *e = embedding + static_cast<size_t>(s) * D;
            float        d_o = 0.F, t = 0.F;
            (void)ok_vithead_position(head, D, H1, H2, e, steer[s], steer_scale, hp.weight, hp.threshold, h1.data(), h2.data(), d1.data(), d2.data(), &d_o, &t);
            for (int j = 0; j < H1; ++j)
            {
                float *w = part.data() + at.w1 + static_cast<size_t>(j) * D;
                for (int k = 0; k < D; ++k)
                    w[k] = __builtin_fmaf(d1[j], e[k], w[k]);
                part[at.b1 + j] = part[at.b1 + j] + d1[j];
            }
            for (int j = 0; j < H2; ++j)
            {
                float *w = part.data() + at.w2 + static_cast<size_t>(j) * H1;
                for (int k = 0; k < H1; ++k)
                    w[k] = __builtin_fmaf(d2[j], h1[k], w[k]);
                part[at.b2 + j] = part[at.b2 + j] + d2[j];
            }
            for (int k = 0; k < H2; ++k)
                part[at.w3 + k] = __builtin_fmaf(d_o, h2[k], part[at.w3 + k]);
            part[at.b3] = part[at.b3] + d_o;
            l_part      = l_part + t;
        }
        if (n < OK_VITHEAD_CHUNK) // the rule's ZERO TERMS
        {
            for (float &v : part)
                v = ok_vithead_fill(v);
            l_part = ok_vithead_fill(l_part);
        }
        for (int k = 0; k < at.total; ++k)
            grad[k] = c0 == 0 ? part[k] : grad[k] + part[k];
        l_joined = c0 == 0 ? l_part : l_joined + l_part;
    }
    const float count = static_cast<float>(Bk);
    for (int k = 0; k < at.total; ++k)
        grad[k] = grad[k] / count;
    *loss = l_joined / count;
}

inline void okVitHeadUpdateHost(const okenv_vit_head_params &hp, const int D, const int H1, const int H2, const float steer_scale, okenv_vit_head_state &st,
                                const float *embedding, const float *steer, const int32_t M, const int32_t B, const int32_t epochs, const int32_t *order,
                                const okenv_vit_head_output &out)
{
    const int                  total = ok_vithead_offsets(D, H1, H2).total, slices = okLearnMinibatches(M, B);
    const okenv_learner_params lp = okVitHeadAdam(hp);
    std::vector<float>         grad(static_cast<size_t>(total));
    for (int e = 0; e < epochs; ++e)
        for (int k = 0; k < slices; ++k)
        {
            const long base = static_cast<long>(k) * B;
            const int  Bk = static_cast<int>(std::min<long>(B, M - base));
            float      loss = 0.F;
            okVitHeadMinibatchHost(st.params, D, H1, H2, steer_scale, hp, embedding, steer, M, order != nullptr ? order + static_cast<size_t>(e) * M : nullptr, base,
                                   Bk, grad, &loss);
            const ok_learn_adam_consts adam = okLearnAdamConsts(lp, st.t + 1);
            for (int i = 0; i < total; ++i)
                ok_learn_adam(st.params + i, st.m + i, st.v + i, grad[i], adam);
            st.t += 1;
            if (out.loss != nullptr)
                out.loss[static_cast<size_t>(e) * slices + k] = loss;
        }
    if (out.grad != nullptr)
        std::copy(grad.begin(), grad.end(), out.grad);
}

inline void okVitHeadEvalHost(const okenv_vit_head_params &hp, const int D, const int H1, const int H2, const float steer_scale, const float *head,
                              const float *embedding, const float *steer, const int32_t M, const int32_t B, float *loss)
{
    const int          slices = okLearnMinibatches(M, B);
    std::vector<float> grad(static_cast<size_t>(ok_vithead_offsets(D, H1, H2).total));
    for (int k = 0; k < slices; ++k)
    {
        const long base = static_cast<long>(k) * B;
        okVitHeadMinibatchHost(head, D, H1, H2, steer_scale, hp, embedding, steer, M, nullptr, base, static_cast<int>(std::min<long>(B, M - base)), grad, loss + k);
    }
}

#endif // OK_VITHEAD_H
