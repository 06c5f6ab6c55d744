/*
 * okenv_memtrain.h -- the rule of the training of the world-model racers' memory (WorldModelVaeRnn/train_rnn.py: the GRUDynamics network
 * on windows of recorded latents and actions, teacher forcing, mean squared error, gradient clipping, AdamW).  Shared bit for bit by the
 * HIP kernels (openkitchen_amd/csrc/ok_memtrain.h) and the host entries okenv_memory_update_host / okenv_memory_eval_host (DESIGN.md
 * section 32).  The first rule of the project with backpropagation through time.
 *
 * THE RULE
 *
 * Data.  latent [rows][Z] and action [rows][2] (throttle, steering as stored), M window starts start [M] (int32 row indices) and a row
 * stride.  Step s = 0 .. S-1 of a window reads row start + s * stride; its target is row start + (s + 1) * stride (ok_memtrain_row: the
 * sum in 64 bits; a row outside 0 .. rows-1 counts as the nearest valid one, ok_learn_clamp_index: device data is not validated).
 * Stride 1 is train_rnn.py's flat dataset; stride N is [T][N][.] tensors with start = t0 * N + n.
 *
 * Normalisation.  Input x0 = [ok_memory_normalise(z_j, z_mean_j, z_std_j) | ok_memory_normalise(a_k, a_mean_k, a_std_k)] and target
 * y_j = ok_memory_normalise(z'_j, z_mean_j, z_std_j) with the network vector's own statistics, as the act does.  The statistics are not
 * trained: the trainable prefix of the network vector is T = ok_memory_offsets(s).z_mean floats, and Adam's moments exist for it only.
 *
 * Minibatches.  okenv_learn.h's: epoch e cuts the M windows into ceil(M / B) minibatches; minibatch k holds B_k = min(B, M - k B)
 * windows q = 0 .. B_k - 1, and window q is start[order[e][k B + q]], or start[k B + q] without an order; an index outside 0 .. M-1
 * counts as the nearest valid one.  One optimiser step per minibatch; every forward uses the parameters from before that step.
 *
 * Positions.  A minibatch has P = B_k * S positions, enumerated STEP-MAJOR: p = s * B_k + q.  Every sum over positions runs in this
 * order.
 *
 * One primitive (ok_memtrain_chain) carries every contraction:  acc = bias;  for each block of OK_MEMTRAIN_BLOCK = 64 terms in
 * ascending order:  part = +0.0f;  part = fmaf(a_k, b_k, part) for k ascending in the block;  acc = acc + part (one rounded addition).
 * With unit strides this is ok_memory_dot, expression for expression.  A block's partial is what sixteen v_mfma_f32_16x16x4_f32 from a
 * zero C give over one K block.  Where no bias is named the bias is +0.0f.
 *     ZERO TERMS.  Section 31's convention holds: a partial last block may be filled up with terms whose a is +0.0f (and whose b is
 *     +0.0f or 1.0f).  A filler term leaves part as it was unless part is -0.0f, which becomes +0.0f.  Here that never reaches a result
 *     of a chain from a +0.0f bias: acc begins at +0.0f, (+0.0f) + (-0.0f) and (+0.0f) + (+0.0f) are both +0.0f, x + (+-0.0f) is x for
 *     every other x, and so acc is never -0.0f and never depends on the sign of a zero partial.  The fillers are therefore free in the
 *     chains over positions, the only ones whose length is no multiple of 4.  The forward chains (from a real bias) have no fillers:
 *     Z and H are multiples of 16.
 *
 * Forward.  Per window, S steps from a zero hidden state in every layer.  Each step is ok_memory_step's own expressions with
 * carry = 1: for layer l, unit j, gate g (r, z, n), x the layer's input (x0, or the layer below's new h of the same step):
 *     gi_g = chain(x, Wih[g H + j], Kin, bih[g H + j])  (+ ok_memory_action_part in layer 0, Kin = Z);   gh_g = chain(h_prev, Whh[g H + j], H, bhh[g H + j])
 *     r = ok_memory_sig(gi_0 + gh_0);  u = ok_memory_sig(gi_1 + gh_1);  a_n = gi_2 + r * gh_2;  n = ok_tanhf(a_n);  h' = (1.0f - u) * n + u * h_prev
 * (ok_memtrain_cell: ok_memory_gate's expressions, which also hands out r, u, n).  zn_j = chain(h_top, head.w[j], H, head.b[j]).
 * A window replayed through ok_memory_step from a zeroed state therefore gives the same hidden states and predictions bit for bit
 * (the prediction up to ok_memory_step's denormalisation zn * z_std + z_mean).
 *     STEP 0's gh is the chain over a zero h_prev, not carry == 0's shortcut gh = bhh.  Every term is fmaf(+0.0f, w, part) = +0.0f for a
 *     finite w, so the chain gives bhh + (+0.0f): bhh's own bits, except that a bias of -0.0f becomes +0.0f.  ok_memory_step with
 *     carry == 1 from a zeroed state computes the same chain, so the replay agrees everywhere; a replay with carry == 0 would differ for
 *     a bias of -0.0f only, and then only in the sign of a zero.
 *
 * Loss and seeds (ok_memtrain_seed), nothing fused.   e = zn_j - y_j;   t = e * e;   dzn_j = 2.0f * e.
 * loss_j = chain over positions of (t_p,j, 1.0f);  loss = chain over j of (loss_j, 1.0f) / count,  count = (float)(B_k * S * Z), one IEEE
 * division.  The factor 1 / count enters nowhere else before the joins: the seeds are undivided, and every parameter's joined sum is
 * divided once (below).
 *
 * Backward through one cell (ok_memtrain_cell_back), torch's formulation, each line one rounding per operation, from dh = dh':
 *     dn = dh * (1.0f - u);   du = dh * (h_prev - n);   keep = dh * u                      (keep: the u . dh' share of dh_prev)
 *     da_n = dn * (1.0f - n * n);   dr = da_n * gh_2;   da_r = dr * (r * (1.0f - r));   da_u = du * (u * (1.0f - u))
 *     dgi = [da_r, da_u, da_n]  (rows j, H + j, 2 H + j);     dgh = [da_r, da_u, da_n * r]
 * dh' of layer l at step s is  (down + keep) + back  in this order (ok_memtrain_dh):
 *     down   top layer: chain over k < Z of (dzn_k, head.w[k][j]);  below it: layer l + 1's dx_j = chain over its 3H gate rows i of
 *            (dgi_i, Wih_{l+1}[i][j]), same step
 *     keep   step s + 1's keep of this layer;  +0.0f at s = S - 1
 *     back   chain over the 3H gate rows i of (dgh_i of step s + 1, Whh_l[i][j]);  +0.0f at s = S - 1
 * No dx is formed for layer 0.  The order in which (layer, step) pairs are visited is free: each dh' depends on its three parts only.
 *
 * Parameter sums, each a chain over the P positions, then divided once by count:
 *     Wih_l[i][k]: (dgi_i, x_k), x the layer's input, in layer 0 all Z + 2 columns alike: the two action columns, a block of their own in
 *     the forward, get their gradient by the same chain over positions as every other column;   bih_l[i]: (dgi_i, 1.0f)
 *     Whh_l[i][k]: (dgh_i, h_prev_k), h_prev of step 0 being +0.0f;   bhh_l[i]: (dgh_i, 1.0f);   head.w[j][k]: (dzn_j, h_top_k);   head.b[j]: (dzn_j, 1.0f)
 *
 * Clipping (torch's clip_grad_norm_).  total = ok_memtrain_sumsq over the T divided gradients in parameter order: level 0 cuts them
 * into blocks of 64, each part = fmaf(g, g, part) from +0.0f ascending; every further level cuts the values of the level before into
 * groups of 64 and sums each by plain additions from +0.0f ascending, until one value is left.  norm = the correctly rounded square
 * root of total: the pre-clip norm, an output of every minibatch.  coef = clip_grad / (norm + 1e-6f), and 1.0f where that is larger
 * (a NaN passes); every gradient is multiplied by coef.  clip_grad == 0 switches clipping off: coef = 1.0f.
 *
 * AdamW (ok_memtrain_step).  p = p * decay, decay = (float)(1 - (double)lr * (double)weight_decay); then ok_learn_adam unchanged on the
 * clipped gradient, with ok_learn_factors' step and bc2 for the step number and the minibatch's lr (ok_memtrain_factors: the same fp64
 * expressions, callable on the device too, where the step number lives so that a captured update replays with its own numbers).
 * weight_decay == 0 gives decay == 1.0f and p * 1.0f == p: ok_learn_adam's bits.  t, m and v persist across calls.
 *
 * Schedule.  The lr of minibatch k of epoch e is lr[e * ceil(M / B) + k] from an optional host array; without one it is the learner's.
 * A cosine belongs to the caller.
 *
 * Eval.  The same per-minibatch loss with no step, in sequential order (the reference's validation loop).
 *
 * Only fmaf, +, -, *, /, comparisons, the correctly rounded square root and ok_tanhf are used; compile with -ffp-contract=off.
 * Plain C99 / C++ / HIP.
 */
#ifndef OKENV_MEMTRAIN_H
#define OKENV_MEMTRAIN_H

#include "okenv_learn.h"
#include "okenv_memory.h"

#define OK_MEMTRAIN_BLOCK 64
#define OK_MEMTRAIN_MAX_SEQ 16

/* Floats of the trainable prefix of the network vector */
OK_HDI int ok_memtrain_trainable(const ok_memory_shape s)
{
    return ok_memory_offsets(s).z_mean;
}

/* The row step s of a window reads (s = S: the last target's) */
OK_HDI int ok_memtrain_row(const int start, const int s, const int stride, const int rows)
{
    return ok_learn_clamp_index((long long)start + (long long)s * (long long)stride, rows);
}

/* Window q of a minibatch whose first position in the epoch is base: its index into start [M] */
OK_HDI int ok_memtrain_window(const int *order, const long long base, const int q, const int M)
{
    return ok_learn_clamp_index(order ? (long long)order[base + q] : base + q, M);
}

/* The primitive: a [K] and b [K] with strides; b == NULL: 1.0f */
OK_HDI float ok_memtrain_chain(const float *a, const long long as, const float *b, const long long bs, const int K, const float bias)
{
    float acc = bias;
    for (int k0 = 0; k0 < K; k0 += OK_MEMTRAIN_BLOCK) {
        const int end  = k0 + OK_MEMTRAIN_BLOCK < K ? k0 + OK_MEMTRAIN_BLOCK : K;
        float     part = 0.0f;
        for (int k = k0; k < end; ++k) part = __builtin_fmaf(a[k * as], b ? b[k * bs] : 1.0f, part);
        acc = acc + part;
    }
    return acc;
}

/* ok_memory_gate, which also hands out what the backward pass needs */
OK_HDI float ok_memtrain_cell(const float gi_r, const float gi_z, const float gi_n, const float gh_r, const float gh_z, const float gh_n,
                              const float h_prev, float *r_out, float *u_out, float *n_out)
{
    const float r = ok_memory_sig(gi_r + gh_r), u = ok_memory_sig(gi_z + gh_z);
    const float n = ok_tanhf(gi_n + r * gh_n);
    const float keep = u * h_prev, fresh = (1.0f - u) * n;
    *r_out = r;
    *u_out = u;
    *n_out = n;
    return fresh + keep;
}

OK_HDI void ok_memtrain_seed(const float zn, const float y, float *t, float *dzn)
{
    const float e = zn - y;
    *t   = e * e;
    *dzn = 2.0f * e;
}

OK_HDI float ok_memtrain_dh(const float down, const float keep, const float back)
{
    return (down + keep) + back;
}

/* d [4]: da_r, da_u, da_n and dgh's third row da_n * r */
OK_HDI void ok_memtrain_cell_back(const float dh, const float r, const float u, const float n, const float gh_n, const float h_prev, float *keep,
                                  float *d)
{
    const float dn = dh * (1.0f - u);
    const float du = dh * (h_prev - n);
    *keep = dh * u;
    const float da_n = dn * (1.0f - n * n);
    const float dr   = da_n * gh_n;
    d[0] = dr * (r * (1.0f - r));
    d[1] = du * (u * (1.0f - u));
    d[2] = da_n;
    d[3] = da_n * r;
}

/* Level 0 of the sum of squares: one block of n <= 64 gradients */
OK_HDI float ok_memtrain_sq_block(const float *g, const int n)
{
    float part = 0.0f;
    for (int k = 0; k < n; ++k) part = __builtin_fmaf(g[k], g[k], part);
    return part;
}

/* A further level: one group of n <= 64 values */
OK_HDI float ok_memtrain_sum_group(const float *v, const int n)
{
    float acc = 0.0f;
    for (int k = 0; k < n; ++k) acc = acc + v[k];
    return acc;
}

/* The whole sum over g [n]; work: (n + 63) / 64 floats.  The host's form; the device runs a launch per level. */
OK_HD float ok_memtrain_sumsq(const float *g, const int n, float *work)
{
    int count = (n + OK_MEMTRAIN_BLOCK - 1) / OK_MEMTRAIN_BLOCK;
    for (int b = 0; b < count; ++b) {
        const int left = n - b * OK_MEMTRAIN_BLOCK;
        work[b] = ok_memtrain_sq_block(g + b * OK_MEMTRAIN_BLOCK, left < OK_MEMTRAIN_BLOCK ? left : OK_MEMTRAIN_BLOCK);
    }
    while (count > 1) {
        const int next = (count + OK_MEMTRAIN_BLOCK - 1) / OK_MEMTRAIN_BLOCK;
        for (int b = 0; b < next; ++b) { /* (in place: group b is read whole before work[b] is written, and b <= 64 b) */
            const int left = count - b * OK_MEMTRAIN_BLOCK;
            work[b] = ok_memtrain_sum_group(work + b * OK_MEMTRAIN_BLOCK, left < OK_MEMTRAIN_BLOCK ? left : OK_MEMTRAIN_BLOCK);
        }
        count = next;
    }
    return work[0];
}

/* The pre-clip norm and the factor every gradient is multiplied by */
OK_HDI float ok_memtrain_clip(const float total, const float clip_grad, float *norm)
{
    *norm = (float)__builtin_sqrt((double)total);
    if (!(clip_grad > 0.0f)) return 1.0f;
    const float coef = clip_grad / (*norm + 1e-6f);
    return coef > 1.0f ? 1.0f : coef;
}

/* One AdamW step of one parameter; returns the clipped gradient */
OK_HDI float ok_memtrain_step(float *p, float *m, float *v, const float g, const float coef, const float decay, const ok_learn_adam_consts c)
{
    const float gc = g * coef;
    *p = *p * decay;
    ok_learn_adam(p, m, v, gc, c);
    return gc;
}

/* ok_learn_factors' expressions, for the host and the device */
OK_HDI void ok_memtrain_factors(const float lr, const float beta1, const float beta2, long long t, float *step, float *bc2)
{
    double p1 = 1.0, p2 = 1.0, b1 = (double)beta1, b2 = (double)beta2;
    while (t > 0) {
        if (t & 1) {
            p1 = p1 * b1;
            p2 = p2 * b2;
        }
        b1 = b1 * b1;
        b2 = b2 * b2;
        t >>= 1;
    }
    *step = (float)((double)lr / (1.0 - p1));
    *bc2  = (float)__builtin_sqrt(1.0 - p2);
}

static inline float ok_memtrain_decay(const float lr, const float weight_decay)
{
    return (float)(1.0 - (double)lr * (double)weight_decay);
}

#endif /* OKENV_MEMTRAIN_H */
