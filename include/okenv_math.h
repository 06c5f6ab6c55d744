/*
 * okenv_math.h -- scalar math shared, bit for bit, by the HIP kernels and the CPU oracle.
 *
 * Why this exists (SURVEY.md section 0 item 5, section 7 "Transcendentals"): the reference's host
 * code calls glibc cosf/sinf (Environment/Agent.cpp:94-97,115-118, Environment/CollisionChecker.cu:
 * 121-124,157-158) and its kernel calls CUDA cosf/sinf (Environment/CollisionChecker.cu:47-48).
 * Those differ from each other and from ROCm's OCML in the last ulp, which is enough to flip the
 * `min_dist2 < 2.0f` crash test.  Crash/done flags must be bit-exact between the GPU path and the
 * CPU oracle, so both sides evaluate sine/cosine through THIS header: an fp64 reduction and fp64
 * polynomials, rounded once to fp32.  Only +, -, *, explicitly requested fused multiply-adds (OK_FMA) and
 * round-to-nearest-even conversions are used, all IEEE-exact on x86-64 and on gfx950, so the two sides agree bit
 * for bit provided the translation unit is compiled with -ffp-contract=off (nothing fused that does not ask for it).
 * tests/test_math.py bounds the distance to glibc sincosf (<= 1 ulp) and to an fp64 reference.
 *
 * Also here: Philox4x32-10 (Salmon et al., SC'11), the counter-based generator the C2 bench recipe
 * draws actions and reset positions from, so the device rollout and the oracle
 * rollout see identical streams.
 *
 * Plain C99 / C++ / HIP.  No dependency on anything under oracle/.
 */
#ifndef OKENV_MATH_H
#define OKENV_MATH_H

#include <stdint.h>

#if defined(__HIPCC__)
#define OK_HD __host__ __device__ static inline
#else
#define OK_HD static inline
#endif
/* For functions that take small arrays the kernels keep in registers: inlined always, so that the array never needs an address. */
#define OK_HDI OK_HD __attribute__((always_inline))

/* Environment/Typedefs.h:10  kDeg2Rad = float(M_PI / 180.0F)  (bit pattern 0x3C8EFA35) */
#define OK_DEG2RAD 0.01745329238474369049072265625f
/* Environment/Agent.cpp:84,110  kDt{0.016} as float (bit pattern 0x3C83126F) */
#define OK_DT 0.016000000759959220886230468750f
/* Environment/Agent.h:10-11 */
#define OK_SENSOR_RANGE 200.0f
#define OK_SPEED_LIMIT 100.0f
/* Environment/CollisionChecker.cu:167 */
#define OK_CRASH_DIST2 2.0f
/* Environment/Environment.h:19-20 */
#define OK_DISP_PERIOD 200u
#define OK_DISP_THRESH2 400.0f /* kDisplamentThreshold^2 = 20*20, exact in fp32 */
/* Environment/CollisionChecker.cu:23 */
#define OK_PARALLEL_EPS 1e-8f

#define OK_RINT(x) __builtin_rint(x) /* round to nearest even: rint() on the host, v_rndne_f64 on gfx950 */
/* a * b + c with ONE rounding, asked for explicitly: v_fma_f64 on gfx950, libm's correctly rounded fma() (or the host's FMA
 * instruction) on x86-64 -- the same bits either way.  The translation units are still compiled -ffp-contract=off: nothing is
 * fused that does not say so here. */
#define OK_FMA(a, b, c) __builtin_fma((a), (b), (c))
/* A double constant of the polynomials below.  On the device it is made opaque and pinned to a scalar register pair: hipcc would
 * otherwise materialise each one in a VECTOR register pair (v_fmac_f64 wants its addend there), hoist all of them out of the
 * kernels' step loops and keep them alive across the raycast -- 22 more VGPRs in every step kernel, scratch spills in the policy
 * ones (profiles/r4/kernel_resource_usage.txt).  As scalar operands of v_fma_f64 they cost s_mov's and no vector registers.  The
 * value is untouched: same bits on both sides. */
#if defined(__HIP_DEVICE_COMPILE__)
static __device__ inline __attribute__((always_inline)) double ok_konst(double c)
{
    asm("" : "+s"(c));
    return c;
}
#else
#define ok_konst(c) (c)
#endif

/*
 * sin and cos of an fp32 angle [rad], from an fp64 evaluation rounded once to fp32 (round 4's form; rounds 1-3 used a
 * three-part Cody-Waite reduction and Taylor series to 1/15! with separate multiplications and additions: ~42 fp64 operations
 * in a dependent chain of ~26; this is 21 operations in a chain of 12).
 *   q = rint(x * 2/pi);  r = x - q * pi/2 by two FMAs against pi/2 = P1 + P2 (P1 the nearest double, P2 the next 53 bits): each FMA
 *   forms its product exactly and rounds once, so r carries a RELATIVE error of ~2^-52 however close x lies to a multiple of
 *   pi/2, for every |q| < 2^31;
 *   sin r = r + (r z) S(z),  cos r = 1 + z C(z),  z = r^2, S and C of degree 5 in z: interpolants at the Chebyshev nodes of
 *   [0, 0.79^2] (tools/fit_math.py prints them; pi/4 = 0.7854, the slack covers q's own rounding), relative errors 2^-55 and
 *   2^-51, evaluated by Horner's rule in FMAs.
 * The result is the correctly rounded fp32 sine / cosine but for about one argument in 10^7 (tests/test_math.py: equal to the
 * rounded fp64 value on 700 000 samples and on the floats nearest to multiples of pi/2 up to 2^31; <= 1 ulp from glibc's
 * sinf / cosf, which the reference's host code calls).  rot_ is never wrapped (Environment/Agent.cpp:86,112), so large arguments
 * do occur: beyond 2^31 rad (fp32 spacing there is 256 rad: the angle carries no information) the argument is folded by an
 * exact fmod first; NaN / Inf give NaN.
 */
OK_HD void ok_sincosf(float x, float *s_out, float *c_out)
{
    double xd = (double)x;
    if (!(__builtin_fabs(xd) < 2147483648.0)) {
        xd = __builtin_fmod(xd, 6.283185307179586476925286766559); /* exact by definition: identical on CPU and GPU */
        if (!(xd == xd)) { /* NaN or Inf in */
            *s_out = (float)xd;
            *c_out = (float)xd;
            return;
        }
    }
    const double q = OK_RINT(xd * ok_konst(0x1.45f306dc9c883p-1)); /* 2/pi */
    double r = OK_FMA(-q, ok_konst(0x1.921fb54442d18p+0), xd);     /* P1 = 1.5707963267948966    */
    r = OK_FMA(-q, ok_konst(0x1.1a62633145c07p-54), r);            /* P2 = 6.123233995736766e-17 */
    const int n = ((int)q) & 3;                          /* quadrant; |q| < 1.4e9 fits an int */
    const double z = r * r;
    double ps = ok_konst(0x1.5e01d1798c2b3p-33);              /*  1.5916480269048027e-10 */
    ps = OK_FMA(ps, z, ok_konst(-0x1.ae5ff116c8d06p-26));     /* -2.505110882200661e-08  */
    ps = OK_FMA(ps, z, ok_konst(0x1.71de377d84985p-19));      /*  2.755731599143529e-06  */
    ps = OK_FMA(ps, z, ok_konst(-0x1.a01a019e70424p-13));     /* -1.9841269836543094e-04 */
    ps = OK_FMA(ps, z, ok_konst(0x1.1111111110b60p-7));       /*  8.333333333330806e-03  */
    ps = OK_FMA(ps, z, ok_konst(-0x1.5555555555555p-3));      /* -1.6666666666666666e-01 */
    const double sr = OK_FMA(r * z, ps, r);
    double pc = ok_konst(0x1.1bfd9695386eap-29);              /*  2.0663034153592203e-09 */
    pc = OK_FMA(pc, z, ok_konst(-0x1.27e0dd327adbcp-22));     /* -2.75558210165445e-07   */
    pc = OK_FMA(pc, z, ok_konst(0x1.a019fc4c6ed87p-16));      /*  2.4801582456863223e-05 */
    pc = OK_FMA(pc, z, ok_konst(-0x1.6c16c168f930cp-10));     /* -1.3888888881805088e-03 */
    pc = OK_FMA(pc, z, ok_konst(0x1.5555555554001p-5));       /*  4.166666666662878e-02  */
    pc = OK_FMA(pc, z, ok_konst(-0x1.ffffffffffffap-2));      /* -4.9999999999999967e-01 */
    const double cr = OK_FMA(z, pc, 1.0);
    double sv, cv;
    if (n == 0) { sv = sr; cv = cr; }
    else if (n == 1) { sv = cr; cv = -sr; }
    else if (n == 2) { sv = -sr; cv = -cr; }
    else { sv = -cr; cv = sr; }
    *s_out = (float)sv;
    *c_out = (float)cv;
}

/* From sin r and cos r, already rounded to fp32, to the sine and cosine of quadrant n: ok_sincosf's four cases without a branch.
 * Odd quadrants swap the two; the sine is negative in quadrants 2 and 3, the cosine in 1 and 2.  ok_sincosf negates the double and
 * then rounds; rounding to nearest even is symmetric in the sign, so flipping the sign bit of the rounded value gives the same bits. */
OK_HD void ok_sincos_quadrant(const int n, const float sr, const float cr, float *s_out, float *c_out)
{
    union { float f; uint32_t u; } s, c;
    s.f = (n & 1) ? cr : sr;
    c.f = (n & 1) ? sr : cr;
    s.u ^= ((uint32_t)n & 2u) << 30;
    c.u ^= (((uint32_t)n + 1u) & 2u) << 30;
    *s_out = s.f;
    *c_out = c.f;
}

/*
 * ok_sincosf of two angles at once: by definition the bits that ok_sincosf(xa, sa, ca) and ok_sincosf(xb, sb, cb) return, for every
 * pair of arguments, on host and device (tests/test_math_pair.py).  The step kernels need the sine and cosine of the agent's
 * heading and of the lane's ray angle in every step; two calls of ok_sincosf compile to two blocks one after the other, each with
 * its own range-reduction loop, its own non-finite exit, its own four-way quadrant branch and its own copy of the constants, and
 * the two dependent fp64 chains run back to back.  Here, where both arguments are finite and below 2^31 in magnitude -- always,
 * but for a heading that has run away -- both reductions and both pairs of polynomials stand in one basic block, operation by
 * operation next to each other, so that one chain's latency is the other's work; every constant is named once; the quadrants are
 * undone by selects and sign bits (ok_sincos_quadrant).  The same operations on the same values as ok_sincosf in every other
 * respect.  Anything else takes the one rare branch to two plain calls.
 */
OK_HD void ok_sincosf_pair(const float xa, const float xb, float *sa_out, float *ca_out, float *sb_out, float *cb_out)
{
    /* (the comparison in fp32 decides what ok_sincosf's in fp64 decides: the conversion is exact) */
    if (__builtin_expect(!((__builtin_fabsf(xa) < 2147483648.0f) & (__builtin_fabsf(xb) < 2147483648.0f)), 0)) {
        ok_sincosf(xa, sa_out, ca_out);
        ok_sincosf(xb, sb_out, cb_out);
        return;
    }
    const double xda = (double)xa, xdb = (double)xb;
    const double two_over_pi = ok_konst(0x1.45f306dc9c883p-1);
    const double qa = OK_RINT(xda * two_over_pi), qb = OK_RINT(xdb * two_over_pi);
    const double p1 = ok_konst(0x1.921fb54442d18p+0);
    double ra = OK_FMA(-qa, p1, xda), rb = OK_FMA(-qb, p1, xdb);
    const double p2 = ok_konst(0x1.1a62633145c07p-54);
    ra = OK_FMA(-qa, p2, ra);
    rb = OK_FMA(-qb, p2, rb);
    const double za = ra * ra, zb = rb * rb;
    /* the coefficients of ok_sincosf's S and C, highest degree first */
    const double s5 = ok_konst(0x1.5e01d1798c2b3p-33), c5 = ok_konst(0x1.1bfd9695386eap-29);
    const double s4 = ok_konst(-0x1.ae5ff116c8d06p-26), c4 = ok_konst(-0x1.27e0dd327adbcp-22);
    double psa = OK_FMA(s5, za, s4), psb = OK_FMA(s5, zb, s4);
    double pca = OK_FMA(c5, za, c4), pcb = OK_FMA(c5, zb, c4);
    const double s3 = ok_konst(0x1.71de377d84985p-19), c3 = ok_konst(0x1.a019fc4c6ed87p-16);
    psa = OK_FMA(psa, za, s3);
    psb = OK_FMA(psb, zb, s3);
    pca = OK_FMA(pca, za, c3);
    pcb = OK_FMA(pcb, zb, c3);
    const double s2 = ok_konst(-0x1.a01a019e70424p-13), c2 = ok_konst(-0x1.6c16c168f930cp-10);
    psa = OK_FMA(psa, za, s2);
    psb = OK_FMA(psb, zb, s2);
    pca = OK_FMA(pca, za, c2);
    pcb = OK_FMA(pcb, zb, c2);
    const double s1 = ok_konst(0x1.1111111110b60p-7), c1 = ok_konst(0x1.5555555554001p-5);
    psa = OK_FMA(psa, za, s1);
    psb = OK_FMA(psb, zb, s1);
    pca = OK_FMA(pca, za, c1);
    pcb = OK_FMA(pcb, zb, c1);
    const double s0 = ok_konst(-0x1.5555555555555p-3), c0 = ok_konst(-0x1.ffffffffffffap-2);
    psa = OK_FMA(psa, za, s0);
    psb = OK_FMA(psb, zb, s0);
    pca = OK_FMA(pca, za, c0);
    pcb = OK_FMA(pcb, zb, c0);
    const double sra = OK_FMA(ra * za, psa, ra), srb = OK_FMA(rb * zb, psb, rb);
    const double cra = OK_FMA(za, pca, 1.0), crb = OK_FMA(zb, pcb, 1.0);
    ok_sincos_quadrant((int)qa, (float)sra, (float)cra, sa_out, ca_out); /* |q| < 1.4e9 fits an int */
    ok_sincos_quadrant((int)qb, (float)srb, (float)crb, sb_out, cb_out);
}

/* ---- Philox4x32-10 -------------------------------------------------------------------------- */

typedef struct ok_u32x4 { uint32_t v[4]; } ok_u32x4;

OK_HD ok_u32x4 ok_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    ok_u32x4 r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

/* u32 -> [0,1) with 24 random bits; every step is exact in fp32 */
OK_HD float ok_u01(uint32_t u)
{
    return (float)(u >> 8) * 5.9604644775390625e-08f; /* 2^-24 */
}

/*
 * The C2 synthetic-action recipe:
 *   counter = (agent, step, 0, 0), key = (seed, 0x6F6B656E /"oken"/)
 *   throttle = U[0,100), steer = U[-5,5), reset_idx = floor(U * P) drawn from the third word.
 * `agent` is the GLOBAL agent id, so a population sharded over ranks reproduces the unsharded streams.
 */
typedef struct ok_random_action { float throttle; float steer; uint32_t reset_word; } ok_random_action;

OK_HD ok_random_action ok_draw_random_action(uint32_t seed, uint32_t agent, uint32_t step)
{
    const ok_u32x4 r = ok_philox4x32(agent, step, 0u, 0u, seed, 0x6F6B656Eu);
    ok_random_action a;
    a.throttle = ok_u01(r.v[0]) * 100.0f;
    a.steer = ok_u01(r.v[1]) * 10.0f - 5.0f;
    a.reset_word = r.v[2];
    return a;
}

/* index in [0,P) from a 32-bit word (multiply-shift, no modulo bias worth speaking of) */
OK_HD uint32_t ok_index_from_word(uint32_t w, uint32_t P)
{
    return (uint32_t)(((uint64_t)w * (uint64_t)P) >> 32);
}

/* start index of agent j in the bench recipe: (j * 2654435761) mod 2^32 mod P */
OK_HD uint32_t ok_start_index(uint32_t agent, uint32_t P)
{
    return (uint32_t)(agent * 2654435761u) % P;
}

/* ---- Environment::resetAgent (Environment/Environment.cpp:79-122) -- */

/* the three booleans of resetAgent(agent, pick_random_point, randomize_lane, randomize_heading) */
#define OK_RESET_RANDOM_POINT 1u
#define OK_RESET_RANDOM_LANE 2u
#define OK_RESET_RANDOM_HEADING 4u
/* batch calls only: leave agents whose crashed_ flag is clear alone */
#define OK_RESET_ONLY_DONE 8u
/* RaceTrack::kStartingIdx (Environment/RaceTrack.h:18) */
#define OK_RESET_START_IDX 3u

/*
 * The random draws of one resetAgent call.  raylib's GetRandomValue(lo, hi) (inclusive integer range, un-vendored,
 * global state) is replaced by one Philox block per (agent, epoch):
 *   counter = (agent, epoch, 1, 0), key = (seed, 0x6F6B656E)
 *   word 0 -> reset_idx in [0, P-1]            (Environment.cpp:76)
 *   word 1 -> heading draw in [0, 45]          (:92)
 *   word 2 -> lane draw in [10, 90], / 100.F   (:111)
 * `ctr` stands for the reference's function-static call counter (:88): even calls turn the heading offset negative.
 * The draws the reference skips (flags off) are simply not used, so one flag does not shift another's stream.
 */
typedef struct ok_reset_draw { uint32_t idx; float heading_offset; float alpha; int use_lane; } ok_reset_draw;

OK_HD ok_reset_draw ok_draw_reset(uint32_t seed, uint32_t agent, uint32_t epoch, uint32_t ctr, uint32_t P, uint32_t flags)
{
    const ok_u32x4 r = ok_philox4x32(agent, epoch, 1u, 0u, seed, 0x6F6B656Eu);
    const int random_point = (flags & OK_RESET_RANDOM_POINT) != 0u;
    ok_reset_draw d;
    d.idx = random_point ? ok_index_from_word(r.v[0], P) : OK_RESET_START_IDX;
    d.heading_offset = 0.0f;
    if (random_point && (flags & OK_RESET_RANDOM_HEADING) != 0u) {
        const float kHeadingRangeDeg = 45.0f;
        const float draw = (float)ok_index_from_word(r.v[1], 46u);
        d.heading_offset = (ctr % 2u == 0u) ? (draw + kHeadingRangeDeg) * -1.0f : draw + kHeadingRangeDeg;
    }
    d.use_lane = random_point && (flags & OK_RESET_RANDOM_LANE) != 0u;
    d.alpha = d.use_lane ? (float)(10u + ok_index_from_word(r.v[2], 81u)) / 100.0f : 0.0f;
    return d;
}

/* Pose of the reset (Environment.cpp:104-121): a point between the inner lane boundaries or the centre-line point,
 * track heading plus the offset.  `li`/`ri` are left_bound_inner_/right_bound_inner_ as xy pairs. */
OK_HD void ok_reset_pose(const ok_reset_draw d, const float *cx, const float *cy, const float *chead, const float *li,
                         const float *ri, float *x, float *y, float *rot)
{
    if (d.use_lane) {
        const float lx = li[2u * d.idx], ly = li[2u * d.idx + 1u];
        const float rx = ri[2u * d.idx], ry = ri[2u * d.idx + 1u];
        *x = lx * d.alpha + rx * (1.0f - d.alpha);
        *y = ly * d.alpha + ry * (1.0f - d.alpha);
    } else {
        *x = cx[d.idx];
        *y = cy[d.idx];
    }
    *rot = chead[d.idx] + d.heading_offset;
}

/* ---- EvolutionaryRacer policy ------------------------------- */

/* Weight layout per agent (floats): w1[(R+2)][OK_MLP_HID_PAD] then w2[OK_MLP_HID_PAD][OK_MLP_OUT_PAD]; entries beyond
 * the hidden width H (30 in the reference, EvolutionaryRacer/Network.hpp:92-95) and beyond the 6 outputs are zero. */
#define OK_MLP_HID_PAD 32
#define OK_MLP_OUT 6
#define OK_MLP_OUT_PAD 8
#define OK_MLP_WEIGHTS(R) (((R) + 2) * OK_MLP_HID_PAD + OK_MLP_HID_PAD * OK_MLP_OUT_PAD)

/* genetic::normalizeAngleDeg (EvolutionaryRacer/Network.hpp:16-27): repeated +-360 in fp32, bit for bit; the loops
 * are capped at 65536 turns each so that an infinite rot_ cannot hang a kernel (the reference would spin forever). */
OK_HD float ok_normalize_angle_deg(float angle)
{
    for (int i = 0; i < 65536 && angle < 360.0f; ++i) angle += 360.0f;
    for (int i = 0; i < 65536 && angle >= 360.0f; ++i) angle -= 360.0f;
    return angle;
}

/* ---- FieldNavigators: the two expert drivers ------------------------------
 * PotFieldAgent::updateAction (FieldNavigators/PotentialFieldAgent.hpp:52-84), DataCollectorAgent::updateAction
 * (FieldNavigators/collect_data/collect_data_random.cpp:59-65), VFHAgent::updateHistograms / findBestSector / updateAction
 * (FieldNavigators/VFHAgent.hpp:53-123) and the goal point of their callers (FieldNavigators/main.cpp:20-25,
 * collect_data_random.cpp:108-120), restated operation by operation in the reference's precisions.  One source for the device
 * kernel (csrc/ok_expert.h) and for okenv_expert_act_host, so the two agree bit for bit; against the reference itself the only
 * licensed difference is the last bit of atan2f (ok_atan2f below is ours, glibc's is not pinned).
 *
 * Two places where the reference is undefined or degenerate are restated, not "fixed":
 *  1. findBestSector indexes binary_histogram_[(goal_sector + i) % num_sectors_] (VFHAgent.hpp:84-88) with a NEGATIVE
 *     goal_sector whenever the goal lies more than 90 deg + one sector to the right: C's remainder is then negative and the
 *     reference reads out of bounds.  Here the index (and the sector returned from it) is the non-negative remainder.
 *  2. With kObstacleDistThreshold = 1 and one ray per sector, `count > threshold` marks a sector occupied only where the fp32
 *     sector index (i / (float)R) * (float)num_sectors, truncated, puts two rays into one sector (it is not always i).  The
 *     threshold is therefore a parameter; 1 is the reference.
 * normalizeAngleDeg (Environment/Utils.h:3-14) spins for ever on an infinite rot_; here both loops are capped (below).
 */

/* atan2f for the experts, evaluated in fp64 with IEEE operations and explicit FMAs only and rounded once to fp32: same bits on
 * host and device (the idea of ok_sincosf / ok_tanhf).  a = min(|x|,|y|) / max(|x|,|y|) in [0, 1]; above tan(pi/8) one
 * reduction t = (a - 1) / (a + 1), atan a = pi/4 + atan t, so |t| <= 0.4143; atan t = t + t z A(z), z = t^2, A of degree 9
 * (interpolant at the Chebyshev nodes of [0, 0.4143^2], tools/fit_math.py: relative error 2^-52.7); then the octant is undone:
 * pi/2 - r where |y| > |x|, pi - r where x is negative (sign bit: -0 counts), the sign of y last.  Zeros, infinities and NaN
 * follow C99 F.9.1.4.  tests/test_expert_rule.py: <= 1 ulp from the rounded fp64 arctan2 and from glibc's atan2f. */
OK_HD float ok_atan2f(const float y, const float x)
{
    const double ay = __builtin_fabs((double)y), ax = __builtin_fabs((double)x);
    if (!(ay == ay) || !(ax == ax)) return x + y; /* NaN in, NaN out */
    const int swap = ay > ax;
    const double hi = swap ? ay : ax, lo = swap ? ax : ay;
    double r;
    if (hi == 0.0) {
        r = 0.0; /* atan2(+-0, +-0) */
    } else {
        const double a = (lo == hi) ? 1.0 : lo / hi; /* (inf / inf: the diagonal) */
        const int fold = a > 0x1.a827999fcef32p-2;   /* tan(pi/8) = 0.41421356237309503 */
        const double t = fold ? (a - 1.0) / (a + 1.0) : a;
        const double z = t * t;
        double p = ok_konst(0x1.74a2d785d5a9fp-6);             /*  0.022743902656055522 */
        p = OK_FMA(p, z, ok_konst(-0x1.6f3c3017cb4e7p-5));     /* -0.04482850449708469  */
        p = OK_FMA(p, z, ok_konst(0x1.d5e885b7ee229p-5));      /*  0.05736185185327642  */
        p = OK_FMA(p, z, ok_konst(-0x1.105e007ccd67cp-4));     /* -0.06649589720185561  */
        p = OK_FMA(p, z, ok_konst(0x1.3b0688e46275ap-4));      /*  0.07691052888381247  */
        p = OK_FMA(p, z, ok_konst(-0x1.745c7f2dc5c2dp-4));     /* -0.09090852431505488  */
        p = OK_FMA(p, z, ok_konst(0x1.c71c6dcf1e479p-4));      /*  0.11111109632646955  */
        p = OK_FMA(p, z, ok_konst(-0x1.2492491dcf6e7p-3));     /* -0.1428571426603675   */
        p = OK_FMA(p, z, ok_konst(0x1.9999999990a20p-3));      /*  0.19999999999898055  */
        p = OK_FMA(p, z, ok_konst(-0x1.5555555555546p-2));     /* -0.3333333333333325   */
        r = OK_FMA(t * z, p, t);
        if (fold) r = ok_konst(0x1.921fb54442d18p-1) + r;      /* pi/4 */
    }
    if (swap) r = ok_konst(0x1.921fb54442d18p+0) - r;          /* pi/2 */
    if (__builtin_signbit(x)) r = ok_konst(0x1.921fb54442d18p+1) - r; /* pi */
    return (float)(__builtin_signbit(y) ? -r : r);
}

/* normalizeAngleDeg (Environment/Utils.h:3-14) for the experts: the two loops of repeated += 360 / -= 360 in fp32 (the rounding of
 * the repeated additions is part of the result), each capped at OK_EXPERT_NORM_TURNS turns -- 4096 turns cover |angle| up to
 * 1.47 million degrees, where the reference's loops and these agree bit for bit.  Beyond that, and for infinities and NaN (where the
 * reference would spin for ever or return NaN), the result is DEFINED as 0: a wave never waits on an absurd rot_. */
#define OK_EXPERT_NORM_TURNS 4096
OK_HD float ok_expert_normalize_angle_deg(float angle)
{
    for (int i = 0; i < OK_EXPERT_NORM_TURNS && angle < 360.0f; ++i) angle += 360.0f;
    for (int i = 0; i < OK_EXPERT_NORM_TURNS && angle >= 360.0f; ++i) angle -= 360.0f;
    return (angle >= 0.0f && angle < 360.0f) ? angle : 0.0f;
}

/* Index of the goal point: nearest centre-line index + lookahead, wrapped modulo P (main.cpp:23) or clamped to P - 1
 * (collect_data_random.cpp:111-112). */
OK_HD int ok_expert_goal_index(const int nearest, const int lookahead, const int P, const int wrap)
{
    const long g = (long)nearest + (long)lookahead;
    return wrap ? (int)(g % (long)P) : (int)(g < (long)P - 1 ? g : (long)P - 1);
}

/* PotFieldAgent::updateAction followed by DataCollectorAgent's clamp (off when clamp_deg <= 0).  dist[i] = sensor_hits_[i].norm();
 * ray_cos / ray_sin [R]: cos / sin (angle_i * M_PI / 180.f) in fp64, made once on the host (they depend on the fan only). */
OK_HD void ok_potfield_action(const float px, const float py, const float rot, const float gx, const float gy, const float *dist,
                              const double *ray_cos, const double *ray_sin, const int R, const float k_att, const float k_rep,
                              const float effect_range, const float clamp_deg, float *throttle, float *steer)
{
    float ax = gx - px, ay = gy - py; /* :54 */
    const float distance_to_goal = __builtin_sqrtf(ax * ax + ay * ay);
    ax = ax / distance_to_goal * k_att; /* :57: Vec2d / float, then Vec2d * float */
    ay = ay / distance_to_goal * k_att;
    float rx = 0.0f, ry = 0.0f;
    for (int i = 0; i < R; ++i) { /* :60-73, ascending ray order */
        const float n = dist[i];
        if (n < effect_range) {
            const float mag = k_rep * (1.0f / n - 1.0f / effect_range);
            rx = (float)((double)rx + ray_cos[i] * (double)mag); /* float += double * float */
            ry = (float)((double)ry + ray_sin[i] * (double)mag);
        }
    }
    const float tx = ax - rx, ty = ay - ry; /* :75 */
    /* :78  atan2(float, float) is the fp32 overload; * 180.F in fp32; / M_PI in fp64 */
    const double goal_rotation = (double)(ok_atan2f(ty, tx) * 180.0f) / 3.14159265358979323846;
    const float len = __builtin_sqrtf(tx * tx + ty * ty);
    *throttle = len < 100.0f ? len : 100.0f; /* std::min(length, 100.F): NaN stays NaN */
    float s = (float)(goal_rotation - (double)rot); /* :81 */
    s = ok_expert_normalize_angle_deg(s);
    if (s > 180.0f) s -= 360.0f;
    if (clamp_deg > 0.0f) s = s < -clamp_deg ? -clamp_deg : (clamp_deg < s ? clamp_deg : s); /* std::clamp */
    *steer = s;
}

/* VFHAgent::updateAction.  first / last: sensor_ray_angles_.front() / .back(); num_sectors_ = R, fov_ = |last - first|,
 * sector_width_ = fov_ / num_sectors_ as in the constructor (VFHAgent.hpp:40-44).  2 <= R <= OK_VFH_MAX_RAYS: the occupancy of the
 * sectors is one 64-bit word (the fp32 sector index is non-decreasing in i, so the rays of a sector are consecutive). */
#define OK_VFH_MAX_RAYS 64
OK_HD void ok_vfh_action(const float px, const float py, const float rot, const float gx, const float gy, const float *dist, const int R,
                         const float first, const float last, const int threshold, const float vfh_throttle, float *throttle, float *steer)
{
    const int ns = R;
    const float fov = __builtin_fabsf(last - first);
    const float sector_width = fov / (float)ns;
    /* updateHistograms (:53-72) */
    uint64_t occupied = 0u;
    int cur = -1, count = 0;
    for (int i = 0; i < R; ++i) {
        if (dist[i] < OK_SENSOR_RANGE) {
            const int sector = (int)(((float)i / (float)R) * (float)ns);
            if (sector != cur) {
                if (cur >= 0 && count > threshold) occupied |= (uint64_t)1 << cur;
                cur = sector;
                count = 0;
            }
            ++count;
        }
    }
    if (cur >= 0 && count > threshold) occupied |= (uint64_t)1 << cur;
    /* updateAction (:97-110): atan2f, / M_PI and * 180.f in fp64, narrowed */
    const float world = (float)((double)ok_atan2f(gy - py, gx - px) / 3.14159265358979323846 * (double)180.0f);
    float a = world - rot;
    a = (float)__builtin_fmod((double)a, 360.0); /* exact, so the same in either precision */
    if (a > 180.0f) a -= 360.0f;
    else if (a <= -180.0f) a += 360.0f;
    /* findBestSector (:74-93) */
    const float gs_f = (a - first) / fov * (float)ns;
    /* the cast of a value outside int's range (or NaN) is undefined in the reference: 0 here */
    const int goal_sector = (gs_f > -2147483000.0f && gs_f < 2147483000.0f) ? (int)gs_f : 0;
    int best = goal_sector; /* fallback :92 */
    for (int i = 0; i < ns; ++i) {
        int s = (int)(((long)goal_sector + i) % ns);
        if (s < 0) s += ns; /* undefined spot 1: the non-negative remainder */
        if (!((occupied >> s) & 1u)) { best = s; break; }
        s = (int)(((long)goal_sector - i + ns) % ns);
        if (s < 0) s += ns;
        if (!((occupied >> s) & 1u)) { best = s; break; }
    }
    *throttle = vfh_throttle;
    *steer = sector_width * (float)best + first; /* :115 */
}

/* tanh for the CMA-ES controller (CovarianceMatrixAdaptationEvolution/Controller.cpp:16-23), evaluated in fp64 with IEEE operations
 * and explicit FMAs only (no library call), so that the device and the CPU oracle produce the same bits -- the same idea as
 * ok_sincosf.  tanh|x| = (1 - e) / (1 + e), e = exp(-2|x|) = 2^n (1 + m), n = rint(-2|x| / ln 2), m = expm1(r), |r| <= ln 2 / 2,
 * r by two FMAs against ln 2 = L1 + L2, m = r + r^2 E(r) with E of degree 8 (interpolant at the Chebyshev nodes of +-0.347,
 * tools/fit_math.py: relative error 2^-48).  Numerator and denominator are formed from m, not from e:
 * 1 - e = (1 - 2^n) - 2^n m and 1 + e = (1 + 2^n) + 2^n m, one FMA each with 1 -+ 2^n exact -- for small |x| (n = 0) the numerator
 * is -m itself, so nothing cancels and no separate small-argument branch is needed beyond the one below.  (Rounds 1-3: Taylor
 * series of exp to r^13 by separate multiplications and additions, 1 - e by subtraction.)  tests/test_math.py: equal to the
 * rounded fp64 tanh on all but a handful of a million samples; glibc's tanhf, not correctly rounded itself, is within 2 ulps. */
OK_HD float ok_tanhf(const float x)
{
    const double ax = __builtin_fabs((double)x);
    if (!(ax >= 0.000244140625)) /* |x| < 2^-12: x^3/3 is below half an ulp of x; NaN takes this exit too and stays NaN */
        return x;
    const double y = -2.0 * (ax < 20.0 ? ax : 20.0); /* tanh(20) is 1 to 17 digits: larger arguments change nothing */
    const double n = OK_RINT(y * ok_konst(0x1.71547652b82fep+0)); /* 1 / ln 2 */
    double r = OK_FMA(-n, ok_konst(0x1.62e42fefa39efp-1), y);     /* L1 = 0.6931471805599453     */
    r = OK_FMA(-n, ok_konst(0x1.abc9e3b39803fp-56), r);           /* L2 = 2.3190468138462996e-17 */
    double p = ok_konst(0x1.28809b1a1156ep-22);           /* 2.7613934750302004e-07 */
    p = OK_FMA(p, r, ok_konst(0x1.72c7b3ac3a215p-19));    /* 2.7625269095508424e-06 */
    p = OK_FMA(p, r, ok_konst(0x1.a019c964743c8p-16));    /* 2.4801536157973374e-05 */
    p = OK_FMA(p, r, ok_konst(0x1.a019ad41ef162p-13));    /* 1.9841208455585307e-04 */
    p = OK_FMA(p, r, ok_konst(0x1.6c16c1739cf9cp-10));    /* 1.388888890599716e-03  */
    p = OK_FMA(p, r, ok_konst(0x1.1111111c5b16fp-7));     /* 8.333333353868181e-03  */
    p = OK_FMA(p, r, ok_konst(0x1.5555555554ca3p-5));     /* 4.166666666665122e-02  */
    p = OK_FMA(p, r, ok_konst(0x1.5555555553b3cp-3));     /* 1.6666666666648122e-01 */
    p = OK_FMA(p, r, 0.5);
    const double m = OK_FMA(r * r, p, r); /* expm1(r) */
    union { uint64_t u; double d; } two_n; /* 2^n, n in [-58, 0] */
    two_n.u = (uint64_t)(1023 + (int)n) << 52;
    const double num = OK_FMA(-two_n.d, m, 1.0 - two_n.d);
    const double den = OK_FMA(two_n.d, m, 1.0 + two_n.d);
    const double t = num / den;
    return (float)(x < 0.0f ? -t : t);
}

/* exp for the shared-network actors' softmax (below), for arguments <= 0: the pieces of ok_tanhf.  n = rint(x / ln 2),
 * r = x - n ln 2 by two FMAs against ln 2 = L1 + L2, |r| <= ln 2 / 2, m = expm1(r) = r + r^2 E(r) with ok_tanhf's E (relative
 * error 2^-48), exp x = 2^n (1 + m): the sum is one fp64 rounding, the scaling by 2^n is exact (n >= -289: a normal double), and the
 * conversion to fp32 is the single rounding into fp32 -- subnormal results included, the conversion rounds those correctly too.
 * Arguments below -200 count as -200 (the result is 0 from -104 on), so -inf gives 0; NaN stays NaN.  Arguments above 0 are not
 * the softmax's business: they are evaluated by the same formula up to +200 (inf from 88.73 on); tests/test_math_cases.py (host) and tests/test_gpu_math.py (device)
 * run every 256th float and the neighbourhoods of 0, of both clamps, of the first subnormal, the first normal and the first infinite
 * result and of every tie of rint: equal to the rounded fp64 exp on all of [-200, 88.7], same bits on host and device everywhere.
 * tests/test_actor_rule.py: equal to the rounded fp64 exp on all but a few of a million arguments in [-104, 0], never more than
 * one ulp away. */
OK_HD float ok_expf(const float x)
{
    if (!(x == x)) return x;
    const double xd = (double)x;
    const double y = xd < -200.0 ? -200.0 : (xd > 200.0 ? 200.0 : xd);
    const double n = OK_RINT(y * ok_konst(0x1.71547652b82fep+0)); /* 1 / ln 2 */
    double r = OK_FMA(-n, ok_konst(0x1.62e42fefa39efp-1), y);     /* L1 = 0.6931471805599453     */
    r = OK_FMA(-n, ok_konst(0x1.abc9e3b39803fp-56), r);           /* L2 = 2.3190468138462996e-17 */
    double p = ok_konst(0x1.28809b1a1156ep-22);           /* E: the coefficients of ok_tanhf */
    p = OK_FMA(p, r, ok_konst(0x1.72c7b3ac3a215p-19));
    p = OK_FMA(p, r, ok_konst(0x1.a019c964743c8p-16));
    p = OK_FMA(p, r, ok_konst(0x1.a019ad41ef162p-13));
    p = OK_FMA(p, r, ok_konst(0x1.6c16c1739cf9cp-10));
    p = OK_FMA(p, r, ok_konst(0x1.1111111c5b16fp-7));
    p = OK_FMA(p, r, ok_konst(0x1.5555555554ca3p-5));
    p = OK_FMA(p, r, ok_konst(0x1.5555555553b3cp-3));
    p = OK_FMA(p, r, 0.5);
    const double m = OK_FMA(r * r, p, r); /* expm1(r) */
    union { uint64_t u; double d; } two_n; /* 2^n, n in [-289, 289] */
    two_n.u = (uint64_t)(1023 + (int)n) << 52;
    return (float)(two_n.d * (1.0 + m));
}

/* log for REINFORCE's loss column (okenv_reinforce.h), for positive finite fp32 arguments, subnormal ones included: evaluated in fp64
 * and rounded once to fp32.  x = 2^e m with m in [sqrt(1/2), sqrt(2)) (the double's own exponent and mantissa, halved once where the
 * mantissa reaches sqrt 2), u = (m - 1) / (m + 1), |u| <= 0.1716, log m = 2 atanh u = 2 (u + u^3/3 + u^5/5 + ...): the series' own
 * coefficients 1/(2k + 1), each the correctly rounded quotient of two small integers, up to u^23 (the first term left out is below
 * 2^-59 of the sum), by Horner's rule in FMAs in z = u^2.  Then e ln 2 with ok_expf's split ln 2 = L1 + L2, the small part first.
 * Zero, negative, infinite and NaN arguments are not the loss's business (the probability is clamped to [1e-8, 1]): what they give is
 * whatever the formula gives, and tests/test_gpu_math.py holds the device to the host's bits for them too.  tests/test_math_cases.py
 * (host) and tests/test_gpu_math.py (device): equal to the rounded fp64 log on every 256th positive finite float and around 2^k and
 * sqrt 2 * 2^k for every k, subnormal arguments included.  tests/test_reinforce_rule.py: equal to the rounded fp64 log on all but a few of a million arguments in [1e-8, 1] and
 * on every binade of the positive normal floats, never more than one ulp away.  No gradient depends on it. */
OK_HD float ok_logf(const float x)
{
    union { uint64_t u; double d; } b;
    b.d = (double)x; /* exact, and a normal double for every positive fp32 number */
    double e = (double)((int)(b.u >> 52) - 1023);
    b.u = (b.u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull; /* the mantissa as a double in [1, 2) */
    double m = b.d;
    if (m >= 0x1.6a09e667f3bcdp+0) { /* sqrt 2 */
        m = m * 0.5;
        e = e + 1.0;
    }
    const double u = (m - 1.0) / (m + 1.0);
    const double z = u * u;
    double p = ok_konst(1.0 / 23.0);
    p = OK_FMA(p, z, ok_konst(1.0 / 21.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 19.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 17.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 15.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 13.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 11.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 9.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 7.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 5.0));
    p = OK_FMA(p, z, ok_konst(1.0 / 3.0));
    const double log_m = 2.0 * OK_FMA(u * z, p, u);
    double r = OK_FMA(e, ok_konst(0x1.abc9e3b39803fp-56), log_m); /* L2 = 2.3190468138462996e-17 */
    r = OK_FMA(e, ok_konst(0x1.62e42fefa39efp-1), r);             /* L1 = 0.6931471805599453     */
    return (float)r;
}

/* erf for the image transformer's GELU (okenv_vit.h), evaluated in fp64 with IEEE operations and explicit FMAs only and rounded once to
 * fp32, as ok_tanhf and ok_expf are.  Four pieces in a = |x|, each the interpolant at the Chebyshev nodes of its interval
 * (tools/fit_math.py prints the rows below and the error of the ROUNDED polynomials):
 *     a <  1:       erf a = a G(a^2), G of degree 12                       (relative error 2^-55.8; G(0) = 2 / sqrt(pi))
 *     1 <= a < 4:   erf a = H_c(a - c), c = 1.5, 2.5, 3.5, H_c of degree 17 (relative error 2^-54.2 each)
 *     a >= 4:       1 (erf 4 = 1 - 1.5e-8 rounds to 1.0f; the first argument that gives 1.0f is about 3.8325, inside the last piece)
 * all by Horner's rule in FMAs.  The branch points are 1, 2, 3 and 4.  The sign is put back at the end, so the function is odd in the
 * bits; a < 1 covers +-0 (a G = +0, negated for -0) and the subnormals (one fp64 product, then the single rounding); +-inf give +-1; NaN
 * fails every comparison and is returned as it came.  The fp64 value is within 2^-52 of erf, so the fp32 result is never more than one
 * ulp from the rounded exact value (tests/test_erf_rule.py counts the arguments where it is not equal). */
OK_HD float ok_erff(const float x)
{
    const double G[13] = {0x1.20dd750429b6dp+0, -0x1.812746b0379e6p-2, 0x1.ce2f21a042b30p-4, -0x1.b82ce31284e00p-6, 0x1.565bcd0dbaa38p-8,
                          -0x1.c02db3dac435fp-11, 0x1.f9a321d5b8e1ep-14, -0x1.f4d1e3183f7aep-17, 0x1.b9df224ca4b97p-20, -0x1.5f1ecb6f0764cp-23,
                          0x1.f7b4bf3b13964p-27, -0x1.389d4f2641625p-30, 0x1.05ffd737fb32ep-34};
    const double H[3][18] = {
        {0x1.eea5557137ae0p-1, 0x1.e723726b824a9p-4, -0x1.6d5a95d0a1b3ap-3, 0x1.1c2a02beb6a99p-3, -0x1.6d5a95d0a8e2dp-5, -0x1.e723726b75a2bp-7,
         0x1.3ca3d72e94d2cp-6, -0x1.36d73a65ecb0ap-8, -0x1.35ae4fb43b234p-9, 0x1.c0380d88e655ap-10, -0x1.85b3d151e9cfdp-14, -0x1.0acf353ecb714p-12,
         0x1.45cc7994de082p-14, 0x1.2d574ba32d17bp-16, -0x1.d70efbc5f9ed6p-17, 0x1.32b587a24f780p-21, 0x1.7c67db8e155e0p-20, -0x1.305d37a851c9dp-22},
        {0x1.ffcaa8f4c9beap-1, 0x1.1d83170fbf6fcp-9, -0x1.64e3dcd3af2d3p-8, 0x1.119da0c46cc88p-7, -0x1.1a89b97cf1214p-7, 0x1.90e81283fccadp-8,
         -0x1.6ecdbf63b4dcep-9, 0x1.1c610bc8e5f86p-11, 0x1.11551b52fb796p-12, -0x1.06717857ad0fap-12, 0x1.4a84c20123815p-14, 0x1.58bbca2bba994p-18,
         -0x1.d88c48f8a82b3p-17, 0x1.3ad68181439ecp-18, 0x1.9f3af4d2b1565p-23, -0x1.595d63766c65ep-21, 0x1.495bf0556d5dep-23, 0x1.8353e53661806p-26},
        {0x1.ffffe710d565ep-1, 0x1.6a597219a93d4p-18, -0x1.3d0e43d6734d9p-16, 0x1.62ccea63cb29ap-15, -0x1.1c07721adce45p-14, 0x1.586bafc9b36e3p-14,
         -0x1.46153fb62cc1cp-14, 0x1.e827fafc968b1p-15, -0x1.1f63056912abap-15, 0x1.013525a7dacb3p-16, -0x1.3773e12d91261p-18, 0x1.dd8021aae75eap-22,
         0x1.dc69f55490dbfp-22, -0x1.43f06e7cae34dp-22, 0x1.8ddc35b8e5308p-24, -0x1.83eccdb1df23fp-28, -0x1.343ba005050efp-27, 0x1.09106bf9376f0p-28}};
    if (!(x == x)) return x;
    const double a = __builtin_fabs((double)x);
    double r;
    if (a < 1.0) {
        const double z = a * a;
        double p = G[12];
        for (int i = 11; i >= 0; --i) p = OK_FMA(p, z, G[i]);
        r = a * p;
    } else if (a < 4.0) {
        const int piece = a < 2.0 ? 0 : (a < 3.0 ? 1 : 2);
        const double t = a - (1.5 + (double)piece);
        double p = H[piece][17];
        for (int i = 16; i >= 0; --i) p = OK_FMA(p, t, H[piece][i]);
        r = p;
    } else {
        r = 1.0;
    }
    return (float)(__builtin_signbit(x) ? -r : r);
}

/* ---- RLRacers: the shared-network actors -----------------------------------
 * updateAction of PPOAgent (RLRacers/PPO/PPOAgent.hpp:68-102 with Actor.hpp:20-27 and Critic.hpp), of the REINFORCE agent
 * (Reinforce/Policy.hpp:22-29; its Dropout is okenv_reinforce.h's, on top of this rule) and of DQAgent (Deep_Q_Learning/DQAgent.hpp:85-104, with one hidden layer): ONE
 * network for all agents, an action index per agent, a table from index to (throttle_delta, steering_delta).  libtorch's summation
 * order, its softmax and its multinomial are not pinned, so the rule is written out here; csrc/ok_actor.h's kernel and
 * okenv_actor_act_host both evaluate THESE functions, so they agree bit for bit.
 *
 *   input     x[i] = dist[i] / 200.0f (OK_SENSOR_RANGE), one IEEE fp32 division: what sensor_hits_[i].norm() / kSensorRange is in
 *             the reference's C++ (PPOAgent.hpp:66-74) and what torch computes on the CPU.  (On the GPU torch divides a tensor
 *             by a scalar as a multiplication by the rounded reciprocal, so VectorEnvironment.observation() can differ from this
 *             in the last place or two; the recorded state is the division's.)
 *   networks  policy R -> H -> A and, optionally, value R -> Hv -> 1, ReLU after the hidden layer (relu(s) = s > 0 ? s : 0, so a
 *             NaN sum gives 0).  Parameters in the order of torch's parameters(): l1.weight [H][R] row-major, l1.bias [H],
 *             l2.weight [A][H], l2.bias [A].  1 <= R <= 64, 1 <= H <= 256, 2 <= A <= 8, 0 <= Hv <= 256 (0: no value network).
 *   sums      fp32, a separate multiplication and addition per term, nothing fused.
 *             hidden unit j:  s = b1[j]; s = s + w1[j][i] * x[i] for i = 0 .. R-1 ascending; h[j] = relu(s).
 *             output k: OK_ACTOR_LANES = 8 interleaved partial sums joined by a fixed tree (the choice the kernel's lane groups
 *             want; it does not depend on the launch shape or on N):
 *               part_l = 0.0f; part_l = part_l + w2[k][j] * h[j] for j = l, l + 8, l + 16, ... < H ascending      (l = 0 .. 7)
 *               z_k = b2[k] + (((part_0 + part_4) + (part_2 + part_6)) + ((part_1 + part_5) + (part_3 + part_7)))
 *             (the butterfly over lane distances 4, 2, 1; IEEE addition commutes, so every lane of a group holds these bits).
 *   softmax   m = max z (the lowest index wins ties), e_k = ok_expf(z_k - m), s = e_0 + e_1 + ... ascending, p_k = e_k / s (IEEE
 *             division), then p_k clamped to [1e-8f, 1.0f]: kProbClamp (PPOAgent.hpp:27,88) is clamp(probs, 1e-8, 1.0 - 1e-8),
 *             and the upper limit 1.0 - 1e-8 is 1.0f once it is an fp32 number, which is what torch compares a float tensor with.
 *             A NaN p_k stays NaN (both comparisons are false).
 *   draws     one Philox block per (seed, global agent id, draw index): counter = (agent, draw, 6, 0), key = (seed, "oken").
 *             Stream 6 is used by nothing else (0: C2 actions, 1: resets and GA weights, 2 / 3: GA mating, 4: Q-learning, 5:
 *             q_racer_sim's episode draws; 7: Deep-Q's sampling, okenv_dqn.h; 8: DDPG's exploration, okenv_ddpg.h; 9: REINFORCE's
 *             dropout masks, okenv_reinforce.h; 10: the Gaussian actor's normal draws, okenv_gauss.h; 11: guided cost learning's
 *             normal draws and 12: its expert rows, okenv_gcl.h; 13: the flow-matching driver's noise, okenv_flow.h).
 *   modes     OK_ACTOR_SAMPLE (PPO, REINFORCE): u = ok_u01(word 0); the action is the first k with u < p_0 + ... + p_k (fp32
 *             sums of the clamped p, ascending), A - 1 if there is none.  Recorded: the clamped p of the action.
 *             OK_ACTOR_GREEDY (evaluation): the arg-max of z, lowest index on ties.  Recorded: the clamped p of the action.
 *             OK_ACTOR_EPS_GREEDY (DQAgent.hpp:89-99): ok_u01(word 0) < epsilon picks ok_index_from_word(word 1, A), otherwise the
 *             arg-max of z.  No softmax; recorded: z of the action.
 * The logarithm is the learner's: torch.log over the recorded [T, N] probabilities gives log_probs once per episode. */
#define OK_ACTOR_SAMPLE 0
#define OK_ACTOR_GREEDY 1
#define OK_ACTOR_EPS_GREEDY 2
#define OK_ACTOR_MAX_RAYS 64
#define OK_ACTOR_MAX_HIDDEN 256
#define OK_ACTOR_MAX_ACTIONS 8
#define OK_ACTOR_LANES 8
#define OK_ACTOR_PROB_MIN 1e-8f
#define OK_ACTOR_PROB_MAX 1.0f /* (float)(1.0 - 1e-8) */

OK_HDI int ok_actor_num_params(const int in, const int hidden, const int out)
{
    return hidden * in + hidden + out * hidden + out;
}

/* The partial sums of interleave lane l for every output: part[k] over the hidden units j = l, l + 8, ... of a network whose first
 * layer's rows lie `w1_stride` floats apart (R in a parameter vector; the kernel pads its copy).  part has OK_ACTOR_MAX_ACTIONS
 * entries; those from `out` on are left alone. */
OK_HDI void ok_actor_partial(const float *w1, const int w1_stride, const float *b1, const float *w2, const int in, const int hidden, const int out,
                            const float *x, const int l, float *part)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < out) part[k] = 0.0f;
    for (int j = l; j < hidden; j += OK_ACTOR_LANES) {
        const float *row = w1 + j * w1_stride;
        float s = b1[j];
        for (int i = 0; i < in; ++i) s = s + row[i] * x[i];
        const float h = s > 0.0f ? s : 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
            if (k < out) part[k] = part[k] + w2[k * hidden + j] * h;
    }
}

/* The fixed tree over the eight partial sums, then the bias */
OK_HDI float ok_actor_join(const float *p, const float bias)
{
    return bias + (((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7])));
}

/* index of the largest of z[0 .. n-1], the lowest index on ties (NaN never wins) */
OK_HDI int ok_actor_argmax(const float *z, const int n)
{
    int best = 0;
    float m = z[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n && z[k] > m) { m = z[k]; best = k; }
    return best;
}

OK_HDI float ok_actor_clamp_prob(const float p)
{
    return p < OK_ACTOR_PROB_MIN ? OK_ACTOR_PROB_MIN : (p > OK_ACTOR_PROB_MAX ? OK_ACTOR_PROB_MAX : p);
}

/* From the exponentials e_k = ok_expf(z_k - max z) to the action and the recorded probability of OK_ACTOR_SAMPLE (u given) and
 * OK_ACTOR_GREEDY (`greedy` = the arg-max of z, or -1 to sample). */
OK_HDI int ok_actor_pick(const float *e, const int n, const float u, const int greedy, float *prob)
{
    float s = e[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n) s = s + e[k];
    int action = greedy >= 0 ? greedy : n - 1;
    int found = greedy >= 0;
    float cum = 0.0f, pa = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n) {
            const float pk = ok_actor_clamp_prob(e[k] / s);
            cum = k == 0 ? pk : cum + pk;
            if (!found && u < cum) { action = k; found = 1; }
            if (k == action) pa = pk; /* (k never passes a later `action`: it is either fixed or n - 1 until found) */
        }
    *prob = pa;
    return action;
}

/* The two words of the action draw */
OK_HDI ok_u32x4 ok_actor_draw(const uint32_t seed, const uint32_t agent, const uint32_t draw)
{
    return ok_philox4x32(agent, draw, 6u, 0u, seed, 0x6F6B656Eu);
}

/* OK_ACTOR_EPS_GREEDY: the action from the arg-max of the logits (its recorded value is z[action], the caller's to look up) */
OK_HDI int ok_actor_eps_greedy(const float epsilon, const uint32_t seed, const uint32_t agent, const uint32_t draw, const int n, const int best)
{
    const ok_u32x4 r = ok_actor_draw(seed, agent, draw);
    return ok_u01(r.v[0]) < epsilon ? (int)ok_index_from_word(r.v[1], (uint32_t)n) : best;
}

/* From the logits to the action: every mode.  z has OK_ACTOR_MAX_ACTIONS entries, n of them used. */
OK_HDI int ok_actor_choose(const int mode, const float epsilon, const uint32_t seed, const uint32_t agent, const uint32_t draw, const float *z,
                          const int n, float *prob)
{
    const int best = ok_actor_argmax(z, n);
    if (mode == OK_ACTOR_EPS_GREEDY) {
        const int action = ok_actor_eps_greedy(epsilon, seed, agent, draw, n, best);
        *prob = z[action];
        return action;
    }
    float e[OK_ACTOR_MAX_ACTIONS];
    float m = z[0]; /* = z[best], without an indexed read of a register array */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k < OK_ACTOR_MAX_ACTIONS; ++k)
        if (k < n && z[k] > m) m = z[k];
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k)
        e[k] = k < n ? ok_expf(z[k] - m) : 0.0f;
    float u = 0.0f;
    if (mode == OK_ACTOR_SAMPLE) u = ok_u01(ok_actor_draw(seed, agent, draw).v[0]);
    return ok_actor_pick(e, n, u, mode == OK_ACTOR_GREEDY ? best : -1, prob);
}

/* One agent on the host (and the reading the kernel's lane groups split up): x from dist, both networks, the choice.
 * `value_out` is written only when value_hidden > 0. */
OK_HD int ok_actor_agent(const float *policy, const float *value, const int in, const int hidden, const int n_actions, const int value_hidden,
                         const int mode, const float epsilon, const uint32_t seed, const uint32_t agent, const uint32_t draw, const float *dist,
                         float *x, float *prob, float *value_out)
{
    for (int i = 0; i < in; ++i) x[i] = dist[i] / OK_SENSOR_RANGE;
    float part[OK_ACTOR_LANES][OK_ACTOR_MAX_ACTIONS], col[OK_ACTOR_LANES], z[OK_ACTOR_MAX_ACTIONS];
    const float *b1 = policy + hidden * in, *w2 = b1 + hidden, *b2 = w2 + n_actions * hidden;
    for (int l = 0; l < OK_ACTOR_LANES; ++l) ok_actor_partial(policy, in, b1, w2, in, hidden, n_actions, x, l, part[l]);
    for (int k = 0; k < OK_ACTOR_MAX_ACTIONS; ++k) {
        for (int l = 0; l < OK_ACTOR_LANES; ++l) col[l] = k < n_actions ? part[l][k] : 0.0f;
        z[k] = k < n_actions ? ok_actor_join(col, b2[k]) : 0.0f;
    }
    if (value_hidden > 0) {
        const float *vb1 = value + value_hidden * in, *vw2 = vb1 + value_hidden, *vb2 = vw2 + value_hidden;
        for (int l = 0; l < OK_ACTOR_LANES; ++l) {
            ok_actor_partial(value, in, vb1, vw2, in, value_hidden, 1, x, l, part[l]);
            col[l] = part[l][0];
        }
        *value_out = ok_actor_join(col, vb2[0]);
    }
    return ok_actor_choose(mode, epsilon, seed, agent, draw, z, n_actions, prob);
}

/* One candidate's controller (Controller.cpp:3-23: fc1 in->h, fc2 h->h/2, fc3 h/2->out, tanh after each) on the input
 * CmaEsAgent::stateToTensor builds (main_eigen.cpp:45-56: ||sensor_hits_[i]|| / kSensorRange).  `params` in the order of
 * torch's parameters(): fc1.weight [h][in] row-major, fc1.bias [h], fc2.weight [h/2][h], fc2.bias, fc3.weight [out][h/2],
 * fc3.bias (Controller.cpp:36-53).  A unit's sum starts from its bias and adds w * x in ascending input order, fp32, no
 * FMA (libtorch's own order inside addmm is not specified): okControllerKernel on the device, ctrl_forward in the oracle.
 * h <= 64. */
#define OK_CTRL_MAX_HIDDEN 64
OK_HD int ok_controller_num_params(const int in, const int hidden, const int out)
{
    const int h2 = hidden / 2;
    return hidden * in + hidden + h2 * hidden + h2 + out * h2 + out;
}
/* nn_output > kOutputActivationLim (GeneticAgent.hpp:45-54) on a PRE-activation z, where nn_output = sigmoid(z) =
 * 1.F / (1.F + exp(-z)) in fp32 (Network.hpp:162-165).  The quotient exceeds 0.5 exactly when the rounded sum 1 + exp(-z)
 * is below 2, i.e. when exp(-z) rounds to 1 - 2^-23 or less, i.e. when exp(-z) <= 1 - 1.5 * 2^-24 (the tie goes to the even
 * neighbour, 1 - 2^-23), i.e. when z >= -ln(1 - 1.5 * 2^-24) = 1.5 * 2^-24 + 4.0e-15: the first float at or above that is
 * 0x33C00001.  So the test is one comparison, with the bits of an fp32 sigmoid whose exp is correctly rounded there (glibc's
 * expf is: tests/test_math.py compares the two over every float around the threshold).  For 0 < z < 8.94e-8 the sigmoid is
 * exactly 0.5 and the output is NOT active. */
OK_HD int ok_sigmoid_above_half(const float z)
{
    union { uint32_t u; float f; } t;
    t.u = 0x33C00001u;
    return z >= t.f; /* false for NaN, like the comparison with the sigmoid */
}

/* GeneticAgent::updateAction's decode (EvolutionaryRacer/GeneticAgent.hpp:45-54) from the six pre-activations z. */
OK_HD void ok_ga_decode_action(const float z[OK_MLP_OUT], float *throttle, float *steer)
{
    float t = 0.0f, s = 0.0f;
    t += ok_sigmoid_above_half(z[0]) ? 0.3f : 0.0f;
    t += ok_sigmoid_above_half(z[1]) ? -0.3f : 0.0f;
    s += ok_sigmoid_above_half(z[2]) ? 1.0f : 0.0f;
    s += ok_sigmoid_above_half(z[3]) ? 4.0f : 0.0f;
    s += ok_sigmoid_above_half(z[4]) ? -1.0f : 0.0f;
    s += ok_sigmoid_above_half(z[5]) ? -4.0f : 0.0f;
    *throttle = t;
    *steer = s;
}

/* Deterministic stand-ins for the reference's unseeded generators (Eigen Random(), std::random_device):
 * initial weight w of agent a:      U[-1,1) from Philox(counter = (a, w, 1, 0), key = (seed, "oken"))
 * mating draws of offspring o, weight w in generation g: Philox(counter = (o, w, 2, g)) -> u_mutate, u_value, u_parent
 * parent choice of offspring o in generation g:          Philox(counter = (o, try, 3, g)) */
OK_HD float ok_ga_initial_weight(uint32_t seed, uint32_t agent, uint32_t w)
{
    const ok_u32x4 r = ok_philox4x32(agent, w, 1u, 0u, seed, 0x6F6B656Eu);
    return ok_u01(r.v[0]) * 2.0f - 1.0f;
}

/* Parent choice (EvolutionaryRacer/Mating.hpp:128-152): offspring 0 clones the best, offspring 1 mates the best with
 * itself, every other offspring draws two DIFFERENT parents with probability proportional to the parents' scores
 * (std::discrete_distribution; uniform when every score is zero).  ps[] = scores of the K best agents, best first.
 * Returns first | second << 8, bit 16 = exact clone. */
OK_HD uint32_t ok_ga_pick_parent(const float *ps, int K, float u)
{
    float total = 0.0f;
    for (int k = 0; k < K; ++k) total += (ps[k] > 0.0f ? ps[k] : 0.0f);
    if (!(total > 0.0f)) {
        const int k = (int)(u * (float)K);
        return (uint32_t)(k < K ? k : K - 1);
    }
    const float x = u * total;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
        acc += (ps[k] > 0.0f ? ps[k] : 0.0f);
        if (x < acc) return (uint32_t)k;
    }
    return (uint32_t)(K - 1);
}

OK_HD uint32_t ok_ga_parent_pair(const float *ps, int K, uint32_t seed, uint32_t offspring, uint32_t generation)
{
    if (offspring == 0u) return 0u | (0u << 8) | (1u << 16); /* clone of the best */
    if (offspring == 1u || K < 2) return 0u | (0u << 8);     /* best mated with itself: mutations only */
    const ok_u32x4 r0 = ok_philox4x32(offspring, 0u, 3u, generation, seed, 0x6F6B656Eu);
    const uint32_t first = ok_ga_pick_parent(ps, K, ok_u01(r0.v[0]));
    uint32_t second = first;
    for (uint32_t attempt = 1u; attempt <= 16u && second == first; ++attempt) {
        const ok_u32x4 r = ok_philox4x32(offspring, attempt, 3u, generation, seed, 0x6F6B656Eu);
        second = ok_ga_pick_parent(ps, K, ok_u01(r.v[0]));
    }
    if (second == first) second = (first + 1u) % (uint32_t)K; /* all but impossible; keeps "two different parents" */
    return first | (second << 8);
}

/* true for the real entries of the padded per-agent weight block (index i in [0, OK_MLP_WEIGHTS(R))) */
OK_HD int ok_mlp_weight_is_real(uint32_t i, int R, int H)
{
    const uint32_t n1 = (uint32_t)((R + 2) * OK_MLP_HID_PAD);
    if (i < n1) return (int)((i % OK_MLP_HID_PAD) < (uint32_t)H);
    const uint32_t q = i - n1;
    return (int)((q / OK_MLP_OUT_PAD) < (uint32_t)H && (q % OK_MLP_OUT_PAD) < OK_MLP_OUT);
}

/* ---- RLRacers/Q_Learning ------------------------------------------------ */

#define OK_Q_STATES 243 /* 5 rays x 3 proximity bins, QAgent.hpp:31-34 */
#define OK_Q_ACTIONS 3
#define OK_Q_INVALID (-3.40282346638528859811704183484516925e+38f) /* numeric_limits<float>::lowest(), QAgent.hpp:36 */

/* QLearnAgent::discretizeState's bin of one ray (QAgent.hpp:72-94): < 5 -> 0, < 10 -> 1, else 2 */
OK_HD int ok_q_bin(float ray_dist)
{
    return (ray_dist < 5.0f) ? 0 : ((ray_dist < 10.0f) ? 1 : 2);
}

/* index of the largest of three values, the first on ties (std::max_element, QAgent.hpp:108-110) */
OK_HD int ok_q_argmax3(float q0, float q1, float q2)
{
    int idx = 0;
    float m = q0;
    if (q1 > m) { m = q1; idx = 1; }
    if (q2 > m) { idx = 2; }
    return idx;
}

/* Epsilon-greedy draw (QAgent.hpp:98-119) with Philox(counter = (agent, step, 4, 0)) standing in for raylib's
 * GetRandomValue: explore iff u0 < epsilon, random action = min(2, floor(3 u1)). */
OK_HD int ok_q_choose_action(uint32_t seed, uint32_t agent, uint32_t step, float epsilon, float q0, float q1, float q2)
{
    const ok_u32x4 r = ok_philox4x32(agent, step, 4u, 0u, seed, 0x6F6B656Eu);
    if (ok_u01(r.v[0]) < epsilon) {
        const int a = (int)(ok_u01(r.v[1]) * 3.0f);
        return a > 2 ? 2 : a;
    }
    return ok_q_argmax3(q0, q1, q2);
}

/* The part of that draw that does not depend on the Q values: -1 = exploit (take the argmax), else the random action.  For
 * callers that make many steps' draws at once (okQSettleKernel); ok_q_choose_action == (d < 0 ? argmax3 : d). */
OK_HD int ok_q_draw_action(uint32_t seed, uint32_t agent, uint32_t step, float epsilon)
{
    const ok_u32x4 r = ok_philox4x32(agent, step, 4u, 0u, seed, 0x6F6B656Eu);
    if (ok_u01(r.v[0]) < epsilon) {
        const int a = (int)(ok_u01(r.v[1]) * 3.0f);
        return a > 2 ? 2 : a;
    }
    return -1;
}

/* kActionMap (QAgent.hpp:40-42): 0 -> (60, 0), 1 -> (30, +5), 2 -> (30, -5) */
OK_HD void ok_q_action_values(int action, float *throttle, float *steer)
{
    *throttle = (action == 0) ? 60.0f : 30.0f;
    *steer = (action == 0) ? 0.0f : ((action == 1) ? 5.0f : -5.0f);
}

/* QLearnAgent::reward (QAgent.hpp:150-168); *prev_idx is updated only when the agent has not crashed */
OK_HD float ok_q_reward(int crashed, int nearest_idx, int *prev_idx, int track_len)
{
    if (crashed) return -200.0f;
    int progression = nearest_idx - *prev_idx;
    *prev_idx = nearest_idx;
    if (progression < 0) progression = -progression;
    return (float)((progression > track_len / 2) ? track_len - progression : progression);
}

/* QLearnAgent::learn (QAgent.hpp:121-138): returns the new Q(s, a) */
OK_HD float ok_q_learn(float old_q, float max_q_next, float reward)
{
    const float target = reward + 0.8f * max_q_next;
    if (old_q == OK_Q_INVALID || max_q_next == OK_Q_INVALID) return reward;
    return old_q + 0.2f * (target - old_q);
}

#endif /* OKENV_MATH_H */
