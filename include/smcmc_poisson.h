/* smcmc_poisson.h -- the Poisson variate of the posterior-predictive check (include/smcmc.h states it under
 * smcmc_predictive_check), one copy for the device kernel (smcmc_predictive_check.hip) and for the host entry point
 * smcmc_poisson_draw.  The reference draws no replicated data, so this definition IS the engine's.
 *
 * It is inversion of the cumulative distribution, term by term: exact in distribution up to the rounding of the terms
 * (far below the 2^-52 resolution of the uniform times the number of terms), a function of its inputs alone, and built
 * only from smcmc_exp of smcmc_detmath.h, __builtin_sqrt, + - * / and the truncation of a positive double, all
 * un-fused: the same bits on the host and on gfx950.  Compile with -ffp-contract=off.  Its cost is O(sqrt(mu)) terms;
 * what that buys is that every single draw can be checked against the exact cumulative distribution
 * (tests/poisson_truth.py), which a rejection sampler does not allow.
 *
 *   mean      mu = expectation < 0.001 ? 0.001 : expectation, the clamp of smcmc_es_bin_term (smcmc_event_sample.h): the
 *             model the likelihood asserts.  INVALID, and nothing is drawn: an expectation that is NaN, +inf or -inf, or
 *             mu > SMCMC_POISSON_MAX_MEAN = 2^20.
 *   block     smcmc_draw_block(seed, chain, step, 0, SMCMC_STREAM_REPLICA), chain the global chain number and
 *             step = slot | row << 28 | replica << 44   (slot < 2^28 the global slot, row < 2^16, replica < 2^16):
 *             one block per variate, words 2 and 3 unused.
 *   uniform   u = ((w0 * 2^20 + (w1 >> 12)) + 0.5) * 2^-52 from words 0 and 1: 52 bits, so that the half is still exact
 *             in binary64 (2 n + 1 < 2^53) and u lies in [2^-53, 1 - 2^-53], never 0 or 1.
 *   mu < 16   inversion from 0:  p = smcmc_exp(-mu), k = 0;  repeat  u -= p;  if (u <= 0) return k;  ++k;
 *             p = (p * mu) / k;  if (p == 0 and k > mu) return k  (the rounding guard: the terms have run out before u).
 *             Bound: p_k <= 16^k / k! is 0 in binary64 long before k = SMCMC_POISSON_SMALL_STEPS = 1024, which ends the loop.
 *   mu >= 16  inversion in the order m, m + 1, m - 1, m + 2, m - 2, ... from the mode m = floor(mu):
 *               p_m = smcmc_exp(-stirlerr(m) - bd0(m, mu)) / sqrt(6.283185307179586 m)         Loader's saddle-point form
 *               stirlerr(m) = (1/12 - (1/360 - (1/1260 - (1/1680 - (1/1188) / m^2) / m^2) / m^2) / m^2) / m
 *               bd0(m, mu) = m ln(m / mu) + mu - m by its series in v = (m - mu) / (m + mu), |v| < 1/32 here:
 *                 s = (m - mu) v, e = 2 m v, w = v v;  for j = 1 ..: e *= w, s' = s + e / (2 j + 1), stop when s' == s.
 *                 Bound: a term is below 2^-10 of the one before, so the sum stands still by j = 7; the loop ends at
 *                 j = SMCMC_POISSON_BD0_TERMS = 16.
 *               t = 1, 2, ...:  p_(m+t) = (p_(m+t-1) * mu) / (m + t);  u -= it;  if (u <= 0) return m + t;
 *                               while t <= m:  p_(m-t) = (p_(m-t+1) * (m - t + 1)) / mu;  u -= it;  if (u <= 0) return m - t;
 *                               once t > m (the downward side has passed 0): if (p_(m+t) < 1e-300) return m + t  (the
 *                               rounding guard).
 *               u -= p_m and its test come first.  Bound: above 2 m a term is below 17/32 of the one before, so it is
 *               below 1e-300 within 1100 terms of t = m: the loop ends at t = m + SMCMC_POISSON_TAIL_STEPS = m + 2048.
 */
#ifndef SMCMC_POISSON_H_SEEN
#define SMCMC_POISSON_H_SEEN

#include "smcmc_detmath.h"

#ifndef SMCMC_POISSON_MAX_MEAN
#define SMCMC_POISSON_MAX_MEAN 1048576.0
#endif
#define SMCMC_POISSON_MIN_MEAN 0.001
#define SMCMC_POISSON_SPLIT 16.0
#define SMCMC_POISSON_SMALL_STEPS 1024
#define SMCMC_POISSON_BD0_TERMS 16
#define SMCMC_POISSON_TAIL_STEPS 2048
#define SMCMC_POISSON_MAX_SLOT (1u << 28)      /* slot_offset + nslots <= this */
#define SMCMC_POISSON_MAX_ROW (1u << 16)       /* row < this */
#define SMCMC_POISSON_MAX_REPLICA (1u << 16)   /* replica < this */

/* nonzero when a variate is drawn at `expectation`: finite, and not above the largest mean */
SMCMC_HD int smcmc_poisson_valid(double expectation) {
    return expectation >= -1.7976931348623157e308 && expectation <= SMCMC_POISSON_MAX_MEAN;
}

SMCMC_HD double smcmc_poisson_mean(double expectation) {
    return expectation < SMCMC_POISSON_MIN_MEAN ? SMCMC_POISSON_MIN_MEAN : expectation;
}

SMCMC_HD uint64_t smcmc_poisson_step(uint32_t slot, uint32_t row, uint32_t replica) {
    return (uint64_t)slot | ((uint64_t)row << 28) | ((uint64_t)replica << 44);
}

SMCMC_HD double smcmc_poisson_uniform(uint32_t w0, uint32_t w1) {
    const uint64_t n = ((uint64_t)w0 << 20) | (uint64_t)(w1 >> 12);
    return ((double)n + 0.5) * 2.220446049250313080847263336181640625e-16;   /* 2^-52 */
}

SMCMC_HD double smcmc_poisson_small(double mu, double u) {
    double p = smcmc_exp(-mu);
    for (int k = 0; k < SMCMC_POISSON_SMALL_STEPS;) {
        u -= p;
        if (u <= 0.0) return (double)k;
        ++k;
        p = (p * mu) / (double)k;
        if (p == 0.0 && (double)k > mu) return (double)k;
    }
    return (double)SMCMC_POISSON_SMALL_STEPS;
}

SMCMC_HD double smcmc_poisson_stirlerr(double m) {
    const double m2 = m * m;
    return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) / m2) / m2) / m2) / m2) / m;
}

SMCMC_HD double smcmc_poisson_bd0(double m, double mu) {
    const double d = m - mu;
    double v = d / (m + mu);
    double s = d * v;
    double e = (2.0 * m) * v;
    v = v * v;
    for (int j = 1; j <= SMCMC_POISSON_BD0_TERMS; ++j) {
        e = e * v;
        const double s1 = s + e / (double)(2 * j + 1);
        if (s1 == s) return s1;
        s = s1;
    }
    return s;
}

SMCMC_HD double smcmc_poisson_large(double mu, double u) {
    const int mi = (int)mu;                     /* floor: 16 <= mu <= 2^20 */
    const double m = (double)mi;
    const double pm = smcmc_exp(-smcmc_poisson_stirlerr(m) - smcmc_poisson_bd0(m, mu)) / __builtin_sqrt(6.283185307179586 * m);
    u -= pm;
    if (u <= 0.0) return m;
    double pu = pm, pd = pm;
    const int last = mi + SMCMC_POISSON_TAIL_STEPS;
    for (int t = 1; t <= last; ++t) {
        pu = (pu * mu) / (double)(mi + t);
        u -= pu;
        if (u <= 0.0) return (double)(mi + t);
        if (t <= mi) {
            pd = (pd * (double)(mi - t + 1)) / mu;
            u -= pd;
            if (u <= 0.0) return (double)(mi - t);
        } else if (pu < 1e-300) {
            return (double)(mi + t);
        }
    }
    return (double)(mi + last);
}

/* the variate at a valid expectation from the uniform u */
SMCMC_HD double smcmc_poisson_from_uniform(double expectation, double u) {
    const double mu = smcmc_poisson_mean(expectation);
    return mu < SMCMC_POISSON_SPLIT ? smcmc_poisson_small(mu, u) : smcmc_poisson_large(mu, u);
}

/* the uniform of (seed, chain, slot, row, replica): chain and slot are the global ones */
SMCMC_HD double smcmc_poisson_uniform_at(uint64_t seed, uint32_t chain, uint32_t slot, uint32_t row, uint32_t replica) {
    const smcmc_u32x4 b = smcmc_draw_block(seed, chain, smcmc_poisson_step(slot, row, replica), 0u, SMCMC_STREAM_REPLICA);
    return smcmc_poisson_uniform(b.v[0], b.v[1]);
}

/* The variate of (seed, chain, slot, row, replica) at `expectation`; returns 0 and NaN when it is invalid. */
SMCMC_HD int smcmc_poisson_variate(uint64_t seed, uint32_t chain, uint32_t slot, uint32_t row, uint32_t replica,
                                   double expectation, double* y) {
    if (!smcmc_poisson_valid(expectation)) {
        *y = __builtin_nan("");
        return 0;
    }
    *y = smcmc_poisson_from_uniform(expectation, smcmc_poisson_uniform_at(seed, chain, slot, row, replica));
    return 1;
}

#endif
