// smcmc_perchain_wg.hip.h -- SMCMC_MODE_PER_CHAIN with ONE CHAIN PER WORKGROUP: the reference's own mode (every chain
// its own running centre, covariance and decomposition, UpdateState every step, TSimpleMCMC.H:1721-1831, and
// UpdateProposal on the chain's own --fNextUpdate schedule, :1009-1106) above the 63 dimensions the two other kernels
// serve (smcmc_perchain_kernel.hip.h, smcmc_perchain_wave.hip.h), up to kWgMaxDim.
//
// A workgroup of 512 threads (8 wavefronts, 2 per SIMD: one workgroup per CU) holds one chain on chip for a whole launch:
//   * the packed covariance AND the upper-triangular decomposition in registers, NE doubles of each per thread.  Slot
//     s = thread + 512 r holds U(a, b), a <= b, at s = a D - a (a - 1) / 2 + (b - a) (U row major), and next to it the
//     covariance element (b, a) -- so a block of rows of U is a contiguous range of slots, and UpdateProposal's Cholesky
//     runs in place in the U registers from a copy of the covariance;
//   * thread i < D owns x[i], the running centre c[i], fLastPoint[i] and the proposal x'[i], and draws r_i;
//   * the proposal x'[j] = x[j] + sum_{i <= j} (sigma r_i) U(i, j), i ascending, un-fused: the threads that hold rows
//     [32 q, 32 q + 32) of U put their products in a double-buffered LDS panel, and thread j adds its column's entries
//     in row order;
//   * what the reference sums in index order (the trial step's square sum, the likelihood, the covariance trace): every
//     thread i forms term i, and every thread adds the terms one after the other from LDS, the reads issued ahead;
//   * UpdateProposal's scalar half replicated in every thread (the same numbers everywhere); the Cholesky right-looking
//     over the workgroup: every element takes row c's subtraction as soon as row c is finished -- the subtractions of
//     SharedProposal::cholesky in its order, the same bits.  A failed pivot stops the chain for the host's ladder.
// The HBM images are those of the other two kernels (a launch reads the chain's state at its start and writes it back
// at its end); the per-chain scalar columns, the chain's scalar step and the stop / resume protocol are the one
// statement of smcmc_perchain_scalars.hip.h, so the host side does not know which kernel ran.
//
// Reference-order arithmetic only (compile with -ffp-contract=off).
#pragma once

#include "smcmc_perchain_limits.h"
#include "smcmc_perchain_wave.hip.h"

namespace smcmc {

constexpr int kWgVec = 256;                  // LDS vectors of one value per coordinate; index 255 is the idle slots' dummy
constexpr int kWgPanelRows = 32;             // rows of U per proposal panel
constexpr int kWgCols = 208;                 // row pitch of a panel (>= kWgMaxDim)
static_assert(kWgMaxDim < 255 && kWgCols >= kWgMaxDim && 3 * kWgMaxDim + kPcRecScalars <= 2 * kWgPanelRows * kWgCols, "LDS sizes");

// registers of packed covariance per thread for dimension D (0: not served)
inline int perchain_wg_elements(int D) {
    const int need = (D * (D + 1) / 2 + kWgThreads - 1) / kWgThreads;
    return need <= 8 ? 8 : need <= 16 ? 16 : need <= kWgMaxNE ? kWgMaxNE : 0;
}

// start of row a of U in the row-major packing of the upper triangle
__host__ __device__ inline int wg_row_start(int a, int D) { return a * D - a * (a - 1) / 2; }

// (row, column) of U for slot m < D (D + 1) / 2 of the row-major packing
__device__ __forceinline__ void wg_unpack(int m, int D, int& a, int& b) {
    const double t = 2.0 * D + 1.0;
    a = (int)((t - __builtin_sqrt(t * t - 8.0 * (double)m)) * 0.5);
    if (a < 0) a = 0;
    while (a > 0 && wg_row_start(a, D) > m) --a;
    while (wg_row_start(a + 1, D) <= m) ++a;
    b = a + (m - wg_row_start(a, D));
}

// s0 + arr[0] + arr[1] + ... + arr[n - 1], one addition after the other (the reference's loops over the dimensions);
// every thread reads the terms (LDS broadcast), a batch of 8 at a time.  arr: kWgVec
// doubles, 16-byte aligned.
constexpr int kWgBatch = 8;
__device__ __forceinline__ void wg_fetch(const double* arr, int i0, double (&v)[kWgBatch]) {
    const lds_cptr_f64x2 a2 = (lds_cptr_f64x2)(uintptr_t)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) const double*)(arr + i0);
#pragma unroll
    for (int k = 0; k < kWgBatch / 2; ++k) {
        const f64x2 w = a2[k];
        v[2 * k] = w[0];
        v[2 * k + 1] = w[1];
    }
}
__device__ __forceinline__ double wg_sum_lds(const double* arr, int n, double s0 = 0.0) {
    double s = s0;
    for (int i0 = 0; i0 < n; i0 += kWgBatch) {
        double v[kWgBatch];
        wg_fetch(arr, i0, v);
        if (i0 + kWgBatch <= n) {
#pragma unroll
            for (int u = 0; u < kWgBatch; ++u) s += v[u];
        } else {
#pragma unroll
            for (int u = 0; u < kWgBatch; ++u)
                if (i0 + u < n) s += v[u];
        }
    }
    return s;
}
// t: this thread's term; threads from n on contribute nothing.  scratch: kWgVec doubles of LDS.
__device__ __forceinline__ double wg_ordered_sum(double t, int n, double* scratch, double s0 = 0.0) {
    __syncthreads();
    if ((int)threadIdx.x < n) scratch[threadIdx.x] = t;
    __syncthreads();
    return wg_sum_lds(scratch, n, s0);
}

// A compiler barrier for memory: the loops over a thread's NE slots read LDS for every slot, and left alone the compiler
// issues all those reads ahead of the arithmetic -- 2 NE doubles live at once on top of the 2 NE of the chain's matrices,
// which spills.  Groups of 8 slots keep enough reads in flight.
__device__ __forceinline__ void wg_fence() { asm volatile("" ::: "memory"); }

// the point in LDS as a user likelihood indexes it (smcmc_user_loglike_at)
struct WgLdsPoint {
    const double* v;
    __device__ __forceinline__ double operator[](int i) const { return v[i]; }
};

// log L of the proposal: p[0 .. D) of an LDS vector of VEC doubles, pi this thread's coordinate of it; the arithmetic of
// pw_loglike
template <int LIKE, int VEC>
__device__ __forceinline__ double wg_loglike(const double* p, double pi, int D, const double* __restrict__ like, const QuadCsr& csr,
                                             double* scratch) {
    const int t = threadIdx.x;
    double lsum = 0.0;
    if constexpr (LIKE == SMCMC_LIKE_ISO_GAUSS) {
        const double h = -0.5 * pi;
        lsum = wg_ordered_sum(h * pi, D, scratch);
    } else if constexpr (LIKE == SMCMC_LIKE_QUADFORM) {
        bool dense = csr.rowptr == nullptr;
        if (!dense) {
            lsum = quadform_csr<true>([&](int j) { return p[j]; }, csr, D);
            dense = !__builtin_isfinite(lsum);
        }
        if (dense) {
            // TDummyLogLikelihood.H:24-28: logL -= 0.5 p[i] Error(j, i) p[j], i outer, j inner, un-fused
            const cptr_f64 et = as_const(like);
            lsum = 0.0;
            for (int i = 0; i < D; ++i) {
                const double h = 0.5 * p[i];
                const cptr_f64 erow = et + (size_t)i * D;
                int j = 0;
                for (; j + kPwBatch <= D; j += kPwBatch) {
                    double pj[kPwBatch];
#pragma unroll
                    for (int u = 0; u < kPwBatch; ++u) pj[u] = p[j + u];
#pragma unroll
                    for (int u = 0; u < kPwBatch; ++u) lsum -= h * erow[j + u] * pj[u];
                }
                for (; j < D; ++j) lsum -= h * erow[j] * p[j];
            }
        }
    } else if constexpr (LIKE == SMCMC_LIKE_ASYM) {
        lsum = wg_ordered_sum((pi < 0.0) ? pi * like[1] : pi * like[0], D, scratch);
    } else if constexpr (LIKE == SMCMC_LIKE_HORRIFIC) {
        const bool outside = __syncthreads_or((t < D) && (__builtin_fabs(pi) > 1.0)) != 0;
        lsum = wg_ordered_sum(pi, D, scratch);
        const double sigma = 0.01;
        lsum /= __builtin_sqrt(D * 4.0 / 12.0);
        lsum = -0.5 * lsum * lsum / sigma / sigma;
        lsum = outside ? -1E+30 : lsum;
    } else if constexpr (LIKE == SMCMC_LIKE_CONSTRAINED) {
        double sum = wg_ordered_sum(pi, D, scratch);
        sum = (sum - like[0]) / like[1];
        lsum -= 0.5 * sum * sum;
        const int il = (t < D) ? t : 0;
        double v = pi - like[2 + il];
        v /= like[2 + D + il];
        lsum = wg_ordered_sum(-(0.5 * v * v), D, scratch, lsum);     // x - t and x + (-t) are the same rounding
#if defined(SMCMC_USER_LIKELIHOOD) && defined(SMCMC_USER_LIKELIHOOD_ANY_DIM)
    } else if constexpr (LIKE == SMCMC_LIKE_USER) {
        lsum = smcmc_user_loglike_at(WgLdsPoint{p}, like, D);
#endif
    } else {
        static_assert(LIKE == SMCMC_LIKE_ROSENBROCK, "the likelihoods the workgroup kernel serves");
        // THardLogLikelihood.H:57-67: term i from p[i] and p[i + 1], the terms subtracted in order
        const double rb = like[0];
        const double nx = p[(t + 1 < VEC) ? t + 1 : t];
        const double a = (1.0 - pi);
        const double b = nx - pi * pi;
        const double term = a * a + rb * b * b;
        lsum = wg_ordered_sum(-term, D - 1, scratch);
    }
    return lsum;
}

// the kernel's first argument (a PerChainParams, at offset 0 of the kernel-argument segment), read with scalar loads
typedef const __attribute__((address_space(4))) PerChainParams* KernargParams;
__device__ __forceinline__ KernargParams wg_launder(KernargParams q) {
    asm volatile("" : "+s"(q));
    return q;
}

// grid = nchains workgroups of 512 threads.  NE: registers of packed covariance per thread (perchain_wg_elements).
template <int LIKE, int NE>
__global__ void __launch_bounds__(kWgThreads, 1) perchain_wg_kernel(const PerChainParams p, const PerChainRecord rec) {
    static_assert(NE % 2 == 0 && NE <= kWgMaxNE, "NE");
    constexpr int P = kWgPanelRows;
    // the proposal's panels; also the Cholesky's rows of U (2 x kWgVec) and one step's record
    __shared__ __attribute__((aligned(16))) double panel[2 * P * kWgCols];
    __shared__ __attribute__((aligned(16))) double dv[kWgVec];   // x - c of UpdateState
    __shared__ __attribute__((aligned(16))) double zv[kWgVec];   // sigma r_i of the step
    __shared__ __attribute__((aligned(16))) double sv[kWgVec];   // the terms of an ordered sum
    __shared__ __attribute__((aligned(16))) double ps[kWgVec];   // the proposal where every thread can read all of it
    __shared__ __attribute__((aligned(16))) double ntab[384];    // tables of the normal transform (as in step_kernel)
    __shared__ double pivs[2];                                    // the Cholesky's pivots
    // (a << 8 | b) of every thread's slots, slot r of thread t at t + 512 r: in LDS, because the NE / 2 registers they
    // would take are registers the step does not have to spare (smcmc_perchain_limits.h).  An idle slot is (255, 255): its row is in no
    // panel, it reads (and never uses) entry 255 of the LDS vectors and it is never stored.
    __shared__ uint16_t abt[NE * kWgThreads];

    const int t = threadIdx.x;
    // The launch's parameters are read from the kernel-argument segment where they are used, through a pointer the
    // compiler must take as new at every step (wg_launder): held in SGPRs across the step loop, they were what spilled.
    const KernargParams kbase = (KernargParams)__builtin_amdgcn_kernarg_segment_ptr();
    KernargParams kp = kbase;
    (void)p;
    const int chain = blockIdx.x;
    if (chain >= kp->nchains) return;
    const int D = kp->dim;
    const int npk = D * (D + 1) / 2;
    const size_t NP = (size_t)kp->npad;
    const uint32_t gid = kp->chain_offset + (uint32_t)chain;
    const bool mine = t < D;             // this thread owns a coordinate
    const size_t own = (size_t)(mine ? t : D - 1) * NP + chain;

    const PerChainNormalTables tabs = fill_normal_tables(ntab, kWgThreads);

    double* lf = kp->lane_f64 + chain;
    int32_t* li = kp->lane_i32 + chain;
    PerChainScalars cs;
    cs.load(lf, li, NP);

    // the chain's state on chip
    double xi = kp->x[own], ci = kp->centre[own], lasti = kp->last_point[own], xpi = kp->proposed[own];
    double x0 = kp->x[chain];              // x[0] of the accepted point, in every thread
    double cov[NE], U[NE];
#pragma unroll
    for (int r = 0; r < NE; ++r) {
        const int m = t + kWgThreads * r;
        int a = 255, b = 255;
        if (m < npk) wg_unpack(m, D, a, b);
        abt[m] = (uint16_t)(a << 8 | b);
        const int k = b * (b + 1) / 2 + a;   // covariance (b, a) row major, U(a, b) column packed: the images' index
        cov[r] = (m < npk) ? kp->cov[pc_tile_index(k, (size_t)chain, npk)] : 0.0;
        U[r] = (m < npk) ? kp->ut[pc_tile_index(k, (size_t)chain, D * D)] : 0.0;
        if ((r & 7) == 7) wg_fence();
    }
    __syncthreads();                     // (the normal tables)
    auto ab_of = [&](int r) __attribute__((always_inline)) { return (uint32_t)abt[t + kWgThreads * r]; };
    auto row_of = [&](int r) __attribute__((always_inline)) { return (int)((ab_of(r) >> 8) & 255u); };
    auto col_of = [&](int r) __attribute__((always_inline)) { return (int)(ab_of(r) & 255u); };
    // does any thread's slot r lie in [m0, m1) (wave-uniform)
    auto slot_meets = [&](int r, int m0, int m1) __attribute__((always_inline)) { return kWgThreads * r < m1 && kWgThreads * (r + 1) > m0; };

    bool resume = cs.status == kPcResume;   // the host finished this chain's UpdateProposal: the step goes on behind it
    if (resume) cs.status = kPcOk;
    const uint32_t aw = smcmc_accept_word((uint32_t)D);

    // trace of the covariance, summed in index order (GetCovarianceTrace :961-967)
    auto trace_now = [&]() __attribute__((always_inline)) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NE; ++r) {
            const int a = row_of(r);
            if (a == col_of(r) && a < D) sv[a] = cov[r];
            if ((r & 7) == 7) wg_fence();
        }
        __syncthreads();
        return wg_sum_lds(sv, D);
    };

    // UpdateProposal (TSimpleMCMC.H:1009-1106); `trace` is the covariance trace.  A failed pivot leaves
    // status = kPcNeedsLadder (the host's ladder takes over, :1134-1389) and the U registers spoiled: the chain stops.
    auto update_proposal = [&](double trace) __attribute__((always_inline)) {
        if (!cs.update_proposal(trace, kp->acc_window, kp->max_up, kp->cov_w, kp->cov_wW, kp->acc_w, kp->acc_wW)) return;
        // SharedProposal::cholesky (smcmc_proposal.hpp), right-looking: W(a, b) = A(a, b) - sum_{c < a} U(c, a) U(c, b),
        // the subtraction of row c as soon as row c is finished (c ascending: the host's order of roundings)
#pragma unroll
        for (int r = 0; r < NE; ++r) U[r] = cov[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NE; ++r)
            if (row_of(r) == 0 && col_of(r) == 0) pivs[0] = U[r];
        __syncthreads();
        bool ok = true;
        for (int c = 0; c < D; ++c) {
            const double piv = pivs[c & 1];
            if (!(piv > 0.0) || !__builtin_isfinite(piv)) {
                ok = false;
                break;
            }
            const double sq = __builtin_sqrt(piv);
            double* rowc = panel + (c & 1) * kWgVec;                   // row c of U
            const int m0 = wg_row_start(c, D), m1 = wg_row_start(c + 1, D);
#pragma unroll
            for (int r = 0; r < NE; ++r) {
                if (slot_meets(r, m0, m1) && row_of(r) == c) {
                    const int b = col_of(r);
                    const double u = (b == c) ? sq : U[r] / sq;
                    U[r] = u;
                    rowc[b] = u;
                }
                if ((r & 7) == 7) wg_fence();
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < NE; ++r) {
                if (slot_meets(r, m1, npk)) {
                    const int a = row_of(r), b = col_of(r);
                    if (a > c && a < D) {
                        U[r] -= rowc[b] * rowc[a];
                        if (a == c + 1 && b == c + 1) pivs[(c + 1) & 1] = U[r];
                    }
                }
                if ((r & 7) == 7) wg_fence();
            }
            __syncthreads();
        }
        if (ok) {
#pragma unroll
            for (int r = 0; r < NE; ++r) {
                const int a = row_of(r), b = col_of(r);
                if (a < D) kp->ut[pc_tile_index(b * (b + 1) / 2 + a, (size_t)chain, D * D)] = U[r];
                if ((r & 7) == 7) wg_fence();
            }
        }
        cs.decomposed(ok);
        __syncthreads();
    };

    if (kp->update_only) {
        update_proposal(trace_now());
    } else {
        bool live = cs.status == kPcOk && (resume || cs.tstep < kp->target_step);
        while (live) {
            kp = wg_launder(kbase);
            if (!resume) ++cs.tstep;                                       // ++fTotalSteps, :376
            const uint64_t step = (uint64_t)cs.tstep;
            const bool forced_now = kp->has_forced && cs.tstep == kp->step0 + 1u;
            const bool upd = !resume && !forced_now;                    // UpdateState runs (:706)
            bool moved = false;
            if (upd) {
                // ---- UpdateState, scalar half (TSimpleMCMC.H:1723-1776) ----
                moved = cs.update_state(x0, kp->acc_window, kp->target, kp->asig);
                // ---- running centre (:1780-1788) ----
                __syncthreads();
                if (mine) {
                    double c = ci;
                    c *= cs.centre_trials;
                    c += xi;
                    c /= cs.centre_trials + 1;
                    ci = c;
                    dv[t] = xi - c;
                }
                cs.centre_trials = dmin(kp->cov_window, cs.centre_trials + 1.0);
                // ---- running covariance about the updated centre (:1795-1820) ----
                if (!kp->cov_frozen) {
                    __syncthreads();
                    const double tv = cs.cov_trials, tv1 = cs.cov_trials + 1.0;
#pragma unroll
                    for (int r = 0; r < NE; ++r) {
                        const double da = dv[col_of(r)], db = dv[row_of(r)];   // element (b, a): row b, column a
                        double v = cov[r];
                        const double rr = da * db;
                        v *= tv;
                        v += rr;
                        v /= tv1;
                        cov[r] = v;
                        if ((r & 7) == 7) wg_fence();
                    }
                    cs.cov_trials = dmin(kp->cov_window, cs.cov_trials + 1.0);
                }
                // ---- UpdateProposal when the chain's own schedule says so (:1824-1826) ----
                bool trigger = false;
                if (moved) trigger = (--cs.next_update) < 1;
                if (trigger) {
                    update_proposal(trace_now());
                    if (cs.status != kPcOk) live = false;                  // this chain waits for the host
                }
            }
            if (live && !forced_now) {                                  // :1829-1830
                cs.last_value = cs.logl;
                cs.last_x0 = x0;
                lasti = xi;
            }
            resume = false;
            if (!live) break;

            // ---- the proposal (:709-724) ----
            uint32_t uword;
            {
                const smcmc_u32x4 blk = smcmc_draw_block(kp->seed, gid, step, aw >> 2, SMCMC_STREAM_STEP);
                uword = smcmc_select_word(blk, aw & 3u);
            }
            if (forced_now) {
                xpi = kp->forced[own];
            } else {
                // thread i draws r_i: normal i of the step is word pair (i & 2) of Philox block i / 4
                double z = 0.0;
                if (mine) {
                    const smcmc_u32x4 blk = smcmc_draw_block(kp->seed, gid, step, (uint32_t)(t >> 2), SMCMC_STREAM_STEP);
                    const uint32_t w0 = (t & 2) ? blk.v[2] : blk.v[0], w1 = (t & 2) ? blk.v[3] : blk.v[1];
                    const NormalTables nt = normal_tables_fetch<false>(w0, w1, tabs.ltab, tabs.atab);
                    double n0, n1;
                    normal_pair_lds(w0, w1, nt, &n0, &n1);
                    z = cs.sigma * ((t & 1) ? n1 : n0);
                }
                __syncthreads();
                if (t < kWgVec) zv[t] = z;
                __syncthreads();
                // column j: x'[j] = x[j] + sum_{i <= j} (sigma r_i) U(i, j), i ascending, un-fused.  Rows [r0, r0 + P)
                // of U are slots [wg_row_start(r0), wg_row_start(r0 + P)): their threads put the products in a panel,
                // thread j adds column j's entries in row order.
                double acc = xi;
                const int nq = (D + P - 1) / P;
                for (int q = 0; q < nq; ++q) {
                    double* buf = panel + (q & 1) * (P * kWgCols);
                    const int r0 = q * P;
                    const int m0 = wg_row_start(r0, D), m1 = wg_row_start(r0 + P < D ? r0 + P : D, D);
#pragma unroll
                    for (int r = 0; r < NE; ++r) {
                        if (slot_meets(r, m0, m1)) {
                            const int a = row_of(r);
                            const unsigned d = (unsigned)(a - r0);
                            if (d < (unsigned)P) buf[d * kWgCols + col_of(r)] = zv[a] * U[r];
                        }
                        if ((r & 7) == 7) wg_fence();
                    }
                    __syncthreads();
                    if (mine) {
                        const int n = (t + 1 - r0 < P) ? t + 1 - r0 : P;    // rows r0 .. min(t, r0 + P - 1)
                        if (n > 0) {
#pragma unroll
                            for (int h = 0; h < P; h += 8) {
                                double v[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) v[u] = buf[(h + u) * kWgCols + t];
#pragma unroll
                                for (int u = 0; u < 8; ++u)
                                    if (h + u < n) acc += v[u];
                                if (h % 16 == 8) wg_fence();
                            }
                        }
                    }
                }
                if (cs.ufull) {
                    // a full decomposition (the eigen rung of the ladder): the rows below the diagonal, which every
                    // x'[j] sees after its upper part (i ascending), from the image
                    for (int i2 = 1; i2 < D; ++i2) {
                        const double zi = zv[i2];
                        if (mine && t < i2) {
                            const double u = kp->ut[pc_tile_index(npk + i2 * (i2 - 1) / 2 + t, (size_t)chain, D * D)];
                            acc += zi * u;
                        }
                    }
                }
                xpi = acc;
            }

            // ---- StepRMS window (:391-406), likelihood (:410), Metropolis test (:432-463), accept copy (:484-491) ----
            if (kp->step_rms_window > 0) {
                const double ts = xpi - xi;
                cs.fold_step_rms(wg_ordered_sum(ts * ts, D, sv), kp->step_rms_window);
            }
            __syncthreads();
            if (mine) ps[t] = xpi;
            __syncthreads();
            const double xp0 = ps[0];
            const QuadCsr csr{kp->like_csr.rowptr, kp->like_csr.cols, kp->like_csr.vals, kp->like_csr.rows};
            const double lp = wg_loglike<LIKE, kWgVec>(ps, xpi, D, kp->like, csr, sv);
            if (cs.metropolis_take(kp->metropolis, lp, uword)) {
                xi = xpi;
                x0 = xp0;
            }
            if (kp->save_x != nullptr && ((cs.tstep - kp->step0) % (uint32_t)kp->save_stride) == 0) {
                const size_t slot = (size_t)((cs.tstep - kp->step0) / (uint32_t)kp->save_stride - 1u);
                if (mine) kp->save_x[(slot * (size_t)D + (size_t)t) * NP + chain] = xi;
                if (t == 0) kp->save_logl[slot * NP + chain] = cs.logl;
            }
            if (rec.rec != nullptr && chain == rec.chain) {          // (one chain per workgroup: the same for all threads)
                double* rr = rec.rec + (size_t)(cs.tstep - kp->step0 - 1u) * rec.stride;
                double* recl = panel;
                __syncthreads();
                if (mine) {
                    recl[t] = xi;
                    recl[D + t] = xpi;
                }
#pragma unroll
                for (int r = 0; r < NE; ++r) {
                    const int a = row_of(r);
                    if (a == col_of(r) && a < D) recl[2 * D + a] = cov[r];
                    if ((r & 7) == 7) wg_fence();
                }
                if (t == 0) cs.write_record_scalars(recl + 3 * D);
                __syncthreads();
                for (int k = t; k < 3 * D + kPcRecScalars; k += kWgThreads) rr[k] = recl[k];
                __syncthreads();
            }
            live = cs.tstep < kp->target_step;
        }
    }

    kp = wg_launder(kbase);
    // the chain's state back to its images
    if (mine) {
        kp->x[own] = xi;
        kp->centre[own] = ci;
        kp->last_point[own] = lasti;
        kp->proposed[own] = xpi;
    }
#pragma unroll
    for (int r = 0; r < NE; ++r) {
        const int a = row_of(r), b = col_of(r);
        if (a < D) kp->cov[pc_tile_index(b * (b + 1) / 2 + a, (size_t)chain, npk)] = cov[r];
        if ((r & 7) == 7) wg_fence();
    }
    if (t == 0) {
        if (cs.status == kPcNeedsLadder || cs.status == kPcInvalidTrace) atomicAdd(kp->flag_count, 1);
        cs.store(lf, li, NP);
    }
}

// the likelihoods the workgroup kernel serves
inline bool perchain_wg_serves(int like) {
#if defined(SMCMC_USER_LIKELIHOOD) && defined(SMCMC_USER_LIKELIHOOD_ANY_DIM)
    if (like == SMCMC_LIKE_USER) return true;      // (a user likelihood with the any-dimension form, smcmc_user_loglike_at)
#endif
    return like == SMCMC_LIKE_ISO_GAUSS || like == SMCMC_LIKE_QUADFORM || like == SMCMC_LIKE_ROSENBROCK ||
           like == SMCMC_LIKE_ASYM || like == SMCMC_LIKE_HORRIFIC || like == SMCMC_LIKE_CONSTRAINED;
}

hipError_t launch_perchain_wg(const PerChainParams& p, const PerChainRecord& rec, int like, hipStream_t stream);

}  // namespace smcmc
