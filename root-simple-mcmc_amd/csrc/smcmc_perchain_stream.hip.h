// smcmc_perchain_stream.hip.h -- SMCMC_MODE_PER_CHAIN with one chain per workgroup and the chain's two matrices
// STREAMED from device memory: the statement of perchain_wg_kernel (smcmc_perchain_wg.hip.h) for the dimensions whose
// packed covariance and decomposition do not fit the register file, 63 < D <= kStMaxDim = 512.
//
// A workgroup of 512 threads holds one chain for a whole launch:
//   * thread i < D owns x[i], the running centre c[i], fLastPoint[i] and the proposal x'[i], and draws r_i; the scalar
//     half of UpdateState and UpdateProposal is replicated in every thread; the sums the reference takes in index order
//     go through LDS (wg_ordered_sum / wg_sum_lds on vectors of 512 doubles) -- all as in the register kernel;
//   * the packed covariance and the upper-triangular decomposition live in two contiguous working copies per chain
//     (smcmc_perchain_stream_index.h: wcov[k] in the tiled image's own order, wU[m] row major), read and written where the
//     step uses them.  The host-visible images stay the wavefront tiles they are (one chain's element is 8 bytes of a
//     512-byte line there): a launch copies the chain's two images into the working copies at its start, the
//     covariance back at its end and the decomposition back when an UpdateProposal has made a new one, so the host
//     side -- ladder, restore, snapshot, getters -- does not know which kernel ran;
//   * the proposal x'[j] = x[j] + sum_{i <= j} (sigma r_i) U(i, j), i ascending, un-fused: thread j reads U(i, j) for a
//     fixed i next to its neighbours' and adds in row order, kStBatch rows' loads in flight;
//   * the covariance v *= T; v += d_a d_b; v /= T + 1 element for element along k, a wavefront's 64 elements contiguous;
//   * UpdateProposal's Cholesky row by row as SharedProposal::cholesky states it: thread b forms
//     W(a, b) = A(a, b) - sum_{c < a} U(c, a) U(c, b), c ascending (column a of the finished rows from LDS, its own column
//     from the working copy), then the pivot's root and the division.  A failed pivot stops the chain for the host's
//     ladder; its working decomposition is spoiled then, and the next launch reads the ladder's from the image.
// A workgroup's stores to the working copies are read by other threads of the same workgroup only, behind a barrier.
// The chain's scalar step is stated once for the lane and the register kernel in smcmc_perchain_scalars.hip.h; THIS
// kernel keeps its own copy of that text: called from there it lost 0.3 - 1.7 % (profiles/perchain_scalars_notes.md).
//
// Reference-order arithmetic only (compile with -ffp-contract=off).
#pragma once

#include "smcmc_perchain_stream_index.h"
#include "smcmc_perchain_wg.hip.h"

namespace smcmc {

constexpr int kStVec = kStMaxDim;            // LDS vectors of one value per coordinate
constexpr int kStBatch = 8;                  // loads of a stream issued together
static_assert(kStVec == kWgThreads && kStVec % kWgBatch == 0 && kStBatch == kWgBatch, "one thread per coordinate");

// the chains' working copies: [nchains][dim (dim + 1) / 2] each
struct PerChainStreamWork {
    double* wcov;
    double* wu;
};

// grid = nchains workgroups of 512 threads
template <int LIKE>
__global__ void __launch_bounds__(kWgThreads, 1) perchain_stream_kernel(const PerChainParams p, const PerChainRecord rec,
                                                                        const PerChainStreamWork work) {
    __shared__ __attribute__((aligned(16))) double dv[kStVec];   // x - c of UpdateState
    __shared__ __attribute__((aligned(16))) double zv[kStVec];   // sigma r_i of the step
    __shared__ __attribute__((aligned(16))) double sv[kStVec];   // the terms of an ordered sum
    __shared__ __attribute__((aligned(16))) double ps[kStVec];   // the proposal where every thread can read all of it
    __shared__ __attribute__((aligned(16))) double colv[kStVec]; // the Cholesky: column a of the finished rows
    __shared__ __attribute__((aligned(16))) double ntab[384];    // tables of the normal transform (as in step_kernel)
    __shared__ double pivs;                                       // the Cholesky's pivot

    const int t = threadIdx.x;
    const int chain = blockIdx.x;
    if (chain >= p.nchains) return;
    const int D = p.dim;
    const int npk = st_packed(D);
    const size_t NP = (size_t)p.npad;
    const uint32_t gid = p.chain_offset + (uint32_t)chain;
    const bool mine = t < D;             // this thread owns a coordinate
    const size_t own = (size_t)(mine ? t : D - 1) * NP + chain;
    double* const wc = work.wcov + (size_t)chain * npk;
    double* const wu = work.wu + (size_t)chain * npk;

    if (t < 128) ntab[t] = smcmc_log_table_dev[t];
    if (t < kWave) {
        // entry 64 + k is entry k turned by pi / 2: (-sin, cos) (SMCMC_NORMAL_PAIR_BODY_HALFCIRCLE)
        const double c = smcmc_angle_table_dev[2 * t], sn = smcmc_angle_table_dev[2 * t + 1];
        ntab[128 + 2 * t] = c;
        ntab[128 + 2 * t + 1] = sn;
        ntab[128 + 128 + 2 * t] = -sn;
        ntab[128 + 128 + 2 * t + 1] = c;
    }
    const uint32_t ltab = (uint32_t)(uintptr_t)(lds_cptr_f64)ntab, atab = ltab + 128u * 8u;   // LDS byte addresses

    double* lf = p.lane_f64 + chain;
    int32_t* li = p.lane_i32 + chain;
    double logl = lf[SMCMC_LANE_LOGL * NP];
    double sigma = lf[SMCMC_LANE_SIGMA * NP];
    double acc_rate = lf[SMCMC_LANE_ACCEPTANCE * NP];
    double acc_trials = lf[SMCMC_LANE_ACCEPTANCE_TRIALS * NP];
    double rigid = lf[SMCMC_LANE_RIGIDITY * NP];
    double last_value = lf[SMCMC_LANE_LAST_VALUE * NP];
    double last_x0 = lf[SMCMC_LANE_LAST_X0 * NP];
    double step_rms = lf[SMCMC_LANE_STEP_RMS * NP];
    double logl_prop = lf[SMCMC_LANE_LOGL_PROPOSED * NP];
    double centre_trials = lf[SMCMC_LANE_CENTER_TRIALS * NP];
    double cov_trials = lf[SMCMC_LANE_COVARIANCE_TRIALS * NP];
    double sigma_trace = lf[SMCMC_LANE_SIGMA_TRACE * NP];
    int trials = li[SMCMC_LANE_TRIALS * NP];
    int succ = li[SMCMC_LANE_SUCCESSES * NP];
    int next_update = li[SMCMC_LANE_NEXT_UPDATE * NP];
    int naccept = li[SMCMC_LANE_NACCEPT * NP];
    int rms_trials = li[SMCMC_LANE_STEP_RMS_TRIALS * NP];
    int last_accept = li[SMCMC_LANE_LAST_ACCEPT * NP];
    int status = li[SMCMC_LANE_UPDATE_STATUS * NP];
    int ufull = li[SMCMC_LANE_DECOMP_FULL * NP];
    uint32_t tstep = (uint32_t)li[SMCMC_LANE_CHAIN_STEPS * NP];
    int update_count = li[SMCMC_LANE_UPDATE_COUNT * NP];
    int last_path = li[SMCMC_LANE_LAST_UPDATE_PATH * NP];

    // the chain's state on chip
    double xi = p.x[own], ci = p.centre[own], lasti = p.last_point[own], xpi = p.proposed[own];
    double x0 = p.x[chain];              // x[0] of the accepted point, in every thread

    // the chain's two images into its working copies.  (ka0, kb0): this thread's first covariance element, k = t.
    int ka0, kb0;
    st_unpack_k(t, ka0, kb0);
    for (int k = t; k < npk; k += kWgThreads) wc[k] = p.cov[pc_tile_index(k, (size_t)chain, npk)];
    {
        int a, b;
        st_unpack_slot(t, D, a, b);      // (D >= kStMinDim: every thread has a first slot)
        for (int m = t; m < npk; m += kWgThreads) {
            wu[m] = p.ut[pc_tile_index(st_tile_k(a, b), (size_t)chain, D * D)];
            st_advance_slot(a, b, D, kWgThreads);
        }
    }
    __syncthreads();                     // (the working copies, the normal tables)

    bool resume = status == kPcResume;   // the host finished this chain's UpdateProposal: the step goes on behind it
    if (resume) status = kPcOk;
    const uint32_t aw = smcmc_accept_word((uint32_t)D);

    // trace of the covariance, summed in index order (GetCovarianceTrace :961-967)
    auto trace_now = [&]() __attribute__((always_inline)) {
        __syncthreads();
        if (mine) sv[t] = wc[st_tile_k(t, t)];
        __syncthreads();
        return wg_sum_lds(sv, D);
    };

    // UpdateProposal (TSimpleMCMC.H:1009-1106); `trace` is the covariance trace.  A failed pivot leaves
    // status = kPcNeedsLadder (the host's ladder takes over, :1134-1389) and the working decomposition spoiled: the
    // chain stops.
    auto update_proposal = [&](double trace) __attribute__((always_inline)) {
        ++update_count;
        if (!(trace > 0)) {                                            // :1025-1028 (the reference throws)
            status = kPcInvalidTrace;
            return;
        }
        const double scale = __builtin_sqrt(sigma_trace / trace);
        sigma = sigma * scale;                                         // :1042
        sigma_trace = trace;                                           // :1043
        const double up = 0.5 * succ;                                  // :1051
        next_update = (int)(p.acc_window + p.max_up - p.max_up / (up + 1.0));   // :1052
        if (p.cov_w >= 0.0) {                                          // :1056-1067
            cov_trials = dmax(1.0, p.cov_w * cov_trials);
            cov_trials = dmin(cov_trials, p.cov_wW);
            centre_trials = dmax(1.0, p.cov_w * centre_trials);
            centre_trials = dmin(centre_trials, p.cov_wW);
        }
        if (p.acc_w >= 0.0) {                                          // :1081-1086
            acc_trials = dmax(1.0, p.acc_w * acc_trials);
            acc_trials = dmin(acc_trials, p.acc_wW);
        }
        // SharedProposal::cholesky (smcmc_proposal.hpp), row a after row a - 1: thread b >= a forms
        // W(a, b) = A(a, b) - sum_{c < a} U(c, a) U(c, b), c ascending (the host's order of roundings)
        bool ok = true;
        for (int a = 0; a < D; ++a) {
            __syncthreads();                                           // (row a - 1 is in the working copy)
            if (t < a) colv[t] = wu[st_slot(t, a, D)];                 // U(c, a), c = t
            __syncthreads();
            const bool has = mine && t >= a;
            double wv = 0.0;
            if ((t | (kWave - 1)) >= a && (t & ~(kWave - 1)) < D) {    // (the wavefronts with no column from a on rest)
                if (has) wv = wc[st_tile_k(a, t)];
                int s = t;                                             // st_slot(c, t, D), c = 0
                for (int c0 = 0; c0 < a; c0 += kStBatch) {
                    double u[kStBatch], ca[kStBatch];
#pragma unroll
                    for (int q = 0; q < kStBatch; ++q) {
                        const int c = c0 + q;
                        u[q] = (has && c < a) ? wu[s] : 0.0;
                        s += D - c - 1;
                    }
                    wg_fetch(colv, c0, ca);
#pragma unroll
                    for (int q = 0; q < kStBatch; ++q)
                        if (c0 + q < a) wv -= ca[q] * u[q];
                }
            }
            if (t == a) pivs = wv;
            __syncthreads();
            const double piv = pivs;
            if (!(piv > 0.0) || !__builtin_isfinite(piv)) {
                ok = false;
                break;
            }
            const double sq = __builtin_sqrt(piv);
            if (has) wu[st_slot(a, t, D)] = (t == a) ? sq : wv / sq;
        }
        __syncthreads();
        if (ok) {
            // the new decomposition to its image
            int a, b;
            st_unpack_slot(t, D, a, b);
            for (int m = t; m < npk; m += kWgThreads) {
                p.ut[pc_tile_index(st_tile_k(a, b), (size_t)chain, D * D)] = wu[m];
                st_advance_slot(a, b, D, kWgThreads);
            }
        }
        ufull = ok ? 0 : ufull;
        last_path = ok ? 0 : last_path;
        status = ok ? status : (int)kPcNeedsLadder;
    };

    if (p.update_only) {
        update_proposal(trace_now());
    } else {
        bool live = status == kPcOk && (resume || tstep < p.target_step);
        while (live) {
            if (!resume) ++tstep;                                       // ++fTotalSteps, :376
            const uint64_t step = (uint64_t)tstep;
            const bool forced_now = p.has_forced && tstep == p.step0 + 1u;
            const bool upd = !resume && !forced_now;                    // UpdateState runs (:706)
            bool moved = false;
            if (upd) {
                // ---- UpdateState, scalar half (TSimpleMCMC.H:1723-1776) ----
                ++trials;
                moved = (logl != last_value) || (x0 != last_x0);
                if (moved) ++succ;
                acc_rate *= acc_trials;
                if (moved) acc_rate = acc_rate + 1.0;
                acc_rate /= acc_trials + 1.0;
                acc_trials = dmin(p.acc_window, acc_trials + 1.0);
                if (rigid < 500.0 && rigid > 0.0) {
                    if (__builtin_fabs(acc_rate - p.target) < p.asig) {
                        rigid += 0.5 * rigid / p.acc_window;
                        rigid = dmin(200.0, rigid);
                    }
                    if (__builtin_fabs(acc_rate - p.target) > 4.0 * p.asig) {
                        rigid -= 1.618 * 0.5 * rigid / p.acc_window;
                        rigid = dmax(2.0, rigid);
                    }
                }
                if (rigid > 0 && rigid < 100.0) {
                    sigma *= smcmc_pow_small(acc_rate / p.target, dmin(1.0 / 500.0, 1.0 / (rigid * p.acc_window)));
                }
                // ---- running centre (:1780-1788) ----
                __syncthreads();
                if (mine) {
                    double c = ci;
                    c *= centre_trials;
                    c += xi;
                    c /= centre_trials + 1;
                    ci = c;
                    dv[t] = xi - c;
                }
                centre_trials = dmin(p.cov_window, centre_trials + 1.0);
                // ---- running covariance about the updated centre (:1795-1820) ----
                if (!p.cov_frozen) {
                    __syncthreads();
                    const double tv = cov_trials, tv1 = cov_trials + 1.0;
                    int a = ka0, b = kb0;                                // element (b, a): row b, column a
                    for (int k0 = t; k0 < npk; k0 += kWgThreads * kStBatch) {
                        double v[kStBatch];
#pragma unroll
                        for (int q = 0; q < kStBatch; ++q) {
                            const int k = k0 + kWgThreads * q;
                            v[q] = (k < npk) ? wc[k] : 0.0;
                        }
#pragma unroll
                        for (int q = 0; q < kStBatch; ++q) {
                            const int k = k0 + kWgThreads * q;
                            if (k < npk) {
                                const double rr = dv[a] * dv[b];
                                double vv = v[q];
                                vv *= tv;
                                vv += rr;
                                vv /= tv1;
                                wc[k] = vv;
                                st_advance_k(a, b, kWgThreads);
                            }
                        }
                    }
                    cov_trials = dmin(p.cov_window, cov_trials + 1.0);
                }
                // ---- UpdateProposal when the chain's own schedule says so (:1824-1826) ----
                bool trigger = false;
                if (moved) trigger = (--next_update) < 1;
                if (trigger) {
                    update_proposal(trace_now());
                    if (status != kPcOk) live = false;                  // this chain waits for the host
                }
            }
            if (live && !forced_now) {                                  // :1829-1830
                last_value = logl;
                last_x0 = x0;
                lasti = xi;
            }
            resume = false;
            if (!live) break;

            // ---- the proposal (:709-724) ----
            uint32_t uword;
            {
                const smcmc_u32x4 blk = smcmc_draw_block(p.seed, gid, step, aw >> 2, SMCMC_STREAM_STEP);
                uword = smcmc_select_word(blk, aw & 3u);
            }
            if (forced_now) {
                xpi = p.forced[own];
            } else {
                // thread i draws r_i: normal i of the step is word pair (i & 2) of Philox block i / 4
                double z = 0.0;
                if (mine) {
                    const smcmc_u32x4 blk = smcmc_draw_block(p.seed, gid, step, (uint32_t)(t >> 2), SMCMC_STREAM_STEP);
                    const uint32_t w0 = (t & 2) ? blk.v[2] : blk.v[0], w1 = (t & 2) ? blk.v[3] : blk.v[1];
                    const NormalTables nt = normal_tables_fetch<false>(w0, w1, ltab, atab);
                    double n0, n1;
                    normal_pair_lds(w0, w1, nt, &n0, &n1);
                    z = sigma * ((t & 1) ? n1 : n0);
                }
                __syncthreads();
                zv[t] = z;
                __syncthreads();
                // column j = t: x'[j] = x[j] + sum_{i <= j} (sigma r_i) U(i, j), i ascending, un-fused.  For a fixed row the
                // wavefront's columns are neighbours in the working copy; a wavefront stops at its last column's row.
                double acc = xi;
                const int wrows = ((t & ~(kWave - 1)) >= D) ? 0 : ((t | (kWave - 1)) + 1 < D) ? (t | (kWave - 1)) + 1 : D;
                int s = t;                                              // st_slot(i, t, D), i = 0
                for (int i0 = 0; i0 < wrows; i0 += kStBatch) {
                    double u[kStBatch], zi[kStBatch];
#pragma unroll
                    for (int q = 0; q < kStBatch; ++q) {
                        const int i = i0 + q;
                        u[q] = (mine && i <= t) ? wu[s] : 0.0;
                        s += D - i - 1;
                    }
                    wg_fetch(zv, i0, zi);
#pragma unroll
                    for (int q = 0; q < kStBatch; ++q)
                        if (mine && i0 + q <= t) acc += zi[q] * u[q];
                }
                if (ufull) {
                    // a full decomposition (the eigen rung of the ladder): the rows below the diagonal, which every
                    // x'[j] sees after its upper part (i ascending), from the image
                    for (int i2 = 1; i2 < D; ++i2) {
                        const double zi = zv[i2];
                        if (mine && t < i2) {
                            const double u = p.ut[pc_tile_index(npk + i2 * (i2 - 1) / 2 + t, (size_t)chain, D * D)];
                            acc += zi * u;
                        }
                    }
                }
                xpi = acc;
            }

            // ---- StepRMS window (:391-406), likelihood (:410), Metropolis test (:432-463), accept copy (:484-491) ----
            if (p.step_rms_window > 0) {
                const double ts = xpi - xi;
                const double sqr = wg_ordered_sum(ts * ts, D, sv);
                double ms = step_rms * step_rms;
                ms *= rms_trials;
                ms += sqr;
                ms /= rms_trials + 1.0;
                rms_trials = (p.step_rms_window < rms_trials + 1) ? p.step_rms_window : rms_trials + 1;
                step_rms = __builtin_sqrt(ms);
            }
            __syncthreads();
            if (mine) ps[t] = xpi;
            __syncthreads();
            const double xp0 = ps[0];
            const QuadCsr csr{p.like_csr.rowptr, p.like_csr.cols, p.like_csr.vals, p.like_csr.rows};
            logl_prop = wg_loglike<LIKE, kStVec>(ps, xpi, D, p.like, csr, sv);
            bool take;
            if (p.metropolis == 2) {
                take = true;
            } else if (!__builtin_isfinite(logl_prop) || logl_prop < -0.999999E+30) {
                take = false;
            } else {
                const double delta = logl_prop - logl;
                take = true;
                if (delta < 0.0) {
                    if (p.metropolis == 1) take = false;
                    else {
                        const double trial = smcmc_log_pos(smcmc_u01(uword));
                        if (delta < trial) take = false;
                    }
                }
            }
            last_accept = take ? 1 : 0;
            if (take) {
                logl = logl_prop;
                ++naccept;
                xi = xpi;
                x0 = xp0;
            }
            if (p.save_x != nullptr && ((tstep - p.step0) % (uint32_t)p.save_stride) == 0) {
                const size_t slot = (size_t)((tstep - p.step0) / (uint32_t)p.save_stride - 1u);
                if (mine) p.save_x[(slot * (size_t)D + (size_t)t) * NP + chain] = xi;
                if (t == 0) p.save_logl[slot * NP + chain] = logl;
            }
            if (rec.rec != nullptr && chain == rec.chain) {          // (one chain per workgroup: the same for all threads)
                double* rr = rec.rec + (size_t)(tstep - p.step0 - 1u) * rec.stride;
                if (mine) {
                    rr[t] = xi;
                    rr[D + t] = xpi;
                    rr[2 * D + t] = wc[st_tile_k(t, t)];              // (written behind the barriers above)
                }
                if (t == 0) {
                    double* s = rr + 3 * D;
                    s[kPcRecLogl] = logl; s[kPcRecLoglProposed] = logl_prop; s[kPcRecStepRms] = step_rms;
                    s[kPcRecLastAccept] = last_accept; s[kPcRecTrials] = trials; s[kPcRecSuccesses] = succ;
                    s[kPcRecNextUpdate] = next_update; s[kPcRecAcceptance] = acc_rate; s[kPcRecAcceptanceTrials] = acc_trials;
                    s[kPcRecSigma] = sigma; s[kPcRecCenterTrials] = centre_trials; s[kPcRecCovarianceTrials] = cov_trials;
                    s[kPcRecTrace] = 0.0;     // (the reader sums the diagonal)
                    s[kPcRecTotalSteps] = (double)tstep; s[kPcRecStatus] = status;
                }
            }
            live = tstep < p.target_step;
        }
    }

    // the chain's state back to its images
    __syncthreads();
    if (mine) {
        p.x[own] = xi;
        p.centre[own] = ci;
        p.last_point[own] = lasti;
        p.proposed[own] = xpi;
    }
    for (int k = t; k < npk; k += kWgThreads) p.cov[pc_tile_index(k, (size_t)chain, npk)] = wc[k];
    if (t == 0) {
        if (status == kPcNeedsLadder || status == kPcInvalidTrace) atomicAdd(p.flag_count, 1);
        lf[SMCMC_LANE_LOGL * NP] = logl;
        lf[SMCMC_LANE_SIGMA * NP] = sigma;
        lf[SMCMC_LANE_ACCEPTANCE * NP] = acc_rate;
        lf[SMCMC_LANE_ACCEPTANCE_TRIALS * NP] = acc_trials;
        lf[SMCMC_LANE_RIGIDITY * NP] = rigid;
        lf[SMCMC_LANE_LAST_VALUE * NP] = last_value;
        lf[SMCMC_LANE_LAST_X0 * NP] = last_x0;
        lf[SMCMC_LANE_STEP_RMS * NP] = step_rms;
        lf[SMCMC_LANE_LOGL_PROPOSED * NP] = logl_prop;
        lf[SMCMC_LANE_CENTER_TRIALS * NP] = centre_trials;
        lf[SMCMC_LANE_COVARIANCE_TRIALS * NP] = cov_trials;
        lf[SMCMC_LANE_SIGMA_TRACE * NP] = sigma_trace;
        li[SMCMC_LANE_TRIALS * NP] = trials;
        li[SMCMC_LANE_SUCCESSES * NP] = succ;
        li[SMCMC_LANE_NEXT_UPDATE * NP] = next_update;
        li[SMCMC_LANE_NACCEPT * NP] = naccept;
        li[SMCMC_LANE_STEP_RMS_TRIALS * NP] = rms_trials;
        li[SMCMC_LANE_LAST_ACCEPT * NP] = last_accept;
        li[SMCMC_LANE_UPDATE_STATUS * NP] = status;
        li[SMCMC_LANE_DECOMP_FULL * NP] = ufull;
        li[SMCMC_LANE_CHAIN_STEPS * NP] = (int32_t)tstep;
        li[SMCMC_LANE_UPDATE_COUNT * NP] = update_count;
        li[SMCMC_LANE_LAST_UPDATE_PATH * NP] = last_path;
    }
}

// the dimensions and likelihoods the streamed kernel serves
inline bool perchain_stream_serves(int like, int dim) { return perchain_wg_serves(like) && dim >= kStMinDim && dim <= kStMaxDim; }

hipError_t launch_perchain_stream(const PerChainParams& p, const PerChainRecord& rec, const PerChainStreamWork& work, int like,
                                  hipStream_t stream);

}  // namespace smcmc
