// smcmc_perchain_scalars.hip.h -- SMCMC_MODE_PER_CHAIN: what a chain does in plain double / int every step, stated once
// for the step kernels that call it: a chain in a lane (smcmc_perchain_kernel.hip.h) and a chain in a workgroup
// (smcmc_perchain_wg.hip.h), and perchain_broadcast_kernel's de-weighting.  The wave kernel (smcmc_perchain_wave.hip.h)
// and the streamed kernel (smcmc_perchain_stream.hip.h) share the status and record enums below and keep their own copy
// of the step's text: called from here they were measurably slower (profiles/perchain_scalars_notes.md).
//
// The kernels differ in where a chain's O(D^2) state lives -- the covariance update, the Cholesky, the proposal product
// and the ordered sums are theirs.  Everything else of TProposeAdaptiveStep is here: the chain's scalar columns
// (SMCMC_LANE_*, smcmc.h), the scalar halves of UpdateState and UpdateProposal, the StepRMS window, the Metropolis test
// with its bookkeeping, the scalars of a recorded step and the LDS tables of the normal transform.  This is where the
// reference's quirks are: the first trial counted as rejected, the acceptance counters one call behind, UpdateState
// skipped on a forced or resumed step (the callers' `upd`).  The images, the scalar columns and the stop / resume
// protocol (SMCMC_LANE_UPDATE_STATUS below) are the same for every kernel, so the host side -- ladder, broadcast,
// restore, snapshot, getters -- does not know which kernel ran.
//
// The launch's parameters come in by value: a kernel reads them where it calls (perchain_wg_kernel from the
// kernel-argument segment, at the point of use), and the lane kernel calls the same functions under its lane conditions.
//
// Reference-order arithmetic only (compile with -ffp-contract=off): every statement as the reference has it, un-fused.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smcmc.h"
#include "smcmc_detmath.h"
#include "smcmc_kernels.hip.h"

namespace smcmc {

// SMCMC_LANE_UPDATE_STATUS
enum { kPcOk = 0, kPcNeedsLadder = 1, kPcResume = 2, kPcInvalidTrace = 3 };

// Per-step record of one chain: rec[(step - step0 - 1) * stride + ...]: [0, D) fAccepted, [D, 2 D) fProposed, [2 D, 3 D) the
// diagonal of the covariance (GetCovarianceTrace is its sum in index order: the reader adds it up when somebody asks),
// then the scalars below.  What TSimpleMCMC::Step() shows its caller after every step (the two likelihoods, StepRMS,
// the accept flag, the Adaptive* scalars SaveStep fills): include/TSimpleMCMC_amd.H runs Step() ahead in launches of
// many steps and serves the calls from it.
enum {
    kPcRecLogl = 0, kPcRecLoglProposed, kPcRecStepRms, kPcRecLastAccept, kPcRecTrials, kPcRecSuccesses, kPcRecNextUpdate,
    kPcRecAcceptance, kPcRecAcceptanceTrials, kPcRecSigma, kPcRecCenterTrials, kPcRecCovarianceTrials, kPcRecTrace,
    kPcRecTotalSteps, kPcRecStatus, kPcRecScalars
};
static_assert(kPcRecScalars == SMCMC_REC_COUNT_ && kPcRecTrace == SMCMC_REC_COVARIANCE_TRACE && kPcRecStatus == SMCMC_REC_UPDATE_STATUS,
              "the record of smcmc_step_recorded (smcmc.h)");
struct PerChainRecord {
    double* rec;     // nullptr: no record
    int chain;
    int stride;      // doubles per step: >= 3 dim + kPcRecScalars
};

// The de-weighting of the covariance / centre trials (TSimpleMCMC.H:1056-1067) and of the acceptance trials
// (:1081-1086) at an UpdateProposal: w = 1 - deweight, wW = w * window; w < 0 = off.
__device__ __forceinline__ void deweight_trials(double& cov_trials, double& centre_trials, double& acc_trials, double cov_w,
                                                double cov_wW, double acc_w, double acc_wW) {
    if (cov_w >= 0.0) {                                                // :1056-1067
        cov_trials = dmax(1.0, cov_w * cov_trials);
        cov_trials = dmin(cov_trials, cov_wW);
        centre_trials = dmax(1.0, cov_w * centre_trials);
        centre_trials = dmin(centre_trials, cov_wW);
    }
    if (acc_w >= 0.0) {                                                // :1081-1086
        acc_trials = dmax(1.0, acc_w * acc_trials);
        acc_trials = dmin(acc_trials, acc_wW);
    }
}

// A chain's scalar columns on chip for a launch: read at its start, written back at its end.
struct PerChainScalars {
    double logl, sigma, acc_rate, acc_trials, rigid, last_value, last_x0, step_rms, logl_prop, centre_trials, cov_trials,
        sigma_trace;
    int trials, succ, next_update, naccept, rms_trials, last_accept, status, ufull;
    uint32_t tstep;            // fTotalSteps
    int update_count, last_path;

    // lf, li: the chain's entry of the first column (lane_f64 + chain, lane_i32 + chain); NP: the column pitch
    __device__ __forceinline__ void load(const double* lf, const int32_t* li, size_t NP) {
        logl = lf[SMCMC_LANE_LOGL * NP];
        sigma = lf[SMCMC_LANE_SIGMA * NP];
        acc_rate = lf[SMCMC_LANE_ACCEPTANCE * NP];
        acc_trials = lf[SMCMC_LANE_ACCEPTANCE_TRIALS * NP];
        rigid = lf[SMCMC_LANE_RIGIDITY * NP];
        last_value = lf[SMCMC_LANE_LAST_VALUE * NP];
        last_x0 = lf[SMCMC_LANE_LAST_X0 * NP];
        step_rms = lf[SMCMC_LANE_STEP_RMS * NP];
        logl_prop = lf[SMCMC_LANE_LOGL_PROPOSED * NP];
        centre_trials = lf[SMCMC_LANE_CENTER_TRIALS * NP];
        cov_trials = lf[SMCMC_LANE_COVARIANCE_TRIALS * NP];
        sigma_trace = lf[SMCMC_LANE_SIGMA_TRACE * NP];
        trials = li[SMCMC_LANE_TRIALS * NP];
        succ = li[SMCMC_LANE_SUCCESSES * NP];
        next_update = li[SMCMC_LANE_NEXT_UPDATE * NP];
        naccept = li[SMCMC_LANE_NACCEPT * NP];
        rms_trials = li[SMCMC_LANE_STEP_RMS_TRIALS * NP];
        last_accept = li[SMCMC_LANE_LAST_ACCEPT * NP];
        status = li[SMCMC_LANE_UPDATE_STATUS * NP];
        ufull = li[SMCMC_LANE_DECOMP_FULL * NP];
        tstep = (uint32_t)li[SMCMC_LANE_CHAIN_STEPS * NP];
        update_count = li[SMCMC_LANE_UPDATE_COUNT * NP];
        last_path = li[SMCMC_LANE_LAST_UPDATE_PATH * NP];
    }
    __device__ __forceinline__ void store(double* lf, int32_t* li, size_t NP) const {
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

    // UpdateState, scalar half (TSimpleMCMC.H:1723-1776).  x0: x[0] of the accepted point.  Returns whether the chain
    // moved since the call before.
    __device__ __forceinline__ bool update_state(double x0, double acc_window, double target, double asig) {
        ++trials;
        const bool moved = (logl != last_value) || (x0 != last_x0);
        if (moved) ++succ;
        acc_rate *= acc_trials;
        if (moved) acc_rate = acc_rate + 1.0;
        acc_rate /= acc_trials + 1.0;
        acc_trials = dmin(acc_window, acc_trials + 1.0);
        if (rigid < 500.0 && rigid > 0.0) {
            if (__builtin_fabs(acc_rate - target) < asig) {
                rigid += 0.5 * rigid / acc_window;
                rigid = dmin(200.0, rigid);
            }
            if (__builtin_fabs(acc_rate - target) > 4.0 * asig) {
                rigid -= 1.618 * 0.5 * rigid / acc_window;
                rigid = dmax(2.0, rigid);
            }
        }
        if (rigid > 0 && rigid < 100.0) {
            sigma *= smcmc_pow_small(acc_rate / target, dmin(1.0 / 500.0, 1.0 / (rigid * acc_window)));
        }
        return moved;
    }

    // UpdateProposal, scalar half (:1024-1086), up to the start of the decomposition; `trace` is the covariance trace.
    // Returns whether the trace was valid: false leaves status = kPcInvalidTrace, and the chain stops for the host.
    __device__ __forceinline__ bool update_proposal(double trace, double acc_window, double max_up, double cov_w, double cov_wW,
                                                    double acc_w, double acc_wW) {
        ++update_count;
        if (!(trace > 0)) {                                            // :1025-1028 (the reference throws)
            status = kPcInvalidTrace;
            return false;
        }
        const double scale = __builtin_sqrt(sigma_trace / trace);
        sigma = sigma * scale;                                         // :1042
        sigma_trace = trace;                                           // :1043
        const double up = 0.5 * succ;                                  // :1051
        next_update = (int)(acc_window + max_up - max_up / (up + 1.0));   // :1052
        deweight_trials(cov_trials, centre_trials, acc_trials, cov_w, cov_wW, acc_w, acc_wW);
        return true;
    }
    // ... and behind the decomposition (:1097-1106): a failed pivot leaves status = kPcNeedsLadder, the host's ladder
    // takes over (:1134-1389).
    // (as selects: stores in the two branches would be merged into one store through a selected address, and the
    // three variables would then live in scratch)
    __device__ __forceinline__ void decomposed(bool ok) {
        ufull = ok ? 0 : ufull;
        last_path = ok ? 0 : last_path;
        status = ok ? status : (int)kPcNeedsLadder;
    }

    // The StepRMS window (:391-406); sqr: the trial step's square sum, in index order.
    __device__ __forceinline__ void fold_step_rms(double sqr, int window) {
        double ms = step_rms * step_rms;
        ms *= rms_trials;
        ms += sqr;
        ms /= rms_trials + 1.0;
        rms_trials = (window < rms_trials + 1) ? window : rms_trials + 1;
        step_rms = __builtin_sqrt(ms);
    }

    // The Metropolis test (:432-463) of a proposal of likelihood lp, with the step's uniform word, and the accept
    // bookkeeping (:484-491) but for the point, which the caller copies when this returns true.
    __device__ __forceinline__ bool metropolis_take(int metropolis, double lp, uint32_t uword) {
        logl_prop = lp;
        bool take;
        if (metropolis == 2) {
            take = true;
        } else if (!__builtin_isfinite(logl_prop) || logl_prop < -0.999999E+30) {
            take = false;
        } else {
            const double delta = logl_prop - logl;
            take = true;
            if (delta < 0.0) {
                if (metropolis == 1) take = false;
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
        }
        return take;
    }

    // the kPcRec* scalars of a recorded step, to global memory or to a record put together in LDS
    __device__ __forceinline__ void write_record_scalars(double* s) const {
        s[kPcRecLogl] = logl; s[kPcRecLoglProposed] = logl_prop; s[kPcRecStepRms] = step_rms;
        s[kPcRecLastAccept] = last_accept; s[kPcRecTrials] = trials; s[kPcRecSuccesses] = succ;
        s[kPcRecNextUpdate] = next_update; s[kPcRecAcceptance] = acc_rate; s[kPcRecAcceptanceTrials] = acc_trials;
        s[kPcRecSigma] = sigma; s[kPcRecCenterTrials] = centre_trials; s[kPcRecCovarianceTrials] = cov_trials;
        s[kPcRecTrace] = 0.0;     // (the reader sums the diagonal)
        s[kPcRecTotalSteps] = (double)tstep; s[kPcRecStatus] = status;
    }
};

// The tables of the normal transform in LDS (as in step_kernel): ntab[384], 16-byte aligned, filled by a workgroup of
// `threads` >= 64 threads; the caller's barrier stands before the first draw.  Returns the LDS byte addresses
// normal_tables_fetch takes.
struct PerChainNormalTables { uint32_t ltab, atab; };
__device__ __forceinline__ PerChainNormalTables fill_normal_tables(double* ntab, int threads) {
    const int t = threadIdx.x;
    for (int k = t; k < 128; k += threads) ntab[k] = smcmc_log_table_dev[k];
    if (t < kWave) {
        // entry 64 + k is entry k turned by pi / 2: (-sin, cos) (SMCMC_NORMAL_PAIR_BODY_HALFCIRCLE)
        const double c = smcmc_angle_table_dev[2 * t], sn = smcmc_angle_table_dev[2 * t + 1];
        ntab[128 + 2 * t] = c;
        ntab[128 + 2 * t + 1] = sn;
        ntab[128 + 128 + 2 * t] = -sn;
        ntab[128 + 128 + 2 * t + 1] = c;
    }
    const uint32_t ltab = (uint32_t)(uintptr_t)(lds_cptr_f64)ntab;
    return {ltab, ltab + 128u * 8u};
}

}  // namespace smcmc
