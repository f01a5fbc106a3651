// smcmc_hmc_engine.hip -- host engine behind the smcmc_hmc_* entry points of
// include/smcmc.h: the many-chain form of sMCMC::TSimpleHMC (reference
// TSimpleHMC.H:119-973).  With a fixed step length and leapfrog count (SetMeanEpsilon(<0) +
// SetLeapFrog(n)) the chains share nothing and a launch runs any number of steps.  Otherwise
// (the reference's default) every chain retunes its own step length and leapfrog count as it
// goes (:302-323, 342-344) and the covariance-driven retuning (:665-858) is pooled over the
// ensemble: one step per launch, the accepted points folded into moment sums on the device
// (smcmc_fold_kernel.hip.h), the pooled running covariance and UpdateErrorMatrix on the host
// (smcmc_hmc_shared.hpp) every `sync_every` steps, the new step length / leapfrog count applied
// per chain on the device.  SMCMC_MODE_PER_CHAIN keeps that tuning per chain instead, on the device after every step
// (smcmc_hmc_perchain.hip.h): chain c is the reference chain, and no host work happens between steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_host.hpp"
#include "smcmc_hmc_kernel.hip.h"
#include "smcmc_hmc_mfma_kernel.hip.h"
#include "smcmc_fold_ring.hip.h"
#include "smcmc_hmc_shared.hpp"
#include "smcmc_hmc_perchain.hip.h"

using namespace smcmc;

constexpr int kHmcSnapArrays = 9;

struct smcmc_hmc {
    int dim = 0, nchains = 0, npad = 0, likelihood = 0, device = 0, W = 4;
    uint64_t seed = 0;
    uint32_t chain_offset = 0, step_count = 0;
    bool started = false;
    bool exact = true;             // false: fused order, the quadratic-form gradient on the matrix pipe
    bool use_mfma = false;
    bool use_matrix_exact = false;   // quadratic form, reference order: the matrix layout on the vector pipe
    double alpha = 0.0;            // fAlpha, TSimpleHMC.H:133
    double mean_epsilon = 0.05;    // fMeanEpsilon, set by Start (:229)
    int leapfrog = 10;             // fLeapFrogSteps (:133); SetLeapFrog(n) stores -n (:190)
    hipStream_t stream = nullptr;
    std::vector<double> like_params;
    DeviceBuffer<double> d_q, d_pm, d_qn, d_pn, d_E, d_like;
    DeviceBuffer<double> d_lane_f64;
    DeviceBuffer<int32_t> d_lane_i32;
    // pooled tuning (adaptive step length / leapfrog count, or track_cov)
    HmcShared* shared = nullptr;
    bool track_cov = false;        // keep the running covariance even with a fixed step and count
    int sync_every = 1, steps_in_window = 0;
    int steps_reduced = 0;   // steps whose moments are in d_moments, waiting for hmc_apply (between reduce and apply)
    int fold_nslices = 0, slice_chains = 0;
    smcmc::FoldRing fold;   // the fold kernel's plan for this ensemble
    DeviceBuffer<double> d_p0, d_qprev, d_gacc, d_moments, d_zero;
    PinnedBuffer<double> h_moments;   // the packed moments come back every sync
    // PotentialGradient types 2 / 3 / 5 (TSimpleHMC.H:467-532): the GENERIC instantiation of hmc_step_kernel
    int gradient_type = 0;
    DeviceBuffer<double> d_Eperm;  // QUADFORM: Error in hmc_step_kernel's layout (d_E holds the matrix kernels')
    DeviceBuffer<double> d_covE, d_cov_avg, d_fd_grad;
    bool cov_dirty = true;         // fEstimatedError / fAveragePoint changed since the last upload
    // the caller's gradient matrix of the quadratic form (smcmc_hmc_set_gradient_matrix): gradient types 0 / 1 / 4 contract
    // with it instead of Error, in the kernel that runs the quadratic form without it
    std::vector<double> grad_matrix;   // [dim][dim] row-major; empty = none
    DeviceBuffer<double> d_Gperm;      // in the layout that kernel reads Error in (hmc_kernel_layout)
    bool grad_dirty = false;           // grad_matrix changed since the last upload
    // the running average point / covariance on the device (hmc_absorb_* kernels): the host copy in *shared follows
    // on demand (hmc_pull) or when UpdateErrorMatrix decides to run
    DeviceBuffer<double> d_avg, d_exxt, d_hcov, d_hscal;
    PinnedBuffer<double> h_hscal;  // {n, average trials, covariance trials, trace}
    bool host_stale = false;       // the device holds newer average / covariance than *shared
    bool shared_on_device = false; // hmc_push has run since the host last (re)initialised *shared
    // SMCMC_MODE_PER_CHAIN: every chain's own running average / covariance and tuning scalars (smcmc_hmc_perchain.hip.h)
    int mode = SMCMC_MODE_POOLED;
    DeviceBuffer<double> d_pc_avg, d_pc_exxt, d_pc_covdiag, d_pc_scal, d_pc_scratch;
    DeviceBuffer<int32_t> d_pc_work;
    int pc_grid = 0;               // workgroups of hmc_pc_error_kernel
    // smcmc_hmc_step_recorded: one row per step of the call, gathered on the device
    DeviceBuffer<double> d_rec;
    // smcmc_hmc_snapshot / smcmc_hmc_rollback: a copy of the ensemble's state on the device (SMCMC_MODE_PER_CHAIN)
    DeviceBuffer<unsigned char> snap[kHmcSnapArrays];
    uint32_t snap_step_count = 0;
    bool snap_valid = false;
    std::string error;
    ~smcmc_hmc() { delete shared; }
};

namespace {

// the chains retune themselves (TSimpleHMC.H:302-345, 833-847) unless both the step length and the count are fixed
bool hmc_adaptive(const smcmc_hmc* h) { return h->mean_epsilon > 0.0 || h->leapfrog > 0; }
// likelihoods without a gradient of their own (the reference's functors throw / return false, TAsymLogLikelihood.H:34-36,
// TSimpleHMC.H:85-89): HMC targets through PotentialGradient types 2 / 3 / 5 only
// (a user library whose header defines SMCMC_USER_GRADIENT has one: smcmc_user_gradient_at)
bool hmc_no_own_gradient(int like) {
#ifdef SMCMC_USER_GRADIENT
    if (like == SMCMC_LIKE_USER) return false;
#endif
    return like == SMCMC_LIKE_USER || like == SMCMC_LIKE_ASYM || like == SMCMC_LIKE_HORRIFIC || like == SMCMC_LIKE_CONSTRAINED;
}
// likelihoods whose device function reads the parameter array as the caller gave it
bool hmc_reads_params(int like) {
    return like == SMCMC_LIKE_USER || like == SMCMC_LIKE_ASYM || like == SMCMC_LIKE_HORRIFIC || like == SMCMC_LIKE_CONSTRAINED;
}
// room for a matrix of the likelihood's and one of the gradient's
size_t hmc_like_doubles(int dim) { return 2 * (size_t)dim * dim + 2 * (size_t)dim + 8; }
bool hmc_generic_gradient(const smcmc_hmc* h) { return h->gradient_type == 2 || h->gradient_type == 3 || h->gradient_type == 5; }
// gradient types 0 / 1 / 4 of the quadratic form with the caller's matrix (reference order only)
bool hmc_gradient_matrix(const smcmc_hmc* h) { return !h->grad_matrix.empty() && !hmc_generic_gradient(h); }
// the covariant gradient reads the running covariance: it has to be kept
bool hmc_tracking(const smcmc_hmc* h) { return hmc_adaptive(h) || h->track_cov || h->gradient_type == 2; }

// What an UpdateErrorMatrix that went through does to every chain (TSimpleHMC.H:833-847)
__global__ void hmc_retune_kernel(double* lane_f64, int32_t* lane_i32, int npad, int nchains, double max_scale,
                                  double min_scale, double orbit, int dim) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchains) return;
    double eps = lane_f64[(size_t)kHmcLaneMeanEpsilon * npad + c];
    int L = lane_i32[(size_t)kHmcLaneLeapfrog * npad + c];
    if (eps > 0) {                                                       // :835-839
        eps = 0.2 * max_scale;
        if (eps > 0.5 * min_scale) eps = 0.5 * min_scale;
        if (eps < 0.05 * max_scale) eps = 0.05 * max_scale;
    }
    if (L > 0) {                                                         // :841-848
        const double target = 0.4 * orbit;
        L = (int)(target / __builtin_fabs(eps));
        L = 2 * (L / 2 + 1);
        if (L > 3 * dim) L = 3 * dim;
        if (eps > 0) eps = target / L;
    }
    lane_f64[(size_t)kHmcLaneMeanEpsilon * npad + c] = eps;
    lane_i32[(size_t)kHmcLaneLeapfrog * npad + c] = L;
}

HmcParams hmc_params(smcmc_hmc* h, int nsteps, int init_only) {
    HmcParams p;
    std::memset(&p, 0, sizeof(p));
    p.nchains = h->nchains; p.npad = h->npad; p.dim = h->dim; p.nsteps = nsteps;
    p.leapfrog = std::abs(h->leapfrog);                    // :300
    p.init_only = init_only;
    p.step0 = h->step_count; p.chain_offset = h->chain_offset; p.seed = h->seed;
    p.alpha = h->alpha; p.abs_eps = std::fabs(h->mean_epsilon);
    p.Eperm = h->d_E; p.like = h->d_like;
    p.q = h->d_q; p.pm = h->d_pm; p.qn = h->d_qn; p.pn = h->d_pn;
    p.lane_f64 = h->d_lane_f64; p.lane_i32 = h->d_lane_i32;
    p.p0 = h->d_p0; p.qprev = h->d_qprev;
    p.gradient_type = h->gradient_type;
    if (hmc_generic_gradient(h)) {
        p.Eperm = h->d_Eperm;
        p.cov_Eperm = h->d_covE; p.cov_average = h->d_cov_avg; p.fd_grad = h->d_fd_grad;
    }
    if (hmc_gradient_matrix(h) && !init_only) {
        if (!h->use_matrix_exact) p.Eperm = h->d_Eperm;
        p.Gperm = h->d_Gperm;
    }
    return p;
}

// M [dim][dim] row-major -> hmc_step_kernel's layout: out[w][j][il] = M(il*W + w, j)
std::vector<double> hmc_permute(const smcmc_hmc* h, const double* M) {
    const int D = h->dim, W = h->W;
    std::vector<double> perm((size_t)W * D * kPanelCW, 0.0);
    for (int w = 0; w < W; ++w)
        for (int j = 0; j < D; ++j)
            for (int il = 0; il < kPanelCW; ++il) {
                const int i = il * W + w;
                if (i < D) perm[((size_t)w * D + j) * kPanelCW + il] = M[(size_t)i * D + j];
            }
    return perm;
}

// M [dim][dim] row-major -> the matrix layout of hmc_mfma_kernel<TI, false>:
// out[(tile * D + j) * 16 + 4 rq + r] = M(16 tile + 4 r + rq, j)
std::vector<double> hmc_exact_layout(const smcmc_hmc* h, const double* M) {
    const int D = h->dim, ntiles = (D + 15) / 16;
    std::vector<double> ex(hmc_exact_ex_doubles(D), 0.0);
    for (int it = 0; it < ntiles; ++it)
        for (int j = 0; j < D; ++j)
            for (int rq = 0; rq < 4; ++rq)
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * it + 4 * r + rq;
                    if (i < D) ex[((size_t)it * D + j) * 16 + 4 * rq + r] = M[(size_t)i * D + j];
                }
    return ex;
}

// the layout the reference-order kernel of this engine's quadratic form reads a matrix in
std::vector<double> hmc_kernel_layout(const smcmc_hmc* h, const double* M) {
    return h->use_matrix_exact ? hmc_exact_layout(h, M) : hmc_permute(h, M);
}

// buffers of the GENERIC gradient types, allocated when one is first asked for; the estimated error matrix and the
// average point go up again whenever the pooled update changed them
int hmc_generic_buffers(smcmc_hmc* h) {
    const int D = h->dim;
    const size_t perm_doubles = (size_t)h->W * D * kPanelCW, perm_bytes = sizeof(double) * perm_doubles;
    const bool step_kernel = hmc_generic_gradient(h) || !h->use_matrix_exact;   // (a gradient matrix alone: d_E serves)
    if (h->likelihood == SMCMC_LIKE_QUADFORM && !h->d_Eperm && step_kernel) {
        DeviceBuffer<double> eperm;
        HIP_TRY(h, eperm.allocate(perm_doubles));
        const std::vector<double> perm = hmc_permute(h, h->like_params.data());
        HIP_TRY(h, hipMemcpyAsync(eperm, perm.data(), perm_bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->d_Eperm = std::move(eperm);
    }
    if (hmc_gradient_matrix(h) && (h->grad_dirty || !h->d_Gperm)) {
        const std::vector<double> perm = hmc_kernel_layout(h, h->grad_matrix.data());
        if (!h->d_Gperm) {
            DeviceBuffer<double> gperm;
            HIP_TRY(h, gperm.allocate(perm.size()));
            h->d_Gperm = std::move(gperm);
        }
        HIP_TRY(h, hipMemcpyAsync(h->d_Gperm, perm.data(), perm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // the staging vector goes out of scope; earlier steps are done with the old matrix
        h->grad_dirty = false;
    }
    if (h->gradient_type == 3 && !h->d_fd_grad) {
        DeviceBuffer<double> fd;
        HIP_TRY(h, fd.allocate((size_t)h->npad * D));
        HIP_TRY(h, hipMemsetAsync(fd, 0, sizeof(double) * (size_t)h->npad * D, h->stream));
        h->d_fd_grad = std::move(fd);
    }
    if (h->gradient_type == 2) {
        if (!h->d_covE) {
            DeviceBuffer<double> covE, cov_avg;
            HIP_TRY(h, covE.allocate(perm_doubles));
            HIP_TRY(h, cov_avg.allocate(D));
            h->d_covE = std::move(covE);
            h->d_cov_avg = std::move(cov_avg);
            h->cov_dirty = true;
        }
        if (h->cov_dirty) {
            const std::vector<double> perm = hmc_permute(h, h->shared->error.data());
            HIP_TRY(h, hipMemcpyAsync(h->d_covE, perm.data(), perm_bytes, hipMemcpyHostToDevice, h->stream));
            if (h->shared_on_device)   // the running average lives on the device
                HIP_TRY(h, hipMemcpyAsync(h->d_cov_avg, h->d_avg, sizeof(double) * D, hipMemcpyDeviceToDevice, h->stream));
            else
                HIP_TRY(h, hipMemcpyAsync(h->d_cov_avg, h->shared->average.data(), sizeof(double) * D, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));   // the staging vector goes out of scope
            h->cov_dirty = false;
        }
    }
    return SMCMC_OK;
}

template <typename T>
int hmc_fill_lane(smcmc_hmc* h, T* col, T v) {
    const hipError_t e = fill<T>(col, (size_t)h->nchains, v, h->stream);
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("lane fill launch: ") + hipGetErrorString(e));
    return SMCMC_OK;
}

// buffers of the pooled tuning, allocated when it is first needed: all of them or none
int hmc_tracking_buffers(smcmc_hmc* h) {
    if (h->d_gacc) return SMCMC_OK;
    const size_t vec = (size_t)h->npad * h->dim;
    DeviceBuffer<double> p0, qprev, gacc, moments, zero, avg, exxt, hcov, hscal;
    PinnedBuffer<double> hmoments, hhscal;
    smcmc::FoldRing fold;
    HIP_TRY(h, p0.allocate(vec));
    HIP_TRY(h, qprev.allocate(vec));
    HIP_TRY(h, gacc.allocate(fold_gacc_doubles(h->dim)));
    HIP_TRY(h, smcmc::fold_ring_prepare(fold, h->dim, h->nchains, h->npad, h->fold_nslices, h->slice_chains));
    HIP_TRY(h, moments.allocate(moments_packed(h->dim)));
    HIP_TRY(h, zero.allocate(h->dim));
    HIP_TRY(h, hmoments.allocate(moments_packed(h->dim)));
    HIP_TRY(h, avg.allocate(h->dim));
    HIP_TRY(h, exxt.allocate((size_t)h->dim * h->dim));
    HIP_TRY(h, hcov.allocate((size_t)h->dim * h->dim));
    HIP_TRY(h, hscal.allocate(8));
    HIP_TRY(h, hhscal.allocate(8));
    HIP_TRY(h, hipMemsetAsync(p0, 0, sizeof(double) * vec, h->stream));
    HIP_TRY(h, hipMemsetAsync(qprev, 0, sizeof(double) * vec, h->stream));
    HIP_TRY(h, hipMemsetAsync(gacc, 0, sizeof(double) * fold_gacc_doubles(h->dim), h->stream));
    HIP_TRY(h, hipMemsetAsync(moments, 0, sizeof(double) * moments_packed(h->dim), h->stream));
    HIP_TRY(h, hipMemsetAsync(zero, 0, sizeof(double) * h->dim, h->stream));
    h->d_p0 = std::move(p0); h->d_qprev = std::move(qprev); h->d_gacc = std::move(gacc);
    h->fold = std::move(fold);
    h->d_moments = std::move(moments); h->d_zero = std::move(zero); h->h_moments = std::move(hmoments);
    h->d_avg = std::move(avg); h->d_exxt = std::move(exxt); h->d_hcov = std::move(hcov);
    h->d_hscal = std::move(hscal); h->h_hscal = std::move(hhscal);
    h->shared_on_device = false;
    return SMCMC_OK;
}

// ---- UpdateCovariance (TSimpleHMC.H:665-695) fed with a batch, on the device: the arithmetic of HmcShared::absorb ----
enum { kHsN = 0, kHsAverageTrials, kHsCovTrials, kHsTrace, kHsCount };

__global__ void hmc_absorb_average_kernel(const double* M, int D, double* avg, const double* scal) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const double* S1 = M + (size_t)D * (D + 1) / 2;
    const double n = S1[D];
    if (!(n > 0.0)) return;
    const double trials = scal[kHsAverageTrials];
    double v = avg[i];                                                   // :671-677
    v *= trials;
    v += S1[i];
    v /= trials + n;
    avg[i] = v;
}

__global__ void __launch_bounds__(256) hmc_absorb_cov_kernel(const double* M, int D, const double* avg, double* exxt, double* cov,
                                                             const double* scal) {
    const int j = blockIdx.x * 16 + (threadIdx.x & 15);
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= D || j > i) return;
    const double n = M[(size_t)D * (D + 1) / 2 + D];
    if (!(n > 0.0)) return;
    const double trials = scal[kHsCovTrials];
    double v = exxt[(size_t)i * D + j];                                  // :681-691
    v *= trials;
    v += M[(size_t)i * (i + 1) / 2 + j];
    v /= trials + n;
    exxt[(size_t)i * D + j] = v;
    exxt[(size_t)j * D + i] = v;
    const double c = v - avg[i] * avg[j];
    cov[(size_t)i * D + j] = c;
    cov[(size_t)j * D + i] = c;
}

// trial counts (:678-679, 692-693) and the trace UpdateErrorMatrix looks at (:708-711): one wavefront
__global__ void __launch_bounds__(64) hmc_absorb_scalars_kernel(const double* M, int D, const double* cov, double* scal,
                                                                double cov_window) {
    __shared__ double diag[512];
    for (int d = threadIdx.x; d < D; d += 64) diag[d] = cov[(size_t)d * D + d];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = M[(size_t)D * (D + 1) / 2 + D];
    scal[kHsN] = n;
    if (!(n > 0.0)) return;
    scal[kHsAverageTrials] = __builtin_fmin(cov_window, scal[kHsAverageTrials] + n);
    scal[kHsCovTrials] = __builtin_fmin(cov_window, scal[kHsCovTrials] + n);
    double trace = 0.0;
    for (int d = 0; d < D; ++d) trace += __builtin_fabs(diag[d]);
    scal[kHsTrace] = trace;
}

// host copy of the running average / covariance -> device (Start, or after the host changed them)
int hmc_push(smcmc_hmc* h) {
    const HmcShared& S = *h->shared;
    const size_t D = (size_t)h->dim;
    double sc[kHsCount] = {0.0, S.averageTrials, S.covTrials, 0.0};
    HIP_TRY(h, hipMemcpyAsync(h->d_avg, S.average.data(), D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_exxt, S.exxt.data(), D * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_hcov, S.cov.data(), D * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_hscal, sc, sizeof(sc), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->host_stale = false;
    return SMCMC_OK;
}

// device -> host copy, when somebody asks for fAveragePoint / fEstimatedCovariance
int hmc_pull(smcmc_hmc* h) {
    if (!h->host_stale) return SMCMC_OK;
    HmcShared& S = *h->shared;
    const size_t D = (size_t)h->dim;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(S.average.data(), h->d_avg, D * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(S.exxt.data(), h->d_exxt, D * D * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(S.cov.data(), h->d_hcov, D * D * sizeof(double), hipMemcpyDeviceToHost));
    h->host_stale = false;
    return SMCMC_OK;
}

// The moment groups of the steps since the last update summed (in group order) into the packed vector M, which is what
// crosses ranks when the ensemble is sharded (smcmc_hmc_export_moments / import).
int hmc_reduce(smcmc_hmc* h) {
    // d_moments holds ONE reduction: a second one (an explicit smcmc_hmc_reduce_moments, or the sync a step triggers
    // between a caller's reduce / import and its apply) would overwrite moments that no update has absorbed yet
    if (h->steps_reduced > 0)
        return fail(h, SMCMC_ERR_LOGIC, "moments of an earlier smcmc_hmc_reduce_moments are waiting for smcmc_hmc_apply_moments");
    h->steps_reduced += h->steps_in_window;
    h->steps_in_window = 0;
    const hipError_t e = smcmc::fold_reduce_clear(h->fold, h->d_gacc, h->d_moments, h->stream);
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("fold reduce launch: ") + hipGetErrorString(e));
    return SMCMC_OK;
}

int hmc_apply(smcmc_hmc* h);

// The pooled UpdateCovariance + UpdateErrorMatrix (TSimpleHMC.H:337-341) for the steps since the last one
int hmc_sync(smcmc_hmc* h) {
    if (h->steps_in_window == 0) return SMCMC_OK;
    int st = hmc_reduce(h);
    if (st) return st;
    return hmc_apply(h);
}

// the running averages absorb the batch M and UpdateErrorMatrix decides (every rank of a sharded ensemble the same)
int hmc_apply(smcmc_hmc* h) {
    const int steps = h->steps_reduced;
    h->steps_reduced = 0;
    if (steps == 0) return SMCMC_OK;
    hipError_t e;
    // the running averages absorb the batch on the device; four scalars come back for UpdateErrorMatrix's decision
    HmcShared& S = *h->shared;
    if (!h->shared_on_device) {
        int pst = hmc_push(h);
        if (pst) return pst;
        h->shared_on_device = true;
    }
    const int D = h->dim, t16 = (D + 15) / 16;
    hipLaunchKernelGGL(hmc_absorb_average_kernel, dim3((D + 255) / 256), dim3(256), 0, h->stream, (const double*)h->d_moments, D,
                       h->d_avg, (const double*)h->d_hscal);
    hipLaunchKernelGGL(hmc_absorb_cov_kernel, dim3(t16, t16), dim3(256), 0, h->stream, (const double*)h->d_moments, D,
                       (const double*)h->d_avg, h->d_exxt, h->d_hcov, (const double*)h->d_hscal);
    hipLaunchKernelGGL(hmc_absorb_scalars_kernel, dim3(1), dim3(64), 0, h->stream, (const double*)h->d_moments, D,
                       (const double*)h->d_hcov, h->d_hscal, S.covWindow);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("absorb launch: ") + hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->h_hscal, h->d_hscal, sizeof(double) * kHsCount, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!(h->h_hscal[kHsN] > 0.0)) return SMCMC_OK;
    S.stepCount = (int)h->step_count;
    S.leapfrogZero = (h->leapfrog == 0);
    S.absorbedOnDevice(steps, h->h_hscal[kHsAverageTrials], h->h_hscal[kHsCovTrials]);
    h->host_stale = true;
    h->cov_dirty = true;
    bool updated = false;
    if (S.wantsUpdate(h->h_hscal[kHsTrace])) {
        // the O(D^3) part (eigenvalues, repair, inverse) stays on the host; it needs the covariance there
        int pst = hmc_pull(h);
        if (pst) return pst;
        S.finishUpdate();
        updated = true;
    }
    if (updated) {
        const int threads = 256;
        hipLaunchKernelGGL(hmc_retune_kernel, dim3((h->nchains + threads - 1) / threads), dim3(threads), 0, h->stream,
                           h->d_lane_f64, h->d_lane_i32, h->npad, h->nchains, S.maxScale, S.minScale, S.orbitLength,
                           h->dim);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("retune launch: ") + hipGetErrorString(e));
    }
    return SMCMC_OK;
}

hipError_t hmc_dispatch(smcmc_hmc* h, const HmcParams& p, const HmcSaveArgs* sv = nullptr);

// ---- smcmc_hmc_step_save ----
// the trace of one call: every `stride`-th of its steps has a slot; `done` counts the steps of the call that have run
struct HmcSave {
    double* x = nullptr;       // [slot][dim][npad]; nullptr: a plain smcmc_hmc_step
    double* logl = nullptr;    // [slot][npad], or nullptr
    int stride = 1;
    int done = 0;
};

// does the step kernel of this engine have a SAVE instantiation that writes the slots itself?  (otherwise the launch
// is cut at the save steps: the GENERIC gradient types, and the matrix kernels above 128 dimensions)
bool hmc_saves_in_kernel(const smcmc_hmc* h) {
    if (hmc_generic_gradient(h) || hmc_no_own_gradient(h->likelihood)) return false;
    if (h->use_mfma || h->use_matrix_exact) return hmc_mfma_saves_in_kernel(h->dim);
    return true;
}

HmcSaveArgs hmc_save_args(const HmcSave& sv) { return HmcSaveArgs{sv.x, sv.logl, sv.stride, sv.done}; }

// fAccepted and SMCMC_LANE_LOGL of every live chain as they stand -> slot `slot` of the trace (the cut launch)
__global__ void __launch_bounds__(256) hmc_save_slot_kernel(const double* q, const double* logl, int nchains, int npad, int dim,
                                                            double* save_x, double* save_logl) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchains) return;
    const int i = blockIdx.y;
    if (i < dim) save_x[(size_t)i * npad + c] = q[(size_t)i * npad + c];
    else if (save_logl != nullptr) save_logl[c] = logl[c];
}

int hmc_save_slot(smcmc_hmc* h, const HmcSave& sv, int slot) {
    const size_t NP = (size_t)h->npad;
    hipLaunchKernelGGL(hmc_save_slot_kernel, dim3((h->nchains + 255) / 256, h->dim + 1), dim3(256), 0, h->stream,
                       (const double*)h->d_q, (const double*)(h->d_lane_f64 + (size_t)SMCMC_LANE_LOGL * NP), h->nchains, h->npad,
                       h->dim, sv.x + (size_t)slot * h->dim * NP, sv.logl ? sv.logl + (size_t)slot * NP : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("trace slot launch: ") + hipGetErrorString(e));
    return SMCMC_OK;
}

// one step of a tuned mode (one step per launch) and, when it has one, its slot
int hmc_one_step(smcmc_hmc* h, HmcSave& sv) {
    HmcParams p = hmc_params(h, 1, 0);
    p.adaptive = 1;
    const bool in_kernel = sv.x != nullptr && hmc_saves_in_kernel(h);
    const HmcSaveArgs args = hmc_save_args(sv);
    hipError_t e = hmc_dispatch(h, p, in_kernel ? &args : nullptr);
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("hmc step launch: ") + hipGetErrorString(e));
    h->step_count += 1u;
    sv.done += 1;
    if (sv.x != nullptr && !in_kernel && sv.done % sv.stride == 0) return hmc_save_slot(h, sv, sv.done / sv.stride - 1);
    return SMCMC_OK;
}

hipError_t hmc_dispatch(smcmc_hmc* h, const HmcParams& p, const HmcSaveArgs* sv) {
    const bool generic = hmc_generic_gradient(h) && !p.init_only;
    if (h->use_mfma && !generic) return launch_hmc_mfma(p, h->stream, sv);
    if (h->use_matrix_exact && !generic) return launch_hmc_matrix_exact(p, h->stream, sv);
    return (h->W == 4) ? launch_hmc<4, kPanelCW>(p, h->likelihood, h->stream, sv)
                       : launch_hmc<8, kPanelCW>(p, h->likelihood, h->stream, sv);
}

// ---- SMCMC_MODE_PER_CHAIN ----
bool hmc_per_chain(const smcmc_hmc* h) { return h->mode == SMCMC_MODE_PER_CHAIN; }

// buffers of the per-chain tuning, allocated at the first Start in this mode: all of them or none
int hmc_pc_buffers(smcmc_hmc* h) {
    if (h->d_pc_scal) return SMCMC_OK;
    const size_t D = (size_t)h->dim, NP = (size_t)h->npad;
    // the error kernel's grid: enough workgroups to cover the CUs a few times over; a D x D image each beyond LDS
    int grid = std::min(1024, h->nchains);
    if (h->dim > kPcLdsDim) grid = std::min<size_t>(grid, std::max<size_t>(1, ((size_t)256 << 20) / (D * D * sizeof(double))));
    grid = std::max(1, grid);
    DeviceBuffer<double> p0, qprev, avg, exxt, covdiag, scratch, scal;
    DeviceBuffer<int32_t> work;
    if (!h->d_p0) HIP_TRY(h, p0.allocate(D * NP));
    if (!h->d_qprev) HIP_TRY(h, qprev.allocate(D * NP));
    HIP_TRY(h, avg.allocate(D * NP));
    HIP_TRY(h, exxt.allocate(pc_npacked(h->dim) * NP));
    HIP_TRY(h, covdiag.allocate(D * NP));
    HIP_TRY(h, work.allocate(NP + 1));
    if (h->dim > kPcLdsDim) HIP_TRY(h, scratch.allocate(D * D * (size_t)grid));
    HIP_TRY(h, scal.allocate(kPcCount * NP));
    if (p0) h->d_p0 = std::move(p0);
    if (qprev) h->d_qprev = std::move(qprev);
    h->d_pc_avg = std::move(avg); h->d_pc_exxt = std::move(exxt); h->d_pc_covdiag = std::move(covdiag);
    h->d_pc_work = std::move(work); h->d_pc_scratch = std::move(scratch); h->d_pc_scal = std::move(scal);
    h->pc_grid = grid;
    return SMCMC_OK;
}

// the covariance part of Start (:236-266) for every chain: fAveragePoint = its own start point, the rest as HmcShared::start
int hmc_pc_start(smcmc_hmc* h, const std::vector<double>& x) {
    int st = hmc_pc_buffers(h);
    if (st) {
        h->error = "per-chain HMC tuning state does not fit in device memory: " + h->error;
        return st;
    }
    const size_t D = (size_t)h->dim, NP = (size_t)h->npad;
    HIP_TRY(h, hipMemcpyAsync(h->d_pc_avg, x.data(), sizeof(double) * D * NP, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_pc_exxt, 0, sizeof(double) * pc_npacked(h->dim) * NP, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_pc_covdiag, 0, sizeof(double) * D * NP, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_pc_work, 0, sizeof(int32_t) * (NP + 1), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_qprev, 0, sizeof(double) * D * NP, h->stream));
    std::vector<double> scal((size_t)kPcCount * NP, 0.0);
    for (size_t c = 0; c < NP; ++c) scal[(size_t)kPcEstTrace * NP + c] = (double)D;   // fEstimatedCovarianceTrace = dim
    HIP_TRY(h, hipMemcpyAsync(h->d_pc_scal, scal.data(), sizeof(double) * scal.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the staging vectors go out of scope
    return SMCMC_OK;
}

// UpdateCovariance + UpdateErrorMatrix (:337-341) of every chain after the step that just ran, on the stream
int hmc_pc_update(smcmc_hmc* h) {
    HmcPcParams q;
    std::memset(&q, 0, sizeof(q));
    const size_t NP = (size_t)h->npad;
    q.nchains = h->nchains; q.npad = h->npad; q.dim = h->dim;
    q.step_count = (int)h->step_count;
    q.cov_window = h->shared->covWindow;
    q.qprev = h->d_qprev;
    q.contributes = h->d_lane_i32 + (size_t)kHmcLaneContributes * NP;
    q.lane_f64 = h->d_lane_f64; q.lane_i32 = h->d_lane_i32;
    q.avg = h->d_pc_avg; q.exxt = h->d_pc_exxt; q.covdiag = h->d_pc_covdiag; q.scal = h->d_pc_scal;
    q.work = h->d_pc_work; q.scratch = h->d_pc_scratch;
    const size_t np = pc_npacked(h->dim);
    const unsigned ny = (unsigned)((np + 4 * kPcExxtRun - 1) / (4 * kPcExxtRun));
    hipLaunchKernelGGL(hmc_pc_exxt_kernel, dim3(h->npad / kWave, ny), dim3(kWave, 4), 0, h->stream, q);
    hipLaunchKernelGGL(hmc_pc_decide_kernel, dim3((h->nchains + 255) / 256), dim3(256), 0, h->stream, q);
    hipLaunchKernelGGL(hmc_pc_error_kernel, dim3(h->pc_grid), dim3(kWave), 0, h->stream, q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("per-chain tuning launch: ") + hipGetErrorString(e));
    return SMCMC_OK;
}

// chain c's fAveragePoint, fEstimatedCovariance and tuning scalars (any pointer may be null)
int hmc_pc_read(smcmc_hmc* h, int c, double* average, double* covariance, double* tuning) {
    if (!h->started || !h->d_pc_scal) return fail(h, SMCMC_ERR_LOGIC, "the per-chain tuning starts with Start");
    const int D = h->dim;
    const size_t NP = (size_t)h->npad;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double sc[kPcCount];
    HIP_TRY(h, hipMemcpy2D(sc, sizeof(double), h->d_pc_scal + c, NP * sizeof(double), sizeof(double), kPcCount,
                           hipMemcpyDeviceToHost));
    if (tuning) std::copy(sc, sc + kPcTuningFields, tuning);
    std::vector<double> avg((size_t)D);
    if (average || covariance)
        HIP_TRY(h, hipMemcpy2D(avg.data(), sizeof(double), h->d_pc_avg + c, NP * sizeof(double), sizeof(double), (size_t)D,
                               hipMemcpyDeviceToHost));
    if (average) std::copy(avg.begin(), avg.end(), average);
    if (!covariance) return SMCMC_OK;
    if (sc[kPcCovTrials] == 0.0) {                                       // Start's identity (:255-258)
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) covariance[(size_t)i * D + j] = (i == j) ? 1.0 : 0.0;
    } else if (sc[kPcCovState] != 0.0) {                                 // what the repair loop left (:793-808)
        std::vector<double> dg((size_t)D);
        HIP_TRY(h, hipMemcpy2D(dg.data(), sizeof(double), h->d_pc_covdiag + c, NP * sizeof(double), sizeof(double),
                               (size_t)D, hipMemcpyDeviceToHost));
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) covariance[(size_t)i * D + j] = (i == j) ? dg[i] : 0.0;
    } else {                                                             // :689
        std::vector<double> ex(pc_npacked(D));
        HIP_TRY(h, hipMemcpy2D(ex.data(), sizeof(double), h->d_pc_exxt + c, NP * sizeof(double), sizeof(double), ex.size(),
                               hipMemcpyDeviceToHost));
        for (int i = 0; i < D; ++i)
            for (int j = 0; j <= i; ++j)
                covariance[(size_t)i * D + j] = covariance[(size_t)j * D + i] =
                    ex[(size_t)i * (i + 1) / 2 + j] - avg[i] * avg[j];
    }
    return SMCMC_OK;
}

}  // namespace

extern "C" {

int smcmc_hmc_create(int dim, int nchains, int likelihood, uint64_t seed, uint32_t chain_offset, int device,
                     smcmc_hmc** out) {
    if (!out) return SMCMC_ERR_INVALID;
    *out = nullptr;
    if (dim < 1 || nchains < 1) return SMCMC_ERR_INVALID;
    if (likelihood == SMCMC_LIKE_EVENT_SAMPLE || likelihood == SMCMC_LIKE_EVENT_TEMPLATE || likelihood == SMCMC_LIKE_EVENT_SHAPE) return SMCMC_ERR_UNSUPPORTED;   // the Metropolis engine serves the event sample, the event template and the event shape: it has no gradient and no HMC kernel
    if (likelihood < SMCMC_LIKE_ISO_GAUSS || likelihood > SMCMC_LIKE_CONSTRAINED) return SMCMC_ERR_INVALID;
#ifndef SMCMC_USER_LIKELIHOOD_ANY_DIM
    // a compiled-in user likelihood is an HMC target when its header has the form that walks a point in device memory
    if (likelihood == SMCMC_LIKE_USER) return SMCMC_ERR_UNSUPPORTED;
#endif
    if (likelihood == SMCMC_LIKE_ROSENBROCK && dim < 2) return SMCMC_ERR_INVALID;
    if (dim > 8 * kPanelCW) return SMCMC_ERR_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return SMCMC_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return SMCMC_ERR_NO_DEVICE;
    smcmc_hmc* h = new (std::nothrow) smcmc_hmc();
    if (!h) return SMCMC_ERR_RUNTIME;
    h->dim = dim; h->nchains = nchains; h->likelihood = likelihood; h->seed = seed;
    h->chain_offset = chain_offset; h->device = device;
    h->W = (dim <= 4 * kPanelCW) ? 4 : 8;
    h->npad = (nchains + kWave - 1) / kWave * kWave;
    h->fold_nslices = fold_slices(dim);
    h->slice_chains = ((h->npad / kWave + h->fold_nslices - 1) / h->fold_nslices) * kWave;
    h->shared = new HmcShared(dim);
    *out = h;
    ON_DEVICE(h);
    const size_t vec = sizeof(double) * (size_t)h->npad * dim;
    HIP_TRY(h, h->d_q.allocate((size_t)h->npad * dim));
    HIP_TRY(h, h->d_pm.allocate((size_t)h->npad * dim));
    HIP_TRY(h, h->d_qn.allocate((size_t)h->npad * dim));
    HIP_TRY(h, h->d_pn.allocate((size_t)h->npad * dim));
    const size_t e_doubles = std::max({(size_t)h->W * dim * kPanelCW, hmc_mfma_eop_doubles(dim), hmc_exact_ex_doubles(dim)});
    HIP_TRY(h, h->d_E.allocate(e_doubles));
    HIP_TRY(h, h->d_like.allocate(hmc_like_doubles(dim)));
    HIP_TRY(h, h->d_lane_f64.allocate((size_t)h->npad * SMCMC_LANE_F64_COUNT_));
    HIP_TRY(h, h->d_lane_i32.allocate((size_t)h->npad * SMCMC_LANE_I32_COUNT_));
    HIP_TRY(h, hipMemset(h->d_q, 0, vec));
    HIP_TRY(h, hipMemset(h->d_pm, 0, vec));
    HIP_TRY(h, hipMemset(h->d_qn, 0, vec));
    HIP_TRY(h, hipMemset(h->d_pn, 0, vec));
    HIP_TRY(h, hipMemset(h->d_E, 0, sizeof(double) * e_doubles));
    HIP_TRY(h, hipMemset(h->d_like, 0, sizeof(double) * hmc_like_doubles(dim)));
    HIP_TRY(h, hipMemset(h->d_lane_f64, 0, sizeof(double) * (size_t)h->npad * SMCMC_LANE_F64_COUNT_));
    HIP_TRY(h, hipMemset(h->d_lane_i32, 0, sizeof(int32_t) * (size_t)h->npad * SMCMC_LANE_I32_COUNT_));
    return SMCMC_OK;
}

int smcmc_hmc_destroy(smcmc_hmc* h) {
    if (!h) return SMCMC_OK;
    ON_DEVICE(h);
    if (h->d_q) (void)hipStreamSynchronize(h->stream);
    delete h;
    return SMCMC_OK;
}

const char* smcmc_hmc_last_error(const smcmc_hmc* h) { return h ? h->error.c_str() : "null engine"; }

int smcmc_hmc_set_stream(smcmc_hmc* h, void* hip_stream) {
    if (!h) return SMCMC_ERR_INVALID;
    h->stream = (hipStream_t)hip_stream;
    return SMCMC_OK;
}

int smcmc_hmc_set_likelihood_params(smcmc_hmc* h, const double* params, int count) {
    if (!h || count < 0 || (count > 0 && !params)) return SMCMC_ERR_INVALID;
    h->like_params.assign(params, params + count);
    return SMCMC_OK;
}

int smcmc_hmc_set_exact_arithmetic(smcmc_hmc* h, int exact) {
    if (!h) return SMCMC_ERR_INVALID;
    if (h->started) return fail(h, SMCMC_ERR_LOGIC, "choose the arithmetic before Start");
    if (!exact && !h->grad_matrix.empty())
        return fail(h, SMCMC_ERR_UNSUPPORTED, "a gradient matrix runs in reference-order arithmetic only");
    h->exact = exact != 0;
    return SMCMC_OK;
}
int smcmc_hmc_set_alpha(smcmc_hmc* h, double a) { if (!h) return SMCMC_ERR_INVALID; h->alpha = a; return SMCMC_OK; }
// SetMeanEpsilon / SetLeapFrog reach every chain's own copy (TSimpleHMC.H:181, 190)
int smcmc_hmc_set_mean_epsilon(smcmc_hmc* h, double e) {
    if (!h) return SMCMC_ERR_INVALID;
    h->mean_epsilon = e;
    if (!h->started) return SMCMC_OK;
    ON_DEVICE(h);
    return hmc_fill_lane<double>(h, h->d_lane_f64 + (size_t)kHmcLaneMeanEpsilon * h->npad, e);
}
int smcmc_hmc_set_leapfrog(smcmc_hmc* h, int n) {
    if (!h) return SMCMC_ERR_INVALID;
    h->leapfrog = -n;
    if (!h->started) return SMCMC_OK;
    ON_DEVICE(h);
    return hmc_fill_lane<int32_t>(h, h->d_lane_i32 + (size_t)kHmcLaneLeapfrog * h->npad, (int32_t)-n);
}
// chain 0's fMeanEpsilon / fLeapFrogSteps (each chain retunes its own unless they are fixed)
int smcmc_hmc_get_mean_epsilon(smcmc_hmc* h, double* e) {
    if (!h || !e) return SMCMC_ERR_INVALID;
    *e = h->mean_epsilon;
    if (!h->started) return SMCMC_OK;
    ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(e, h->d_lane_f64 + (size_t)kHmcLaneMeanEpsilon * h->npad, sizeof(double), hipMemcpyDeviceToHost));
    return SMCMC_OK;
}
int smcmc_hmc_get_leapfrog(smcmc_hmc* h, int* steps) {
    if (!h || !steps) return SMCMC_ERR_INVALID;
    *steps = h->leapfrog;
    if (!h->started) return SMCMC_OK;
    ON_DEVICE(h);
    int32_t v = 0;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(&v, h->d_lane_i32 + (size_t)kHmcLaneLeapfrog * h->npad, sizeof(int32_t), hipMemcpyDeviceToHost));
    *steps = v;
    return SMCMC_OK;
}
int smcmc_hmc_set_sync_interval(smcmc_hmc* h, int steps) {
    if (!h || steps < 1) return SMCMC_ERR_INVALID;
    h->sync_every = steps;
    return SMCMC_OK;
}
// Step(save, gradientType) (TSimpleHMC.H:279, 467-532).  0, 1 and 4 are the likelihood's own gradient here (every
// device likelihood has one); 2 the covariant approximation from the pooled running covariance (which is then kept
// whatever the tuning); 3 finite differences of the potential; 5 zero.
int smcmc_hmc_set_gradient_type(smcmc_hmc* h, int type) {
    if (!h || type < 0 || type > 5) return SMCMC_ERR_INVALID;
    if (!h->exact && (type == 2 || type == 3 || type == 5))
        return fail(h, SMCMC_ERR_UNSUPPORTED, "gradient types 2, 3 and 5 run in reference-order arithmetic only");
    if (type == 2 && hmc_per_chain(h))
        return fail(h, SMCMC_ERR_UNSUPPORTED, "the covariant gradient (type 2) is not available in SMCMC_MODE_PER_CHAIN");
    h->gradient_type = type;
    return SMCMC_OK;
}
int smcmc_hmc_get_gradient_type(const smcmc_hmc* h) { return h ? h->gradient_type : -1; }
int smcmc_hmc_has_gradient(const smcmc_hmc* h) { return (h && !hmc_no_own_gradient(h->likelihood)) ? 1 : 0; }
// GradientError of BadGrad.C:33-41 for the built-in quadratic form; applied by the next step (hmc_generic_buffers)
int smcmc_hmc_set_gradient_matrix(smcmc_hmc* h, const double* G, int count) {
    if (!h || count < 0 || (count > 0 && !G)) return SMCMC_ERR_INVALID;
    if (h->likelihood != SMCMC_LIKE_QUADFORM)
        return fail(h, SMCMC_ERR_INVALID, "a gradient matrix belongs to SMCMC_LIKE_QUADFORM");
    if (count == 0) {
        h->grad_matrix.clear();
        h->grad_dirty = false;
        return SMCMC_OK;
    }
    if ((size_t)count != (size_t)h->dim * h->dim) return fail(h, SMCMC_ERR_INVALID, "the gradient matrix has dim*dim entries");
    if (!h->exact) return fail(h, SMCMC_ERR_UNSUPPORTED, "a gradient matrix runs in reference-order arithmetic only");
    h->grad_matrix.assign(G, G + count);
    h->grad_dirty = true;
    return SMCMC_OK;
}
int smcmc_hmc_set_track_covariance(smcmc_hmc* h, int on) {
    if (!h) return SMCMC_ERR_INVALID;
    h->track_cov = on != 0;
    return SMCMC_OK;
}
int smcmc_hmc_moment_group(const smcmc_hmc* h) { return h ? h->slice_chains : 0; }
int smcmc_hmc_set_mode(smcmc_hmc* h, int mode) {
    if (!h) return SMCMC_ERR_INVALID;
    if (mode != SMCMC_MODE_POOLED && mode != SMCMC_MODE_PER_CHAIN)
        return fail(h, SMCMC_ERR_INVALID, "HMC modes: SMCMC_MODE_POOLED, SMCMC_MODE_PER_CHAIN");
    if (h->started) return fail(h, SMCMC_ERR_LOGIC, "choose the mode before Start");
    if (mode == SMCMC_MODE_PER_CHAIN && h->gradient_type == 2)
        return fail(h, SMCMC_ERR_UNSUPPORTED, "the covariant gradient (type 2) is not available in SMCMC_MODE_PER_CHAIN");
    h->mode = mode;
    return SMCMC_OK;
}
int smcmc_hmc_get_mode(const smcmc_hmc* h) { return h ? h->mode : -1; }
int smcmc_hmc_read_chain_tuning(smcmc_hmc* h, int chain, double* average, double* covariance, double* tuning) {
    if (!h || chain < 0 || chain >= h->nchains) return SMCMC_ERR_INVALID;
    if (!hmc_per_chain(h)) {
        int st = SMCMC_OK;
        if (average) st = smcmc_hmc_get_average_point(h, average);
        if (!st && covariance) st = smcmc_hmc_get_covariance(h, covariance);
        if (!st && tuning) st = smcmc_hmc_get_tuning(h, tuning);
        return st;
    }
    ON_DEVICE(h);
    return hmc_pc_read(h, chain, average, covariance, tuning);
}
int smcmc_hmc_get_tuning(smcmc_hmc* h, double* out) {
    if (!h || !out) return SMCMC_ERR_INVALID;
    if (hmc_per_chain(h) && h->started) return smcmc_hmc_read_chain_tuning(h, 0, nullptr, nullptr, out);
    const HmcShared& S = *h->shared;
    out[0] = S.curTrace; out[1] = S.orbitLength; out[2] = S.updateCount; out[3] = S.covTrials;
    out[4] = S.averageTrials; out[5] = S.stepsRemaining; out[6] = S.stepsSinceUpdate; out[7] = S.maxScale;
    out[8] = S.minScale; out[9] = S.estTrace;
    return SMCMC_OK;
}
int smcmc_hmc_get_average_point(smcmc_hmc* h, double* out) {
    if (!h || !out) return SMCMC_ERR_INVALID;
    if (hmc_per_chain(h) && h->started) return smcmc_hmc_read_chain_tuning(h, 0, out, nullptr, nullptr);
    { int pst = hmc_pull(h); if (pst) return pst; }
    std::copy(h->shared->average.begin(), h->shared->average.end(), out);
    return SMCMC_OK;
}
int smcmc_hmc_get_covariance(smcmc_hmc* h, double* out) {
    if (!h || !out) return SMCMC_ERR_INVALID;
    if (hmc_per_chain(h) && h->started) return smcmc_hmc_read_chain_tuning(h, 0, nullptr, out, nullptr);
    { int pst = hmc_pull(h); if (pst) return pst; }
    std::copy(h->shared->cov.begin(), h->shared->cov.end(), out);
    return SMCMC_OK;
}

int smcmc_hmc_start(smcmc_hmc* h, const double* x0, int broadcast) {
    if (!h || !x0) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    const int D = h->dim, N = h->nchains;
    const size_t NP = (size_t)h->npad;
    // (HORRIFIC reads no parameters: this engine holds what it is given to the user likelihood's limit)
    std::vector<double> prm;
    int st = check_like_params(h, h->likelihood == SMCMC_LIKE_HORRIFIC ? (int)SMCMC_LIKE_USER : h->likelihood,
                               hmc_like_doubles(D), "a user likelihood takes at most 2 dim^2 + 2 dim + 8 parameters", prm);
    if (st) return st;
    if (h->likelihood == SMCMC_LIKE_QUADFORM) {
        h->use_mfma = !h->exact && D <= kMfDimMax;
        h->use_matrix_exact = h->exact && D <= kMfDimMax;
        if (h->use_matrix_exact) {
            const std::vector<double> ex = hmc_exact_layout(h, h->like_params.data());
            HIP_TRY(h, hipMemcpyAsync(h->d_E, ex.data(), ex.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        if (h->use_mfma) {
            // Eop[(tile * nkq + kq) * 64 + lane] = Error(16 tile + (lane & 15), 4 kq + (lane >> 4)): the A operand
            // of every matrix instruction as one contiguous 512-byte read
            const int ntiles = (D + 15) / 16, nkq = (D + 3) / 4, nkqp = panel_mfma_nkq_padded(D);
            std::vector<double> eop(hmc_mfma_eop_doubles(D), 0.0);
            for (int it = 0; it < ntiles; ++it)
                for (int kq = 0; kq < nkq; ++kq)
                    for (int l = 0; l < 64; ++l) {
                        const int i = 16 * it + (l & 15), j = 4 * kq + (l >> 4);
                        if (i < D && j < D) eop[((size_t)it * nkqp + kq) * 64 + l] = h->like_params[(size_t)i * D + j];
                    }
            HIP_TRY(h, hipMemcpyAsync(h->d_E, eop.data(), eop.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        // Eperm[w][j][il] = Error(il*W + w, j): the rows a wavefront owns, contiguous per source column j
        const std::vector<double> perm = hmc_permute(h, h->like_params.data());
        if (h->d_Eperm) {
            HIP_TRY(h, hipMemcpyAsync(h->d_Eperm, perm.data(), perm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        if (!h->use_mfma && !h->use_matrix_exact) {
            HIP_TRY(h, hipMemcpyAsync(h->d_E, perm.data(), perm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
    } else {
        h->use_mfma = false;
        h->use_matrix_exact = false;
    }
    if (hmc_reads_params(h->likelihood)) {
        if (!prm.empty())
            HIP_TRY(h, hipMemcpyAsync(h->d_like, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
        const double b = prm.empty() ? 100.0 : prm[0];   // ROSENBROCK's, or the unused default of the others
        HIP_TRY(h, hipMemcpyAsync(h->d_like, &b, sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    std::vector<double> x(NP * D, 0.0);
    for (int d = 0; d < D; ++d)
        for (int c = 0; c < N; ++c) x[(size_t)d * NP + c] = broadcast ? x0[d] : x0[(size_t)d * N + c];
    HIP_TRY(h, hipMemcpyAsync(h->d_q, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_pm, 0, sizeof(double) * NP * D, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_lane_f64, 0, sizeof(double) * NP * SMCMC_LANE_F64_COUNT_, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_lane_i32, 0, sizeof(int32_t) * NP * SMCMC_LANE_I32_COUNT_, h->stream));
    h->step_count = 0;                                   // :211
    h->mean_epsilon = 0.05;                              // :229
    HmcParams p = hmc_params(h, 0, 1);
    hipError_t e = hmc_dispatch(h, p);
    if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("hmc start launch: ") + hipGetErrorString(e));
    // fCurrentAcceptance = fTargetAcceptance = 0.65 (:234-235)
    std::vector<double> acc(NP, 0.0);
    for (int c = 0; c < N; ++c) acc[c] = 0.65;
    HIP_TRY(h, hipMemcpyAsync(h->d_lane_f64 + (size_t)SMCMC_LANE_ACCEPTANCE * NP, acc.data(), NP * sizeof(double),
                              hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // every chain's own fMeanEpsilon = 0.05 (:229), fLeapFrogSteps as the constructor / SetLeapFrog left it, fReversalLen = 0
    st = hmc_fill_lane<double>(h, h->d_lane_f64 + (size_t)kHmcLaneMeanEpsilon * NP, h->mean_epsilon);
    if (st) return st;
    st = hmc_fill_lane<int32_t>(h, h->d_lane_i32 + (size_t)kHmcLaneLeapfrog * NP, (int32_t)h->leapfrog);
    if (st) return st;
    // the running covariance starts from chain 0's point (:236-266)
    std::vector<double> p0(D);
    for (int d = 0; d < D; ++d) p0[d] = x[(size_t)d * NP];
    h->shared->start(p0.data());
    if (hmc_per_chain(h)) {
        st = hmc_pc_start(h, x);
        if (st) return st;
    }
    h->shared_on_device = false;   // pushed again at the next pooled update
    h->host_stale = false;
    h->cov_dirty = true;
    h->steps_in_window = 0;
    h->snap_valid = false;         // a snapshot belongs to the run it was taken in
    if (h->d_gacc) HIP_TRY(h, hipMemsetAsync(h->d_gacc, 0, sizeof(double) * fold_gacc_doubles(h->dim), h->stream));
    h->started = true;
    return SMCMC_OK;
}

}  // extern "C"

namespace {

// nsteps x Step(false) for every chain; sv.x != nullptr: with the trace of smcmc_hmc_step_save.  after_step (per-chain
// mode only): called on the stream's order after each step's update, with the index of the step in the call
template <typename AfterStep>
int hmc_run(smcmc_hmc* h, int nsteps, HmcSave sv, AfterStep&& after_step) {
    if (nsteps <= 0) return SMCMC_OK;
    if (hmc_no_own_gradient(h->likelihood) && !hmc_generic_gradient(h))
        return fail(h, SMCMC_ERR_RUNTIME, "the likelihood has no gradient (TSimpleHMC.H:85-89: its functor returns false): "
                                           "choose gradient type 2 (covariant), 3 (finite differences) or 5 (none)");
    if (hmc_generic_gradient(h)) {
        if (!h->exact) return fail(h, SMCMC_ERR_UNSUPPORTED, "gradient types 2, 3 and 5 run in reference-order arithmetic only");
        int gst = hmc_generic_buffers(h);
        if (gst) return gst;
    } else if (hmc_gradient_matrix(h)) {
        int gst = hmc_generic_buffers(h);   // the gradient matrix in the layout of the kernel that runs
        if (gst) return gst;
    }
    if (hmc_per_chain(h)) {
        // every chain tunes itself after every step (:337-341), whatever is fixed; nothing waits on the device
        for (int s = 0; s < nsteps; ++s) {
            int st = hmc_one_step(h, sv);
            if (st) return st;
            st = hmc_pc_update(h);
            if (st) return st;
            st = after_step(s);
            if (st) return st;
        }
        return SMCMC_OK;
    }
    if (!hmc_tracking(h)) {
        // fixed step length and leapfrog count: the chains share nothing, one launch runs all the steps -- or, with a
        // trace and a kernel that does not write it, one launch up to each save step
        const bool cut = sv.x != nullptr && !hmc_saves_in_kernel(h);
        while (sv.done < nsteps) {
            int n = nsteps - sv.done;
            const bool to_slot = cut && sv.done + sv.stride <= (nsteps / sv.stride) * sv.stride;
            if (to_slot) n = sv.stride;
            HmcParams p = hmc_params(h, n, 0);
            const HmcSaveArgs args = hmc_save_args(sv);
            hipError_t e = hmc_dispatch(h, p, (sv.x != nullptr && !cut) ? &args : nullptr);
            if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("hmc step launch: ") + hipGetErrorString(e));
            h->step_count += (uint32_t)n;
            sv.done += n;
            if (to_slot) {
                int st = hmc_save_slot(h, sv, sv.done / sv.stride - 1);
                if (st) return st;
            }
        }
        return SMCMC_OK;
    }
    int st = hmc_tracking_buffers(h);
    if (st) return st;
    for (int s = 0; s < nsteps; ++s) {
        if (h->gradient_type == 2 && h->cov_dirty) {
            st = hmc_generic_buffers(h);
            if (st) return st;
        }
        st = hmc_one_step(h, sv);
        if (st) return st;
        // UpdateCovariance (:338): the point each chain stood on, if its proposal's potential was finite (:336)
        const double* qprev = h->d_qprev;
        hipError_t e = smcmc::fold_points(h->fold, &qprev, 1, h->d_zero, h->d_lane_i32 + (size_t)kHmcLaneContributes * h->npad,
                                          h->d_gacc, h->stream);
        if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("fold launch: ") + hipGetErrorString(e));
        if (++h->steps_in_window >= h->sync_every) {
            st = hmc_sync(h);
            if (st) return st;
        }
    }
    return SMCMC_OK;
}

// ---- smcmc_hmc_step_recorded ----
// the row of one chain after a step and its update: what smcmc_hmc_read_state, the lanes and smcmc_hmc_read_chain_tuning
// would return at that moment
__global__ void __launch_bounds__(kWave) hmc_record_kernel(const double* q, const double* avg, const double* lane_f64,
                                                           const int32_t* lane_i32, const double* scal, int npad, int dim,
                                                           int chain, uint32_t step_count, double* row) {
    const size_t NP = (size_t)npad;
    for (int i = threadIdx.x; i < dim; i += kWave) {
        row[i] = q[(size_t)i * NP + chain];
        row[dim + i] = avg[(size_t)i * NP + chain];
    }
    double* sc = row + 2 * dim;
    if (threadIdx.x == 0) {
        sc[SMCMC_HMC_REC_POTENTIAL] = -lane_f64[(size_t)SMCMC_LANE_LOGL * NP + chain];
        sc[SMCMC_HMC_REC_PROPOSED_POTENTIAL] = -lane_f64[(size_t)SMCMC_LANE_LOGL_PROPOSED * NP + chain];
        sc[SMCMC_HMC_REC_ACCEPTANCE] = lane_f64[(size_t)SMCMC_LANE_ACCEPTANCE * NP + chain];
        sc[SMCMC_HMC_REC_LAST_ACCEPT] = (double)lane_i32[(size_t)SMCMC_LANE_LAST_ACCEPT * NP + chain];
        sc[SMCMC_HMC_REC_MEAN_EPSILON] = lane_f64[(size_t)kHmcLaneMeanEpsilon * NP + chain];
        sc[SMCMC_HMC_REC_LEAPFROG] = (double)lane_i32[(size_t)kHmcLaneLeapfrog * NP + chain];
        sc[SMCMC_HMC_REC_REVERSAL_LEN] = lane_f64[(size_t)kHmcLaneReversalLen * NP + chain];
        sc[SMCMC_HMC_REC_STEP_COUNT] = (double)step_count;
    }
    if (threadIdx.x < kPcTuningFields) sc[SMCMC_HMC_REC_TUNING0 + threadIdx.x] = scal[(size_t)threadIdx.x * NP + chain];
}

// the arrays of a snapshot (SMCMC_MODE_PER_CHAIN, started)
int hmc_snap_arrays(smcmc_hmc* h, void** arr, size_t* bytes) {
    const size_t D = (size_t)h->dim, NP = (size_t)h->npad;
    arr[0] = h->d_q; bytes[0] = sizeof(double) * D * NP;
    arr[1] = h->d_pm; bytes[1] = sizeof(double) * D * NP;
    arr[2] = h->d_lane_f64; bytes[2] = sizeof(double) * NP * SMCMC_LANE_F64_COUNT_;
    arr[3] = h->d_lane_i32; bytes[3] = sizeof(int32_t) * NP * SMCMC_LANE_I32_COUNT_;
    arr[4] = h->d_qprev; bytes[4] = sizeof(double) * D * NP;
    arr[5] = h->d_pc_avg; bytes[5] = sizeof(double) * D * NP;
    arr[6] = h->d_pc_exxt; bytes[6] = sizeof(double) * pc_npacked(h->dim) * NP;
    arr[7] = h->d_pc_covdiag; bytes[7] = sizeof(double) * D * NP;
    arr[8] = h->d_pc_scal; bytes[8] = sizeof(double) * kPcCount * NP;
    for (int k = 0; k < kHmcSnapArrays; ++k)
        if (!arr[k]) return fail(h, SMCMC_ERR_LOGIC, "the ensemble has not been started in SMCMC_MODE_PER_CHAIN");
    return SMCMC_OK;
}

}  // namespace

extern "C" {

int smcmc_hmc_step(smcmc_hmc* h, int nsteps) {
    if (!h) return SMCMC_ERR_INVALID;
    if (!h->started) return fail(h, SMCMC_ERR_INVALID, "Must initialize starting point");   // :280-284
    if (nsteps <= 0) return SMCMC_OK;
    ON_DEVICE(h);
    return hmc_run(h, nsteps, HmcSave{}, [](int) { return (int)SMCMC_OK; });
}

int smcmc_hmc_step_save(smcmc_hmc* h, int nsteps, int stride, double* save_x_device, double* save_logl_device) {
    if (!h) return SMCMC_ERR_INVALID;
    if (!h->started) return fail(h, SMCMC_ERR_INVALID, "Must initialize starting point");
    if (!save_x_device || stride < 1 || nsteps < 0)
        return fail(h, SMCMC_ERR_INVALID, "smcmc_hmc_step_save: a trace buffer, stride >= 1, nsteps >= 0");
    ON_DEVICE(h);
    HmcSave sv;
    sv.x = save_x_device; sv.logl = save_logl_device; sv.stride = stride;
    return hmc_run(h, nsteps, sv, [](int) { return (int)SMCMC_OK; });
}

int smcmc_hmc_record_stride(const smcmc_hmc* h) { return h ? 2 * h->dim + SMCMC_HMC_REC_COUNT_ : 0; }

int smcmc_hmc_step_recorded(smcmc_hmc* h, int nsteps, int chain, double* records) {
    if (!h) return SMCMC_ERR_INVALID;
    if (!h->started) return fail(h, SMCMC_ERR_INVALID, "Must initialize starting point");
    if (!records) return fail(h, SMCMC_ERR_INVALID, "smcmc_hmc_step_recorded: no record array");
    if (!hmc_per_chain(h))
        return fail(h, SMCMC_ERR_UNSUPPORTED, "smcmc_hmc_step_recorded serves SMCMC_MODE_PER_CHAIN (the pooled update decides on the host)");
    if (chain < 0 || chain >= h->nchains) return fail(h, SMCMC_ERR_INVALID, "no such chain");
    if (nsteps <= 0) return SMCMC_OK;
    ON_DEVICE(h);
    const int stride = smcmc_hmc_record_stride(h);
    const size_t need = (size_t)nsteps * stride;
    if (need > h->d_rec.size()) HIP_TRY(h, h->d_rec.allocate(need));
    const int st = hmc_run(h, nsteps, HmcSave{}, [&](int s) {
        hipLaunchKernelGGL(hmc_record_kernel, dim3(1), dim3(kWave), 0, h->stream, (const double*)h->d_q, (const double*)h->d_pc_avg,
                           (const double*)h->d_lane_f64, (const int32_t*)h->d_lane_i32, (const double*)h->d_pc_scal, h->npad,
                           h->dim, chain, h->step_count, h->d_rec + (size_t)s * stride);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(h, SMCMC_ERR_HIP, std::string("record launch: ") + hipGetErrorString(e));
        return (int)SMCMC_OK;
    });
    if (st) return st;
    HIP_TRY(h, hipMemcpyAsync(records, h->d_rec, need * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SMCMC_OK;
}

int smcmc_hmc_snapshot(smcmc_hmc* h) {
    if (!h) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    if (!hmc_per_chain(h)) return fail(h, SMCMC_ERR_UNSUPPORTED, "smcmc_hmc_snapshot serves SMCMC_MODE_PER_CHAIN");
    if (!h->started) return fail(h, SMCMC_ERR_INVALID, "Must initialize starting point");
    void* arr[kHmcSnapArrays]; size_t bytes[kHmcSnapArrays];
    int st = hmc_snap_arrays(h, arr, bytes);
    if (st) return st;
    h->snap_valid = false;
    for (int k = 0; k < kHmcSnapArrays; ++k) {
        if (h->snap[k].size() == bytes[k]) continue;
        const hipError_t e = h->snap[k].allocate(bytes[k]);
        if (e != hipSuccess) {
            // a second copy of the per-chain state does not fit: nothing is kept, and the engine steps on as it was
            for (int j = 0; j < kHmcSnapArrays; ++j) h->snap[j] = DeviceBuffer<unsigned char>();
            (void)hipGetLastError();
            return fail(h, SMCMC_ERR_HIP, std::string("the snapshot does not fit in device memory: ") + hipGetErrorString(e));
        }
    }
    for (int k = 0; k < kHmcSnapArrays; ++k)
        HIP_TRY(h, hipMemcpyAsync(h->snap[k], arr[k], bytes[k], hipMemcpyDeviceToDevice, h->stream));
    h->snap_step_count = h->step_count;
    h->snap_valid = true;
    return SMCMC_OK;
}

int smcmc_hmc_rollback(smcmc_hmc* h) {
    if (!h) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    if (!hmc_per_chain(h)) return fail(h, SMCMC_ERR_UNSUPPORTED, "smcmc_hmc_rollback serves SMCMC_MODE_PER_CHAIN");
    if (!h->started) return fail(h, SMCMC_ERR_INVALID, "Must initialize starting point");
    if (!h->snap_valid) return fail(h, SMCMC_ERR_LOGIC, "no snapshot to return to");
    void* arr[kHmcSnapArrays]; size_t bytes[kHmcSnapArrays];
    int st = hmc_snap_arrays(h, arr, bytes);
    if (st) return st;
    for (int k = 0; k < kHmcSnapArrays; ++k)
        HIP_TRY(h, hipMemcpyAsync(arr[k], h->snap[k], bytes[k], hipMemcpyDeviceToDevice, h->stream));
    h->step_count = h->snap_step_count;
    return SMCMC_OK;
}

// the pooled update now, whatever the interval (a partial window at the end of a run)
int smcmc_hmc_sync(smcmc_hmc* h) {
    if (!h) return SMCMC_ERR_INVALID;
    if (hmc_per_chain(h)) return SMCMC_OK;   // nothing is pooled
    if (!h->started) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    if (!h->d_gacc) return SMCMC_OK;
    return hmc_sync(h);
}

// The same in pieces, for an ensemble sharded over engines / ranks: reduce, export, (sum over ranks), import, apply.
int smcmc_hmc_moments_size(const smcmc_hmc* h) { return h ? (int)moments_packed(h->dim) : 0; }

int smcmc_hmc_reduce_moments(smcmc_hmc* h) {
    if (!h) return SMCMC_ERR_INVALID;
    if (hmc_per_chain(h)) return fail(h, SMCMC_ERR_LOGIC, "SMCMC_MODE_PER_CHAIN pools no moments: shard by chain_offset");
    if (!h->started) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    int st = hmc_tracking_buffers(h);
    if (st) return st;
    return hmc_reduce(h);
}

int smcmc_hmc_export_moments(smcmc_hmc* h, double* dst_device) {
    if (h && hmc_per_chain(h)) return fail(h, SMCMC_ERR_LOGIC, "SMCMC_MODE_PER_CHAIN pools no moments: shard by chain_offset");
    if (!h || !dst_device || !h->d_moments) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    HIP_TRY(h, hipMemcpyAsync(dst_device, h->d_moments, sizeof(double) * (size_t)smcmc_hmc_moments_size(h), hipMemcpyDeviceToDevice,
                              h->stream));
    return SMCMC_OK;
}

int smcmc_hmc_import_moments(smcmc_hmc* h, const double* src_device) {
    if (h && hmc_per_chain(h)) return fail(h, SMCMC_ERR_LOGIC, "SMCMC_MODE_PER_CHAIN pools no moments: shard by chain_offset");
    if (!h || !src_device || !h->d_moments) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    HIP_TRY(h, hipMemcpyAsync(h->d_moments, src_device, sizeof(double) * (size_t)smcmc_hmc_moments_size(h), hipMemcpyDeviceToDevice,
                              h->stream));
    return SMCMC_OK;
}

int smcmc_hmc_apply_moments(smcmc_hmc* h) {
    if (h && hmc_per_chain(h)) return fail(h, SMCMC_ERR_LOGIC, "SMCMC_MODE_PER_CHAIN pools no moments: shard by chain_offset");
    if (!h || !h->started || !h->d_moments) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    return hmc_apply(h);
}

int smcmc_hmc_read_state(smcmc_hmc* h, double* q, double* momentum, double* logl) {
    if (!h) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    const int D = h->dim, N = h->nchains;
    const size_t NP = (size_t)h->npad;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (q) HIP_TRY(h, hipMemcpy2D(q, (size_t)N * sizeof(double), h->d_q, NP * sizeof(double), (size_t)N * sizeof(double),
                                  (size_t)D, hipMemcpyDeviceToHost));
    if (momentum) HIP_TRY(h, hipMemcpy2D(momentum, (size_t)N * sizeof(double), h->d_pm, NP * sizeof(double),
                                         (size_t)N * sizeof(double), (size_t)D, hipMemcpyDeviceToHost));
    if (logl) HIP_TRY(h, hipMemcpy(logl, h->d_lane_f64 + (size_t)SMCMC_LANE_LOGL * NP, (size_t)N * sizeof(double),
                                   hipMemcpyDeviceToHost));
    return SMCMC_OK;
}

int smcmc_hmc_copy_positions(smcmc_hmc* h, double* dst_device) {
    if (!h || !dst_device || !h->started) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    HIP_TRY(h, hipMemcpyAsync(dst_device, h->d_q, sizeof(double) * (size_t)h->dim * h->npad, hipMemcpyDeviceToDevice, h->stream));
    return SMCMC_OK;
}

int smcmc_hmc_nchains_padded(const smcmc_hmc* h) { return h ? h->npad : 0; }

int smcmc_hmc_read_lane_f64(smcmc_hmc* h, int field, double* out) {
    if (!h || !out || field < 0 || field >= SMCMC_LANE_F64_COUNT_) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, h->d_lane_f64 + (size_t)field * h->npad, (size_t)h->nchains * sizeof(double),
                         hipMemcpyDeviceToHost));
    return SMCMC_OK;
}

int smcmc_hmc_read_lane_i32(smcmc_hmc* h, int field, int32_t* out) {
    if (!h || !out || field < 0 || field >= SMCMC_LANE_I32_COUNT_) return SMCMC_ERR_INVALID;
    ON_DEVICE(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, h->d_lane_i32 + (size_t)field * h->npad, (size_t)h->nchains * sizeof(int32_t),
                         hipMemcpyDeviceToHost));
    return SMCMC_OK;
}

}  // extern "C"

// :760-830 on one covariance: device >= 0 the per-chain mode's device routine (hmc_pc_selftest_kernel), device < 0 the
// host's HmcShared.  out: [dim*dim] covariance after the repair loop, [dim] eigenvalues of the last pass, max scale,
// min scale, repair passes, trace, orbit length
extern "C" int smcmc_selftest_hmc_error_matrix(int device, int dim, double est_trace, const double* cov, double* out) {
    if (dim < 1 || dim > kPcMaxDim || !cov || !out) return SMCMC_ERR_INVALID;
    const size_t D = (size_t)dim, nout = D * D + D + 5;
    if (device < 0) {
        HmcShared S(dim);
        S.cov.assign(cov, cov + D * D);
        S.estTrace = est_trace;
        std::vector<double> eig(D);
        int passes = 0;
        S.scaleFromCovariance(eig, passes);
        std::copy(S.cov.begin(), S.cov.end(), out);
        std::copy(eig.begin(), eig.end(), out + D * D);
        double* t = out + D * D + D;
        t[0] = S.maxScale; t[1] = S.minScale; t[2] = passes; t[3] = S.curTrace; t[4] = S.orbitLength;
        return SMCMC_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device >= ndev) return SMCMC_ERR_NO_DEVICE;
    DeviceGuard guard(device);
    DeviceBuffer<double> d_cov, d_out, d_scratch;
    if (d_cov.allocate(D * D) != hipSuccess || d_out.allocate(nout) != hipSuccess || d_scratch.allocate(D * D) != hipSuccess)
        return SMCMC_ERR_HIP;
    if (hipMemcpy(d_cov, cov, sizeof(double) * D * D, hipMemcpyHostToDevice) != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(hmc_pc_selftest_kernel, dim3(1), dim3(kWave), 0, nullptr, dim, est_trace, (const double*)d_cov,
                       d_scratch.get(), d_out.get());
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost) != hipSuccess)
        return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
