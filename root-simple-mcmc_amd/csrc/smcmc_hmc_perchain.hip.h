// smcmc_hmc_perchain.hip.h -- SMCMC_MODE_PER_CHAIN of the HMC engine: every chain keeps its own running covariance and
// runs UpdateCovariance (reference TSimpleHMC.H:665-695) and UpdateErrorMatrix (:703-858) on it after each of its steps,
// as a TSimpleHMC chain does.  Three launches follow every step kernel (adaptive = 1), none waits on the host:
//   hmc_pc_exxt_kernel     fEXXT of every contributing chain (:681-691), one thread per (chain, run of packed elements);
//   hmc_pc_decide_kernel   fAveragePoint (:671-677), the trial counts (:678-679, 692-693), the step counters (:667-668),
//                          the trace and the decision of :704-719, one thread per chain; a chain whose update goes
//                          through is appended to a device work list;
//   hmc_pc_error_kernel    a fixed grid of one-wavefront workgroups drains the list: eigenvalues of the chain's
//                          covariance with the repair loop (:760-830), then the new step length and leapfrog count
//                          (:833-847).
// Storage is [element][chain] throughout (a wavefront's 64 lanes read 64 consecutive doubles).  fEstimatedCovariance is
// not stored: after an UpdateCovariance it is fEXXT - avg avg^T element for element (:689), which is what the error
// kernel and the readback compute; the repair loop (:793-808) leaves a diagonal matrix, kept as its diagonal until the
// chain's next UpdateCovariance.
//
// The eigenvalues are HmcShared::eigenvalues (smcmc_hmc_shared.hpp) statement for statement; only sums that are
// independent of each other are spread over the lanes (each g of the j loop, the rank-2 update element by element,
// the new e[j]).  The serial parts (scale, h, f, the QL sweeps) run on lane 0 in the host's order.  The library is
// built with -ffp-contract=off, and the device's double division and sqrt are correctly rounded (smcmc_selftest_detmath
// kinds 5 and 6), so the bits are the host's; smcmc_selftest_hmc_error_matrix checks it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smcmc.h"
#include "smcmc_hmc_kernel.hip.h"

namespace smcmc {

// per-chain tuning scalars, [field][npad]; fields 0..9 are the layout of smcmc_hmc_get_tuning
enum {
    kPcTrace = 0, kPcOrbit, kPcUpdates, kPcCovTrials, kPcAverageTrials, kPcStepsRemaining, kPcStepsSinceUpdate,
    kPcMaxScale, kPcMinScale, kPcEstTrace,
    kPcCovState,   // 0: fEstimatedCovariance = fEXXT - avg avg^T (the identity while cov_trials == 0); 1: the repaired diagonal
    kPcCount
};
constexpr int kPcTuningFields = 10;
constexpr int kPcLdsDim = 63;          // up to this dimension the error kernel keeps the matrix in LDS
constexpr int kPcMaxDim = 512;
constexpr int kPcExxtRun = 32;         // packed elements per thread of hmc_pc_exxt_kernel

struct HmcPcParams {
    int nchains, npad, dim;
    int step_count;              // fStepCount after the step (:760)
    double cov_window;           // fCovarianceWindow (:134)
    const double* qprev;         // the point each chain stood on before the step (:338)   [dim][npad]
    const int32_t* contributes;  // kHmcLaneContributes                                       [npad]
    double* lane_f64;            // fMeanEpsilon lane
    int32_t* lane_i32;           // fLeapFrogSteps lane
    double* avg;                 // fAveragePoint                                             [dim][npad]
    double* exxt;                // fEXXT, packed rows: k = i (i + 1) / 2 + j, j <= i         [packed][npad]
    double* covdiag;             // the repaired diagonal (kPcCovState == 1)                  [dim][npad]
    double* scal;                // [kPcCount][npad]
    int32_t* work;               // [0] chains whose update goes through this step, [1 + k] their indices
    double* scratch;             // dim > kPcLdsDim: [grid][dim * dim] matrix images
};

__host__ __device__ inline size_t pc_npacked(int D) { return (size_t)D * (D + 1) / 2; }

// ---- UpdateCovariance :681-691 for every (chain, element): v *= t; v += x_i x_j; v /= t + 1 ----
// x_i x_j is the one-point moment fma(x_i, x_j, 0), the pooled fold's arithmetic with one point
__global__ void __launch_bounds__(256) hmc_pc_exxt_kernel(const HmcPcParams p) {
    const int c = blockIdx.x * kWave + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) p.work[0] = 0;   // this step's list
    if (c >= p.nchains) return;
    const size_t NP = (size_t)p.npad;
    if (p.contributes[c] == 0) return;
    const int D = p.dim;
    const size_t np = pc_npacked(D);
    const size_t k0 = ((size_t)blockIdx.y * blockDim.y + threadIdx.y) * kPcExxtRun;
    if (k0 >= np) return;
    const size_t k1 = (k0 + kPcExxtRun < np) ? k0 + kPcExxtRun : np;
    // row i of the first element: i (i + 1) / 2 <= k0 < (i + 1) (i + 2) / 2
    int i = (int)((__builtin_sqrt(8.0 * (double)k0 + 1.0) - 1.0) * 0.5);
    while ((size_t)i * (i + 1) / 2 > k0) --i;
    while ((size_t)(i + 1) * (i + 2) / 2 <= k0) ++i;
    int j = (int)(k0 - (size_t)i * (i + 1) / 2);
    const double t = p.scal[(size_t)kPcCovTrials * NP + c];
    // one element after the other: with 40 waves per CU in flight this measured faster than batching the loads
    // (more registers, fewer waves)
    double xi = p.qprev[(size_t)i * NP + c];
    for (size_t k = k0; k < k1; ++k) {
        const double xj = p.qprev[(size_t)j * NP + c];
        double v = p.exxt[k * NP + c];
        v *= t;
        v += __builtin_fma(xi, xj, 0.0);
        v /= t + 1.0;
        p.exxt[k * NP + c] = v;
        if (++j > i) {
            ++i;
            j = 0;
            if (i < D) xi = p.qprev[(size_t)i * NP + c];
        }
    }
}

// ---- the rest of UpdateCovariance and the decision of UpdateErrorMatrix (:704-719), one thread per chain ----
__global__ void __launch_bounds__(256) hmc_pc_decide_kernel(const HmcPcParams p) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.nchains) return;
    if (p.contributes[c] == 0) return;                                    // :336: no UpdateCovariance, no update
    const int D = p.dim;
    const size_t NP = (size_t)p.npad;
    double* sc = p.scal + c;
    const double steps_since = sc[kPcStepsSinceUpdate * NP] + 1.0;       // :667-668
    const double steps_rem = sc[kPcStepsRemaining * NP] - 1.0;
    const double at = sc[kPcAverageTrials * NP];
    double trace = 0.0;
    constexpr int kB = 16;   // every load of a batch before its first store (the stores may alias them)
    for (int i0 = 0; i0 < D; i0 += kB) {
        double av[kB], xv[kB], ev[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int i = i0 + u;
            if (i < D) {
                av[u] = p.avg[(size_t)i * NP + c];
                xv[u] = p.qprev[(size_t)i * NP + c];
                ev[u] = p.exxt[((size_t)i * (i + 1) / 2 + i) * NP + c];
            }
        }
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int i = i0 + u;
            if (i < D) {                                                  // :671-677
                double v = av[u];
                v *= at;
                v += __builtin_fma(1.0, xv[u], 0.0);
                v /= at + 1.0;
                p.avg[(size_t)i * NP + c] = v;
                trace += __builtin_fabs(ev[u] - v * v);                   // :689 on the diagonal, :708-711 in index order
            }
        }
    }
    const double cov_trials = __builtin_fmin(p.cov_window, sc[kPcCovTrials * NP] + 1.0);   // :692-693
    sc[kPcAverageTrials * NP] = __builtin_fmin(p.cov_window, at + 1.0);  // :678-679
    sc[kPcCovTrials * NP] = cov_trials;
    sc[kPcStepsSinceUpdate * NP] = steps_since;
    sc[kPcStepsRemaining * NP] = steps_rem;
    sc[kPcCovState * NP] = 0.0;
    if (p.lane_i32[(size_t)kHmcLaneLeapfrog * NP + c] == 0) return;      // :704
    if (cov_trials < 2 * D) return;                                       // :705
    sc[kPcTrace * NP] = trace;
    const double est = sc[kPcEstTrace * NP];
    const double change = __builtin_fabs(trace - est);
    bool do_it = false;                                                   // :715-719
    if (steps_rem < 0) do_it = true;
    if (steps_since > 2.0 * D && change > 0.01 * est) do_it = true;
    if (!do_it) return;
    const int slot = atomicAdd(p.work, 1);
    p.work[1 + slot] = c;
}

// ---- :760-830 on one covariance, by one wavefront ----
struct PcErrorOut {
    double max_scale, min_scale, trace, orbit;
    int passes;   // repair passes (:793-808); > 0: the covariance is now diag[]
};

// Eigenvalues of the symmetric D x D matrix a (destroyed) into d: HmcShared::eigenvalues statement for statement.
// d, e, sh in LDS; a in LDS or global memory.  Called by all 64 lanes; d is valid on return in every lane.
__device__ inline void pc_eigenvalues(double* a, int n, double* d, double* e, double* sh) {
    const int tid = threadIdx.x;
    for (int k = tid; k <= n; k += kWave) e[k] = 0.0;
    __syncthreads();
    for (int i = n - 1; i >= 1; --i) {
        const int l = i - 1;
        double* ai = a + (size_t)i * n;
        if (l > 0) {
            if (tid == 0) {
                double scale = 0.0;
                for (int k = 0; k <= l; ++k) scale += __builtin_fabs(ai[k]);
                sh[0] = scale;
            }
            __syncthreads();
            const double scale = sh[0];
            if (scale == 0.0) {
                if (tid == 0) e[i] = ai[l];
            } else {
                for (int k = tid; k <= l; k += kWave) ai[k] /= scale;
                __syncthreads();
                if (tid == 0) {
                    double h = 0.0;
                    for (int k = 0; k <= l; ++k) h += ai[k] * ai[k];
                    const double f = ai[l];
                    const double g = (f >= 0.0) ? -__builtin_sqrt(h) : __builtin_sqrt(h);
                    e[i] = scale * g;
                    h -= f * g;
                    ai[l] = f - g;
                    sh[1] = h;
                }
                __syncthreads();
                const double h = sh[1];
                for (int j = tid; j <= l; j += kWave) {                   // each g its own ordered sum over k
                    double g = 0.0;
                    for (int k = 0; k <= j; ++k) g += a[(size_t)j * n + k] * ai[k];
                    for (int k = j + 1; k <= l; ++k) g += a[(size_t)k * n + j] * ai[k];
                    e[j] = g / h;
                }
                __syncthreads();
                if (tid == 0) {
                    double f = 0.0;
                    for (int j = 0; j <= l; ++j) f += e[j] * ai[j];
                    sh[2] = f / (h + h);
                }
                __syncthreads();
                const double hh = sh[2];
                for (int j = tid; j <= l; j += kWave) e[j] = e[j] - hh * ai[j];
                __syncthreads();
                // a[j][k] -= (f e[k] + g a[i][k]) with f = a[i][j], g = the new e[j]: every element once
                const int w = l + 1;
                for (int idx = tid; idx < w * w; idx += kWave) {
                    const int j = idx / w, k = idx - j * w;
                    if (k <= j) a[(size_t)j * n + k] -= (ai[j] * e[k] + e[j] * ai[k]);
                }
            }
        } else {
            if (tid == 0) e[i] = ai[l];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int i = 0; i < n; ++i) d[i] = a[(size_t)i * n + i];
        for (int i = 1; i < n; ++i) e[i - 1] = e[i];
        e[n - 1] = 0.0;
        for (int l = 0; l < n; ++l) {
            int iter = 0, m;
            do {
                for (m = l; m < n - 1; ++m) {
                    const double dd = __builtin_fabs(d[m]) + __builtin_fabs(d[m + 1]);
                    if (__builtin_fabs(e[m]) + dd == dd) break;
                }
                if (m != l) {
                    if (iter++ == 60) break;
                    double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                    double r = __builtin_sqrt(g * g + 1.0);
                    g = d[m] - d[l] + e[l] / (g + ((g >= 0.0) ? __builtin_fabs(r) : -__builtin_fabs(r)));
                    double s = 1.0, c = 1.0, pp = 0.0;
                    int i;
                    for (i = m - 1; i >= l; --i) {
                        double f = s * e[i];
                        const double b = c * e[i];
                        r = __builtin_sqrt(f * f + g * g);
                        e[i + 1] = r;
                        if (r == 0.0) {
                            d[i + 1] -= pp;
                            e[m] = 0.0;
                            break;
                        }
                        s = f / r;
                        c = g / r;
                        g = d[i + 1] - pp;
                        r = (d[i] - g) * s + 2.0 * c * b;
                        pp = s * r;
                        d[i + 1] = g + pp;
                        g = c * r - b;
                    }
                    if (r == 0.0 && i >= l) continue;
                    d[l] -= pp;
                    e[l] = g;
                    e[m] = 0.0;
                }
            } while (m != l);
        }
    }
    __syncthreads();
}

// :764-830 (HmcShared::finishUpdate without the counters and the inverse): load(i, j) gives the covariance as
// UpdateCovariance left it.  diag receives the repaired diagonal when a repair pass ran.  Valid in lane 0.
template <typename Load>
__device__ inline PcErrorOut pc_error_matrix(double* a, int D, double est_trace, Load&& load, double* d, double* e,
                                             double* diag, double* sh) {
    const int tid = threadIdx.x;
    double max_s = 0.0, min_s = 1E+20;                                    // :764-765
    int passes = 0;
    for (;;) {                                                            // :766-809
        for (int idx = tid; idx < D * D; idx += kWave) {
            const int i = idx / D, j = idx - i * D;
            a[idx] = (passes == 0) ? load(i, j) : ((i == j) ? diag[i] : 0.0);
        }
        __syncthreads();
        pc_eigenvalues(a, D, d, e, sh);
        if (tid == 0) {
            bool positive = true;
            for (int i = 0; i < D; ++i) {
                const double ev = d[i];
                if (max_s < __builtin_fabs(ev)) max_s = __builtin_fabs(ev);
                if (min_s > __builtin_fabs(ev)) min_s = __builtin_fabs(ev);
                if (ev < 0) positive = false;
            }
            sh[3] = positive ? 1.0 : 0.0;
        }
        __syncthreads();
        if (sh[3] != 0.0) break;
        double r = est_trace * 1E-6;
        r /= D;
        r = __builtin_fabs(r);
        for (int i = tid; i < D; i += kWave) {
            double v = (passes == 0) ? load(i, i) : diag[i];
            if (v < r) v = r;
            diag[i] = v;
        }
        ++passes;
        __syncthreads();
    }
    PcErrorOut o;
    o.passes = passes;
    double trace = 0.0;                                                   // :815-819
    if (tid == 0)
        for (int i = 0; i < D; ++i) trace += __builtin_fabs((passes == 0) ? load(i, i) : diag[i]);
    o.trace = trace;
    max_s = __builtin_sqrt(max_s);                                        // :822-827
    if (max_s < 0.1) max_s = 0.1;
    min_s = __builtin_sqrt(min_s);
    if (min_s < 0.01) min_s = 0.01;
    o.orbit = 2.0 * 3.14 * max_s;                                         // :830
    o.max_scale = max_s;
    o.min_scale = min_s;
    return o;
}

struct PcLds {
    double a[kPcLdsDim * kPcLdsDim];
    double d[kPcMaxDim], e[kPcMaxDim + 1], diag[kPcMaxDim], sh[8];
};

// ---- the chains whose update goes through: a fixed grid of one-wavefront workgroups drains the list ----
__global__ void __launch_bounds__(kWave) hmc_pc_error_kernel(const HmcPcParams p) {
    __shared__ PcLds s;
    const int D = p.dim;
    const size_t NP = (size_t)p.npad;
    const int count = p.work[0];
    double* a = (D <= kPcLdsDim) ? s.a : p.scratch + (size_t)blockIdx.x * D * D;
    for (int item = blockIdx.x; item < count; item += gridDim.x) {
        const int c = p.work[1 + item];
        double* sc = p.scal + c;
        const double est = sc[kPcEstTrace * NP];
        auto load = [&](int i, int j) {                                   // :689
            const int r = (i >= j) ? i : j, q = (i >= j) ? j : i;
            return p.exxt[((size_t)r * (r + 1) / 2 + q) * NP + c] - p.avg[(size_t)i * NP + c] * p.avg[(size_t)j * NP + c];
        };
        const PcErrorOut o = pc_error_matrix(a, D, est, load, s.d, s.e, s.diag, s.sh);
        if (o.passes > 0)
            for (int i = threadIdx.x; i < D; i += kWave) p.covdiag[(size_t)i * NP + c] = s.diag[i];
        if (threadIdx.x == 0) {
            sc[kPcStepsRemaining * NP] = 2.0 * D + p.step_count;          // :760
            sc[kPcStepsSinceUpdate * NP] = 0.0;
            sc[kPcTrace * NP] = o.trace;
            sc[kPcEstTrace * NP] = o.trace;
            sc[kPcMaxScale * NP] = o.max_scale;
            sc[kPcMinScale * NP] = o.min_scale;
            sc[kPcOrbit * NP] = o.orbit;
            sc[kPcUpdates * NP] = sc[kPcUpdates * NP] + 1.0;
            sc[kPcCovState * NP] = (o.passes > 0) ? 1.0 : 0.0;
            // :833-847, the chain's own step length and leapfrog count (hmc_retune_kernel for one chain)
            double eps = p.lane_f64[(size_t)kHmcLaneMeanEpsilon * NP + c];
            int L = p.lane_i32[(size_t)kHmcLaneLeapfrog * NP + c];
            if (eps > 0) {
                eps = 0.2 * o.max_scale;
                if (eps > 0.5 * o.min_scale) eps = 0.5 * o.min_scale;
                if (eps < 0.05 * o.max_scale) eps = 0.05 * o.max_scale;
            }
            if (L > 0) {
                const double target = 0.4 * o.orbit;
                L = (int)(target / __builtin_fabs(eps));
                L = 2 * (L / 2 + 1);
                if (L > 3 * D) L = 3 * D;
                if (eps > 0) eps = target / L;
            }
            p.lane_f64[(size_t)kHmcLaneMeanEpsilon * NP + c] = eps;
            p.lane_i32[(size_t)kHmcLaneLeapfrog * NP + c] = L;
        }
        __syncthreads();
    }
}

// ---- smcmc_selftest_hmc_error_matrix's device side: one covariance, one workgroup ----
// out: [D*D] the covariance after the repair loop, [D] the eigenvalues of the last pass, then max scale, min scale,
// repair passes, trace, orbit
__global__ void __launch_bounds__(kWave) hmc_pc_selftest_kernel(int D, double est_trace, const double* cov, double* scratch,
                                                                 double* out) {
    __shared__ PcLds s;
    double* a = (D <= kPcLdsDim) ? s.a : scratch;
    auto load = [&](int i, int j) { return cov[(size_t)i * D + j]; };
    const PcErrorOut o = pc_error_matrix(a, D, est_trace, load, s.d, s.e, s.diag, s.sh);
    for (int idx = threadIdx.x; idx < D * D; idx += kWave) {
        const int i = idx / D, j = idx - i * D;
        out[idx] = (o.passes == 0) ? cov[idx] : ((i == j) ? s.diag[i] : 0.0);
    }
    for (int i = threadIdx.x; i < D; i += kWave) out[(size_t)D * D + i] = s.d[i];
    if (threadIdx.x == 0) {
        double* t = out + (size_t)D * D + D;
        t[0] = o.max_scale; t[1] = o.min_scale; t[2] = o.passes; t[3] = o.trace; t[4] = o.orbit;
    }
}

}  // namespace smcmc
