// smcmc_autocorr_grid.hip -- the lagged-product sums of a saved trace on a lag grid k_i = lag_first + i * lag_step:
// what MakeAutocorrelation.C:98-124 evaluates (lags 1, 1 + lagStep, ... < maxLag, about 200 of them spread over up to
// 30 000 slots), where smcmc_autocorr.hip covers the 64 consecutive lags 0 .. 63 only.  The inner block is that
// kernel's: one lane owns one chain of one dimension, a wavefront covers 64 chains and 32 lags (one pass; the passes of
// a call are grid z), and everything sits in registers with static indices -- 16 loaded values, a sliding window of
// the 47 values the 32 lags reach back to, 32 accumulators, 512 fused multiply-adds per 16 loaded values, no LDS.
// A grid of step S keeps that shape because the slots are walked by residue class: for t = r + a S (0 <= r < S) the
// partner of lag k0 + i S is y[(r - k0) + (a - i) S], so per residue r the sums are the contiguous-lag recurrence
//   acc[i] += u[a] * w[a - i],     u[a] = y[r + a S],   w[a] = y[r - k0 + a S]   (0 before the first slot)
// on two decimated sequences.  The loop over r runs outside the block loop inside one lane, the window is zeroed again
// at the start of every residue and the accumulators carry across residues.  Every load is still a coalesced
// 512-byte piece of a trace row; only the slot stride changes (all slot arithmetic in 64 bits).  A pass whose first
// lag lies beyond the trace loads nothing, and a residue starts at the first block whose window can hold a slot.
// Summation order, fixed (the same bits on every run):
//   per lane   one fused multiply-add per term y_t y_(t-k) into an accumulator that starts at +0, the terms ordered by
//              residue class t mod lag_step ascending, slots ascending inside a class; terms whose partner lies before
//              slot 0 multiply by 0 or are skipped, which is the same (finite trace).  `sum` adds y_t and `sumsq` fuses
//              y_t y_t in that order of t.
//   then       the xor 32, 16, 8, 4, 2, 1 butterfly over the 64 chains of the wavefront,
//   then       chain blocks ascending, from +0.
// So a row's bits depend on (k, lag_step, trace, centre) only, not on lag_first or nlags: a grid split over several
// calls gives the same rows.  With lag_step = 1 the order is slots ascending, which is smcmc_autocorr.hip's: rows
// k < 64 and `sum` then have the bits smcmc_autocorrelation_sums returns.
// Measured times: profiles/autocorr_grid_notes.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smcmc.h"
#include "smcmc_host.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kPassLags = 32;                // lags per wavefront
constexpr int kBlock = 16;                   // decimated slots per register block
constexpr int kWin = kBlock + kPassLags - 1; // w[a0 - 31 .. a0 + 15]

// partial[cb][d][0 .. nrows - 1] the rows of the grid (nrows = 32 * passes), [nrows] sum, [nrows + 1] sumsq
__global__ void __launch_bounds__(kWave) autocorr_grid_partial_kernel(const double* __restrict__ trace, int nslots, int dim,
                                                                      size_t dim_stride, int nchains, size_t npad,
                                                                      const double* __restrict__ centre, int lag_first,
                                                                      int lag_step, int nrows, double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const int cb = blockIdx.x;   // neighbouring workgroups read neighbouring 512-byte pieces of a trace row
    const int d = blockIdx.y;
    const int pass = blockIdx.z;
    const size_t chain = (size_t)cb * kWave + lane;
    const bool active = chain < (size_t)nchains;
    const double c0 = centre[d];
    const double* src = trace + (size_t)d * npad + chain;
    const size_t slot_stride = dim_stride * npad;
    const int64_t S = lag_step;
    const int64_t k0 = lag_first + (int64_t)pass * kPassLags * S;   // the pass's first lag: at most the grid's last, an int
    const bool sums = pass == 0;                                  // the first pass also takes sum and sumsq
    const bool same = k0 == 0;                                    // w is u: load once
    auto y = [&](int64_t t) __attribute__((always_inline)) {
        return (active && t >= 0 && t < nslots) ? src[(size_t)t * slot_stride] - c0 : 0.0;
    };
    double win[kWin], acc[kPassLags], v[kBlock];
#pragma unroll
    for (int k = 0; k < kPassLags; ++k) acc[k] = 0.0;
    double sum = 0.0, sumsq = 0.0;
    if (sums || k0 < nslots) {
        const int64_t nres = S < nslots ? S : nslots;
        for (int64_t r = 0; r < nres; ++r) {
#pragma unroll
            for (int i = 0; i < kWin; ++i) win[i] = 0.0;
            // the first a with r - k0 + a S >= 0: before it every partner of every lag of the pass is 0
            int64_t a = 0;
            if (!sums && k0 > r) a = (int64_t)((uint32_t)(k0 - r - 1) / (uint32_t)lag_step) + 1;
            for (int64_t t0 = r + a * S; t0 < nslots; t0 += kBlock * S) {
#pragma unroll
                for (int j = 0; j < kBlock; ++j) {
                    const int64_t t = t0 + j * S;
                    v[j] = y(t);
                    win[kPassLags - 1 + j] = same ? v[j] : y(t - k0);
                }
                if (sums) {
#pragma unroll
                    for (int j = 0; j < kBlock; ++j) {
                        sum += v[j];
                        sumsq = __builtin_fma(v[j], v[j], sumsq);
                    }
                }
                // acc[i] += u[a0 + j] * w[a0 + j - i]
#pragma unroll
                for (int j = 0; j < kBlock; ++j)
#pragma unroll
                    for (int i = 0; i < kPassLags; ++i) acc[i] = __builtin_fma(v[j], win[kPassLags - 1 + j - i], acc[i]);
#pragma unroll
                for (int i = 0; i < kPassLags - 1; ++i) win[i] = win[i + kBlock];
            }
        }
    }
    // butterfly over the wavefront's chains
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off, kWave);
        sumsq += __shfl_xor(sumsq, off, kWave);
#pragma unroll
        for (int k = 0; k < kPassLags; ++k) acc[k] += __shfl_xor(acc[k], off, kWave);
    }
    if (lane == 0) {
        double* out = partial + ((size_t)cb * dim + d) * ((size_t)nrows + 2);
#pragma unroll
        for (int k = 0; k < kPassLags; ++k) out[pass * kPassLags + k] = acc[k];
        if (sums) {
            out[nrows] = sum;
            out[nrows + 1] = sumsq;
        }
    }
}

// out[i][d], i < nlags the rows, then sum, then sumsq: the chain blocks added ascending
__global__ void autocorr_grid_reduce_kernel(const double* __restrict__ partial, int nblocks, int dim, int nlags, int nrows,
                                            double* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= dim * (nlags + 2)) return;
    const int d = idx / (nlags + 2), k = idx % (nlags + 2);
    const int col = k < nlags ? k : nrows + (k - nlags);
    double s = 0.0;
    for (int cb = 0; cb < nblocks; ++cb) s += partial[((size_t)cb * dim + d) * ((size_t)nrows + 2) + col];
    out[(size_t)k * dim + d] = s;
}

}  // namespace

extern "C" int smcmc_autocorrelation_grid_sums(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                               int nchains_padded, const double* centre, int lag_first, int lag_step,
                                               int nlags, double* sum, double* sumsq, double* lagged, void* stream) {
    if (!trace_device || !sum || !sumsq || !lagged) return SMCMC_ERR_INVALID;
    if (nslots < 1 || dim < 1 || dim_stride < dim || nchains < 1 || nchains_padded < nchains || nchains_padded % kWave != 0)
        return SMCMC_ERR_INVALID;
    if (lag_first < 0 || lag_step < 1 || nlags < 1 || nlags > SMCMC_AUTOCORR_GRID_MAX_LAGS) return SMCMC_ERR_INVALID;
    if ((int64_t)lag_first + (int64_t)(nlags - 1) * lag_step > INT32_MAX) return SMCMC_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = nchains_padded / kWave;
    const int npasses = (nlags + kPassLags - 1) / kPassLags;
    const int nrows = npasses * kPassLags;
    const size_t nout = (size_t)dim * (nlags + 2);
    smcmc::DeviceBuffer<double> d_centre, d_partial, d_out;
    if (d_centre.allocate(dim) != hipSuccess || d_partial.allocate((size_t)nblocks * dim * (nrows + 2)) != hipSuccess ||
        d_out.allocate(nout) != hipSuccess)
        return SMCMC_ERR_HIP;
    const hipError_t c = centre ? hipMemcpyAsync(d_centre, centre, sizeof(double) * dim, hipMemcpyHostToDevice, s)
                                : hipMemsetAsync(d_centre, 0, sizeof(double) * dim, s);
    if (c != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(autocorr_grid_partial_kernel, dim3(nblocks, dim, npasses), dim3(kWave), 0, s, trace_device, nslots, dim,
                       (size_t)dim_stride, nchains, (size_t)nchains_padded, d_centre.get(), lag_first, lag_step, nrows,
                       d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(autocorr_grid_reduce_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, d_partial.get(),
                       nblocks, dim, nlags, nrows, d_out.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(lagged, d_out, sizeof(double) * dim * nlags, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sum, d_out + (size_t)dim * nlags, sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sumsq, d_out + (size_t)dim * (nlags + 1), sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
