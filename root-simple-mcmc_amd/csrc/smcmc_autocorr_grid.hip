// smcmc_autocorr_grid.hip -- the lagged-product sums of a saved trace on a lag grid k_i = lag_first + i * lag_step:
// what MakeAutocorrelation.C:98-124 evaluates (lags 1, 1 + lagStep, ... < maxLag, about 200 of them spread over up to
// 30 000 slots), where smcmc_autocorr.hip covers the 64 consecutive lags 0 .. 63 only.  The inner block is the lagged
// register block of smcmc_trace_reduce.hip.h, the one that kernel uses: one lane owns one chain of one dimension, a
// wavefront covers 64 chains and 32 lags (one pass; the passes of a call are grid z).
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
#include "smcmc_trace_reduce.hip.h"

namespace {

// kWave, kPassLags, kBlock (decimated slots here), LaggedBlock: its window is w[a0 - 31 .. a0 + 15]
using namespace smcmc::reduce;

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
    LaggedBlock b;
    b.clear_sums();
    double sum = 0.0, sumsq = 0.0;
    if (sums || k0 < nslots) {
        const int64_t nres = S < nslots ? S : nslots;
        for (int64_t r = 0; r < nres; ++r) {
            b.clear_window();
            // the first a with r - k0 + a S >= 0: before it every partner of every lag of the pass is 0
            int64_t a = 0;
            if (!sums && k0 > r) a = (int64_t)((uint32_t)(k0 - r - 1) / (uint32_t)lag_step) + 1;
            for (int64_t t0 = r + a * S; t0 < nslots; t0 += kBlock * S) {
#pragma unroll
                for (int j = 0; j < kBlock; ++j) {
                    const int64_t t = t0 + j * S;
                    b.v[j] = y(t);
                    b.partner(j) = same ? b.v[j] : y(t - k0);
                }
                if (sums) {
#pragma unroll
                    for (int j = 0; j < kBlock; ++j) {
                        sum += b.v[j];
                        sumsq = __builtin_fma(b.v[j], b.v[j], sumsq);
                    }
                }
                b.fold();   // acc[i] += u[a0 + j] * w[a0 + j - i]
            }
        }
    }
    // butterfly over the wavefront's chains
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off, kWave);
        sumsq += __shfl_xor(sumsq, off, kWave);
        b.butterfly(off);
    }
    if (lane == 0) {
        double* out = partial + ((size_t)cb * dim + d) * ((size_t)nrows + 2);
        b.store(out + pass * kPassLags);
        if (sums) {
            out[nrows] = sum;
            out[nrows + 1] = sumsq;
        }
    }
}

}  // namespace

extern "C" int smcmc_autocorrelation_grid_sums(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                               int nchains_padded, const double* centre, int lag_first, int lag_step,
                                               int nlags, double* sum, double* sumsq, double* lagged, void* stream) {
    if (bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded) || !sum || !sumsq || !lagged)
        return SMCMC_ERR_INVALID;
    if (lag_first < 0 || lag_step < 1 || nlags < 1 || nlags > SMCMC_AUTOCORR_GRID_MAX_LAGS) return SMCMC_ERR_INVALID;
    if ((int64_t)lag_first + (int64_t)(nlags - 1) * lag_step > INT32_MAX) return SMCMC_ERR_INVALID;
    if (no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = nchains_padded / kWave;
    const int npasses = (nlags + kPassLags - 1) / kPassLags;
    const int nrows = npasses * kPassLags;
    const size_t nout = (size_t)dim * (nlags + 2);
    smcmc::DeviceBuffer<double> d_centre, d_partial, d_out;
    if (centre_on_device(d_centre, centre, dim, s) != hipSuccess ||
        d_partial.allocate((size_t)nblocks * dim * (nrows + 2)) != hipSuccess || d_out.allocate(nout) != hipSuccess)
        return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(autocorr_grid_partial_kernel, dim3(nblocks, dim, npasses), dim3(kWave), 0, s, trace_device, nslots, dim,
                       (size_t)dim_stride, nchains, (size_t)nchains_padded, d_centre.get(), lag_first, lag_step, nrows,
                       d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    // out[i][d], i < nlags the rows, then sum, then sumsq: the chain blocks added ascending
    launch_ordered_rows_reduce(s, d_partial.get(), nblocks, dim, nlags + 2, nrows + 2, nrows, d_out.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(lagged, d_out, sizeof(double) * dim * nlags, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sum, d_out + (size_t)dim * nlags, sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sumsq, d_out + (size_t)dim * (nlags + 1), sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
