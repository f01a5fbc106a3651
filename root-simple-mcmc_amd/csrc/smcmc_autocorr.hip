// smcmc_autocorr.hip -- the lagged-product sums behind the autocorrelation of a saved trace
// (MakeAutocorrelation.C:108-148: a(lag) = (E[x_t x_{t-lag}] - mean^2) / var per dimension), taken
// on the device so that the trace (slots x dim x chains doubles, gigabytes at 65 536 chains) never
// crosses PCIe.  One lane owns one chain of one dimension; a wavefront covers 64 chains and 32 of the
// 64 lags (two passes over the trace, the second mostly out of L2).  The sums are taken in the lagged
// register block of smcmc_trace_reduce.hip.h: 512 fused multiply-adds per 16 loaded values and no
// LDS.  Measured on the headline trace (512 slots x 50 x 65 536, 13.4 GB):
// 5.1 ms for lags 0..31 (2.6 TB/s), 11.1 ms for lags 32..63 (it loads the lagged block as well);
// an LDS ring with 64 accumulators per lane took 36.5 ms (five instructions per lag step, one
// wavefront per SIMD).  Bounds: 1.7 ms of HBM time per pass, 2.7 ms of FP64 vector time in all
// (64 multiply-adds per 8-byte value at 78.6 TFLOP/s); what is left is load latency at two to three
// wavefronts per SIMD (the next block is not prefetched yet).
// The sums may be taken about a reference point so that E[x x] - mean^2 cancels less; that changes a(lag)
// only through the edges of the lagged sums (O(lag / slots)); the macro itself uses the origin.
// Summation order is fixed: slots ascending per chain, a butterfly over the 64 chains of a wavefront,
// wavefronts ascending -- the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smcmc.h"
#include "smcmc_host.hpp"
#include "smcmc_trace_reduce.hip.h"

namespace {

constexpr int kLags = SMCMC_AUTOCORR_LAGS;   // lags 0 .. 63
using namespace smcmc::reduce;               // kWave, kPassLags, kBlock, LaggedBlock: its window is y[t0 - K0 - 31 .. t0 - K0 + 15]
static_assert(kLags == 2 * kPassLags, "two passes cover the lags");

template <int K0>
__global__ void __launch_bounds__(kWave) autocorr_partial_kernel(const double* __restrict__ trace, int nslots, int dim,
                                                                 size_t dim_stride, int nchains, size_t npad,
                                                                 const double* __restrict__ centre,
                                                                 double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const int cb = blockIdx.x;   // neighbouring workgroups read neighbouring 512-byte pieces of a trace row
    const int d = blockIdx.y;
    const size_t chain = (size_t)cb * kWave + lane;
    const bool active = chain < (size_t)nchains;
    const double c0 = centre[d];
    const double* src = trace + (size_t)d * npad + chain;
    const size_t slot_stride = dim_stride * npad;
    auto y = [&](int t) __attribute__((always_inline)) {
        return (active && t >= 0 && t < nslots) ? src[(size_t)t * slot_stride] - c0 : 0.0;
    };
    LaggedBlock b;
    b.clear_window();
    b.clear_sums();
    double sum = 0.0;
    for (int t0 = 0; t0 < nslots; t0 += kBlock) {
#pragma unroll
        for (int j = 0; j < kBlock; ++j) {
            b.v[j] = y(t0 + j);
            b.partner(j) = (K0 == 0) ? b.v[j] : y(t0 - K0 + j);
        }
        if (K0 == 0) {
#pragma unroll
            for (int j = 0; j < kBlock; ++j) sum += b.v[j];
        }
        b.fold();   // acc[kk] += y[t0 + j] * y[t0 + j - K0 - kk]
    }
    // butterfly over the wavefront's chains
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off, kWave);
        b.butterfly(off);
    }
    if (lane == 0) {
        double* out = partial + ((size_t)cb * dim + d) * (kLags + 1);
        b.store(out + K0);
        if (K0 == 0) out[kLags] = sum;
    }
}

}  // namespace

extern "C" int smcmc_autocorrelation_sums(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                          int nchains_padded, const double* centre, double* sum, double* lagged,
                                          void* stream) {
    if (bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded) || !sum || !lagged)
        return SMCMC_ERR_INVALID;
    if (no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = nchains_padded / kWave;
    const size_t nout = (size_t)dim * (kLags + 1);
    smcmc::DeviceBuffer<double> d_centre, d_partial, d_out;
    if (centre_on_device(d_centre, centre, dim, s) != hipSuccess || d_partial.allocate(nout * nblocks) != hipSuccess ||
        d_out.allocate(nout) != hipSuccess)
        return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(autocorr_partial_kernel<0>, dim3(nblocks, dim), dim3(kWave), 0, s, trace_device, nslots, dim,
                       (size_t)dim_stride, nchains, (size_t)nchains_padded, d_centre.get(), d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(autocorr_partial_kernel<kPassLags>, dim3(nblocks, dim), dim3(kWave), 0, s, trace_device, nslots,
                       dim, (size_t)dim_stride, nchains, (size_t)nchains_padded, d_centre.get(), d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    // out[k][d] = the sum over the chain blocks, ascending
    launch_ordered_rows_reduce(s, d_partial.get(), nblocks, dim, kLags + 1, kLags + 1, kLags, d_out.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(lagged, d_out, sizeof(double) * dim * kLags, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sum, d_out + (size_t)dim * kLags, sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
