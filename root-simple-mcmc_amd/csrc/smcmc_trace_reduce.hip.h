// smcmc_trace_reduce.hip.h -- what the reducers over a saved trace share (smcmc_autocorr.hip, smcmc_autocorr_grid.hip,
// smcmc_convergence.hip, smcmc_marginals.hip, smcmc_trace_moments.hip): the lagged register block, the ordered
// reduction of its partial sums, and the host prologue of the entry points.
//
// The lagged block.  One lane owns one chain of one dimension; a wavefront covers 64 chains and 32 lags.  Everything
// sits in registers with static indices: the 16 values v of the current block of slots, a sliding window of the 47
// values the 32 lags reach back to (the macro's ring buffer, MakeAutocorrelation.C:106-124) and 32 accumulators: 512
// fused multiply-adds per 16 loaded values and no LDS.  A kernel loads v[j] and the partner slot partner(j) -- the
// value K0 slots behind v[j], K0 the first lag of the wavefront -- for its 16 slots, then fold() does
//   acc[k] = fma(v[j], win[31 + j - k], acc[k])      j ascending outside, k ascending inside
// and slides the window by 16.  After the last block the xor 32, 16, .., 1 butterfly adds the 64 chains of the wavefront
// and lane 0 stores the 32 sums.  This order is part of the published definition of every sum taken with the block
// (the same bits on every run, and the same bits from every kernel that uses it); the kernels differ in what they
// load and in which order they walk the slots, which their own files state.
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>

#include "smcmc.h"
#include "smcmc_host.hpp"

namespace smcmc {
namespace reduce {

constexpr int kWave = 64;
constexpr int kPassLags = 32;                // lags per wavefront
constexpr int kBlock = 16;                   // slots per register block
constexpr int kWin = kBlock + kPassLags - 1; // the partners of v[0 .. 15] at the lags K0 .. K0 + 31

struct LaggedBlock {
    double win[kWin], acc[kPassLags], v[kBlock];

    // nothing behind the next slot: the start of a trace, of a segment, of a residue class
    __device__ __forceinline__ void clear_window() {
#pragma unroll
        for (int i = 0; i < kWin; ++i) win[i] = 0.0;
    }
    __device__ __forceinline__ void clear_sums() {
#pragma unroll
        for (int k = 0; k < kPassLags; ++k) acc[k] = 0.0;
    }
    // the value K0 slots behind v[j]
    __device__ __forceinline__ double& partner(int j) { return win[kPassLags - 1 + j]; }
    // acc[k] += v[j] * (the value K0 + k slots behind v[j]), then the window moves on by a block
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int j = 0; j < kBlock; ++j)
#pragma unroll
            for (int k = 0; k < kPassLags; ++k) acc[k] = __builtin_fma(v[j], win[kPassLags - 1 + j - k], acc[k]);
#pragma unroll
        for (int i = 0; i < kPassLags - 1; ++i) win[i] = win[i + kBlock];
    }
    // one step of the butterfly over the wavefront's chains: off = 32, 16, .., 1
    __device__ __forceinline__ void butterfly(int off) {
#pragma unroll
        for (int k = 0; k < kPassLags; ++k) acc[k] += __shfl_xor(acc[k], off, kWave);
    }
    __device__ __forceinline__ void store(double* __restrict__ out) const {
#pragma unroll
        for (int k = 0; k < kPassLags; ++k) out[k] = acc[k];
    }
};

// out[k][d], k < nout, = the sum over the pieces p ascending, from +0, of partial[p][d][col(k)]: a piece holds `pitch`
// columns per dimension, of which the last pitch - tail_at (sum, sumsq, ...) follow the rows asked for in `out`
// whatever the rows a piece was padded to: col(k) = k below the tail, tail_at + (k - first tail row) in it.
// A template so that only the units that launch it carry a copy.
template <typename T>
__global__ void ordered_rows_reduce_kernel(const T* __restrict__ partial, long long npieces, int dim, int nout, int pitch,
                                           int tail_at, T* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= dim * nout) return;
    const int d = idx / nout, k = idx % nout;
    const int nlead = nout - (pitch - tail_at);
    const int col = k < nlead ? k : tail_at + (k - nlead);
    const T* src = partial + (size_t)d * pitch + col;
    const size_t piece = (size_t)dim * pitch;
    T s = 0.0;
#pragma unroll 8
    for (long long p = 0; p < npieces; ++p) s += src[(size_t)p * piece];
    out[(size_t)k * dim + d] = s;
}

template <typename T>
void launch_ordered_rows_reduce(hipStream_t s, const T* partial, long long npieces, int dim, int nout, int pitch, int tail_at,
                                T* out) {
    hipLaunchKernelGGL(ordered_rows_reduce_kernel<T>, dim3((unsigned)(((size_t)dim * nout + 255) / 256)), dim3(256), 0, s,
                       partial, npieces, dim, nout, pitch, tail_at, out);
}

// ---- the host prologue of the entry points ---------------------------------------------------------------------------

// What every entry point refuses (SMCMC_ERR_INVALID) of a trace [nslots][dim_stride][nchains_padded]; max_dim is the
// entry point's own bound on dim (the grid's y extent, smcmc_max_dim(), or none).
inline bool bad_trace_shape(const void* trace, int nslots, int dim, int dim_stride, int nchains, int nchains_padded,
                            int max_dim = INT_MAX) {
    return !trace || nslots < 1 || dim < 1 || dim > max_dim || dim_stride < dim || nchains < 1 || nchains_padded < nchains ||
           nchains_padded % kWave != 0;
}

// SMCMC_ERR_NO_DEVICE
inline bool no_device() {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1;
}

// the reference point of the sums on the device: the caller's centre[dim], or the origin when it is NULL
inline hipError_t centre_on_device(DeviceBuffer<double>& d_centre, const double* centre, int dim, hipStream_t s) {
    const hipError_t e = d_centre.allocate(dim);
    if (e != hipSuccess) return e;
    return centre ? hipMemcpyAsync(d_centre, centre, sizeof(double) * dim, hipMemcpyHostToDevice, s)
                  : hipMemsetAsync(d_centre, 0, sizeof(double) * dim, s);
}

}  // namespace reduce
}  // namespace smcmc
