// smcmc_convergence.hip -- the sums behind split R-hat and the multi-chain effective sample size of a saved trace
// (include/smcmc.h has the definition; the reference is single chain and has no counterpart), taken on the device so
// that the trace (slots x dim x chains doubles, 13.4 GB at the headline size) never crosses PCIe.  Every live chain is cut
// into S segments of L slots; a segment of a chain is one "segment-chain" m with its own sum s1_m and its own mean.
//
// Pass 1, chain_sums_kernel: one lane is one chain of one (dimension, segment), a wavefront 64 consecutive chains, so a
// load is one coalesced 512-byte piece of a trace row.  The slots are taken sixteen at a time; the sixteen loads of the
// next block are issued before the current block is added, so sixteen loads of later slots are on their way while
// earlier ones are summed (these passes are bound by the bytes a wavefront keeps in flight, not by arithmetic).  s1 is
// stored as [S][dim][nchains_padded] (0 in the lanes >= nchains, by a select: the padding is not read), then s1 and s1^2
// go through a butterfly over the wavefront into the block's partial sums.
//
// Pass 2, within_partial_kernel<K0>: the lagged register block of smcmc_trace_reduce.hip.h, as autocorr_partial_kernel<K0>
// (smcmc_autocorr.hip) uses it; one launch for the lags 0..31 and one for 32..63.  The value is z_t = (x - centre) - s1 / L,
// the lane's own mean taken off with the two subtractions of the definition, and a wavefront owns one segment: its
// window starts empty at the segment's first slot, so no lag reaches across it.
//
// ordered_rows_reduce_kernel (smcmc_trace_reduce.hip.h) adds the block partials in order.
// Summation order, fixed for a shape: slots ascending per lane; a butterfly over the 64 chains of a wavefront (offsets
// 32, 16, .., 1); then one running sum over the blocks of 64 chains ascending within a segment, the segments ascending.
// The same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smcmc.h"
#include "smcmc_host.hpp"
#include "smcmc_trace_reduce.hip.h"

namespace {

constexpr int kLags = SMCMC_AUTOCORR_LAGS;   // lags 0 .. 63
using namespace smcmc::reduce;               // kWave, kPassLags, kBlock, LaggedBlock: its window is z[t0 - K0 - 31 .. t0 - K0 + 15]
constexpr int kRows = kLags + 2;             // a partial: within[0 .. 63], sum, sumsq_of_sums
constexpr int kMaxSegments = 65535;          // the grid's z extent
static_assert(kLags == 2 * kPassLags, "two passes cover the lags");

// Where a wavefront's segment starts and what its lanes are.  grid (blocks of 64 chains, dim, segments); the partials
// are [segment][live block][dim][kRows].  A lane >= nchains of a live block loads what the block's last live chain
// loads and drops it with a select: every load is unconditional (the compiler batches them) and the padding is not read.
struct Piece {
    const double* src;   // the value the lane loads at the segment's first slot
    size_t sums_at;      // the lane's place in chain_sums
    size_t partial_at;   // the wavefront's place in the partials
    bool active;
};

__device__ __forceinline__ Piece piece_of(const double* trace, int first_slot, int L, int dim, size_t dim_stride, int nchains,
                                          size_t npad, int nlive) {
    const int cb = blockIdx.x, d = blockIdx.y, s = blockIdx.z;
    const size_t chain = (size_t)cb * kWave + threadIdx.x;
    Piece p;
    p.active = chain < (size_t)nchains;
    p.src = trace + ((size_t)first_slot + (size_t)s * L) * dim_stride * npad + (size_t)d * npad +
            (p.active ? chain : (size_t)nchains - 1);
    p.sums_at = ((size_t)s * dim + d) * npad + chain;
    p.partial_at = (((size_t)s * nlive + cb) * dim + d) * kRows;
    return p;
}

// grid.x covers every block of the padded width: the lanes of a dead block store their 0 and read nothing
__global__ void __launch_bounds__(kWave) chain_sums_kernel(const double* __restrict__ trace, int first_slot, int L, int dim,
                                                           size_t dim_stride, int nchains, size_t npad, int nlive,
                                                           const double* __restrict__ centre,
                                                           double* __restrict__ chain_sums, double* __restrict__ partial) {
    const Piece p = piece_of(trace, first_slot, L, dim, dim_stride, nchains, npad, nlive);
    if ((int)blockIdx.x >= nlive) {                                // wave-uniform
        chain_sums[p.sums_at] = 0.0;
        return;
    }
    const size_t slot_stride = dim_stride * npad;
    const double c0 = centre[blockIdx.y];
    auto fetch = [&](double (&buf)[kBlock], int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kBlock; ++j) buf[j] = p.src[(size_t)(t0 + j) * slot_stride];
    };
    double s1 = 0.0;
    auto add = [&](const double (&buf)[kBlock]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kBlock; ++j) s1 += buf[j] - c0;
    };
    const int whole = L / kBlock * kBlock;
    double a[kBlock], b[kBlock];                                   // two blocks in turn: no copy waits on a load
    if (whole) {
        fetch(a, 0);
        int t0 = kBlock;
        for (; t0 + kBlock < whole; t0 += 2 * kBlock) {
            fetch(b, t0);                                          // sixteen loads in flight while the block before is added
            __builtin_amdgcn_sched_barrier(0);                     // the scheduler would gather both fetches and drain them
            add(a);
            __builtin_amdgcn_sched_barrier(0);
            fetch(a, t0 + kBlock);
            __builtin_amdgcn_sched_barrier(0);
            add(b);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (t0 < whole) {
            fetch(b, t0);
            add(a);
            add(b);
        } else {
            add(a);
        }
    }
    for (int t = whole; t < L; ++t) s1 += p.src[(size_t)t * slot_stride] - c0;
    s1 = p.active ? s1 : 0.0;                                      // a select: +0 from a lane >= nchains
    chain_sums[p.sums_at] = s1;
    double sq = s1 * s1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s1 += __shfl_xor(s1, off, kWave);
        sq += __shfl_xor(sq, off, kWave);
    }
    if (threadIdx.x == 0) {
        partial[p.partial_at + kLags] = s1;
        partial[p.partial_at + kLags + 1] = sq;
    }
}

// grid.x covers the live blocks only
template <int K0>
__global__ void __launch_bounds__(kWave) within_partial_kernel(const double* __restrict__ trace, int first_slot, int L, int dim,
                                                               size_t dim_stride, int nchains, size_t npad, int nlive,
                                                               const double* __restrict__ centre,
                                                               const double* __restrict__ chain_sums,
                                                               double* __restrict__ partial) {
    const Piece p = piece_of(trace, first_slot, L, dim, dim_stride, nchains, npad, nlive);
    const size_t slot_stride = dim_stride * npad;
    const double c0 = centre[blockIdx.y];
    const double mean = chain_sums[p.sums_at] / (double)L;         // 0 in a lane >= nchains
    // z of a slot of the segment (0 <= t < L)
    auto z = [&](int t) __attribute__((always_inline)) {
        const double r = (p.src[(size_t)t * slot_stride] - c0) - mean;
        return p.active ? r : 0.0;
    };
    LaggedBlock b;
    b.clear_window();                                              // the segment's first slot: nothing behind it
    b.clear_sums();
    // the partners of the block at t0, acc[kk] += z[t0 + j] * z[t0 + j - K0 - kk]: the lagged block of the second launch
    // lies K0 = 2 kBlock slots back, wholly before the segment or wholly inside it
    auto partners = [&](int t0) __attribute__((always_inline)) {
        if (K0 == 0) {
#pragma unroll
            for (int j = 0; j < kBlock; ++j) b.partner(j) = b.v[j];
        } else if (t0 >= K0) {
#pragma unroll
            for (int j = 0; j < kBlock; ++j) b.partner(j) = z(t0 - K0 + j);
        } else {
#pragma unroll
            for (int j = 0; j < kBlock; ++j) b.partner(j) = 0.0;
        }
    };
    const int whole = L / kBlock * kBlock;
    for (int t0 = 0; t0 < whole; t0 += kBlock) {                   // whole blocks: every load unconditional
#pragma unroll
        for (int j = 0; j < kBlock; ++j) b.v[j] = z(t0 + j);
        partners(t0);
        b.fold();
    }
    if (whole < L) {                                               // the last, partial block
#pragma unroll
        for (int j = 0; j < kBlock; ++j) b.v[j] = whole + j < L ? z(whole + j) : 0.0;
        partners(whole);
        b.fold();
    }
    // butterfly over the wavefront's chains
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) b.butterfly(off);
    if (threadIdx.x == 0) b.store(partial + p.partial_at + K0);
}

}  // namespace

extern "C" int smcmc_trace_convergence(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                       int nchains_padded, int nsegments, const double* centre, double* chain_sums_device,
                                       double* sum, double* sumsq_of_sums, double* within, void* stream) {
    if (!sum || !sumsq_of_sums || !within) return SMCMC_ERR_INVALID;
    if (nsegments < 1 || nslots / nsegments < 2 ||
        bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded, smcmc_max_dim()))
        return SMCMC_ERR_INVALID;
    if (nsegments > kMaxSegments) return SMCMC_ERR_UNSUPPORTED;
    if (no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int S = nsegments, L = nslots / S, first_slot = nslots - S * L;
    const int nblocks = nchains_padded / kWave, nlive = (nchains + kWave - 1) / kWave;
    const size_t nout = (size_t)dim * kRows;
    smcmc::DeviceBuffer<double> d_centre, d_partial, d_out, d_sums;
    if (centre_on_device(d_centre, centre, dim, s) != hipSuccess || d_partial.allocate(nout * nlive * S) != hipSuccess ||
        d_out.allocate(nout) != hipSuccess)
        return SMCMC_ERR_HIP;
    if (!chain_sums_device && d_sums.allocate((size_t)S * dim * nchains_padded) != hipSuccess) return SMCMC_ERR_HIP;
    double* sums = chain_sums_device ? chain_sums_device : d_sums.get();
    hipLaunchKernelGGL(chain_sums_kernel, dim3(nblocks, dim, S), dim3(kWave), 0, s, trace_device, first_slot, L, dim,
                       (size_t)dim_stride, nchains, (size_t)nchains_padded, nlive, d_centre.get(), sums, d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(within_partial_kernel<0>, dim3(nlive, dim, S), dim3(kWave), 0, s, trace_device, first_slot, L, dim,
                       (size_t)dim_stride, nchains, (size_t)nchains_padded, nlive, d_centre.get(), sums, d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(within_partial_kernel<kPassLags>, dim3(nlive, dim, S), dim3(kWave), 0, s, trace_device, first_slot, L,
                       dim, (size_t)dim_stride, nchains, (size_t)nchains_padded, nlive, d_centre.get(), sums, d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    // out[row][d] = one running sum over the segments ascending and, within a segment, the live blocks ascending
    launch_ordered_rows_reduce(s, d_partial.get(), (long long)nlive * S, dim, kRows, kRows, kLags, d_out.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(within, d_out, sizeof(double) * dim * kLags, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sum, d_out + (size_t)dim * kLags, sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(sumsq_of_sums, d_out + (size_t)dim * (kLags + 1), sizeof(double) * dim, hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
