// smcmc_marginals.hip -- the marginal and pair histograms of a saved trace (TestMarginalization.C: the ranges of
// :45-63, the 1-D histograms of :66-76, 97-98, the pair histograms of :78-92, 99-103), counted on the device so that
// the trace (slots x dim x chains doubles) never crosses PCIe.  include/smcmc.h has the definition: the bin rule
//   bin(x; n, lo, hi) = 0 if x < lo, n + 1 if !(x < hi), else 1 + (int)(n * (x - lo) / (hi - lo))
// in un-fused IEEE double with a correctly rounded division, counters of 64 bits.  The rule is ROOT's TAxis::FindBin for
// equal bins as this project states it (include/smcmc.h); it has not been checked against ROOT itself.
//
// Three kernels, all bound by the HBM reads of the trace (8 bytes, one bin rule and one LDS atomic per value):
//  * trace_ranges_partial_kernel: one wavefront per (64 chains, dimension) as autocorr_partial_kernel, a running
//    min / max per lane over the sampled slots, a butterfly over the wavefront, then one wavefront per dimension over
//    the chain blocks.  min / max are exact and order-free, NaN never replaces a value (std::min / std::max comparisons).
//  * marginal_fill1_kernel: a workgroup of 256 chains owns one dimension and one chunk of slots and counts into a
//    private u32 histogram in LDS, kept in `copies` copies selected by the low bits of the lane number so that lanes
//    that hit the same bin (a posterior is concentrated) do not serialise on one address; the copies are added up and
//    the non-zero counters go to the u64 result with vector global atomics.
//  * marginal_fill2_kernel: a workgroup of 1024 chains owns row i of the pair tables (the tables (i, j), j >= i, as
//    many as the LDS holds: ten 52 x 52 tables are 108 KB) and one chunk of slots; table (j, i) is written out as the
//    transpose of (i, j).
// A private u32 counter cannot wrap: a workgroup counts at most kFillThreads2 * kMaxChunk = 2^10 * 2^15.01 < 2^26
// points between clearing its LDS and flushing it (fill_chunk() below bounds the slots of a chunk).  Integer adds
// commute: the result is the same on every run whatever the arrival order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>

#include "smcmc.h"
#include "smcmc_host.hpp"
#include "smcmc_trace_reduce.hip.h"

namespace {

using smcmc::reduce::kWave;
constexpr int kRangeBlock = 8;        // sampled slots in flight per lane (ranges)
constexpr int kFillThreads1 = 256;    // chains per workgroup, 1-D fill
constexpr int kFillThreads2 = 1024;   // chains per workgroup, pair fill (one workgroup per CU: the tables fill its LDS)
constexpr int kFillChunk = 256;       // slots per workgroup
constexpr int kMaxChunk = 32769;      // what fill_chunk() can return at most (nslots < 2^31 over 65 535 chunks)
constexpr int kBlock1 = 8;            // slots per register block, 1-D fill (the next block loads while this one is binned)
constexpr int kBlock2 = 4;            // slots per register block, pair fill
constexpr int kDefaultCopies = 16;    // copies of the 1-D histogram per workgroup (profiles/marginals_notes.md)
constexpr size_t kLds1Bytes = 64 * 1024;    // 1-D: copies * stride words fit the default dynamic LDS limit
constexpr size_t kLds2Bytes = 144 * 1024;   // pair: of the CU's 160 KB
static_assert((long long)kFillThreads2 * kMaxChunk < (1ll << 32), "a private u32 counter cannot wrap");
static_assert((size_t)SMCMC_MARGINAL_MAX_BINS1 + 3 <= kLds1Bytes / 4 / kDefaultCopies, "the default copies fit the 1-D maximum");
static_assert(((size_t)SMCMC_MARGINAL_MAX_BINS2 + 2) * (SMCMC_MARGINAL_MAX_BINS2 + 2) * 4 * 2 <= kLds2Bytes,
              "two pair tables of the largest size fit the LDS");

typedef unsigned long long u64;

// the bin rule of include/smcmc.h; width = hi - lo, dn = (double)n.  With finite lo <= x < hi the quotient is in
// [0, n]; should n * (x - lo) or hi - lo overflow it is inf or NaN, which the comparison sends to the overflow
// counter instead of into an undefined conversion (q == n gives n + 1 either way).
__device__ __forceinline__ int bin_index(double x, int n, double dn, double lo, double hi, double width) {
    if (x < lo) return 0;
    if (!(x < hi)) return n + 1;
    const double q = dn * (x - lo) / width;
    return q < dn ? 1 + (int)q : n + 1;
}

__global__ void __launch_bounds__(kWave) trace_ranges_partial_kernel(const double* __restrict__ trace, int nslots, int dim,
                                                                     size_t dim_stride, int nchains, size_t npad,
                                                                     int sample_stride, double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const int cb = blockIdx.x;   // neighbouring workgroups read neighbouring 512-byte pieces of a trace row
    const int d = blockIdx.y;
    const size_t chain = (size_t)cb * kWave + lane;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    if (chain < (size_t)nchains) {
        const double* src = trace + (size_t)d * npad + chain;
        const size_t slot_stride = dim_stride * npad;
        const long long step = sample_stride;
        for (long long t0 = 0; t0 < nslots; t0 += step * kRangeBlock) {
            double v[kRangeBlock];
#pragma unroll
            for (int j = 0; j < kRangeBlock; ++j) {
                const long long t = t0 + step * j;
                v[j] = t < nslots ? src[(size_t)t * slot_stride] : NAN;   // past the end: a NaN replaces nothing
            }
#pragma unroll
            for (int j = 0; j < kRangeBlock; ++j) {
                lo = v[j] < lo ? v[j] : lo;   // std::min(lo, x)
                hi = hi < v[j] ? v[j] : hi;   // std::max(hi, x)
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double l = __shfl_xor(lo, off, kWave), h = __shfl_xor(hi, off, kWave);
        lo = l < lo ? l : lo;
        hi = hi < h ? h : hi;
    }
    if (lane == 0) {
        partial[((size_t)cb * dim + d) * 2] = lo;
        partial[((size_t)cb * dim + d) * 2 + 1] = hi;
    }
}

// out[0][d] = min, out[1][d] = max over the chain blocks: one wavefront per dimension, lanes striding over the blocks
// (a single thread per dimension took 0.42 ms over the 1 024 blocks of the headline trace), then the same butterfly
__global__ void __launch_bounds__(kWave) trace_ranges_reduce_kernel(const double* __restrict__ partial, int nblocks, int dim,
                                                                    double* __restrict__ out) {
    const int d = blockIdx.x, lane = threadIdx.x;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int cb = lane; cb < nblocks; cb += kWave) {
        const double l = partial[((size_t)cb * dim + d) * 2], h = partial[((size_t)cb * dim + d) * 2 + 1];
        lo = l < lo ? l : lo;
        hi = hi < h ? h : hi;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double l = __shfl_xor(lo, off, kWave), h = __shfl_xor(hi, off, kWave);
        lo = l < lo ? l : lo;
        hi = hi < h ? h : hi;
    }
    if (lane == 0) {
        out[d] = lo;
        out[dim + d] = hi;
    }
}

// grid (chain groups of 256, dim, slot chunks); dynamic LDS: copies * stride words, stride odd so that the copies of one
// bin lie in different banks
__global__ void __launch_bounds__(kFillThreads1) marginal_fill1_kernel(const double* __restrict__ trace, int nslots,
                                                                       size_t dim_stride, int nchains, size_t npad, int chunk,
                                                                       int n1, const double* __restrict__ lo1,
                                                                       const double* __restrict__ hi1, int copies, int stride,
                                                                       u64* __restrict__ counts1) {
    extern __shared__ uint32_t hist[];
    const int tid = threadIdx.x;
    const int d = blockIdx.y;
    const int t_begin = blockIdx.z * chunk;
    const int t_end = min(nslots, t_begin + chunk);
    const size_t chain = (size_t)blockIdx.x * kFillThreads1 + tid;
    for (int k = tid; k < copies * stride; k += kFillThreads1) hist[k] = 0u;
    __syncthreads();
    if (chain < (size_t)nchains) {
        const double lo = lo1[d], hi = hi1[d], width = hi - lo, dn = (double)n1;
        uint32_t* mine = hist + (tid & (copies - 1)) * stride;
        const size_t slot_stride = dim_stride * npad;
        const double* src = trace + (size_t)d * npad + chain;
        double cur[kBlock1], nxt[kBlock1];
#pragma unroll
        for (int j = 0; j < kBlock1; ++j) nxt[j] = t_begin + j < t_end ? src[(size_t)(t_begin + j) * slot_stride] : 0.0;
        for (int t0 = t_begin; t0 < t_end; t0 += kBlock1) {
#pragma unroll
            for (int j = 0; j < kBlock1; ++j) cur[j] = nxt[j];
#pragma unroll
            for (int j = 0; j < kBlock1; ++j) {
                const int t = t0 + kBlock1 + j;
                nxt[j] = t < t_end ? src[(size_t)t * slot_stride] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < kBlock1; ++j)
                if (t0 + j < t_end) atomicAdd(&mine[bin_index(cur[j], n1, dn, lo, hi, width)], 1u);
        }
    }
    __syncthreads();
    for (int b = tid; b < n1 + 2; b += kFillThreads1) {
        uint32_t c = 0;
        for (int k = 0; k < copies; ++k) c += hist[k * stride + b];   // at most 256 * chunk points: no wrap
        if (c) atomicAdd(&counts1[(size_t)d * (n1 + 2) + b], (u64)c);
    }
}

// grid (chain groups of 1024, P * ngroups, slot chunks): blockIdx.y = i * ngroups + g serves the tables (i, j) with
// j >= i inside the g-th group of `group` list positions; dynamic LDS: group * (n2 + 2)^2 words, table[bin of i][bin of j]
__global__ void __launch_bounds__(kFillThreads2) marginal_fill2_kernel(const double* __restrict__ trace, int nslots,
                                                                       size_t dim_stride, int nchains, size_t npad, int chunk,
                                                                       int P, const int* __restrict__ dims, int n2,
                                                                       const double* __restrict__ lo2,
                                                                       const double* __restrict__ hi2, int group, int ngroups,
                                                                       u64* __restrict__ counts2) {
    extern __shared__ uint32_t tab[];
    const int tid = threadIdx.x;
    const int i = blockIdx.y / ngroups, g = blockIdx.y % ngroups;
    const int j_begin = max(i, g * group), j_end = min(P, (g + 1) * group);
    if (j_begin >= j_end) return;   // the same for the whole workgroup
    const int nb = n2 + 2, tsz = nb * nb, ntab = j_end - j_begin;
    const int t_begin = blockIdx.z * chunk;
    const int t_end = min(nslots, t_begin + chunk);
    const size_t chain = (size_t)blockIdx.x * kFillThreads2 + tid;
    for (int k = tid; k < ntab * tsz; k += kFillThreads2) tab[k] = 0u;
    __syncthreads();
    if (chain < (size_t)nchains) {
        const double dn = (double)n2;
        const double lo_i = lo2[i], hi_i = hi2[i], width_i = hi_i - lo_i;
        const size_t slot_stride = dim_stride * npad;
        const double* src_i = trace + (size_t)dims[i] * npad + chain;
        for (int t0 = t_begin; t0 < t_end; t0 += kBlock2) {
            double v[kBlock2];
            int row[kBlock2];
#pragma unroll
            for (int u = 0; u < kBlock2; ++u) v[u] = t0 + u < t_end ? src_i[(size_t)(t0 + u) * slot_stride] : 0.0;
#pragma unroll
            for (int u = 0; u < kBlock2; ++u) row[u] = bin_index(v[u], n2, dn, lo_i, hi_i, width_i) * nb;
            for (int j = j_begin; j < j_end; ++j) {
                const double lo_j = lo2[j], hi_j = hi2[j], width_j = hi_j - lo_j;
                const double* src_j = trace + (size_t)dims[j] * npad + chain;
                uint32_t* table = tab + (j - j_begin) * tsz;
#pragma unroll
                for (int u = 0; u < kBlock2; ++u) v[u] = t0 + u < t_end ? src_j[(size_t)(t0 + u) * slot_stride] : 0.0;
#pragma unroll
                for (int u = 0; u < kBlock2; ++u)
                    if (t0 + u < t_end) atomicAdd(&table[row[u] + bin_index(v[u], n2, dn, lo_j, hi_j, width_j)], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < ntab * tsz; k += kFillThreads2) {
        const uint32_t c = tab[k];   // at most 1024 * chunk points: no wrap
        if (!c) continue;
        const int j = j_begin + k / tsz, r = k % tsz, a = r / nb, b = r % nb;
        atomicAdd(&counts2[(((size_t)i * P + j) * nb + a) * nb + b], (u64)c);
        if (j != i) atomicAdd(&counts2[(((size_t)j * P + i) * nb + b) * nb + a], (u64)c);
    }
}

constexpr int kMaxDim = 65535;        // the grid's y extent

bool bad_axis(double lo, double hi) { return !std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi); }

// slots per workgroup: kFillChunk, more only where the grid's z extent (65 535) would not cover the trace
int fill_chunk(int nslots) {
    const int need = (int)(((long long)nslots + 65534) / 65535);
    return need > kFillChunk ? need : kFillChunk;
}

// copies of the 1-D histogram per workgroup: a power of two up to 64 (one per lane of a wavefront), as many as asked
// for and as fit the LDS.  SMCMC_MARGINAL_COPIES in the environment overrides the default: the knob
// tools/marginals_time.py turns, not part of the interface.
int fill_copies(int stride) {
    int want = kDefaultCopies;
    if (const char* env = std::getenv("SMCMC_MARGINAL_COPIES")) {
        const int v = std::atoi(env);
        if (v >= 1 && v <= kWave && (v & (v - 1)) == 0) want = v;
    }
    while (want > 1 && (size_t)want * stride * sizeof(uint32_t) > kLds1Bytes) want /= 2;
    return want;
}

}  // namespace

extern "C" int smcmc_trace_ranges(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                  int nchains_padded, int sample_stride, double* lo, double* hi, void* stream) {
    if (smcmc::reduce::bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded, kMaxDim) ||
        sample_stride < 1 || !lo || !hi)
        return SMCMC_ERR_INVALID;
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (nchains + kWave - 1) / kWave;
    smcmc::DeviceBuffer<double> d_partial, d_out;
    if (d_partial.allocate((size_t)nblocks * dim * 2) != hipSuccess || d_out.allocate((size_t)dim * 2) != hipSuccess)
        return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(trace_ranges_partial_kernel, dim3(nblocks, dim), dim3(kWave), 0, s, trace_device, nslots, dim,
                       (size_t)dim_stride, nchains, (size_t)nchains_padded, sample_stride, d_partial.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(trace_ranges_reduce_kernel, dim3(dim), dim3(kWave), 0, s, d_partial.get(), nblocks, dim, d_out.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(lo, d_out, sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(hi, d_out + dim, sizeof(double) * dim, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    return SMCMC_OK;
}

extern "C" int smcmc_marginal_histograms(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                         int nchains_padded, int n1, const double* lo1, const double* hi1,
                                         uint64_t* counts1, int npair_dims, const int32_t* pair_dims, int n2,
                                         const double* lo2, const double* hi2, uint64_t* counts2, void* stream) {
    if (smcmc::reduce::bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded, kMaxDim))
        return SMCMC_ERR_INVALID;
    if (n1 < 0 || npair_dims < 0) return SMCMC_ERR_INVALID;
    const bool do1 = n1 > 0 && counts1, do2 = npair_dims > 0;
    if (!do1 && !do2) return SMCMC_ERR_INVALID;   // nothing asked for
    if (do1) {
        if (n1 > SMCMC_MARGINAL_MAX_BINS1 || !lo1 || !hi1) return SMCMC_ERR_INVALID;
        for (int d = 0; d < dim; ++d)
            if (bad_axis(lo1[d], hi1[d])) return SMCMC_ERR_INVALID;
    }
    const int P = npair_dims;
    if (do2) {
        if (P > SMCMC_MARGINAL_MAX_PAIR_DIMS || n2 < 1 || n2 > SMCMC_MARGINAL_MAX_BINS2 || !pair_dims || !lo2 || !hi2 || !counts2)
            return SMCMC_ERR_INVALID;
        for (int p = 0; p < P; ++p)
            if (pair_dims[p] < 0 || pair_dims[p] >= dim || bad_axis(lo2[p], hi2[p])) return SMCMC_ERR_INVALID;
    }
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int chunk = fill_chunk(nslots);
    const unsigned nchunks = (unsigned)((nslots + chunk - 1) / chunk);
    smcmc::DeviceBuffer<double> d_axes1, d_axes2;
    smcmc::DeviceBuffer<int> d_dims;
    smcmc::DeviceBuffer<u64> d_counts1, d_counts2;
    const size_t nc1 = (size_t)dim * (n1 + 2);
    const size_t nc2 = do2 ? (size_t)P * P * (n2 + 2) * (n2 + 2) : 0;
    if (do1) {
        if (d_axes1.allocate((size_t)dim * 2) != hipSuccess || d_counts1.allocate(nc1) != hipSuccess) return SMCMC_ERR_HIP;
        if (hipMemcpyAsync(d_axes1, lo1, sizeof(double) * dim, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(d_axes1 + dim, hi1, sizeof(double) * dim, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemsetAsync(d_counts1, 0, sizeof(u64) * nc1, s) != hipSuccess)
            return SMCMC_ERR_HIP;
        const int stride = (n1 + 2) | 1;
        const int copies = fill_copies(stride);
        hipLaunchKernelGGL(marginal_fill1_kernel, dim3((nchains + kFillThreads1 - 1) / kFillThreads1, dim, nchunks),
                           dim3(kFillThreads1), (size_t)copies * stride * sizeof(uint32_t), s, trace_device, nslots,
                           (size_t)dim_stride, nchains, (size_t)nchains_padded, chunk, n1, d_axes1.get(), d_axes1.get() + dim,
                           copies, stride, d_counts1.get());
        if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    }
    if (do2) {
        if (d_axes2.allocate((size_t)P * 2) != hipSuccess || d_dims.allocate(P) != hipSuccess ||
            d_counts2.allocate(nc2) != hipSuccess)
            return SMCMC_ERR_HIP;
        if (hipMemcpyAsync(d_axes2, lo2, sizeof(double) * P, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(d_axes2 + P, hi2, sizeof(double) * P, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(d_dims, pair_dims, sizeof(int) * P, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemsetAsync(d_counts2, 0, sizeof(u64) * nc2, s) != hipSuccess)
            return SMCMC_ERR_HIP;
        const size_t table_bytes = (size_t)(n2 + 2) * (n2 + 2) * sizeof(uint32_t);
        const int fit = (int)(kLds2Bytes / table_bytes);
        const int group = fit < P ? fit : P;
        const int ngroups = (P + group - 1) / group;
        const size_t lds = group * table_bytes;
        // more dynamic LDS than the default limit
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(marginal_fill2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kLds2Bytes) != hipSuccess)
            return SMCMC_ERR_HIP;
        hipLaunchKernelGGL(marginal_fill2_kernel, dim3((nchains + kFillThreads2 - 1) / kFillThreads2, P * ngroups, nchunks),
                           dim3(kFillThreads2), lds, s, trace_device, nslots, (size_t)dim_stride, nchains,
                           (size_t)nchains_padded, chunk, P, d_dims.get(), n2, d_axes2.get(), d_axes2.get() + P, group,
                           ngroups, d_counts2.get());
        if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    }
    if (do1 && hipMemcpyAsync(counts1, d_counts1, sizeof(u64) * nc1, hipMemcpyDeviceToHost, s) != hipSuccess) return SMCMC_ERR_HIP;
    if (do2 && hipMemcpyAsync(counts2, d_counts2, sizeof(u64) * nc2, hipMemcpyDeviceToHost, s) != hipSuccess) return SMCMC_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return SMCMC_ERR_HIP;
    return SMCMC_OK;
}
