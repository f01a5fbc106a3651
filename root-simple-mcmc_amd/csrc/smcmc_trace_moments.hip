// smcmc_trace_moments.hip -- the mean and covariance sums of a saved trace (MakeCovariance.C:63-89) and the Gaussian
// stand-in chain of a mean and a covariance (CholeskyChain.C:18-66), both on the device so that the trace
// (slots x dim x chains doubles, 13.4 GB at the headline size) never crosses PCIe.
//
// smcmc_trace_moments.  With y = (x - centre, 1), a vector of dim + 1 rows per (slot, chain), the result is the lower
// triangle of E = sum y y^T: rows < dim hold sumsq, row dim holds sum (and E[dim][dim] the number of points).  E is cut
// into 16 x 16 tiles, four tile rows (64 rows of y) to a tile block.  A wavefront owns a run of consecutive units --
// a unit is one slot of one block of 64 chains, unit = slot * blocks + block -- and, for one pair of tile blocks
// (bi, bj <= bi), keeps every tile of the pair in registers over its whole run: per unit it loads the rows of y (lane =
// chain, 512-byte pieces of a trace row, on the diagonal the next unit's in flight while this one is folded), subtracts the centre,
// writes them to its own piece of LDS as [row][chain] with a pitch of 66 doubles (rows two bank pairs apart: operand
// reads and staging writes are free of bank conflicts, as in fold_ring_kernel), and folds them with chains of
// v_mfma_f64_16x16x4_f64, k running over the 64 chains in 16 quads.  The A operand of tile (a, b) is rows 16 a .. of
// y, the B operand rows 16 b ..: both are the same read, so a quad costs one LDS read per tile row for up to ten matrix
// instructions.  dim <= 63 is one tile block and one launch (at most ten tiles, four wavefronts per workgroup, one
// workgroup per CU: its LDS holds four staging pieces); above that the diagonal pairs are one launch and the
// off-diagonal pairs (sixteen tiles, two wavefronts per workgroup) another, over a smaller grid.
// Rows >= dim of the trace are never loaded (a tile row beyond y is 0), and a lane whose chain is >= nchains is
// replaced by 0 with a select before it reaches LDS: NaN in the padding cannot reach a matrix operand.
// Bounds on the headline trace (512 slots x 50 x 65 536): 1.7 ms of HBM time, 2.2 ms of matrix time (ten instructions
// of 2 048 flops per 4 points at 78.6 TFLOP/s).  Measured: 4.98 ms for the kernel (2.7 TB/s), the time of
// autocorr_partial_kernel<0> on the same bytes (4.93 ms): one wavefront per SIMD with one unit in flight does not keep
// more bytes on their way; the fill of the same shape takes 26.3 ms (profiles/trace_moments_notes.md says why).
// Summation order, fixed for a shape: within a wavefront its units ascending, within a unit the chains ascending, one
// fused multiply-add each (test_mfma_f64_is_an_ascending_k_fma_chain); the wavefronts of a workgroup ascending; the
// workgroups ascending (trace_moments_reduce_kernel).  Wavefront g of G takes units [U g / G, U (g + 1) / G); G depends
// on the shape alone.  The same bits on every run.
//
// smcmc_cholesky_chain.  One lane per chain, U wave-uniform through the constant address space (scalar loads), the
// normals of an entry drawn as a chain-step's (Philox block b gives normals 4b .. 4b + 3); the accumulators of up to 64
// columns j sit in registers while i ascends, a * U(i, j) and the add un-fused as the macro's loop has them.  It is the
// frozen step kernel's proposal without the Metropolis half.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "smcmc.h"
#include "smcmc_detmath.h"
#include "smcmc_host.hpp"
#include "smcmc_proposal.hpp"
#include "smcmc_trace_reduce.hip.h"

namespace {

using smcmc::f64x4;

using smcmc::reduce::kWave;
constexpr int kPitch = kWave + 2;     // doubles per LDS row: the 64 chains of a unit + 2 (row stride = 2 mod 32 bank pairs)
constexpr int kBlockRows = 64;        // rows of y per tile block: four operand tiles
constexpr int kQuads = kWave / 4;     // matrix instructions per tile and unit
constexpr int kMaxWgOne = 256;        // workgroups of the single-block launch: one per CU
constexpr int kMaxWgMany = 32;        // workgroups per tile-block pair above 63 dimensions (the partial sums stay small)

constexpr int moment_waves(bool diag) { return diag ? 4 : 2; }   // wavefronts per workgroup

// TA: tile rows of block bi that are computed (4 unless the launch has one block); DIAG: bj == bi
template <int TA, bool DIAG>
struct MomentShape {
    static constexpr int NW = moment_waves(DIAG);
    static constexpr int RA = 16 * TA;                          // staged rows of block bi
    static constexpr int R = RA + (DIAG ? 0 : kBlockRows);      // ... and of block bj
    static constexpr int NT = DIAG ? TA * (TA + 1) / 2 : TA * 4;
    static constexpr size_t kLdsBytes = sizeof(double) * NW * R * kPitch;
    static_assert(NT * 4 * kWave <= R * kPitch, "a wavefront's tiles fit its staging piece (the workgroup's sum)");
};

// partial[pair][workgroup][tile][4][64]: the tiles of the pair in the accumulator layout of the matrix instruction
// (column = lane & 15, row = (lane >> 4) + 4 * register), summed over the workgroup's wavefronts in order.
// grid (workgroups, pairs): DIAG pair = block bi; otherwise pair = bi (bi - 1) / 2 + bj, bj < bi.
template <int TA, bool DIAG>
__global__ void __launch_bounds__(moment_waves(DIAG) * kWave)
    trace_moments_kernel(const double* __restrict__ trace, int nslots, int dim, size_t dim_stride, int nchains, size_t npad,
                         const double* __restrict__ centre, double* __restrict__ partial) {
    typedef MomentShape<TA, DIAG> S;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    int bi = (int)blockIdx.y, bj = (int)blockIdx.y;
    if (!DIAG) {
        int p = (int)blockIdx.y;
        bi = 1;
        while (p >= bi) { p -= bi; ++bi; }
        bj = p;
    }
    const long long nblk = (nchains + kWave - 1) / kWave, units = (long long)nslots * nblk;
    const long long G = (long long)gridDim.x * S::NW, g = (long long)blockIdx.x * S::NW + wv;
    const long long u0 = units * g / G, u1 = units * (g + 1) / G;
    double* st = lds + (size_t)wv * S::R * kPitch;
    const size_t slot_stride = dim_stride * npad;
    // row i of the staged image is row `row(i)` of y
    auto row = [&](int i) __attribute__((always_inline)) {
        return i < S::RA ? kBlockRows * bi + i : kBlockRows * bj + (i - S::RA);
    };
    double raw[S::R];
    auto fetch = [&](long long slot, int cb) __attribute__((always_inline)) {
        const double* src = trace + (size_t)slot * slot_stride + (size_t)cb * kWave + lane;
#pragma unroll
        for (int i = 0; i < S::R; ++i) {
            const int r = row(i);
            raw[i] = r < dim ? src[(size_t)r * npad] : 0.0;       // wave-uniform: a row >= dim is not read
        }
    };
    f64x4 acc[S::NT];
#pragma unroll
    for (int t = 0; t < S::NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    // the off-diagonal pairs stage twice the rows: no room in the register file for a second unit in flight
    constexpr bool kPrefetch = DIAG;
    long long slot = u0 / nblk;                                   // the unit's (slot, chain block), counted along
    int cb = (int)(u0 % nblk);
    if (kPrefetch && u0 < u1) fetch(slot, cb);
    for (long long u = u0; u < u1; ++u) {
        if (!kPrefetch) fetch(slot, cb);
        const bool live = cb * kWave + lane < nchains;
#pragma unroll
        for (int i = 0; i < S::R; ++i) {
            const int r = row(i);
            const double v = r < dim ? raw[i] - centre[r] : (r == dim ? 1.0 : 0.0);
            st[i * kPitch + lane] = live ? v : 0.0;               // a select: the padding may hold NaN
        }
        if (++cb == (int)nblk) { cb = 0; ++slot; }
        if (kPrefetch && u + 1 < u1) fetch(slot, cb);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < kQuads; ++q) {
            double op[S::R / 16];
#pragma unroll
            for (int t = 0; t < S::R / 16; ++t) op[t] = st[(16 * t + (lane & 15)) * kPitch + 4 * q + (lane >> 4)];
            if (DIAG) {
#pragma unroll
                for (int a = 0; a < TA; ++a)
#pragma unroll
                    for (int b = 0; b <= a; ++b)
                        acc[a * (a + 1) / 2 + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[a], op[b], acc[a * (a + 1) / 2 + b], 0, 0, 0);
            } else {
#pragma unroll
                for (int a = 0; a < TA; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a * 4 + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[a], op[TA + b], acc[a * 4 + b], 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // the workgroup's sum, wavefronts ascending
    __syncthreads();
#pragma unroll
    for (int t = 0; t < S::NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(t * 4 + r) * kWave + lane] = acc[t][r];
    __syncthreads();
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (S::NT * 4 * kWave);
    for (int e = (int)threadIdx.x; e < S::NT * 4 * kWave; e += S::NW * kWave) {
        double s = lds[e];
#pragma unroll
        for (int w = 1; w < S::NW; ++w) s += lds[(size_t)w * S::R * kPitch + e];
        out[e] = s;
    }
}

// E[i][j] = E[j][i] = the sum over the workgroups, ascending, of element (i, j <= i); n = dim + 1 rows.  ta: the TA of
// the diagonal launch, nwg_d / nwg_o the workgroups per pair of the diagonal and off-diagonal launch.
__global__ void trace_moments_reduce_kernel(const double* __restrict__ pdiag, const double* __restrict__ poff, int n, int ta,
                                            int nwg_d, int nwg_o, double* __restrict__ E) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx % n;
    if (j > i) return;
    const int bi = i / kBlockRows, bj = j / kBlockRows, a = (i % kBlockRows) / 16, b = (j % kBlockRows) / 16;
    const int ii = i % 16, jj = j % 16;
    const int within = (ii / 4) * kWave + (ii % 4) * 16 + jj;     // register ii / 4 of lane (ii % 4) * 16 + jj
    const double* p;
    size_t stride;
    int nwg;
    if (bi == bj) {
        const int nt = ta * (ta + 1) / 2;
        stride = (size_t)nt * 4 * kWave;
        p = pdiag + (size_t)bi * nwg_d * stride + (size_t)(a * (a + 1) / 2 + b) * 4 * kWave + within;
        nwg = nwg_d;
    } else {
        stride = (size_t)16 * 4 * kWave;
        p = poff + (size_t)(bi * (bi - 1) / 2 + bj) * nwg_o * stride + (size_t)(a * 4 + b) * 4 * kWave + within;
        nwg = nwg_o;
    }
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += p[(size_t)w * stride];
    E[(size_t)i * n + j] = s;
    E[(size_t)j * n + i] = s;
}

template <int TA, bool DIAG>
hipError_t launch_moments(int nwg, int npairs, hipStream_t s, const double* trace, int nslots, int dim, int dim_stride,
                          int nchains, int npad, const double* centre, double* partial) {
    typedef MomentShape<TA, DIAG> S;
    auto kernel = trace_moments_kernel<TA, DIAG>;
    // more dynamic LDS than the default limit
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)S::kLdsBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(nwg, npairs), dim3(S::NW * kWave), S::kLdsBytes, s, trace, nslots, dim, (size_t)dim_stride,
                       nchains, (size_t)npad, centre, partial);
    return hipGetLastError();
}

// accepted[j] = mean[j] + sum_i r_i U(i, j), i ascending, for the columns j0 .. j0 + JB - 1 at a time; U and mean are
// padded with zeros to `pitch` columns (a multiple of JB) so that the inner loop carries no bounds.
// grid (chain groups of 256, slots: a stride loop where the grid's y extent does not cover them)
template <int JB>
__global__ void __launch_bounds__(256) cholesky_chain_kernel(const double* __restrict__ mean, const double* __restrict__ U,
                                                             int dim, int pitch, int nslots, int nchains, size_t npad,
                                                             size_t dim_stride, uint64_t seed, uint32_t chain_offset,
                                                             double* __restrict__ trace) {
    const size_t chain = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (chain >= (size_t)nchains) return;
    const uint32_t stream_chain = chain_offset + (uint32_t)chain;
    for (int slot = (int)blockIdx.y; slot < nslots; slot += (int)gridDim.y) {
        double* dst = trace + (size_t)slot * dim_stride * npad + chain;
        for (int j0 = 0; j0 < dim; j0 += JB) {
            double a[JB];
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) a[jj] = mean[j0 + jj];
            for (int i0 = 0; i0 < dim; i0 += 4) {
                const smcmc_u32x4 w = smcmc_draw_block(seed, stream_chain, (uint64_t)slot, (uint32_t)(i0 / 4), SMCMC_STREAM_CHOLESKY);
                double r[4];
                smcmc_normal_pair(w.v[0], w.v[1], &r[0], &r[1]);
                smcmc_normal_pair(w.v[2], w.v[3], &r[2], &r[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (i0 + k < dim) {                                   // wave-uniform
                        const double* u = U + (size_t)(i0 + k) * pitch + j0;
#pragma unroll
                        for (int jj = 0; jj < JB; ++jj) {
                            const double t = r[k] * u[jj];                // un-fused, CholeskyChain.C:58
                            a[jj] = a[jj] + t;
                        }
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < JB; ++jj)
                if (j0 + jj < dim) dst[(size_t)(j0 + jj) * npad] = a[jj];
        }
    }
}

}  // namespace

extern "C" int smcmc_trace_moments(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                   int nchains_padded, const double* centre, double* sum, double* sumsq, void* stream) {
    if (smcmc::reduce::bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded, smcmc_max_dim()) ||
        !sum || !sumsq)
        return SMCMC_ERR_INVALID;
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int n = dim + 1;                                        // rows of y = (x - centre, 1)
    const int B = (n + kBlockRows - 1) / kBlockRows;              // tile blocks
    const int ta = B == 1 ? (n + 15) / 16 : 4;
    const long long units = (long long)nslots * ((nchains + kWave - 1) / kWave);
    auto workgroups = [&](int nw) {
        const long long need = (units + nw - 1) / nw, cap = B == 1 ? kMaxWgOne : kMaxWgMany;
        return (int)(need < cap ? need : cap);
    };
    const int nwg_d = workgroups(4), nwg_o = workgroups(2), npairs_o = B * (B - 1) / 2;
    const size_t tile = 4 * kWave;
    smcmc::DeviceBuffer<double> d_centre, d_pdiag, d_poff, d_E;
    if (smcmc::reduce::centre_on_device(d_centre, centre, dim, s) != hipSuccess || d_pdiag.allocate((size_t)B * nwg_d * (ta * (ta + 1) / 2) * tile) != hipSuccess ||
        d_E.allocate((size_t)n * n) != hipSuccess)
        return SMCMC_ERR_HIP;
    if (npairs_o && d_poff.allocate((size_t)npairs_o * nwg_o * 16 * tile) != hipSuccess) return SMCMC_ERR_HIP;
    hipError_t e = hipSuccess;
    switch (ta) {
#define SMCMC_TM_CASE(t)                                                                                              \
    case t:                                                                                                           \
        e = launch_moments<t, true>(nwg_d, B, s, trace_device, nslots, dim, dim_stride, nchains, nchains_padded,     \
                                    d_centre.get(), d_pdiag.get());                                                  \
        break;
        SMCMC_TM_CASE(1) SMCMC_TM_CASE(2) SMCMC_TM_CASE(3) SMCMC_TM_CASE(4)
#undef SMCMC_TM_CASE
        default: return SMCMC_ERR_INVALID;
    }
    if (e != hipSuccess) return SMCMC_ERR_HIP;
    if (npairs_o) {
        e = launch_moments<4, false>(nwg_o, npairs_o, s, trace_device, nslots, dim, dim_stride, nchains, nchains_padded,
                                     d_centre.get(), d_poff.get());
        if (e != hipSuccess) return SMCMC_ERR_HIP;
    }
    hipLaunchKernelGGL(trace_moments_reduce_kernel, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, s, d_pdiag.get(),
                       d_poff.get(), n, ta, nwg_d, nwg_o, d_E.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    std::vector<double> E((size_t)n * n);
    if (hipMemcpyAsync(E.data(), d_E, sizeof(double) * n * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    for (int i = 0; i < dim; ++i) {
        sum[i] = E[(size_t)dim * n + i];
        for (int j = 0; j < dim; ++j) sumsq[(size_t)i * dim + j] = E[(size_t)i * n + j];
    }
    return SMCMC_OK;
}

extern "C" int smcmc_cholesky_chain(const double* mean, const double* covariance, int dim, int nslots, int nchains,
                                    int nchains_padded, int dim_stride, uint64_t seed, uint32_t chain_offset,
                                    double* trace_device, double* decomposition, void* stream) {
    if (smcmc::reduce::bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded, smcmc_max_dim()) ||
        !mean || !covariance)
        return SMCMC_ERR_INVALID;
    smcmc::SharedProposal prop(dim);
    prop.cov.assign(covariance, covariance + (size_t)dim * dim);
    if (!prop.choleskyOnly()) return SMCMC_ERR_RUNTIME;          // "Decomposition of the covariance has failed" :41-45
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int jb = dim <= 16 ? 16 : dim <= 32 ? 32 : 64;
    const int pitch = (dim + jb - 1) / jb * jb;
    std::vector<double> padded((size_t)(dim + 1) * pitch, 0.0);   // U, then the mean
    for (int i = 0; i < dim; ++i)
        for (int j = 0; j < dim; ++j) padded[(size_t)i * pitch + j] = prop.decomp[(size_t)i * dim + j];
    for (int j = 0; j < dim; ++j) padded[(size_t)dim * pitch + j] = mean[j];
    smcmc::DeviceBuffer<double> d_u;
    if (d_u.allocate(padded.size()) != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(d_u, padded.data(), sizeof(double) * padded.size(), hipMemcpyHostToDevice, s) != hipSuccess)
        return SMCMC_ERR_HIP;
    const dim3 grid((nchains + 255) / 256, nslots < 65535 ? nslots : 65535), block(256);
    const double* d_mean = d_u.get() + (size_t)dim * pitch;
#define SMCMC_CC_LAUNCH(JB)                                                                                             \
    hipLaunchKernelGGL(cholesky_chain_kernel<JB>, grid, block, 0, s, d_mean, d_u.get(), dim, pitch, nslots, nchains,    \
                       (size_t)nchains_padded, (size_t)dim_stride, seed, chain_offset, trace_device)
    if (jb == 16) SMCMC_CC_LAUNCH(16);
    else if (jb == 32) SMCMC_CC_LAUNCH(32);
    else SMCMC_CC_LAUNCH(64);
#undef SMCMC_CC_LAUNCH
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return SMCMC_ERR_HIP;   // `padded` is pageable: the copy has been staged, the kernel not run
    if (decomposition)
        for (size_t k = 0; k < (size_t)dim * dim; ++k) decomposition[k] = prop.decomp[k];
    return SMCMC_OK;
}
