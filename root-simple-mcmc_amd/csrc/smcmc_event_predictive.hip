// smcmc_event_predictive.hip -- smcmc_event_predictive_sums (include/smcmc.h): the simulated histograms of the likelihoods
// over a simulated event sample (SMCMC_LIKE_EVENT_SAMPLE, _TEMPLATE, _SHAPE) at every point of a saved trace, and their
// sums and sums of squares per bin -- WriteSimulation (example/FakeLikelihood.H:173-179, example2/:201-207,
// example3/:232-239) for the whole trace on the device, where the reference writes one point at a time.
//
// A work item is one slot of one block of 64 chains, item = slot * nblocks + block, nblocks = ceil(nchains / 64), and one
// wavefront -- a workgroup of its own -- runs it: lane l loads its point from trace[slot][d][64 block + l] (a row is one
// coalesced 512-byte read), evaluates it with the family's functions (include/smcmc_event_sample.h, smcmc_event_shape.h)
// and keeps the histograms in dynamic LDS as hist[row][lane], the step kernels' layout (smcmc_kernels.hip.h): NH nbins rows,
// one more for the events a cut or the axis drops, and for the shape its tables behind them.  The walk is the step
// kernels': event_fill's batches of kEsBatch, event order inside a bin; the two-pass members fill the signal, take its
// integral and its share ws * S[r], fill the background.  The packed sample is uploaded once per call and read through
// the constant address space.  Unlike the step kernels this one finishes the histograms: after the second pass the
// lane's column holds h[r] = share[r] + wb * B[r], the host evaluators' `hist`, bit for bit.
//
// The grid is persistent: as many workgroups as the device holds at once (at 50 bins (3 * 50 + 1) * 512 bytes of LDS, two to
// a compute unit), workgroup w taking the items w, w + G, w + 2 G ...  Between the passes the signal's share is parked
// in park[w][row][lane], a column block of the call's own per workgroup: a lane reads only what it wrote itself, in
// program order (no fence), and the call's scratch memory does not grow with the trace beyond the items' partial sums.
//
// A lane whose chain is >= nchains runs the walk on whatever its padding holds (NaN, anything): no index derived from the
// point leaves the lane's column -- a bin is smcmc_es_axis_bin's, -1 (the spare row) for any mass that is not inside
// [xmin, xmax), NaN included, and the shape's k comes from the packed event -- and its values are replaced by +0.0 with a
// select before they reach an output or a sum.
//
// Summation order, fixed: with y = h[t][r][c] - centre[r] and y * y rounded once, a wavefront adds the 64 lanes of its
// item by the xor 32, 16, 8, 4, 2, 1 butterfly (smcmc_trace_reduce.hip.h), lanes >= nchains as +0.0, and writes
// partial[item][2][rows]; ordered_rows_reduce_kernel then adds the items ascending from +0.  Which workgroup ran an item
// does not enter: the same bits on every run and on every grid.  A NaN histogram (a point that makes a class's integral
// 0) goes into its rows' sums as the NaN it is.
//
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample_error.hpp"
#include "smcmc_event_sample_host.hpp"
#include "smcmc_host.hpp"
#include "smcmc_kernels.hip.h"
#include "smcmc_trace_reduce.hip.h"

namespace {

using smcmc::as_const;
using smcmc::cptr_f64;
using smcmc::kWave;

// Without the step kernels' static LDS the whole compute unit is the histograms'
static_assert(smcmc::event_sample_lds_bytes(SMCMC_EVENT_SAMPLE_MAX_BINS) <= smcmc::kEsLdsLimit &&
              smcmc::event_shape_lds_bytes(SMCMC_EVENT_SHAPE_MAX_BINS) <= smcmc::kEsLdsLimit,
              "the histograms of one workgroup fit a compute unit's LDS at the parameter rules' largest nbins");
static_assert(2 * smcmc::event_sample_lds_bytes(50) <= smcmc::kEsLdsLimit,
              "two workgroups share a compute unit at the examples' 50 bins (example/, example2/)");

constexpr int predictive_dim(int like) { return like == SMCMC_LIKE_EVENT_SHAPE ? SMCMC_ESH_DIM : SMCMC_ES_DIM; }
constexpr int predictive_nh(int like) { return like == SMCMC_LIKE_EVENT_SHAPE ? 4 : 3; }

// grid: the persistent workgroups; block: one wavefront; dynamic LDS: event_lds_bytes(LIKE, nbins)
template <int LIKE>
__global__ void __launch_bounds__(kWave)
    event_predictive_kernel(const double* __restrict__ packed, const double* __restrict__ trace, long long nitems, int nblocks,
                            size_t dim_stride, int nchains, size_t npad, const double* __restrict__ centre_,
                            double* __restrict__ park_, double* __restrict__ hist_out, double* __restrict__ logl_out,
                            double* __restrict__ partial) {
    constexpr bool SHAPE = LIKE == SMCMC_LIKE_EVENT_SHAPE, TWO_PASS = LIKE != SMCMC_LIKE_EVENT_SAMPLE;
    constexpr int DIM = predictive_dim(LIKE), NH = predictive_nh(LIKE);
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = (int)threadIdx.x;
    const cptr_f64 prm = as_const(packed), centre = as_const(centre_);
    const int nev = (int)prm[SMCMC_ES_H_NEVENTS], nbins = (int)prm[SMCMC_ES_H_NBINS], nsig = (int)prm[SMCMC_ES_H_NSIGNAL];
    const double xmin = prm[SMCMC_ES_H_XMIN], xmax = prm[SMCMC_ES_H_XMAX], range = prm[SMCMC_ES_H_RANGE];
    const double cut = prm[SMCMC_ES_H_CUT], cut_very_close = SHAPE ? prm[SMCMC_ESH_H_CUT_VERY_CLOSE] : 0.0;
    const int rows = NH * nbins;                // row `rows`: the dropped events'
    double* const col = lds + lane;
    double* const tab = col + (size_t)(rows + 1) * kWave;       // (the shape's alone)
    double* const park = park_ + (size_t)blockIdx.x * rows * kWave + lane;      // (the two-pass members' alone)
    const cptr_f64 ev = prm + (SHAPE ? SMCMC_ESH_EVENTS(nbins) : SMCMC_ES_HEADER + rows);
    const cptr_f64 data = prm + SMCMC_ES_HEADER;
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const long long slot = item / nblocks;
        const size_t chain = (size_t)(item % nblocks) * kWave + lane;         // < npad: nblocks * 64 <= npad
        const bool live = chain < (size_t)nchains;
        const double* src = trace + (size_t)slot * dim_stride * npad + chain;
        double pt[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) pt[d] = src[(size_t)d * npad];
        smcmc_es_scalars s;
        double logl = 0.0;
        if constexpr (!TWO_PASS) {
            smcmc_es_point_scalars(pt, prm[SMCMC_ES_H_EXPOSURE], prm[SMCMC_ES_H_TRUE_FAKES], prm[SMCMC_ES_H_TRUE_EFF],
                                   prm[SMCMC_ES_H_TAN_FAKES], prm[SMCMC_ES_H_TAN_EFF], &s);
            for (int r = 0; r <= rows; ++r) col[r * kWave] = 0.0;
            smcmc::event_fill<false>(col, tab, 0, ev, 0, nev, s, nbins, rows, xmin, xmax, range, cut_very_close, cut);
            // FakeLikelihood.H:53-78: the bins of Close, Separated, DecayTag, in that order
            for (int r = 0; r < rows; ++r) logl += smcmc_es_bin_term(data[r], col[r * kWave]);
        } else {
            double yb[SHAPE ? SMCMC_ESH_NB : 1], ys[SHAPE ? SMCMC_ESH_NS : 1];
            if constexpr (SHAPE) {
                smcmc_esh_point_scalars(pt, prm[SMCMC_ES_H_TRUE_FAKES], prm[SMCMC_ES_H_TRUE_EFF], prm[SMCMC_ES_H_TAN_FAKES],
                                        prm[SMCMC_ES_H_TAN_EFF], &s);
#pragma unroll
                for (int i = 0; i < SMCMC_ESH_NB; ++i) yb[i] = smcmc_esh_control_b(pt, i);
#pragma unroll
                for (int i = 0; i < SMCMC_ESH_NS; ++i) ys[i] = smcmc_esh_control_s(pt, i);
            } else {
                smcmc_et_point_scalars(pt, prm[SMCMC_ES_H_TRUE_FAKES], prm[SMCMC_ES_H_TRUE_EFF], prm[SMCMC_ES_H_TAN_FAKES],
                                       prm[SMCMC_ES_H_TAN_EFF], &s);
            }
            double wb = 0.0;
#pragma nounroll
            for (int c = 0; c < 2; ++c) {           // (one copy of the fill's code)
                for (int r = 0; r <= rows; ++r) col[r * kWave] = 0.0;
                if constexpr (SHAPE) {
                    if (c == 0) smcmc::event_shape_tables<SMCMC_ESH_NS>(tab, ys, prm + SMCMC_ESH_CENTRE_S(nbins));
                    else smcmc::event_shape_tables<SMCMC_ESH_NB>(tab, yb, prm + SMCMC_ESH_CENTRE_B(nbins));
                }
                smcmc::event_fill<SHAPE>(col, tab, c ? SMCMC_ESH_NB : SMCMC_ESH_NS, ev, c ? nsig : 0, c ? nev : nsig, s, nbins,
                                         rows, xmin, xmax, range, cut_very_close, cut);
                const double norm = smcmc_et_norm(c ? pt[1] : pt[0], smcmc::event_integral<NH>(col, nbins));
                if (c == 0)
                    for (int r = 0; r < rows; ++r) park[(size_t)r * kWave] = smcmc_et_mc_signal(norm, col[r * kWave]);
                else wb = norm;
            }
            // the expectation before the clamp replaces the background's bin: the column is the evaluators' `hist`
            for (int r = 0; r < rows; ++r) {
                const double mc = smcmc_et_mc(park[(size_t)r * kWave], wb, col[r * kWave]);
                col[r * kWave] = mc;
                logl += smcmc_es_bin_term(data[r], mc);
            }
            if constexpr (SHAPE) {
                const double pen_b = smcmc::event_shape_penalty<SMCMC_ESH_NB>(yb, prm + SMCMC_ESH_KINV_B(nbins));
                const double pen_s = smcmc::event_shape_penalty<SMCMC_ESH_NS>(ys, prm + SMCMC_ESH_KINV_S(nbins));
                logl = smcmc_esh_penalties(logl, pt, pen_b, pen_s);
            } else {
                logl = smcmc_et_penalties(logl, pt[0], pt[1], pt[6], pt[7], pt[8]);
            }
        }
        if (logl_out) logl_out[(size_t)slot * npad + chain] = live ? logl : 0.0;
        // the rows' sums over the item's lanes, 64 rows at a time: lane j keeps row r0 + j, one store per 64 rows
        double* const pout = partial + (size_t)item * 2 * rows;
        double* const hout = hist_out ? hist_out + (size_t)slot * rows * npad + chain : nullptr;
        for (int r0 = 0; r0 < rows; r0 += kWave) {
            const int nr = rows - r0 < kWave ? rows - r0 : kWave;
            double keep_sum = 0.0, keep_sq = 0.0;
            for (int j = 0; j < nr; ++j) {
                const int r = r0 + j;
                const double h = col[r * kWave];
                if (hout) hout[(size_t)r * npad] = live ? h : 0.0;
                const double y = h - centre[r];
                const double yy = y * y;
                double a = live ? y : 0.0, b = live ? yy : 0.0;     // a select: the padding may hold NaN
#pragma unroll
                for (int off = kWave / 2; off >= 1; off >>= 1) {
                    a += __shfl_xor(a, off, kWave);
                    b += __shfl_xor(b, off, kWave);
                }
                keep_sum = (lane == j) ? a : keep_sum;
                keep_sq = (lane == j) ? b : keep_sq;
            }
            if (lane < nr) {
                pout[r0 + lane] = keep_sum;
                pout[rows + r0 + lane] = keep_sq;
            }
        }
    }
}

struct Launch {
    hipError_t status;
    int workgroups;
};

// the persistent grid of `kernel` at `lds` bytes of dynamic LDS: what the device holds at once, at most one per item
template <int LIKE>
Launch predictive_grid(int lds, long long nitems) {
    auto kernel = event_predictive_kernel<LIKE>;
    constexpr int cap = smcmc::event_lds_bytes(LIKE, smcmc::event_max_bins(LIKE));
    // more dynamic LDS than the default limit, as the engine sets it for the step kernels
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e != hipSuccess) return {e, 0};
    int device = 0, ncu = 0, per_cu = 0;
    if ((e = hipGetDevice(&device)) != hipSuccess) return {e, 0};
    if ((e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return {e, 0};
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWave, (size_t)lds)) != hipSuccess) return {e, 0};
    if (ncu < 1 || per_cu < 1) return {hipErrorInvalidValue, 0};
    const long long resident = (long long)ncu * per_cu;
    return {hipSuccess, (int)(nitems < resident ? nitems : resident)};
}

template <int LIKE>
hipError_t predictive_launch(int workgroups, int lds, hipStream_t s, const double* packed, const double* trace, long long nitems,
                             int nblocks, int dim_stride, int nchains, int npad, const double* centre, double* park,
                             double* hist_out, double* logl_out, double* partial) {
    hipLaunchKernelGGL(event_predictive_kernel<LIKE>, dim3((unsigned)workgroups), dim3(kWave), (size_t)lds, s, packed, trace,
                       nitems, nblocks, (size_t)dim_stride, nchains, (size_t)npad, centre, park, hist_out, logl_out, partial);
    return hipGetLastError();
}

// lanes [first, npad) of every one of `nrows` rows of npad doubles: +0.0 (the chain blocks no work item covers)
hipError_t zero_dead_blocks(double* image, size_t npad, size_t first, size_t nrows, hipStream_t s) {
    if (first >= npad) return hipSuccess;
    return hipMemset2DAsync(image + first, npad * sizeof(double), 0, (npad - first) * sizeof(double), nrows, s);
}

int refuse(const std::string& why) {
    smcmc::es_set_last_error("smcmc_event_predictive_sums: " + why);
    return SMCMC_ERR_INVALID;
}

}  // namespace

extern "C" int smcmc_event_predictive_sums(int likelihood, const double* params, int count, const double* trace_device,
                                           int nslots, int dim_stride, int nchains, int nchains_padded, const double* centre,
                                           double* hist_device, double* logl_device, double* sum, double* sumsq,
                                           void* stream) {
    if (!smcmc::event_likelihood(likelihood))
        return refuse("SMCMC_LIKE_EVENT_SAMPLE, SMCMC_LIKE_EVENT_TEMPLATE or SMCMC_LIKE_EVENT_SHAPE");
    if (count < 0) return refuse("count must not be negative");
    const char* why = smcmc::es_check_like(likelihood, params, (size_t)count);
    if (why) {
        smcmc::es_set_last_error(why);
        return SMCMC_ERR_INVALID;
    }
    const int dim = smcmc::event_likelihood_dim(likelihood);
    if (smcmc::reduce::bad_trace_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded))
        return refuse("a trace [nslots >= 1][dim_stride >= dim][nchains_padded], nchains_padded >= nchains >= 1 a multiple of 64");
    if (!sum || !sumsq) return refuse("sum and sumsq must be given");
    smcmc::es_set_last_error("");
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;

    hipStream_t s = (hipStream_t)stream;
    std::vector<double> packed;
    smcmc::es_pack(likelihood, params, packed);
    const int nbins = (int)packed[SMCMC_ES_H_NBINS], rows = predictive_nh(likelihood) * nbins;
    const int lds = smcmc::event_lds_bytes(likelihood, nbins);
    const int nblocks = (nchains + kWave - 1) / kWave;
    const long long nitems = (long long)nslots * nblocks;
    const bool two_pass = likelihood != SMCMC_LIKE_EVENT_SAMPLE;

    Launch grid{hipErrorInvalidValue, 0};
    switch (likelihood) {
        case SMCMC_LIKE_EVENT_SAMPLE: grid = predictive_grid<SMCMC_LIKE_EVENT_SAMPLE>(lds, nitems); break;
        case SMCMC_LIKE_EVENT_TEMPLATE: grid = predictive_grid<SMCMC_LIKE_EVENT_TEMPLATE>(lds, nitems); break;
        case SMCMC_LIKE_EVENT_SHAPE: grid = predictive_grid<SMCMC_LIKE_EVENT_SHAPE>(lds, nitems); break;
    }
    if (grid.status != hipSuccess) return SMCMC_ERR_HIP;

    smcmc::DeviceBuffer<double> d_packed, d_centre, d_park, d_partial, d_out;
    if (d_packed.allocate(packed.size()) != hipSuccess || d_partial.allocate((size_t)nitems * 2 * rows) != hipSuccess ||
        d_out.allocate((size_t)2 * rows) != hipSuccess ||
        (two_pass && d_park.allocate((size_t)grid.workgroups * rows * kWave) != hipSuccess))
        return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(d_packed, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        smcmc::reduce::centre_on_device(d_centre, centre, rows, s) != hipSuccess)
        return SMCMC_ERR_HIP;
    const size_t npad = (size_t)nchains_padded, covered = (size_t)nblocks * kWave;
    if (hist_device && zero_dead_blocks(hist_device, npad, covered, (size_t)nslots * rows, s) != hipSuccess) return SMCMC_ERR_HIP;
    if (logl_device && zero_dead_blocks(logl_device, npad, covered, (size_t)nslots, s) != hipSuccess) return SMCMC_ERR_HIP;

    hipError_t e = hipErrorInvalidValue;
#define SMCMC_EP_CASE(like)                                                                                              \
    case like:                                                                                                          \
        e = predictive_launch<like>(grid.workgroups, lds, s, d_packed.get(), trace_device, nitems, nblocks, dim_stride, \
                                    nchains, nchains_padded, d_centre.get(), d_park.get(), hist_device, logl_device,   \
                                    d_partial.get());                                                                   \
        break;
    switch (likelihood) {
        SMCMC_EP_CASE(SMCMC_LIKE_EVENT_SAMPLE)
        SMCMC_EP_CASE(SMCMC_LIKE_EVENT_TEMPLATE)
        SMCMC_EP_CASE(SMCMC_LIKE_EVENT_SHAPE)
    }
#undef SMCMC_EP_CASE
    if (e != hipSuccess) return SMCMC_ERR_HIP;
    // out[row][2] = the items' partial sums, ascending
    smcmc::reduce::launch_ordered_rows_reduce<double>(s, d_partial.get(), nitems, 2, rows, rows, rows, d_out.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    std::vector<double> out((size_t)2 * rows);
    if (hipMemcpyAsync(out.data(), d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    for (int r = 0; r < rows; ++r) {
        sum[r] = out[(size_t)2 * r];
        sumsq[r] = out[(size_t)2 * r + 1];
    }
    return SMCMC_OK;
}
