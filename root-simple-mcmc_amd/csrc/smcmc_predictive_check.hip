// smcmc_predictive_check.hip -- smcmc_predictive_check and smcmc_poisson_draw (include/smcmc.h): the posterior-predictive
// check of a buffer of Poisson means hist[slot][rows][nchains_padded] -- the hist_device of smcmc_event_predictive_sums --
// against the observed counts.  For every point it draws the replicated data y[r] ~ Poisson(mu[r]) with the variate of
// include/smcmc_poisson.h, sums the likelihood's own bin term (smcmc_es_bin_term) over the observed and over the
// replicated data per group of rows and over all rows, and counts: per row how often the replicate fell below / on the
// observed count, per group how often its statistic did.
//
// A work item is one slot of one block of 64 chains, item = slot * nblocks + block, nblocks = ceil(nchains / 64), and one
// wavefront -- a workgroup of its own -- runs it; the grid is persistent (what the device holds at once, workgroup w
// taking the items w, w + G, ...).  Lane l owns the point (slot, 64 block + l) and walks its rows twice:
//   pass 1  reads the rows (one coalesced 512-byte load each, eight in flight) and decides whether the point is valid:
//           whether every row's mean is (smcmc_poisson_valid).  An invalid point draws nothing and enters no count.
//   pass 2  rows ascending: the next two rows' loads are issued ahead of the draw; data[r] is wave-uniform and read
//           through the constant address space; the draw's loop diverges between lanes by the uniform alone where the
//           means of a row are close.  Only the current group's two sums and the total's two are live in a lane.
// A lane whose chain is >= nchains, or whose point is invalid, skips the draw; what it writes is a select (+0.0 for the
// padding, NaN for an invalid point) and its predicate is false in every ballot.
//
// Counts.  Everything counted is an integer and wave-uniform: __popcll(__ballot(predicate)).  Row r's two counts are
// kept by lane r % 64 -- in a register while the walk is inside the row's block of 64 rows, then added to the lane's own
// words of the workgroup's LDS (below[rows], equal[rows]; no other lane touches them, so no barrier) -- and the
// statistic counts by lane 3 g + {0, 1, 2}, the invalid points by lane 3 (ngroups + 1), in a register for the whole
// launch.  At its end a workgroup adds its counts to the call's with one integer atomic per counter.  Integer addition
// commutes: the same numbers on every run and on every grid.  No floating-point value crosses a lane.
//
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "smcmc.h"
#include "smcmc_event_sample.h"
#include "smcmc_event_sample_error.hpp"
#include "smcmc_host.hpp"
#include "smcmc_kernels.hip.h"
#include "smcmc_poisson.h"
#include "smcmc_trace_reduce.hip.h"

namespace {

using smcmc::as_const;
using smcmc::cptr_f64;
using smcmc::kWave;
using u64 = unsigned long long;

static_assert(3 * (SMCMC_PREDICTIVE_CHECK_MAX_GROUPS + 1) + 1 <= kWave, "a lane per statistic counter");
static_assert(2 * SMCMC_PREDICTIVE_CHECK_MAX_ROWS * sizeof(u64) <= 65536, "the rows' counters fit the default LDS limit");
static_assert(SMCMC_PREDICTIVE_CHECK_MAX_ROWS <= SMCMC_POISSON_MAX_ROW, "a row fits its field of the counter");

// the statistic counters behind the rows' in `counts`: [ngroups + 1][3], then the invalid points
constexpr int stat_counters(int ngroups) { return 3 * (ngroups + 1) + 1; }

// grid: the persistent workgroups; block: one wavefront; dynamic LDS: 2 rows 64-bit counters
__global__ void __launch_bounds__(kWave)
    predictive_check_kernel(const double* __restrict__ hist, const double* __restrict__ data_, long long nitems, int nblocks,
                            int rows, int group_rows, int ngroups, int nchains, size_t npad, uint64_t seed,
                            uint32_t chain_offset, uint32_t slot_offset, uint32_t replica, double* __restrict__ rep,
                            double* __restrict__ stat, u64* __restrict__ counts) {
    extern __shared__ u64 cnt[];                // below[rows], equal[rows]; row r's two words are lane r % 64's alone
    const int lane = (int)threadIdx.x;
    const cptr_f64 data = as_const(data_);
    for (int r = lane; r < rows; r += kWave) {
        cnt[r] = 0;
        cnt[rows + r] = 0;
    }
    u64 keep_stat = 0;
    const int nstat_rows = 2 * (ngroups + 1);
    for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const long long slot = item / nblocks;
        const size_t chain = (size_t)(item % nblocks) * kWave + lane;         // < npad: nblocks * 64 <= npad
        const bool live = chain < (size_t)nchains;
        const double* const src = hist + (size_t)slot * rows * npad + chain;
        // pass 1: is every row's mean one a variate is drawn at?
        int ok = 1;
#pragma unroll 8
        for (int r = 0; r < rows; ++r) ok &= smcmc_poisson_valid(src[(size_t)r * npad]);
        const bool draw = live && ok;
        const double fill = live ? __builtin_nan("") : 0.0;                   // what a lane that does not draw writes
        const uint32_t gchain = chain_offset + (uint32_t)chain, gslot = slot_offset + (uint32_t)slot;
        double* const rout = rep ? rep + (size_t)slot * rows * npad + chain : nullptr;
        double* const sout = stat ? stat + (size_t)slot * nstat_rows * npad + chain : nullptr;
        // pass 2
        double group_obs = 0.0, group_rep = 0.0, total_obs = 0.0, total_rep = 0.0;
        uint32_t keep_below = 0, keep_equal = 0;
        int g = 0, group_end = group_rows;
        double e1 = src[0], e2 = rows > 1 ? src[npad] : 0.0;
        for (int r = 0; r < rows; ++r) {
            const double e = e1;
            e1 = e2;
            if (r + 2 < rows) e2 = src[(size_t)(r + 2) * npad];
            const double d = data[r];
            double y = fill;
            if (draw) {
                y = smcmc_poisson_from_uniform(e, smcmc_poisson_uniform_at(seed, gchain, gslot, (uint32_t)r, replica));
                const double t_obs = smcmc_es_bin_term(d, e), t_rep = smcmc_es_bin_term(y, e);
                group_obs += t_obs;
                group_rep += t_rep;
                total_obs += t_obs;
                total_rep += t_rep;
            }
            if (rout) rout[(size_t)r * npad] = y;
            const uint32_t nbelow = (uint32_t)__popcll(__ballot(draw && y < d));
            const uint32_t nequal = (uint32_t)__popcll(__ballot(draw && y == d));
            const int j = r & (kWave - 1);
            keep_below += lane == j ? nbelow : 0u;
            keep_equal += lane == j ? nequal : 0u;
            if (j == kWave - 1 || r + 1 == rows) {      // the block of 64 rows is done: lane l holds row r - j + l
                if (lane <= j) {
                    cnt[r - j + lane] += keep_below;
                    cnt[rows + r - j + lane] += keep_equal;
                }
                keep_below = 0;
                keep_equal = 0;
            }
            if (r + 1 == group_end) {
                if (sout) {
                    sout[(size_t)(2 * g) * npad] = draw ? group_obs : fill;
                    sout[(size_t)(2 * g + 1) * npad] = draw ? group_rep : fill;
                }
                const u64 less = (u64)__popcll(__ballot(draw && group_rep < group_obs));
                const u64 same = (u64)__popcll(__ballot(draw && group_rep == group_obs));
                const u64 compared = (u64)__popcll(__ballot(draw));
                keep_stat += lane == 3 * g ? less : lane == 3 * g + 1 ? same : lane == 3 * g + 2 ? compared : 0ull;
                group_obs = 0.0;
                group_rep = 0.0;
                ++g;
                group_end += group_rows;
            }
        }
        // entry ngroups: all rows, running sums of their own
        if (sout) {
            sout[(size_t)(2 * ngroups) * npad] = draw ? total_obs : fill;
            sout[(size_t)(2 * ngroups + 1) * npad] = draw ? total_rep : fill;
        }
        const u64 less = (u64)__popcll(__ballot(draw && total_rep < total_obs));
        const u64 same = (u64)__popcll(__ballot(draw && total_rep == total_obs));
        const u64 compared = (u64)__popcll(__ballot(draw));
        const u64 bad = (u64)__popcll(__ballot(live && !ok));
        const int at = 3 * ngroups;
        keep_stat += lane == at ? less : lane == at + 1 ? same : lane == at + 2 ? compared : lane == at + 3 ? bad : 0ull;
    }
    for (int r = lane; r < rows; r += kWave) {
        if (cnt[r]) atomicAdd(&counts[r], cnt[r]);
        if (cnt[rows + r]) atomicAdd(&counts[rows + r], cnt[rows + r]);
    }
    if (lane < stat_counters(ngroups) && keep_stat) atomicAdd(&counts[2 * rows + lane], keep_stat);
}

// lanes [first, npad) of every one of `nrows` rows of npad doubles: +0.0 (the chain blocks no work item covers)
hipError_t zero_dead_blocks(double* image, size_t npad, size_t first, size_t nrows, hipStream_t s) {
    if (first >= npad) return hipSuccess;
    return hipMemset2DAsync(image + first, npad * sizeof(double), 0, (npad - first) * sizeof(double), nrows, s);
}

int refuse(const std::string& why) {
    smcmc::es_set_last_error("smcmc_predictive_check: " + why);
    return SMCMC_ERR_INVALID;
}

}  // namespace

extern "C" int smcmc_poisson_draw(uint64_t seed, uint32_t chain, uint32_t slot, uint32_t row, uint32_t replica,
                                  double expectation, double* y, int* valid) {
    if (!y || !valid || slot >= SMCMC_POISSON_MAX_SLOT || row >= SMCMC_POISSON_MAX_ROW || replica >= SMCMC_POISSON_MAX_REPLICA)
        return SMCMC_ERR_INVALID;
    double v;
    *valid = smcmc_poisson_variate(seed, chain, slot, row, replica, expectation, &v);
    *y = v;
    return SMCMC_OK;
}

extern "C" int smcmc_predictive_check(const double* hist_device, int nslots, int rows, int nchains, int nchains_padded,
                                      const double* data, int ngroups, uint64_t seed, uint32_t chain_offset,
                                      uint32_t slot_offset, uint32_t replica, double* rep_device, double* stat_device,
                                      uint64_t* below, uint64_t* equal, uint64_t* stat_counts, uint64_t* invalid,
                                      void* stream) {
    if (!data || !below || !equal || !stat_counts || !invalid)
        return refuse("data, below, equal, stat_counts and invalid must be given");
    if (smcmc::reduce::bad_trace_shape(hist_device, nslots, rows, rows, nchains, nchains_padded,
                                       SMCMC_PREDICTIVE_CHECK_MAX_ROWS))
        return refuse("a buffer [nslots >= 1][1 <= rows <= SMCMC_PREDICTIVE_CHECK_MAX_ROWS][nchains_padded], "
                      "nchains_padded >= nchains >= 1 a multiple of 64");
    if (ngroups < 1 || ngroups > SMCMC_PREDICTIVE_CHECK_MAX_GROUPS || rows % ngroups != 0)
        return refuse("1 <= ngroups <= SMCMC_PREDICTIVE_CHECK_MAX_GROUPS must divide rows");
    for (int r = 0; r < rows; ++r)
        if (!(data[r] >= 0.0) || std::isinf(data[r])) return refuse("data must be finite and not negative");
    if ((uint64_t)slot_offset + (uint64_t)nslots > SMCMC_POISSON_MAX_SLOT || replica >= SMCMC_POISSON_MAX_REPLICA)
        return refuse("slot_offset + nslots <= 2^28 and replica < 2^16 (the variate's counter, include/smcmc_poisson.h)");
    smcmc::es_set_last_error("");
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;

    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (nchains + kWave - 1) / kWave;
    const long long nitems = (long long)nslots * nblocks;
    const size_t lds = (size_t)2 * rows * sizeof(u64);
    int device = 0, ncu = 0, per_cu = 0;
    if (hipGetDevice(&device) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, predictive_check_kernel, kWave, lds) != hipSuccess || ncu < 1 ||
        per_cu < 1)
        return SMCMC_ERR_HIP;
    const long long resident = (long long)ncu * per_cu;
    const unsigned workgroups = (unsigned)(nitems < resident ? nitems : resident);

    const size_t ncounts = (size_t)2 * rows + stat_counters(ngroups);
    smcmc::DeviceBuffer<double> d_data;
    smcmc::DeviceBuffer<u64> d_counts;
    if (d_data.allocate(rows) != hipSuccess || d_counts.allocate(ncounts) != hipSuccess) return SMCMC_ERR_HIP;
    if (hipMemcpyAsync(d_data, data, sizeof(double) * rows, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_counts, 0, sizeof(u64) * ncounts, s) != hipSuccess)
        return SMCMC_ERR_HIP;
    const size_t npad = (size_t)nchains_padded, covered = (size_t)nblocks * kWave;
    if (rep_device && zero_dead_blocks(rep_device, npad, covered, (size_t)nslots * rows, s) != hipSuccess) return SMCMC_ERR_HIP;
    if (stat_device && zero_dead_blocks(stat_device, npad, covered, (size_t)nslots * 2 * (ngroups + 1), s) != hipSuccess)
        return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(predictive_check_kernel, dim3(workgroups), dim3(kWave), lds, s, hist_device, d_data.get(), nitems,
                       nblocks, rows, rows / ngroups, ngroups, nchains, npad, seed, chain_offset, slot_offset, replica,
                       rep_device, stat_device, d_counts.get());
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    std::vector<u64> out(ncounts);
    if (hipMemcpyAsync(out.data(), d_counts, sizeof(u64) * ncounts, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    for (int r = 0; r < rows; ++r) {
        below[r] = out[r];
        equal[r] = out[(size_t)rows + r];
    }
    for (int k = 0; k < 3 * (ngroups + 1); ++k) stat_counts[k] = out[(size_t)2 * rows + k];
    *invalid = out[(size_t)2 * rows + 3 * (ngroups + 1)];
    return SMCMC_OK;
}
