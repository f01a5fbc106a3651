// smcmc_order_statistics.hip -- smcmc_trace_digit_counts and smcmc_trace_order_statistics (include/smcmc.h): exact order
// statistics of the rows of a saved trace -- medians, credible intervals, the quantile band of a predicted bin -- selected
// on the device, so that the trace (slots x dim x chains doubles) never crosses PCIe and is never sorted.  The order is
// that of include/smcmc_order_key.h: unsigned comparison of key(x).
//
// A radix selection from the most significant byte down, eight passes of eight bits.  Before pass p every (row, rank)
// knows the top 8p bits of its answer's key (its prefix) and its residual rank among the entries that share them.  Pass p
// counts, per row and per DISTINCT prefix of the row, the entries that share the prefix by their next byte -- 256
// counters -- and the pick kernel walks the counters' running sum to the byte the residual rank falls into, appends it to
// the prefix, and takes the entries in front of it off the residual rank (and onto `below`).  After pass 7 the prefix is
// the key; the last counter picked is `equal`.
//
// Two kernels, the first bound by the HBM reads of the trace (eight reads of it in all):
//  * digit_count_kernel: a row is nslots pieces of nchains_padded doubles; taken two doubles at a time (16 bytes per lane
//    when the trace's address allows, otherwise two 8-byte loads) it is a sequence of nslots * nchains_padded / 2 items,
//    and a workgroup of 256 lanes counts one chunk of consecutive items: lanes run along the chain axis, four loads in
//    flight per lane (eight entries: a batch).  The key is taken as its two 32-bit words.  An entry's top 8p bits cost
//    one range test of the high word against the smallest and largest prefix of the row (from pass 1 on most entries
//    match none, and a wavefront without a candidate goes on to its next batch), then one comparison per distinct
//    prefix.  Hits go to a 32-bit histogram in LDS, [prefix][256].  A posterior's values share sign and exponent, so in
//    the early passes nearly every entry of a wavefront's batch hits the same counter: the entries are aggregated first
//    -- take the first active lane's counter, ballot the entries that share it, add the popcounts once -- for up to
//    kPeel rounds; entries still left after that are on scattered counters and add 1 each.  At the end the non-zero
//    counters are added to the global 64-bit counts with vector atomics.  Integer adds commute: the same counts on
//    every run.
//  * digit_pick_kernel: one workgroup per row, one wavefront per rank in turn: lane l sums the counters 4l .. 4l + 3, an
//    inclusive scan over the lanes finds the lane, that lane the byte.  Then one lane lists the row's distinct new
//    prefixes for the next pass, and the workgroup clears the counters the pass used.
// A 32-bit LDS counter cannot wrap: a workgroup counts each entry of its chunk once per pass, and a chunk is at most
// kMaxChunkEntries = 2^31 entries (static_assert below).
//
// Padding lanes (chain >= nchains) are loaded -- they lie inside the trace -- and dropped by a select before anything
// is counted; rows >= dim are never addressed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "smcmc.h"
#include "smcmc_host.hpp"
#include "smcmc_order_key.h"
#include "smcmc_trace_reduce.hip.h"

namespace {

using smcmc::reduce::kWave;
typedef unsigned long long u64;

constexpr int kThreads = 256;                   // lanes per workgroup, both kernels
constexpr int kInFlight = 4;                    // 16-byte loads in flight per lane
constexpr int kDigits = 1 << SMCMC_ORDER_DIGIT_BITS;
constexpr int kPeel = 4;                        // rounds of wavefront aggregation before the lanes add 1 each
constexpr long long kChunkEntries = 2048;       // entries per workgroup: one round of kInFlight loads, so that a small
                                                // trace still fills the device (a pass over it is bound by latency)
constexpr long long kMaxChunkEntries = 1ll << 31;
constexpr long long kTargetGroups = 2048;       // workgroups per launch beyond which the chunk is doubled
static_assert(kMaxChunkEntries < (1ll << 32), "a 32-bit LDS counter cannot wrap: a chunk's entries are counted once each");
static_assert(kChunkEntries % (2 * kThreads * kInFlight) == 0 && kChunkEntries <= kMaxChunkEntries, "whole rounds per chunk");
static_assert(SMCMC_ORDER_DIGIT_BITS * SMCMC_ORDER_PASSES == 64, "the passes cover the key");
static_assert(kDigits == 4 * kWave, "the pick kernel: four counters per lane");
static_assert((size_t)SMCMC_ORDER_MAX_RANKS * kDigits * sizeof(uint32_t) <= 32 * 1024, "the LDS histogram: 32 KB at most");

// hist[index] += 1 for every entry of the wavefront's batch with index >= 0 (eight entries a lane), the entries that share
// a counter aggregated first: take the counter of the first lane that still holds an entry, ballot every entry of the
// batch against it, add the popcounts once.  kPeel such rounds, then the entries still left add 1 each.  Called by whole
// wavefronts.
__device__ __forceinline__ void count_batch(uint32_t* hist, int (&index)[kInFlight][2], int lane) {
#pragma unroll 1
    for (int round = 0; round < kPeel; ++round) {
        int lead = -1;                   // the lane's first entry still to count
#pragma unroll
        for (int k = 2 * kInFlight - 1; k >= 0; --k) lead = index[k / 2][k % 2] >= 0 ? index[k / 2][k % 2] : lead;
        const u64 have = __ballot(lead >= 0);
        if (have == 0) return;           // the same for the whole wavefront
        const int first = __builtin_amdgcn_readlane(lead, __ffsll(have) - 1);
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < 2 * kInFlight; ++k) {
            const bool same = index[k / 2][k % 2] == first;
            total += (uint32_t)__popcll(__ballot(same));
            index[k / 2][k % 2] = same ? -1 : index[k / 2][k % 2];
        }
        if (lane == 0) atomicAdd(&hist[first], total);
    }
#pragma unroll
    for (int k = 0; k < 2 * kInFlight; ++k)
        if (index[k / 2][k % 2] >= 0) atomicAdd(&hist[index[k / 2][k % 2]], 1u);
}

// grid (chunks, dim); dynamic LDS: cap * 256 words.  uniq[d][cap]: the distinct prefixes of row d, nuniq[d] of them
// (pass 0: not read, one empty prefix).  counts[d][cap][256] += this chunk's.
template <bool WIDE>
__global__ void __launch_bounds__(kThreads)
    digit_count_kernel(const double* __restrict__ trace, int nslots, size_t slot_stride, int nchains, size_t npad,
                       long long chunk_items, int pass, int cap, const u64* __restrict__ uniq, const int* __restrict__ nuniq,
                       u64* __restrict__ counts) {
    extern __shared__ uint32_t hist[];
    // the row's distinct prefixes, left-aligned in the key and split into its two words
    __shared__ uint32_t s_hi[SMCMC_ORDER_MAX_RANKS], s_lo[SMCMC_ORDER_MAX_RANKS];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int d = blockIdx.y;
    // the top 8p bits of a key as masks of its two words, and the word and shift of the next byte; everything on the
    // entries is 32-bit arithmetic
    const int bits = SMCMC_ORDER_DIGIT_BITS * pass;
    const uint32_t mask_hi = bits == 0 ? 0u : (bits >= 32 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (32 - bits));
    const uint32_t mask_lo = bits <= 32 ? 0u : 0xFFFFFFFFu << (64 - bits);
    const bool digit_in_hi = bits < 32;
    const int digit_shift = (56 - bits) & 31;
    int n = 1;
    if (pass > 0) {
        n = nuniq[d];
        n = n < 1 ? 1 : (n > cap ? cap : n);    // (never outside: the histogram's bounds do not hang on it)
        if (tid < n) {
            const u64 p = uniq[(size_t)d * cap + tid] << (64 - bits);
            s_hi[tid] = (uint32_t)(p >> 32);
            s_lo[tid] = (uint32_t)p;
        }
    } else if (tid == 0) {
        s_hi[0] = s_lo[0] = 0u;                 // the empty prefix: under masks of 0 every entry shares it
    }
    for (int k = tid; k < n * kDigits; k += kThreads) hist[k] = 0u;
    __syncthreads();
    // the range the prefixes' high words span: what an entry is tested against first
    uint32_t hmin = s_hi[0], hmax = s_hi[0];
    for (int i = 1; i < n; ++i) {
        const uint32_t p = s_hi[i];
        hmin = p < hmin ? p : hmin;
        hmax = p > hmax ? p : hmax;
    }
    const uint32_t hspan = hmax - hmin;

    const long long half = (long long)(npad / 2);                     // items per slot
    const long long total = (long long)nslots * half;
    const long long begin = (long long)blockIdx.x * chunk_items;
    const long long end = begin + chunk_items < total ? begin + chunk_items : total;
    const double* const row = trace + (size_t)d * npad;
    // this lane's item as (slot, pair of chains) and as an offset into the row, and what a step of kThreads items does
    // to them
    const long long slot0 = (begin + tid) / half;
    long long pair = (begin + tid) - slot0 * half;
    size_t offset = (size_t)slot0 * slot_stride + (size_t)pair * 2;
    const long long step_pairs = kThreads % half;
    const size_t step_offset = (size_t)(kThreads / half) * slot_stride + (size_t)step_pairs * 2;
    const size_t wrap_offset = slot_stride - npad;                    // a pair past the slot's end: on to the next slot

    for (long long base = begin; base < end; base += (long long)kThreads * kInFlight) {   // the same for the whole workgroup
        double v[kInFlight][2];
        bool live[kInFlight][2];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const bool in = base + (long long)u * kThreads + tid < end;
            // a lane past the chunk's end loads the row's first item and drops it: no branch around a load
            const double* src = row + (in ? offset : 0);
            if constexpr (WIDE) {
                const double2 w = *reinterpret_cast<const double2*>(src);
                v[u][0] = w.x;
                v[u][1] = w.y;
            } else {
                v[u][0] = src[0];
                v[u][1] = src[1];
            }
            live[u][0] = in && pair * 2 < nchains;
            live[u][1] = in && pair * 2 + 1 < nchains;
            pair += step_pairs;
            offset += step_offset;
            if (pair >= half) {
                pair -= half;
                offset += wrap_offset;
            }
        }
        int index[kInFlight][2];         // prefix number * 256 + digit, -1: not counted
        int digit[kInFlight][2];
        uint32_t top_hi[kInFlight][2], top_lo[kInFlight][2];
        bool candidate[kInFlight][2], any = false;
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                // key(x) of include/smcmc_order_key.h on the two words of x
                const double x = v[u][e];
                const uint32_t b_hi = (uint32_t)__double2hiint(x), b_lo = (uint32_t)__double2loint(x);
                const uint32_t flip = (uint32_t)((int32_t)b_hi >> 31);          // all ones for a negative x
                const bool nan = x != x;
                const uint32_t key_hi = nan ? 0xFFFFFFFFu : b_hi ^ (flip | 0x80000000u);
                const uint32_t key_lo = nan ? 0xFFFFFFFFu : b_lo ^ flip;
                digit[u][e] = (int)(((digit_in_hi ? key_hi : key_lo) >> digit_shift) & (kDigits - 1));
                top_hi[u][e] = key_hi & mask_hi;
                top_lo[u][e] = key_lo & mask_lo;
                // the range test: from pass 1 on most entries fail it, and a wavefront without a candidate skips the
                // comparisons below
                candidate[u][e] = live[u][e] && top_hi[u][e] - hmin <= hspan;
                any = any || candidate[u][e];
                index[u][e] = -1;
            }
        if (__ballot(any) == 0) continue;       // the same for the whole wavefront
        // which prefix: the row's are distinct, so at most one matches
        for (int i = 0; i < n; ++i) {
            const uint32_t p_hi = s_hi[i], p_lo = s_lo[i];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u)
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    index[u][e] = candidate[u][e] && top_hi[u][e] == p_hi && top_lo[u][e] == p_lo ? i * kDigits + digit[u][e]
                                                                                                  : index[u][e];
        }
        count_batch(hist, index, lane);
    }
    __syncthreads();
    for (int k = tid; k < n * kDigits; k += kThreads) {
        const uint32_t c = hist[k];
        if (c) atomicAdd(&counts[(size_t)d * cap * kDigits + k], (u64)c);
    }
}

// What a (row, rank) carries from pass to pass, [dim][nranks] each, and the row's distinct prefixes.
struct SelectState {
    u64* prefix;     // the top 8p bits of the answer's key
    u64* resid;      // the rank among the entries that share them
    u64* below;      // the entries in front of them
    u64* equal;      // after the last pass: the entries with the key
    u64* uniq;       // [dim][cap] the row's distinct prefixes
    int* nuniq;      // [dim]
    int* slot_of;    // [dim][cap] rank -> its prefix's place in uniq
};

struct RankList {
    u64 r[SMCMC_ORDER_MAX_RANKS];
};

// resid[d][r] = ranks[r]; everything else of the state was cleared with the buffer
__global__ void select_init_kernel(RankList ranks, int dim, int nranks, u64* __restrict__ resid) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < dim * nranks) resid[idx] = ranks.r[idx % nranks];
}

// grid (dim); cap = nranks.  After pass p's counts.
__global__ void __launch_bounds__(kThreads) digit_pick_kernel(int pass, int nranks, SelectState st, u64* __restrict__ counts) {
    __shared__ u64 s_new[SMCMC_ORDER_MAX_RANKS];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int d = blockIdx.x, cap = nranks;
    int n_old = pass == 0 ? 1 : st.nuniq[d];
    n_old = n_old < 1 ? 1 : (n_old > cap ? cap : n_old);
    for (int r = wave; r < nranks; r += kThreads / kWave) {    // the same for the whole wavefront
        const size_t at = (size_t)d * nranks + r;
        int place = pass == 0 ? 0 : st.slot_of[(size_t)d * cap + r];
        place = place < 0 ? 0 : (place >= cap ? cap - 1 : place);
        const u64* c = counts + ((size_t)d * cap + place) * kDigits + 4 * lane;
        const u64 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        const u64 mine = c0 + c1 + c2 + c3;
        u64 incl = mine;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const u64 t = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += t;
        }
        const u64 res = st.resid[at];
        const u64 excl = incl - mine;
        const u64 hit = __ballot(excl <= res && res < incl);
        // the residual rank is below the number of entries that share the prefix, so a lane holds it; should the
        // counts ever not add up, the last lane answers and nothing is indexed out of range
        const int owner = hit ? __ffsll(hit) - 1 : kWave - 1;
        if (lane == owner) {
            u64 before = excl, cnt = c0;
            int g = 0;
            if (res >= before + c0) { before += c0; cnt = c1; g = 1;
                if (res >= before + c1) { before += c1; cnt = c2; g = 2;
                    if (res >= before + c2) { before += c2; cnt = c3; g = 3; } } }
            const u64 p = (pass == 0 ? 0 : st.prefix[at] << SMCMC_ORDER_DIGIT_BITS) | (u64)(4 * lane + g);
            st.prefix[at] = p;
            st.resid[at] = res - before;
            st.below[at] += before;
            if (pass == SMCMC_ORDER_PASSES - 1) st.equal[at] = cnt;
            s_new[r] = p;
        }
    }
    __syncthreads();
    // the counters this pass used, for the next one
    for (int k = tid; k < n_old * kDigits; k += kThreads) counts[(size_t)d * cap * kDigits + k] = 0;
    if (tid == 0 && pass < SMCMC_ORDER_PASSES - 1) {
        int n = 0;
        for (int r = 0; r < nranks; ++r) {
            int place = -1;
            for (int k = 0; k < n; ++k)
                if (st.uniq[(size_t)d * cap + k] == s_new[r]) place = k;
            if (place < 0) {
                place = n++;
                st.uniq[(size_t)d * cap + place] = s_new[r];
            }
            st.slot_of[(size_t)d * cap + r] = place;
        }
        st.nuniq[d] = n;
    }
}

// the chunk of a launch over `total_items` items per row and `dim` rows
long long chunk_items_for(long long total_items, int dim) {
    long long chunk = kChunkEntries / 2;
    while (((total_items + chunk - 1) / chunk) * dim > kTargetGroups && chunk * 2 <= kMaxChunkEntries / 2) chunk *= 2;
    return chunk;
}

hipError_t launch_count(hipStream_t s, const double* trace, int nslots, int dim, int dim_stride, int nchains, int npad,
                        int pass, int cap, const u64* uniq, const int* nuniq, u64* counts) {
    const long long total_items = (long long)nslots * (npad / 2);
    const long long chunk = chunk_items_for(total_items, dim);
    const dim3 grid((unsigned)((total_items + chunk - 1) / chunk), (unsigned)dim);
    const size_t lds = (size_t)(pass == 0 ? 1 : cap) * kDigits * sizeof(uint32_t);
    const size_t slot_stride = (size_t)dim_stride * npad;
    if (reinterpret_cast<uintptr_t>(trace) % 16 == 0)
        hipLaunchKernelGGL(digit_count_kernel<true>, grid, dim3(kThreads), lds, s, trace, nslots, slot_stride, nchains,
                           (size_t)npad, chunk, pass, cap, uniq, nuniq, counts);
    else
        hipLaunchKernelGGL(digit_count_kernel<false>, grid, dim3(kThreads), lds, s, trace, nslots, slot_stride, nchains,
                           (size_t)npad, chunk, pass, cap, uniq, nuniq, counts);
    return hipGetLastError();
}

bool bad_order_shape(const double* trace, int nslots, int dim, int dim_stride, int nchains, int npad) {
    return smcmc::reduce::bad_trace_shape(trace, nslots, dim, dim_stride, nchains, npad, SMCMC_ORDER_MAX_DIM);
}

}  // namespace

extern "C" uint64_t smcmc_order_key(double x) { return smcmc_order_key_of(x); }

extern "C" double smcmc_order_value(uint64_t key) { return smcmc_order_value_of(key); }

extern "C" int smcmc_order_chunk_entries(void) { return (int)kChunkEntries; }

extern "C" int smcmc_trace_digit_counts(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                        int nchains_padded, int pass, int nprefix, const uint64_t* prefixes,
                                        uint64_t* counts, void* stream) {
    if (bad_order_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded) || pass < 0 ||
        pass >= SMCMC_ORDER_PASSES || nprefix < 1 || nprefix > SMCMC_ORDER_MAX_RANKS || !counts || (pass > 0 && !prefixes))
        return SMCMC_ERR_INVALID;
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    // the kernel counts a row's DISTINCT prefixes: list them, and where each of the caller's is in the list
    std::vector<int> place((size_t)dim * nprefix, 0), nuniq(dim, 1);
    int cap = 1;
    if (pass > 0) {
        for (int d = 0; d < dim; ++d) {
            const uint64_t* p = prefixes + (size_t)d * nprefix;
            int n = 0;
            for (int i = 0; i < nprefix; ++i) {
                if (p[i] >> (SMCMC_ORDER_DIGIT_BITS * pass)) {     // bits above the pass's: no entry's prefix
                    place[(size_t)d * nprefix + i] = -1;
                    continue;
                }
                int at = -1;
                for (int k = 0; k < i && at < 0; ++k)
                    if (p[k] == p[i]) at = place[(size_t)d * nprefix + k];
                place[(size_t)d * nprefix + i] = at < 0 ? n++ : at;
            }
            nuniq[d] = n;                                          // (0: the kernel counts one prefix, 0, that nobody reads)
            cap = n > cap ? n : cap;
        }
    }
    std::vector<u64> uniq((size_t)dim * cap, 0);
    if (pass > 0)
        for (int d = 0; d < dim; ++d)
            for (int i = 0; i < nprefix; ++i)
                if (place[(size_t)d * nprefix + i] >= 0)
                    uniq[(size_t)d * cap + place[(size_t)d * nprefix + i]] = prefixes[(size_t)d * nprefix + i];
    const size_t ncounts = (size_t)dim * cap * kDigits;
    smcmc::DeviceBuffer<u64> d_counts, d_uniq;
    smcmc::DeviceBuffer<int> d_nuniq;
    if (d_counts.allocate(ncounts) != hipSuccess || d_uniq.allocate(uniq.size()) != hipSuccess ||
        d_nuniq.allocate(dim) != hipSuccess)
        return SMCMC_ERR_HIP;
    if (hipMemsetAsync(d_counts, 0, sizeof(u64) * ncounts, s) != hipSuccess ||
        hipMemcpyAsync(d_uniq, uniq.data(), sizeof(u64) * uniq.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_nuniq, nuniq.data(), sizeof(int) * dim, hipMemcpyHostToDevice, s) != hipSuccess)
        return SMCMC_ERR_HIP;
    if (launch_count(s, trace_device, nslots, dim, dim_stride, nchains, nchains_padded, pass, cap, d_uniq.get(), d_nuniq.get(),
                     d_counts.get()) != hipSuccess)
        return SMCMC_ERR_HIP;
    std::vector<u64> got(ncounts);
    if (hipMemcpyAsync(got.data(), d_counts, sizeof(u64) * ncounts, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    for (int d = 0; d < dim; ++d)
        for (int i = 0; i < nprefix; ++i) {
            const int at = place[(size_t)d * nprefix + i];
            const u64* src = got.data() + ((size_t)d * cap + (at < 0 ? 0 : at)) * kDigits;
            uint64_t* dst = counts + ((size_t)d * nprefix + i) * kDigits;
            for (int g = 0; g < kDigits; ++g) dst[g] = at < 0 ? 0 : src[g];
        }
    return SMCMC_OK;
}

extern "C" int smcmc_trace_order_statistics(const double* trace_device, int nslots, int dim, int dim_stride, int nchains,
                                            int nchains_padded, int nranks, const uint64_t* ranks, double* values,
                                            uint64_t* below, uint64_t* equal, void* stream) {
    if (bad_order_shape(trace_device, nslots, dim, dim_stride, nchains, nchains_padded) || !ranks || !values || nranks < 1 ||
        nranks > SMCMC_ORDER_MAX_RANKS)
        return SMCMC_ERR_INVALID;
    const u64 N = (u64)nslots * (u64)nchains;
    RankList list{};
    for (int r = 0; r < nranks; ++r) {
        if (ranks[r] >= N) return SMCMC_ERR_INVALID;
        list.r[r] = ranks[r];
    }
    if (smcmc::reduce::no_device()) return SMCMC_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    // one buffer of 64-bit words: counts[dim][cap][256], four arrays [dim][nranks], uniq[dim][cap], then the two int arrays
    const int cap = nranks;
    const size_t per = (size_t)dim * nranks, ncounts = (size_t)dim * cap * kDigits;
    const size_t words = ncounts + 5 * per + (per + 1) / 2 + ((size_t)dim + 1) / 2;
    smcmc::DeviceBuffer<u64> buf;
    if (buf.allocate(words) != hipSuccess) return SMCMC_ERR_HIP;
    u64* const d_counts = buf.get();
    SelectState st;
    st.prefix = d_counts + ncounts;
    st.resid = st.prefix + per;
    st.below = st.resid + per;
    st.equal = st.below + per;
    st.uniq = st.equal + per;
    st.slot_of = reinterpret_cast<int*>(st.uniq + per);
    st.nuniq = reinterpret_cast<int*>(st.uniq + per + (per + 1) / 2);
    if (hipMemsetAsync(buf, 0, sizeof(u64) * words, s) != hipSuccess) return SMCMC_ERR_HIP;
    hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)((per + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, list, dim,
                       nranks, st.resid);
    if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    for (int pass = 0; pass < SMCMC_ORDER_PASSES; ++pass) {
        if (launch_count(s, trace_device, nslots, dim, dim_stride, nchains, nchains_padded, pass, cap, st.uniq, st.nuniq,
                         d_counts) != hipSuccess)
            return SMCMC_ERR_HIP;
        hipLaunchKernelGGL(digit_pick_kernel, dim3((unsigned)dim), dim3(kThreads), 0, s, pass, nranks, st, d_counts);
        if (hipGetLastError() != hipSuccess) return SMCMC_ERR_HIP;
    }
    // prefix (now the key), resid, below, equal lie one behind the other
    std::vector<u64> out(4 * per);
    if (hipMemcpyAsync(out.data(), st.prefix, sizeof(u64) * out.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SMCMC_ERR_HIP;
    for (size_t k = 0; k < per; ++k) {
        values[k] = smcmc_order_value_of(out[k]);
        if (below) below[k] = out[2 * per + k];
        if (equal) equal[k] = out[3 * per + k];
    }
    return SMCMC_OK;
}
